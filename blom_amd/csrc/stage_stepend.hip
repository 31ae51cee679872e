// The end of blom_step (phy/mod_blom_step.F90:96-252), as far as it touches device arrays and no file: step_time on the host in front of
// every step (phy/mod_time.F90:182-219), updswa behind getfrc (phy/mod_swabs.F90:611-732; iniswa :216-609), fwbbal behind diaacc
// (phy/mod_forcing.F90:361-441) and chkvar last (phy/mod_chkvar.F90:77-141).  Everything here is off until its option declares it
// (api.hip: g_stepend_opts): step_time, swamth (+ blomgpu_iniswa), sprfac, chkvar.
//
// The per-step scalars (xmi, l1mi..l5mi, baclin) are kernel arguments, so none of these stages is part of a captured graph: blomgpu_step
// refuses use_graph = 1 beside them, as the coupled experiment does.
#include "blomgpu_internal.h"
#include "swabs_constants.h"
#include "thermf_relax.h"
#include <cmath>
#include <cstdio>

// one thread per point of the padded plane; the reference's loops over isp / ifp / ilp are the owned wet p-points
#define OWNED_WET_P(V) (i >= 1 && i <= (V).ii && j >= 1 && j <= (V).jj && (V).m[I_ip][c] != 0)

// ---- iniswa / updswa ---------------------------------------------------------------------------------------------------------------------
// 'top-layer' (:229-245) and 'jerlov' (:247-271): the four band planes at the owned wet p-points, every other point as it was
__global__ void k_swa_fill(const DevView *__restrict__ Vp, double fc1, double fc2, double al1, double al2) {
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  V.f[F_swfc1][c] = fc1;
  V.f[F_swfc2][c] = fc2;
  V.f[F_swal1][c] = al1;
  V.f[F_swal2][c] = al2;
}

struct UpdswaPar {
  int l1mi, l2mi, l3mi, l4mi, l5mi;
  double xmi;
  int ohl03;                                   // 0: chlorophyll_ma94, 1: chlorophyll_ohl03
  const double *lut;                           // a1_lut a2_lut b1_lut b2_lut, nval_lut entries each
  double log10chl_min, dlog10chl;
};

// updswa, :629-712: the climatology interpolated in time, the clamp, then Morel and Antoine's polynomials or Ohlmann's table
__global__ void k_updswa(const DevView *__restrict__ Vp, UpdswaPar U) {
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  const size_t np = V.nplane;
  const double chl10 = intp5(V.e[E_chl10c] + c, np, U.l1mi, U.l2mi, U.l3mi, U.l4mi, U.l5mi, U.xmi);      // :637-639
  V.e[E_chl10][c] = chl10;
  const double q = fmax2(swabs::chl10_min, fmin2(swabs::chl10_max, chl10));                                // :662, :700
  if (!U.ohl03) {
    using namespace swabs;
    const double v2 = (((((ma94_v2[5] * q + ma94_v2[4]) * q + ma94_v2[3]) * q + ma94_v2[2]) * q + ma94_v2[1]) * q + ma94_v2[0]);   // :663-668
    V.f[F_swfc1][c] = (1. - ma94_irfc) * (1. - v2);
    V.f[F_swfc2][c] = (1. - ma94_irfc) * v2;
    V.f[F_swal1][c] = ((((ma94_z1[5] * q + ma94_z1[4]) * q + ma94_z1[3]) * q + ma94_z1[2]) * q + ma94_z1[1]) * q + ma94_z1[0];
    V.f[F_swal2][c] = ((((ma94_z2[5] * q + ma94_z2[4]) * q + ma94_z2[3]) * q + ma94_z2[2]) * q + ma94_z2[1]) * q + ma94_z2[0];
  } else {
    // the nearest neighbour of the table (:702; nint rounds half away from zero, as round() does).  The clamp of q keeps n in 101..401;
    // the bounds below only keep a NaN in chl10c from indexing outside the table
    int n = (int)round((q - U.log10chl_min) / U.dlog10chl) + 1;
    n = n < 1 ? 1 : n > swabs::nval_lut ? swabs::nval_lut : n;
    gcd_t lut = global_ptr(U.lut);
    const int L = swabs::nval_lut;
    V.f[F_swfc1][c] = lut[L + n - 1];                  // a2_lut
    V.f[F_swfc2][c] = lut[n - 1];                      // a1_lut
    V.f[F_swal1][c] = 1. / lut[3 * L + n - 1];         // 1 / b2_lut
    V.f[F_swal2][c] = 1. / lut[2 * L + n - 1];         // 1 / b1_lut
  }
}

static int stepend_field(blomgpu_ctx *c, int e, const char *name) {
  if (int rc = frc_alloc(c, &c->h.e[e], kStepEndLevels[e])) return rc;
  c->real_ids[name] = FID_STEPEND + e;
  c->dirty = true;
  return 0;
}

// the four 401-entry tables of chlorophyll_ohl03, :407-441.  The reference's compiler calls pow() for 10._r8**x and log10() for log10
// (read from the object the golden generator builds); the two log10 have the exact results -3 and 1 in every libm.
static void ohl03_tables(double *lut, double *log10chl_min_out, double *dlog10chl_out) {
  using namespace swabs;
  const double log10chl_min = std::log10(chl_tab1a[0]);
  const double log10chl_max = std::log10(chl_tab1a[nval_tab1a - 1]);
  const double dlog10chl = (log10chl_max - log10chl_min) / (double)(nval_lut - 1);
  int m = 2;
  for (int n = 1; n <= nval_lut; n++) {
    const double log10chl_lut = log10chl_min + (double)(n - 1) * dlog10chl;
    double chl = std::pow(10., log10chl_lut);
    chl = fmax2(chl_tab1a[0], fmin2(chl, chl_tab1a[nval_tab1a - 1]));
    while (m < nval_tab1a && chl > chl_tab1a[m - 1]) m++;          // the interval (m-1, m] of Table 1a
    const int mm1 = m - 1;
    const double w2 = (chl - chl_tab1a[mm1 - 1]) / (chl_tab1a[m - 1] - chl_tab1a[mm1 - 1]);
    const double w1 = 1. - w2;
    lut[n - 1] = w1 * a1_tab1a[mm1 - 1] + w2 * a1_tab1a[m - 1];
    lut[nval_lut + n - 1] = w1 * a2_tab1a[mm1 - 1] + w2 * a2_tab1a[m - 1];
    lut[2 * nval_lut + n - 1] = w1 * b1_tab1a[mm1 - 1] + w2 * b1_tab1a[m - 1];
    lut[3 * nval_lut + n - 1] = w1 * b2_tab1a[mm1 - 1] + w2 * b2_tab1a[m - 1];
  }
  *log10chl_min_out = log10chl_min;
  *dlog10chl_out = dlog10chl;
}

int stepend_iniswa(blomgpu_ctx *c) {
  DevView &h = c->h;
  switch (c->swamth) {
    case SWA_NONE:
      return ctx_fail(c, "blomgpu_iniswa: swamth has not been set");
    case SWA_TOP_LAYER:
    case SWA_JERLOV: {
      double fc1 = 0., fc2 = 0., al1 = c->swamxd, al2 = c->swamxd;
      if (c->swamth == SWA_JERLOV) {
        if (c->jwtype < 1 || c->jwtype > 5) {                                                       // :252-259
          char buf[96];
          snprintf(buf, sizeof buf, " jwtype = %11d is outside the valid interval of [1,5]!", c->jwtype);
          return ctx_fail(c, buf);
        }
        const int w = c->jwtype - 1;
        fc1 = swabs::ps77_irfc[w]; fc2 = 1. - swabs::ps77_irfc[w]; al1 = swabs::ps77_al1[w]; al2 = swabs::ps77_al2[w];
      }
      ctx_sync_view(c);
      hipLaunchKernelGGL(k_swa_fill, plane_grid(h), dim3(256), 0, c->stream, c->d, fc1, fc2, al1, al2);
      HIPCHK(c, hipGetLastError());
      break;
    }
    case SWA_MA94:
    case SWA_OHL03: {
      if (c->chlopt != "climatology") return ctx_fail(c, " iniswa: chlopt = " + c->chlopt + " is unsupported!");   // :443-450
      if (c->use_graph)
        return ctx_fail(c, "blomgpu_iniswa: updswa's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
      ctx_drop_graphs(c);
      if (int rc = stepend_field(c, E_chl10c, "chl10c")) return rc;
      if (int rc = stepend_field(c, E_chl10, "chl10")) return rc;
      if (c->swamth == SWA_OHL03) {
        std::vector<double> lut(4 * swabs::nval_lut);
        ohl03_tables(lut.data(), &c->swa_log10chl_min, &c->swa_dlog10chl);
        if (!c->swa_lut) HIPCHK(c, hipMalloc((void **)&c->swa_lut, sizeof(double) * lut.size()));
        HIPCHK(c, hipMemcpyAsync(c->swa_lut, lut.data(), sizeof(double) * lut.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
      }
      break;
    }
    case SWA_SPATIAL:      // the four planes are the host's uploads (:452-599)
      break;
  }
  c->swa_ready = true;
  return 0;
}

int st_updswa(blomgpu_ctx *c) {
  if (!swa_chlorophyll(c)) return 0;                                                                // :622-627
  if (!c->swa_ready) return ctx_fail(c, "updswa: swamth names a chlorophyll method but blomgpu_iniswa has not been called");
  if (c->chlopt != "climatology") return ctx_fail(c, " updswa: chlopt = " + c->chlopt + " is unsupported!");        // :644-651
  if (c->use_graph) return ctx_fail(c, "updswa: its per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  UpdswaPar U;
  U.l1mi = c->lmi[0]; U.l2mi = c->lmi[1]; U.l3mi = c->lmi[2]; U.l4mi = c->lmi[3]; U.l5mi = c->lmi[4];
  U.xmi = c->xmi;
  U.ohl03 = c->swamth == SWA_OHL03;
  U.lut = c->swa_lut;
  U.log10chl_min = c->swa_log10chl_min;
  U.dlog10chl = c->swa_dlog10chl;
  ctx_sync_view(c);
  TimeScope ts(c, "updswa");
  hipLaunchKernelGGL(k_updswa, plane_grid(c->h), dim3(256), 0, c->stream, c->d, U);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- fwbbal ------------------------------------------------------------------------------------------------------------------------------
__global__ void k_fwbbal_acc(const DevView *__restrict__ Vp, double baclin) {                       // :379-390
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  V.e[E_eiacc][c] = V.e[E_eiacc][c] + (V.f[F_eva][c] + V.f[F_fmltfz][c]) * baclin;
  V.e[E_pracc][c] = V.e[E_pracc][c] + (((V.f[F_lip][c] + V.f[F_sop][c]) + V.f[F_rnf][c]) + V.f[F_rfi][c]) * baclin;
}
// the area weighting of the year's end, :398-407.  to_util (tiles): the weighted values go to util1 / util2 instead, zero outside the world
// ocean's mask -- the sums across tiles know registered planes and the ip mask only, and a zero added leaves a sum's bits as they are;
// eiacc and pracc are zeroed behind the sums either way
__global__ void k_fwbbal_scale(const DevView *__restrict__ Vp, int to_util) {
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  const double s = V.f[F_scp2][c];
  const double ei = V.e[E_eiacc][c] * s, pr = V.e[E_pracc][c] * s;
  if (to_util) {
    const bool in = V.m[I_ipwocn][c] == 1;
    V.f[F_util1][c] = in ? ei : 0.;
    V.f[F_util2][c] = in ? pr : 0.;
  } else {
    V.e[E_eiacc][c] = ei;
    V.e[E_pracc][c] = pr;
  }
}
__global__ void k_fwbbal_zero(const DevView *__restrict__ Vp) {                                     // :345-357, :419-429
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  V.e[E_eiacc][c] = 0.;
  V.e[E_pracc][c] = 0.;
}

// sprfac = 1: what inivar_forcing does for it (:345-357)
int stepend_set_sprfac(blomgpu_ctx *c) {
  DevView &h = c->h;
  if (!c->sprfac) return 0;
  c->prfac = 1.;
  if (int rc = stepend_field(c, E_eiacc, "eiacc")) return rc;
  if (int rc = stepend_field(c, E_pracc, "pracc")) return rc;
  if (!h.m[I_ipwocn]) {                                  // the coupled experiment's mask of the world ocean: the host uploads it
    const size_t bytes = sizeof(int) * (size_t)h.nplane;
    HIPCHK(c, hipMalloc((void **)&h.m[I_ipwocn], bytes));
    HIPCHK(c, hipMemsetAsync(h.m[I_ipwocn], 0, bytes, c->stream));
  }
  c->int_ids["ipwocn"] = I_ipwocn;
  c->dirty = true;
  ctx_sync_view(c);
  hipLaunchKernelGGL(k_fwbbal_zero, plane_grid(h), dim3(256), 0, c->stream, c->d);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int st_fwbbal(blomgpu_ctx *c) {
  if (!c->sprfac) return 0;                                                                         // :373
  DevView &h = c->h;
  if (!h.e[E_eiacc] || !h.e[E_pracc]) return ctx_fail(c, "fwbbal: eiacc and pracc have no memory");
  if (c->use_graph) return ctx_fail(c, "fwbbal: its per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  if (c->nstep_in_day < 1) return ctx_fail(c, "fwbbal: nstep_in_day has not been set");
  ctx_sync_view(c);
  TimeScope ts(c, "fwbbal");
  hipLaunchKernelGGL(k_fwbbal_acc, plane_grid(h), dim3(256), 0, c->stream, c->d, h.P.baclin);
  HIPCHK(c, hipGetLastError());
  if (!(c->nday_of_year == 1 && h.P.nstep % c->nstep_in_day == 0)) return 0;                        // :394
  // the end of a year: the two sums under the world ocean's mask in xcsum's order, the new factor on the host, the planes to zero
  const bool tiles = c->tiling.multi();
  if (tiles && h.nreg == 2) return ctx_fail(c, "fwbbal: the sums of the year's end across the arctic seam are built for a single tile");
  if (!c->fwb_buf) HIPCHK(c, hipMalloc((void **)&c->fwb_buf, sizeof(double) * (2 + 2 * (size_t)h.jtdm)));
  hipLaunchKernelGGL(k_fwbbal_scale, plane_grid(h), dim3(256), 0, c->stream, c->d, tiles ? 1 : 0);
  HIPCHK(c, hipGetLastError());
  const double *planes[2] = {tiles ? h.f[F_util1] : h.e[E_eiacc], tiles ? h.f[F_util2] : h.e[E_pracc]};
  if (!tiles) {
    const int *masks[2] = {h.m[I_ipwocn], h.m[I_ipwocn]};
    if (int rc = st_xcsum_batch(c, 2, planes, masks, c->fwb_buf + 2, c->fwb_buf)) return rc;
  } else {
    for (int q = 0; q < 2; q++) {                        // the one-plane sums in global order (thermf_channel's), ip mask
      double *sums = nullptr;
      if (int rc = st_xcsum_dev(c, planes[q], 1, 7, &sums)) return rc;
      HIPCHK(c, hipMemcpyAsync(c->fwb_buf + q, sums + 7, sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    }
  }
  double tot[2] = {0., 0.};
  HIPCHK(c, hipMemcpyAsync(tot, c->fwb_buf, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->prfac = -c->prfac * tot[0] / tot[1];                                                           // :412
  hipLaunchKernelGGL(k_fwbbal_zero, plane_grid(h), dim3(256), 0, c->stream, c->d);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- chkvar ------------------------------------------------------------------------------------------------------------------------------
// One thread per owned wet p-point walks k = 1..kk of time level n and tests dp, temp, saln as the reference does: a /= a, then a*0 /= 0
// (:42-71).  A hit sets the error word and lowers the key of the first hit in the SERIAL reference's loop order -- j, then k, then i,
// then the six tests in the routine's order (:88-138): the OpenMP build reports whichever thread comes first, and a check needs one answer.
// The thread's own first hit in k is its smallest key, so it stops there.  Both are ordinary vector atomics on device words.
__device__ inline int chk_test(double a) { return a != a ? 0 : a * 0. != 0. ? 1 : -1; }
__global__ void k_chkvar(const DevView *__restrict__ Vp, int nn, unsigned long long *words) {
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  if (!OWNED_WET_P(V)) return;
  const size_t np = V.nplane;
  gcd_t dp = V.f[F_dp] + c + (size_t)nn * np, temp = V.f[F_temp] + c + (size_t)nn * np, saln = V.f[F_saln] + c + (size_t)nn * np;
  const int kk = V.kk;
  for (int k0 = 0; k0 < kk; k0 += COLUMN_U) {
    const int nu = kk - k0 < COLUMN_U ? kk - k0 : COLUMN_U;
    double d[COLUMN_U], t[COLUMN_U], s[COLUMN_U];
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++)
      if (u < nu) { d[u] = dp[(size_t)(k0 + u) * np]; t[u] = temp[(size_t)(k0 + u) * np]; s[u] = saln[(size_t)(k0 + u) * np]; }
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++) {
      if (u >= nu) break;
      int hit = chk_test(d[u]);
      if (hit < 0) { hit = chk_test(t[u]); if (hit >= 0) hit += 2; }
      if (hit < 0) { hit = chk_test(s[u]); if (hit >= 0) hit += 4; }
      if (hit >= 0) {
        const unsigned long long key =
            ((((unsigned long long)(j - 1) * (unsigned)kk + (unsigned)(k0 + u)) * (unsigned)V.ii + (unsigned)(i - 1)) * 6ull) + (unsigned)hit;
        atomicOr(&words[0], 1ull);
        atomicMin(&words[1], key);
        return;
      }
    }
  }
}

static int chk_words(blomgpu_ctx *c) {
  if (c->chk_dev) return 0;
  const unsigned long long init[2] = {0ull, ~0ull};
  HIPCHK(c, hipMalloc((void **)&c->chk_dev, sizeof(init)));
  HIPCHK(c, hipMemcpy(c->chk_dev, init, sizeof(init), hipMemcpyHostToDevice));
  return 0;
}

int st_chkvar(blomgpu_ctx *c, int nn) {
  if (!c->chkvar) return 0;
  if (nn != 0 && nn != c->h.kk) return ctx_fail(c, "chkvar: nn is neither 0 nor kk");
  if (c->use_graph) return ctx_fail(c, "chkvar: its error words are read back by the host every check_period steps, outside a captured graph (set use_graph = 0)");
  if (int rc = chk_words(c)) return rc;
  ctx_sync_view(c);
  {
    TimeScope ts(c, "chkvar");
    hipLaunchKernelGGL(k_chkvar, plane_grid(c->h), dim3(256), 0, c->stream, c->d, nn, c->chk_dev);
    HIPCHK(c, hipGetLastError());
  }
  if (!c->seq.defer_checks) return ctx_check_errors(c);
  return 0;
}

// Fortran's i4 edit descriptor: four characters, right-justified; asterisks when the value does not fit
static std::string fmt_i4(long long v) {
  char buf[32];
  snprintf(buf, sizeof buf, "%4lld", v);
  return std::string(buf).size() > 4 ? "****" : buf;
}
// the key of k_chkvar back into the reference's line (:94-96 and its five siblings), with the global indices i0 + i, j0 + j
static std::string stepend_chkvar_line(unsigned long long key, int ii, int kk, int i0, int j0) {
  static const char *const what[6] = {"dp is NaN", "dp is Inf", "temp is NaN", "temp is Inf", "saln is NaN", "saln is Inf"};
  const int t = (int)(key % 6ull);
  key /= 6ull;
  const long long i = (long long)(key % (unsigned long long)ii) + 1;
  key /= (unsigned long long)ii;
  const long long k = (long long)(key % (unsigned long long)kk) + 1;
  const long long j = (long long)(key / (unsigned long long)kk) + 1;
  return std::string(" chkvar: ") + what[t] + " at (i =" + fmt_i4(i0 + i) + ", j =" + fmt_i4(j0 + j) + ", k =" + fmt_i4(k) + ")";
}

int stepend_check_errors(blomgpu_ctx *c) {
  if (!c->chk_dev) return 0;
  unsigned long long w[2] = {0ull, ~0ull};
  HIPCHK(c, hipMemcpyAsync(w, c->chk_dev, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!w[0]) return 0;
  const unsigned long long init[2] = {0ull, ~0ull};      // reported once: the words start over
  HIPCHK(c, hipMemcpyAsync(c->chk_dev, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return ctx_fail(c, "blom:" + stepend_chkvar_line(w[1], c->h.ii, c->h.kk, c->h.i0, c->h.j0));
}

// ---- step_time ---------------------------------------------------------------------------------------------------------------------------
// phy/mod_time.F90:193-217 with the incremented step number ns1: the day of the year moves on when a day ends -- date_offset +
// set_day_of_year inside a year, and across a year's end whose successor has the same length -- then the position in the year in months,
// in double and in the reference's order (this file is compiled without contraction).  The values go where the setters put them.
int stepend_step_time(blomgpu_ctx *c, int ns1) {
  const int sd = c->nstep_in_day, nd = c->h.P.nday_in_year;
  if (ns1 % sd == 0) c->nday_of_year = c->nday_of_year % nd + 1;
  double xmi = ((double)(c->nday_of_year - 1) + (double)(ns1 % sd) / (double)sd) * 12. / (double)nd;
  const int l3mi = (int)xmi + 1;
  if (l3mi < 1 || l3mi > 12) return ctx_fail(c, "blomgpu_step: step_time: nday_of_year lies outside the year of nday_in_year days");
  xmi = xmi - (double)(l3mi - 1);
  c->xmi = xmi;
  c->lmi[0] = (l3mi + 9) % 12 + 1;
  c->lmi[1] = (l3mi + 10) % 12 + 1;
  c->lmi[2] = l3mi;
  c->lmi[3] = l3mi % 12 + 1;
  c->lmi[4] = (l3mi + 1) % 12 + 1;
  return 0;
}

int stepend_step_check(blomgpu_ctx *c) {
  if (c->step_time && (c->nstep_in_day < 1 || c->h.P.nday_in_year < 1))
    return ctx_fail(c, "blomgpu_step: step_time = 1 needs nstep_in_day >= 1 and nday_in_year >= 1 (set both before the call)");
  if (c->use_graph) {
    const char *who = c->step_time ? "step_time" : swa_chlorophyll(c) ? "updswa (a chlorophyll swamth)" : c->sprfac ? "fwbbal (sprfac)" : c->chkvar ? "chkvar" : nullptr;
    if (who)
      return ctx_fail(c, std::string("blomgpu_step: ") + who + ": the per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  }
  return 0;
}

void stepend_free(blomgpu_ctx *c) {
  for (int e = 0; e < NF_STEPEND; e++)
    if (c->h.e[e]) { (void)hipFree(c->h.e[e]); c->h.e[e] = nullptr; }
  if (c->swa_lut) (void)hipFree(c->swa_lut);
  if (c->chk_dev) (void)hipFree(c->chk_dev);
  if (c->fwb_buf) (void)hipFree(c->fwb_buf);
  c->swa_lut = nullptr; c->chk_dev = nullptr; c->fwb_buf = nullptr;
}
