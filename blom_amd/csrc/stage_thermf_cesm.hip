// The surface forcing of the coupled experiment (expcnf = 'cesm', BLOM inside NorESM): getfrc_cesm, sfcstr_cesm, thermf_cesm.
//
//   k_getfrc_cesm           cesm/mod_cesm.F90:213-262: the coupler's fields of two coupling intervals interpolated in time,
//                           w1*x_da(l1ci) + w2*x_da(l2ci), fourteen fields in one launch (w1 from the host: its own cos)
//   k_sfcstr_cesm           cesm/mod_sfcstr_cesm.F90:43-55: taux = ztx at u-points, tauy = mty at v-points
//   k_thermf_cesm_flux      cesm/mod_thermf_cesm.F90:87-332 per owned wet p-point: freezing temperatures, fresh water / brine / virtual
//                           salt fluxes, freezing and melting potentials, heat fluxes, tracer fluxes, the relaxation towards SST and
//                           SSS (climatology or streams; both vertical coordinates), the applied and the diagnosed relaxation fluxes,
//                           the friction velocity -- and the area weighted planes of every global sum that follows
//   st_xcsum_batch          :342, :363-364, :398: 1 + ntr' + 2 sums in two launches (halo.hip), left ON THE DEVICE
//   k_thermf_cesm_corr      :343-410: the corrections that need the sums
// so that thermf_cesm is four launches up to 32 planes in the batch (ntr' <= 31, 29 with srxbal; two more per further 32).  The per-step scalars (w1; y, m1..m5, ntld of :74-84) are
// formed on the host and passed as kernel arguments.  swtfrz is the stand-alone driver's (drivers/nocoupler/mod_swtfrz.F:
// atf*s+btf+ctf*p with inieos' coefficients for 'cesm', phy/mod_eos.F90:133-136); the NUOPC driver's form needs CESM's share code.
// Not built: the coupler fields no device stage reads (hmat slp abswnd lamult lasl ustokes vstokes atm*).
// Roofline: HBM, ~45 two-dimensional planes (plus 2 kk + 2 (kk+1) levels under the hybrid coordinate); launch-bound at channel size.
#include "blomgpu_internal.h"
#include "pow_libm.h"
#include "thermf_relax.h"
#include <cmath>

struct GetfrcPar { double w1, w2; int l1, l2; };      // l1, l2: 0-based levels of the _da pairs

struct ThermfCesmPar {
  double trxday, srxday, trxdpt, srxdpt, trxlim, srxlim, xmi, sref, area, baclin, y;
  double atf, btf, ctf;          // swtfrz
  double gls_c, gls_vk, gls_z;   // gls_cmu0**gls_p, vonKar**gls_n, Zos**(gls_n-1.) (phy/mod_tke.F90:36-58)
  int l1mi, l2mi, l3mi, l4mi, l5mi, m1, m2, m3, m4, m5, ntld;   // 1-based, as the reference's
  int use_gls, stream, aptflx, apsflx, ditflx, disflx, srxbal, hybrid;
};

__global__ void k_getfrc_cesm(const DevView *__restrict__ Vp, GetfrcPar G) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii) return;
  const size_t o1 = c + (size_t)G.l1 * V.nplane, o2 = c + (size_t)G.l2 * V.nplane;
#define GETFRC(dst, src) V.f[dst][c] = G.w1 * V.f[src][o1] + G.w2 * V.f[src][o2]
  if (V.m[I_ip][c]) {
    GETFRC(F_ustarw, F_ustarw_da); GETFRC(F_lip, F_lip_da); GETFRC(F_sop, F_sop_da); GETFRC(F_eva, F_eva_da);
    GETFRC(F_rnf, F_rnf_da); GETFRC(F_rfi, F_rfi_da); GETFRC(F_fmltfz, F_fmltfz_da); GETFRC(F_sfl, F_sfl_da);
    GETFRC(F_swa, F_swa_da); GETFRC(F_nsf, F_nsf_da); GETFRC(F_hmlt, F_hmlt_da); GETFRC(F_ficem, F_ficem_da);
  }
  if (V.m[I_iu][c]) GETFRC(F_ztx, F_ztx_da);
  if (V.m[I_iv][c]) GETFRC(F_mty, F_mty_da);
#undef GETFRC
}

__global__ void k_sfcstr_cesm(const DevView *__restrict__ Vp) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii) return;
  if (V.m[I_iu][c]) V.f[F_taux][c] = V.f[F_ztx][c];
  if (V.m[I_iv][c]) V.f[F_tauy][c] = V.f[F_mty][c];
}

__global__ void k_thermf_cesm_flux(const DevView *__restrict__ Vp, ThermfCesmPar T, int nn, int k1m, int k1n) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii || !V.m[I_ip][c]) return;
  const size_t np = V.nplane, o1 = c + (size_t)nn * np, o2 = o1 + np, okm = c + (size_t)(k1m - 1) * np, okn = c + (size_t)(k1n - 1) * np;
  const int kk = V.kk, ntr = V.ntr;
  gcd_t dp = V.f[F_dp], temp = V.f[F_temp], saln = V.f[F_saln];
  const double p1 = V.f[F_p][c];
  // freezing temperatures of sea water, :87-88
  const double tfrz = T.atf * saln[okn] + T.btf + T.ctf * p1;
  const double tfrzm = T.atf * (.5 * (saln[okm] + saln[okn])) + T.btf + T.ctf * p1;
  // ocean top layer quantities, :104-109
  const double dpotl = dp[okn];
  const double totl = temp[okn] + T0DEG;
  const double sotl = saln[okn];
  const double tice_f = tfrz + T0DEG;
  // fresh water and salt fluxes, :116-135
  const double fmltfz = V.f[F_fmltfz][c], sfl = V.f[F_sfl][c];
  const double fwflx = V.f[F_eva][c] + V.f[F_lip][c] + V.f[F_sop][c] + V.f[F_rnf][c] + V.f[F_rfi][c] + fmltfz;
  V.f[F_brnflx][c] = fmax2(0., -sotl * fmltfz * G2KG + sfl);
  const double vrtsfl = -sotl * fwflx * G2KG;
  WK2(V, S2_VRTSFL)[c] = vrtsfl;
  const double scp2 = V.f[F_scp2][c];
  gd_t util = V.f[F_thermf_util] + c;
  util[0] = -(T.sref * fwflx * G2KG + vrtsfl + V.f[F_salt_corr][c] * G2KG / (2. * T.baclin)) * scp2;
  V.f[F_salt_corr][c] = 0.;
  // heat fluxes, :146-158
  const double frzpot = fmax2(0., tice_f - totl) * SPCIFH * dpotl / (2. * GRAV);
  V.f[F_frzpot][c] = frzpot;
  V.f[F_mltpot][c] = fmin2(0., tfrzm - .5 * (temp[okm] + temp[okn])) * SPCIFH * .5 * (dp[okm] + dp[okn]) / GRAV;
  const double hmltfz = V.f[F_hmlt][c] + frzpot / T.baclin;
  V.f[F_hmltfz][c] = hmltfz;
  const double swa = V.f[F_swa][c];
  V.f[F_surflx][c] = -(swa + V.f[F_nsf][c] + hmltfz);
  V.f[F_sswflx][c] = -swa;
  // tracer fluxes (positive downwards), :165-186; and the area weighted plane of each tracer's global sum with the reset of its
  // correction, :391-393 (nothing in between changes trflx)
  int q = 1;
  for (int nt = 0; nt < ntr; nt++) {
    gd_t trflx = V.f[F_trflx] + c + (size_t)nt * np;
    if (V.P.itrtke >= 1 && nt + 1 == V.P.itrtke) { *trflx = 0.; continue; }
    if (V.P.itrtke >= 1 && nt + 1 == V.P.itrgls) {
      *trflx = T.use_gls ? V.f[F_difdia][c] * T.gls_c * pow_libm(V.f[F_trc][okn + (size_t)(V.P.itrtke - 1) * 2 * kk * np], 1.5) * T.gls_vk * T.gls_z   // (-gls_n = 1)
                         : 0.;
      continue;
    }
    const double tf = -V.f[F_trc][okn + (size_t)nt * 2 * kk * np] * fwflx;
    *trflx = tf;
    gd_t corr = V.f[F_trc_corr] + c + (size_t)nt * np;
    util[(size_t)q * np] = -(tf + *corr / (2. * T.baclin)) * scp2;
    *corr = 0.;
    q++;
  }
  // relaxation fluxes, :193-322
  double pbot = p1;
  if (T.hybrid && (T.trxday > EPSILT || T.srxday > EPSILT)) {            // :218-222, :279-283
    int k = 0;
    for (; k + COLUMN_U <= kk; k += COLUMN_U) {
      double d[COLUMN_U];
#pragma unroll
      for (int u = 0; u < COLUMN_U; u++) d[u] = dp[o1 + (size_t)(k + u) * np];
#pragma unroll
      for (int u = 0; u < COLUMN_U; u++) pbot = pbot + d[u];
    }
    for (; k < kk; k++) pbot = pbot + dp[o1 + (size_t)k * np];
  }
  double surrlx = 0., trxflx = 0.;
  if (T.trxday > EPSILT) {
    double sstc, rice;
    if (T.stream) {
      sstc = V.f[F_sst_stream][c];
      rice = V.f[F_ice_stream][c];
    } else {
      sstc = intp5(V.f[F_sstclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
      rice = intp5(V.f[F_ricclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
    }
    sstc = (1. - rice) * fmax2(sstc, tice_f) + rice * tice_f;
    if (!T.hybrid) {
      const double dpmxl = dp[o1] + dp[o2];
      const double hmxl = dpmxl / ONEM;
      const double tmxl = (temp[o1] * dp[o1] + temp[o2] * dp[o2]) / dpmxl + T0DEG;
      trxflx = SPCIFH * fmin2(hmxl, T.trxdpt) / (T.trxday * 86400.) * fmin2(T.trxlim, fmax2(-T.trxlim, sstc - tmxl)) / ALPHA0;
    } else {
      const double dprsi = 1. / fmin2(T.trxdpt * ONEM, pbot - p1);
      const double tmxl = rs_walk(dp + o1, temp + o1, V.f[F_t_rs_nonloc] + c, np, kk, dprsi, true);
      trxflx = SPCIFH * T.trxdpt / (T.trxday * 86400.) * fmin2(T.trxlim, fmax2(-T.trxlim, sstc - tmxl)) / ALPHA0;
    }
    surrlx = -trxflx;
  }
  if (T.aptflx) surrlx = surrlx - intp5(V.f[F_tflxap] + c, np, T.m1, T.m2, T.m3, T.m4, T.m5, T.y);
  V.f[F_surrlx][c] = surrlx;
  if (T.ditflx) {
    gd_t di = V.f[F_tflxdi] + c + (size_t)(T.ntld - 1) * np;
    *di = *di + trxflx;
  }
  double salrlx = 0., srxflx = 0.;
  if (T.srxday > EPSILT) {
    const double sssc = T.stream ? V.f[F_sss_stream][c] : intp5(V.f[F_sssclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
    if (!T.hybrid) {
      const double dpmxl = dp[o1] + dp[o2];
      const double hmxl = dpmxl / ONEM;
      const double smxl = (saln[o1] * dp[o1] + saln[o2] * dp[o2]) / dpmxl;
      srxflx = fmin2(hmxl, T.srxdpt) / (T.srxday * 86400.) * fmin2(T.srxlim, fmax2(-T.srxlim, sssc - smxl)) / ALPHA0;
    } else {
      const double dprsi = 1. / fmin2(T.srxdpt * ONEM, pbot - p1);
      const double smxl = rs_walk(dp + o1, saln + o1, V.f[F_s_rs_nonloc] + c, np, kk, dprsi, false);
      srxflx = T.srxdpt / (T.srxday * 86400.) * fmin2(T.srxlim, fmax2(-T.srxlim, sssc - smxl)) / ALPHA0;
    }
    salrlx = -srxflx;
    V.f[F_util2][c] = fmax2(0., salrlx) * scp2;
    V.f[F_util3][c] = fmin2(0., salrlx) * scp2;
  }
  if (T.apsflx) salrlx = salrlx - intp5(V.f[F_sflxap] + c, np, T.m1, T.m2, T.m3, T.m4, T.m5, T.y);
  V.f[F_salrlx][c] = salrlx;
  if (T.disflx) {
    gd_t di = V.f[F_sflxdi] + c + (size_t)(T.ntld - 1) * np;
    *di = *di + srxflx;
  }
  // friction velocity, :328
  V.f[F_ustar][c] = V.f[F_ustarw][c];
}

// :343-410; sums[0] = the salt plane's sum, sums[1 .. ntr'] the tracers' in their order, sums[ntr'+1], sums[ntr'+2] = totsrp, totsrn
__global__ void k_thermf_cesm_corr(const DevView *__restrict__ Vp, ThermfCesmPar T, const double *__restrict__ sums, int nq) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii || !V.m[I_ip][c]) return;
  const size_t np = V.nplane;
  const double sflxc = sums[0] / T.area;
  V.f[F_salflx][c] = -(WK2(V, S2_VRTSFL)[c] + sflxc + V.f[F_sfl][c]) * KG2G;
  V.f[F_brnflx][c] = -V.f[F_brnflx][c] * KG2G;
  if (T.srxday > EPSILT && T.srxbal) {
    const double totsrp = sums[nq], totsrn = sums[nq + 1];
    if (fabs(totsrp - totsrn) > 0.) {
      const double qp = 2. * totsrn / (totsrn - totsrp);
      const double qn = 2. * totsrp / (totsrp - totsrn);
      if (V.m[I_ipwocn][c] == 1) {
        const double s = V.f[F_salrlx][c];
        V.f[F_salrlx][c] = qp * fmax2(0., s) + qn * fmin2(0., s);
      }
    }
  }
  int q = 1;
  for (int nt = 0; nt < V.ntr; nt++) {
    if (V.P.itrtke >= 1 && (nt + 1 == V.P.itrtke || nt + 1 == V.P.itrgls)) continue;
    const double trflxc = sums[q++] / T.area;
    gd_t trflx = V.f[F_trflx] + c + (size_t)nt * np;
    *trflx = -(*trflx + trflxc);
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int frc_alloc(blomgpu_ctx *c, double **p, int nlev) {
  if (*p) return 0;
  const size_t bytes = sizeof(double) * (size_t)nlev * c->h.nplane;
  HIPCHK(c, hipMalloc((void **)p, bytes));
  HIPCHK(c, hipMemsetAsync(*p, 0, bytes, c->stream));
  c->dirty = true;
  return 0;
}
static bool cesm_lazy(int fid) { return fid == F_tflxap || fid == F_sflxap || fid == F_tflxdi || fid == F_sflxdi; }

int cesm_field(blomgpu_ctx *c, int fid) {
  if (fid < NF_BASE_REAL || fid >= NF_REAL || c->h.f[fid]) return 0;
  if (!frc_declared(c)) return ctx_fail(c, "a field of the coupled experiment does not exist until blomgpu_inifrc_cesm has been called");
  return frc_alloc(c, &c->h.f[fid], c->nlev_real[fid]);
}

// the global sums of thermf (3 + ntr, on the device) and their row sums
int frc_sum_buffers(blomgpu_ctx *c) {
  const DevView &h = c->h;
  const int nsum = 3 + (h.ntr > 0 ? h.ntr : 1);
  if (!c->cesm_sums) HIPCHK(c, hipMalloc((void **)&c->cesm_sums, sizeof(double) * nsum));
  if (!c->cesm_rows) HIPCHK(c, hipMalloc((void **)&c->cesm_rows, sizeof(double) * (size_t)nsum * h.jtdm));
  HIPCHK(c, hipMemsetAsync(c->cesm_sums, 0, sizeof(double) * nsum, c->stream));
  return 0;
}

// inifrc_cesm, cesm/mod_cesm.F90:175-200.  The file reads of initai / rdcsic / rdctsf / rdcsss / idarlx stay the host's (sstclm ricclm
// sssclm tflxap sflxap are uploaded by name); idarlx's zeroing of the diagnosed fluxes and their counts (phy/mod_idarlx.F90:89-114) and
// the time level indices are done here.  The call is also the declaration that the coupler's forcing exists: it allocates and names
// the fields of BLOM_CESM_REAL_FIELDS / BLOM_CESM_INT_FIELDS.
int cesm_inifrc(blomgpu_ctx *c) {
  DevView &h = c->h;
  ctx_drop_graphs(c);
  if (!c->cesm_declared) {
    int id = NF_BASE_REAL;
#define X(name, lev) c->real_ids[#name] = id++;
    BLOM_CESM_REAL_FIELDS(X)
#undef X
    id = NF_BASE_INT;
#define X(name, lev) c->int_ids[#name] = id++;
    BLOM_CESM_INT_FIELDS(X)
#undef X
    c->cesm_declared = true;
  }
  for (int f = NF_BASE_REAL; f < NF_REAL; f++)
    if (!cesm_lazy(f))
      if (int rc = frc_alloc(c, &h.f[f], c->nlev_real[f])) return rc;
  for (int f = NF_BASE_INT; f < NF_INT; f++) {
    if (h.m[f]) continue;
    const size_t bytes = sizeof(int) * (size_t)c->nlev_int[f] * h.nplane;
    HIPCHK(c, hipMalloc((void **)&h.m[f], bytes));
    HIPCHK(c, hipMemsetAsync(h.m[f], 0, bytes, c->stream));
  }
  if (int rc = frc_sum_buffers(c)) return rc;
  // the 48-level arrays whose option is on already (one switched on later: api.hip's option table allocates it then, outside the step)
  if (c->aptflx) if (int rc = frc_alloc(c, &h.f[F_tflxap], NLEV_RLX)) return rc;
  if (c->apsflx) if (int rc = frc_alloc(c, &h.f[F_sflxap], NLEV_RLX)) return rc;
  if (c->ditflx || c->disflx) {                                   // phy/mod_idarlx.F90:89-114
    for (int &n : c->nflxdi) n = 0;
    for (int f : {(int)F_tflxdi, (int)F_sflxdi}) {
      if (!(f == F_tflxdi ? c->ditflx : c->disflx)) continue;
      if (int rc = frc_alloc(c, &h.f[f], NLEV_RLX)) return rc;
      HIPCHK(c, hipMemsetAsync(h.f[f], 0, sizeof(double) * (size_t)NLEV_RLX * h.nplane, c->stream));
    }
  }
  c->l1ci = c->l2ci = 1;
  c->dirty = true;
  return 0;
}

void cesm_free(blomgpu_ctx *c) {
  if (c->cesm_sums) (void)hipFree(c->cesm_sums);
  if (c->cesm_rows) (void)hipFree(c->cesm_rows);
  c->cesm_sums = c->cesm_rows = nullptr;
}

// what the coupled stages refuse before they launch anything
static int cesm_ready(blomgpu_ctx *c, const char *who) {
  if (!cesm_on(c)) return ctx_fail(c, std::string(who) + ": the coupler's forcing has not been declared (blomgpu_inifrc_cesm, expcnf = 'cesm')");
  if (c->use_graph)
    return ctx_fail(c, std::string(who) + ": the coupled experiment's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  return 0;
}

int st_getfrc_cesm(blomgpu_ctx *c) {
  if (int rc = cesm_ready(c, "getfrc_cesm")) return rc;
  if (c->l1ci < 1 || c->l1ci > 2 || c->l2ci < 1 || c->l2ci > 2) return ctx_fail(c, "getfrc_cesm: l1ci and l2ci are 1 or 2");
  GetfrcPar G;
  G.w1 = 0.;
  if (c->smtfrc) {                                                 // cesm/mod_cesm.F90:213-219 (the reference's own pi)
    if (c->nstep_in_cpl < 1) return ctx_fail(c, "getfrc_cesm: nstep_in_cpl has not been set");
    G.w1 = .5 * (1. + std::cos((double)((c->h.P.nstep - 1) % c->nstep_in_cpl + 1) * PI_BLOM / (double)c->nstep_in_cpl));
  }
  G.w2 = 1. - G.w1;
  G.l1 = c->l1ci - 1;
  G.l2 = c->l2ci - 1;
  ctx_sync_view(c);
  TimeScope ts(c, "getfrc_cesm");
  hipLaunchKernelGGL(k_getfrc_cesm, plane_grid(c->h), dim3(256), 0, c->stream, c->d, G);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int st_sfcstr_cesm(blomgpu_ctx *c) {
  if (int rc = cesm_ready(c, "sfcstr_cesm")) return rc;
  ctx_sync_view(c);
  TimeScope ts(c, "sfcstr");
  hipLaunchKernelGGL(k_sfcstr_cesm, plane_grid(c->h), dim3(256), 0, c->stream, c->d);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int st_thermf_cesm(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  (void)m; (void)n; (void)mm;
  if (int rc = cesm_ready(c, "thermf_cesm")) return rc;
  DevView &h = c->h;
  if (c->area <= 0.) return ctx_fail(c, "thermf_cesm: the ocean area (mod_grid: area) has not been set");
  if (c->nstep_in_day < 1 || h.P.nday_in_year < 1) return ctx_fail(c, "thermf_cesm: nstep_in_day and nday_in_year have not been set");
  ThermfCesmPar T;
  T.trxday = c->trxday; T.srxday = c->srxday; T.trxdpt = c->trxdpt; T.srxdpt = c->srxdpt; T.trxlim = c->trxlim; T.srxlim = c->srxlim;
  T.xmi = c->xmi; T.sref = c->sref; T.area = c->area; T.baclin = h.P.baclin;
  T.atf = 0.; T.btf = -1.8; T.ctf = 0.;                                                          // phy/mod_eos.F90:133-136
  T.use_gls = h.P.itrtke >= 1 && h.P.gls ? 1 : 0;
  T.gls_c = std::pow(.527, 3.); T.gls_vk = std::pow(.4, -1.); T.gls_z = std::pow(.0002, -1. - 1.);
  T.l1mi = c->lmi[0]; T.l2mi = c->lmi[1]; T.l3mi = c->lmi[2]; T.l4mi = c->lmi[3]; T.l5mi = c->lmi[4];
  // time interpolation of the diagnosed relaxation fluxes, :74-84
  double y = ((double)(c->nday_of_year - 1) + (double)(h.P.nstep % c->nstep_in_day) / (double)c->nstep_in_day) * 48. / (double)h.P.nday_in_year;
  const int m3 = (int)y + 1;
  y = y - (double)(m3 - 1);
  if (m3 < 1 || m3 > NLEV_RLX) return ctx_fail(c, "thermf_cesm: nday_of_year lies outside the year");
  T.y = y;
  T.m3 = m3; T.m1 = (m3 + 45) % 48 + 1; T.m2 = (m3 + 46) % 48 + 1; T.m4 = m3 % 48 + 1; T.m5 = (m3 + 1) % 48 + 1;
  T.ntld = m3;
  T.stream = c->use_stream_relaxation; T.aptflx = c->aptflx; T.apsflx = c->apsflx; T.ditflx = c->ditflx; T.disflx = c->disflx;
  T.srxbal = c->srxbal; T.hybrid = h.P.vcoord_tag != 1;
  const bool bal = c->srxday > EPSILT && c->srxbal;
  if (bal && c->tiling.multi()) return ctx_fail(c, "thermf_cesm: the balanced salinity relaxation (srxbal) is built for a single tile");
  if (c->aptflx) if (int rc = cesm_field(c, F_tflxap)) return rc;
  if (c->apsflx) if (int rc = cesm_field(c, F_sflxap)) return rc;
  if (c->ditflx) if (int rc = cesm_field(c, F_tflxdi)) return rc;
  if (c->disflx) if (int rc = cesm_field(c, F_sflxdi)) return rc;
  ctx_sync_view(c);
  if (c->ditflx || c->disflx) c->nflxdi[T.ntld - 1]++;                                           // :90
  // the planes of the batch: salt, the tracers that are not turbulence tracers, then totsrp / totsrn with the world ocean's mask
  int nq = 1;
  for (int nt = 1; nt <= h.ntr; nt++)
    if (!(h.P.itrtke >= 1 && (nt == h.P.itrtke || nt == h.P.itrgls))) nq++;
  std::vector<const double *> planes;
  std::vector<const int *> masks;
  for (int q = 0; q < nq; q++) { planes.push_back(h.f[F_thermf_util] + (size_t)q * h.nplane); masks.push_back(nullptr); }
  if (bal) {
    planes.push_back(h.f[F_util2]); masks.push_back(h.m[I_ipwocn]);
    planes.push_back(h.f[F_util3]); masks.push_back(h.m[I_ipwocn]);
  }
  // (the stage's timer, and one per part of it: each part's count is its number of launch groups, tools/gpu_thermf_cesm_cost.py)
  TimeScope ts(c, "thermf");
  {
    TimeScope t1(c, "thermf_cesm_flux");
    hipLaunchKernelGGL(k_thermf_cesm_flux, plane_grid(h), dim3(256), 0, c->stream, c->d, T, nn, k1m, k1n);
    c->cesm_launches++;
  }
  if (c->cesm_single_sums) {                         // (A/B: the reference's 1 + ntr' + 2 separate sums)
    for (size_t q = 0; q < planes.size(); q++) {
      TimeScope t2(c, "thermf_cesm_sums");
      if (int rc = st_xcsum_batch(c, 1, &planes[q], &masks[q], c->cesm_rows, c->cesm_sums + q)) return rc;
    }
  } else {
    TimeScope t2(c, "thermf_cesm_sums");
    if (int rc = st_xcsum_batch(c, (int)planes.size(), planes.data(), masks.data(), c->cesm_rows, c->cesm_sums)) return rc;
  }
  {
    TimeScope t3(c, "thermf_cesm_corr");
    hipLaunchKernelGGL(k_thermf_cesm_corr, plane_grid(h), dim3(256), 0, c->stream, c->d, T, c->cesm_sums, nq);
    c->cesm_launches++;
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
