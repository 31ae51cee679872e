// mod_budget, the reference's conservation monitor (phy/mod_budget.F90): budget_init (:73-93), budget_sums (:95-196) and the sums of
// budget_output (:335-352) on the device, the records of the steps and the lines of salbud tembud tkebud glsbud trcbud trcbudtot
// (:211-331) on the host.  Active with cnsvdi = 1; inside blomgpu_step with the option budget_step = 1 (api.hip: g_budget_opts).
//
// One call of budget_sums inside a step is TWO launches and no host synchronisation:
//   k_budget_rows<NT>   a workgroup per row j.  A thread per point of a round of strips walks k = 1..kk of dp, saln, temp and the tracer
//                       planes in play ONCE (several levels' loads in flight, no LDS inside the k loop), q = dp*scp2 formed once per
//                       level, util_x = util_x + fld*q in the reference's order (:124-143, :165-177).  The column sums go to LDS, not to
//                       HBM planes, and are reduced there exactly as xcsum does (halo.hip: k_xcsum_rows_batch): strips of 2*nbdy+1 points
//                       added serially in i, the strip sums added in order, the seam row of an arctic patch left out (ips).  Rows of any
//                       width: rounds of at most 64 strips, the row sum carried from round to round.  blockIdx.y = 1 (the call that
//                       carries sc, :182-194): the row sums of salt_corr*scp2 in the same launch.
//   k_budget_total      a workgroup per quantity adds its row sums serially (k_xcsum_total_batch's definition) into the step's record
//                       ON THE DEVICE -- call 7 also into call 1 of the next step's record (blomgpu_step of several steps: nothing
//                       between the two writes dp, temp, saln or trc, so the seven numbers are copied, not computed again).
// budget_output's three sums (sf tf trf) take the same two launches: k_budget_rows2d forms the products in the statement's order.
// The records of a blomgpu_step call come back in ONE device-to-host copy in front of the call's last error check.
//
// Tiles of one process and blomgpu_budget_sums / _init / _output called from a host that sequences the stages itself go through the
// reference's own util planes and halo.hip's st_xcsum_batch (global order, the single tile's bits on every tile); over RCCL ranks
// budget_step = 1 is refused at the first step.
#include "blomgpu_internal.h"
#include <algorithm>
#include <cstring>

#define BUD_W (2 * NBDY + 1)
constexpr int BUD_NQ = 5;                      // sdp tdp trdp tkedp glsdp
constexpr int BUD_REC = 7 * BUD_NQ + 4;        // [(ncall-1)*5 + q], then sc, sf, tf, trf
constexpr int BUD_SC = 7 * BUD_NQ, BUD_SF = BUD_SC + 1;
constexpr int BUD_KU = 4;                      // levels whose loads are in flight
constexpr int BUD_KEEP = 64;                   // records kept for a host that sequences the stages itself

struct BudgetState {
  double *dev = nullptr;       // the records of the running call, BUD_REC doubles a step
  int cap = 0;                 // ... as many records
  double *rows = nullptr;      // row sums: (BUD_NQ + 1) * jtdm doubles
  int slot = 0, nslots = 0;    // the record of the running step, the records of the running call
  std::vector<double> stage;   // where the one copy of a call lands
  int first = 0;               // recs holds the steps first, first + 1, ...
  std::vector<double> recs;
  double mass0 = 0.;
  bool have_mass0 = false;
};

static int bud_state(blomgpu_ctx *c, int nrec) {
  if (!c->bud) c->bud = new BudgetState();
  BudgetState &B = *c->bud;
  if (nrec > B.cap) {
    if (B.dev) (void)hipFree(B.dev);
    B.dev = nullptr; B.cap = 0;
    HIPCHK(c, hipMalloc((void **)&B.dev, sizeof(double) * BUD_REC * (size_t)nrec));
    B.cap = nrec;
  }
  if (!B.rows) HIPCHK(c, hipMalloc((void **)&B.rows, sizeof(double) * (BUD_NQ + 1) * (size_t)c->h.jtdm));
  return 0;
}
void budget_free(blomgpu_ctx *c) {
  if (!c->bud) return;
  if (c->bud->dev) (void)hipFree(c->bud->dev);
  if (c->bud->rows) (void)hipFree(c->bud->rows);
  delete c->bud;
  c->bud = nullptr;
}
// the host's record of a step; create: the steps are kept while they follow each other
static double *bud_host_rec(BudgetState &B, int step, bool create) {
  const int n = (int)(B.recs.size() / BUD_REC);
  if (n && step >= B.first && step < B.first + n) return B.recs.data() + (size_t)(step - B.first) * BUD_REC;
  if (!create) return nullptr;
  if (!n || step != B.first + n) { B.recs.clear(); B.first = step; }
  else if (n >= BUD_KEEP) { B.recs.erase(B.recs.begin(), B.recs.begin() + BUD_REC); B.first++; }
  B.recs.resize(B.recs.size() + BUD_REC, 0.);
  return B.recs.data() + B.recs.size() - BUD_REC;
}
// which tracer planes a call reads: 0 none, 1 tracer 1 (use_TRC), 2 + the TKE tracer, 3 + the GLS tracer
static int bud_ntq(blomgpu_ctx *c, int *nt) {
  const DevView &h = c->h;
  *nt = h.ntr < 1 ? 0 : h.P.itrtke < 1 ? 1 : !(h.P.gls && h.P.itrgls >= 1) ? 2 : 3;
  if (*nt >= 2 && h.P.itrtke > h.ntr) return ctx_fail(c, "budget_sums: itrtke is larger than the number of tracers");
  if (*nt >= 3 && h.P.itrgls > h.ntr) return ctx_fail(c, "budget_sums: itrgls is larger than the number of tracers");
  return 0;
}
static inline int bud_sc_call(const blomgpu_ctx *c) { return c->h.P.vcoord_tag == 1 ? 5 : 4; }      // :182-183

// ---- the row reduction: NQ quantities of row j, their values at a point produced by load(c, v) ---------------------------------------
// LDS: col[NQ][npts] | strip[NQ][64] | mk[npts] with npts = chs * BUD_W points a round (chs <= 64 strips; blockDim.x >= npts)
template <int NQ, class F>
__device__ __forceinline__ void bud_row(const DevView &V, int j, int chs, double *lds, double *__restrict__ rowsum, F &&load) {
  const int ii = V.ii, npts = chs * BUD_W, t = (int)threadIdx.x;
  double *col = lds, *strip = lds + (size_t)NQ * npts;
  int *mk = (int *)(strip + NQ * 64);
  const int nstrip = (ii + BUD_W - 1) / BUD_W;
  double sum8 = 0.;
  for (int s0 = 0; s0 < nstrip; s0 += chs) {
    if (t < npts) {
      const int i = 1 + s0 * BUD_W + t;
      int on = 0;
      if (i <= ii) {
        const size_t c = IDX(V, i, j);
        if (V.m[I_ip][c] == 1) {
          on = 1;
          double v[NQ];
          load(c, v);
#pragma unroll
          for (int q = 0; q < NQ; q++) col[q * npts + t] = v[q];
        }
      }
      mk[t] = on;
    }
    __syncthreads();
    if (t < NQ * chs) {
      const int q = t / chs, s = t - q * chs;
      double sum8p = 0.;
      for (int p = 0; p < BUD_W; p++) {
        const int x = s * BUD_W + p;
        if (mk[x]) sum8p = sum8p + col[q * npts + x];
      }
      strip[q * 64 + s] = sum8p;
    }
    __syncthreads();
    if (t < NQ) {
      const int n = nstrip - s0 < chs ? nstrip - s0 : chs;
      for (int s = 0; s < n; s++) sum8 = sum8 + strip[t * 64 + s];
    }
    __syncthreads();
  }
  if (t < NQ) rowsum[(size_t)t * V.jj + j - 1] = sum8;
}
static size_t bud_lds_bytes(int nq, int chs) { return sizeof(double) * (size_t)nq * (chs * BUD_W + 64) + sizeof(int) * (size_t)chs * BUD_W; }
static void bud_geometry(const DevView &h, int *chs, int *nthr) {
  const int nstrip = (h.ii + BUD_W - 1) / BUD_W;
  *chs = nstrip < 64 ? nstrip : 64;
  *nthr = (*chs * BUD_W + 63) / 64 * 64;
}

template <int NT>
__global__ __launch_bounds__(576) void k_budget_rows(const DevView *__restrict__ Vp, int nn, int chs, double *__restrict__ rowsum) {
  const DevView &V = *Vp;
  HIP_DYNAMIC_SHARED(double, lds)
  constexpr int NQ = 2 + NT;
  const int j = blockIdx.x + 1, jj = V.jj, kk = V.kk;
  if (V.nreg == 2 && j >= jj) {                                   // ips: the seam row adds nothing (every strip sum of it is 0.)
    if (threadIdx.x == 0) {
      if (blockIdx.y == 0)
        for (int q = 0; q < NQ; q++) rowsum[(size_t)q * jj + j - 1] = 0.;
      else rowsum[(size_t)NQ * jj + j - 1] = 0.;
    }
    return;
  }
  if (blockIdx.y == 1) {                                          // :188
    bud_row<1>(V, j, chs, lds, rowsum + (size_t)NQ * jj, [&](size_t c, double *v) { v[0] = V.f[F_salt_corr][c] * V.f[F_scp2][c]; });
    return;
  }
  const size_t np = V.nplane;
  bud_row<NQ>(V, j, chs, lds, rowsum, [&](size_t c, double *s) {
    const double scp2 = V.f[F_scp2][c];
    const size_t o0 = c + (size_t)nn * np;
    gcd_t dp = V.f[F_dp] + o0, sa = V.f[F_saln] + o0, te = V.f[F_temp] + o0;
    gcd_t t1 = V.f[F_trc] + o0, tk = t1, gl = t1;
    if constexpr (NT >= 2) tk = V.f[F_trc] + o0 + (size_t)(V.P.itrtke - 1) * 2 * kk * np;
    if constexpr (NT >= 3) gl = V.f[F_trc] + o0 + (size_t)(V.P.itrgls - 1) * 2 * kk * np;
#pragma unroll
    for (int q = 0; q < NQ; q++) s[q] = 0.;
    for (int k0 = 0; k0 < kk; k0 += BUD_KU) {
      double d[BUD_KU], a[NQ][BUD_KU];
#pragma unroll
      for (int u = 0; u < BUD_KU; u++) {
        const size_t o = (size_t)(k0 + u < kk ? k0 + u : kk - 1) * np;
        d[u] = dp[o];
        a[0][u] = sa[o];
        a[1][u] = te[o];
        if constexpr (NT >= 1) a[2][u] = t1[o];
        if constexpr (NT >= 2) a[3][u] = tk[o];
        if constexpr (NT >= 3) a[4][u] = gl[o];
      }
#pragma unroll
      for (int u = 0; u < BUD_KU; u++) {
        if (k0 + u >= kk) break;
        const double q = d[u] * scp2;                             // :130
#pragma unroll
        for (int x = 0; x < NQ; x++) s[x] = s[x] + a[x][u] * q;   // :131-136, :172
      }
    }
  });
}

// budget_output's products (:339-342), one per blockIdx.y, in the statement's order: (a + b)*scp2*delt1
__global__ __launch_bounds__(576) void k_budget_rows2d(const DevView *__restrict__ Vp, int chs, double *__restrict__ rowsum) {
  const DevView &V = *Vp;
  HIP_DYNAMIC_SHARED(double, lds)
  const int j = blockIdx.x + 1, jj = V.jj, w = blockIdx.y;
  double *__restrict__ out = rowsum + (size_t)w * jj;
  if (V.nreg == 2 && j >= jj) {
    if (threadIdx.x == 0) out[j - 1] = 0.;
    return;
  }
  const double delt1 = V.P.delt1;
  if (w == 0) bud_row<1>(V, j, chs, lds, out, [&](size_t c, double *v) { v[0] = (V.f[F_salflx][c] + V.f[F_salrlx][c]) * V.f[F_scp2][c] * delt1; });
  else if (w == 1) bud_row<1>(V, j, chs, lds, out, [&](size_t c, double *v) { v[0] = (V.f[F_surflx][c] + V.f[F_surrlx][c]) * V.f[F_scp2][c] * delt1; });
  else bud_row<1>(V, j, chs, lds, out, [&](size_t c, double *v) { v[0] = V.f[F_trflx][c] * V.f[F_scp2][c] * delt1; });
}

// the row sums of quantity blockIdx.x added serially (halo.hip: k_xcsum_total_batch), into rec[pos] and, where next >= 0, rec2[next]
struct BudDst { int pos[BUD_NQ + 1], next[BUD_NQ + 1]; };
__global__ __launch_bounds__(256) void k_budget_total(const double *__restrict__ rowsum, int jj, BudDst D, double *__restrict__ rec, double *__restrict__ rec2) {
  HIP_DYNAMIC_SHARED(double, rs)
  const int q = blockIdx.x;
  const double *__restrict__ mine = rowsum + (size_t)q * jj;
  for (int j = threadIdx.x; j < jj; j += blockDim.x) rs[j] = mine[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = rs[0];
    for (int j = 1; j < jj; j++) s = s + rs[j];
    rec[D.pos[q]] = s;
    if (rec2 && D.next[q] >= 0) rec2[D.next[q]] = s;
  }
}

// ---- the reference's own form: the column sums and the products in the util planes (:107-143, :155-177, :184-192, :82-90, :335-347) -----
// which: 0 S, T (and the TKE, GLS tracers) -> util1, util2 (util3, util4); 1 tracer 1 -> util1; 2 salt_corr*scp2 -> util1;
// 3 pb(:,:,1)*scp2 -> util1; 4 budget_output's products -> util1, util2 (util3)
__global__ void k_budget_planes(const DevView *__restrict__ Vp, int nn, int which) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii || !V.m[I_ip][c]) return;
  const size_t np = V.nplane;
  const double scp2 = V.f[F_scp2][c];
  if (which == 2) { V.f[F_util1][c] = V.f[F_salt_corr][c] * scp2; return; }
  if (which == 3) { V.f[F_util1][c] = V.f[F_pb][c] * scp2; return; }
  if (which == 4) {
    const double delt1 = V.P.delt1;
    V.f[F_util1][c] = (V.f[F_salflx][c] + V.f[F_salrlx][c]) * scp2 * delt1;
    V.f[F_util2][c] = (V.f[F_surflx][c] + V.f[F_surrlx][c]) * scp2 * delt1;
    if (V.ntr >= 1) V.f[F_util3][c] = V.f[F_trflx][c] * scp2 * delt1;
    return;
  }
  double s1 = 0., s2 = 0., s3 = 0., s4 = 0.;
  const bool tke = which == 0 && V.ntr >= 1 && V.P.itrtke >= 1, gls = tke && V.P.gls && V.P.itrgls >= 1;
  for (int k = 0; k < V.kk; k++) {
    const size_t o = c + (size_t)(k + nn) * np;
    const double q = V.f[F_dp][o] * scp2;
    if (which == 0) {
      s1 = s1 + V.f[F_saln][o] * q;
      s2 = s2 + V.f[F_temp][o] * q;
      if (tke) s3 = s3 + V.f[F_trc][o + (size_t)(V.P.itrtke - 1) * 2 * V.kk * np] * q;
      if (gls) s4 = s4 + V.f[F_trc][o + (size_t)(V.P.itrgls - 1) * 2 * V.kk * np] * q;
    } else {
      s1 = s1 + V.f[F_trc][o] * q;
    }
  }
  V.f[F_util1][c] = s1;
  if (which == 0) V.f[F_util2][c] = s2;
  if (tke) V.f[F_util3][c] = s3;
  if (gls) V.f[F_util4][c] = s4;
}
static int bud_plane_sum(blomgpu_ctx *c, int fid, double *out) {
  const double *pl[1] = {c->h.f[fid]};
  const int *mk[1] = {nullptr};
  const long long keep = c->cesm_launches;         // (st_xcsum_batch counts its launches for the coupled experiment's thermf: not these)
  const int rc = st_xcsum_batch(c, 1, pl, mk, c->bud->rows, out);
  c->cesm_launches = keep;
  return rc;
}
// k_budget_total holds a quantity's row sums in LDS, as k_xcsum_total_batch does
static int bud_rows_fit(blomgpu_ctx *c, const char *who) {
  if (sizeof(double) * (size_t)c->h.jj > 64 * 1024) return ctx_fail(c, std::string(who) + ": more than 8192 rows do not fit the total kernel's LDS");
  return 0;
}
// one call of budget_sums through the planes, its numbers into rec (device)
static int bud_sums_planes(blomgpu_ctx *c, int ncall, int off, double *rec) {
  const DevView &h = c->h;
  int nt = 0;
  if (int rc = bud_ntq(c, &nt)) return rc;
  double *r = rec + (ncall - 1) * BUD_NQ;
  hipLaunchKernelGGL(k_budget_planes, plane_grid(h, 1, 64), dim3(64), 0, c->stream, c->d, off, 0);
  if (int rc = bud_plane_sum(c, F_util1, r + 0)) return rc;
  if (int rc = bud_plane_sum(c, F_util2, r + 1)) return rc;
  if (nt >= 2)
    if (int rc = bud_plane_sum(c, F_util3, r + 3)) return rc;
  if (nt >= 3)
    if (int rc = bud_plane_sum(c, F_util4, r + 4)) return rc;
  if (nt >= 1) {
    hipLaunchKernelGGL(k_budget_planes, plane_grid(h, 1, 64), dim3(64), 0, c->stream, c->d, off, 1);
    if (int rc = bud_plane_sum(c, F_util1, r + 2)) return rc;
  }
  if (ncall == bud_sc_call(c)) {
    hipLaunchKernelGGL(k_budget_planes, plane_grid(h, 1, 64), dim3(64), 0, c->stream, c->d, off, 2);
    if (int rc = bud_plane_sum(c, F_util1, rec + BUD_SC)) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return 0;
}
static int bud_output_planes(blomgpu_ctx *c, double *rec) {
  const DevView &h = c->h;
  hipLaunchKernelGGL(k_budget_planes, plane_grid(h, 1, 64), dim3(64), 0, c->stream, c->d, 0, 4);
  if (int rc = bud_plane_sum(c, F_util1, rec + BUD_SF)) return rc;
  if (int rc = bud_plane_sum(c, F_util2, rec + BUD_SF + 1)) return rc;
  if (h.ntr >= 1)
    if (int rc = bud_plane_sum(c, F_util3, rec + BUD_SF + 2)) return rc;
  HIPCHK(c, hipGetLastError());
  return 0;
}

// ---- inside blomgpu_step -------------------------------------------------------------------------------------------------------------
// in front of the first step of a call: the records of the call on the device, zeroed; of the host's records the one of the step before stays
int budget_call_begin(blomgpu_ctx *c, int ns, int nsteps) {
  if (c->bud) c->bud->nslots = 0;                  // (a call that failed behind this point has left its count)
  if (!budget_on(c) || nsteps < 1) return 0;
  if (c->tiling.rccl) return ctx_fail(c, "blomgpu_step: budget_step = 1 is not built for RCCL ranks (the sums need the global context of every plane): set budget_step = 0");
  if (int rc = bud_state(c, nsteps)) return rc;
  BudgetState &B = *c->bud;
  HIPCHK(c, hipMemsetAsync(B.dev, 0, sizeof(double) * BUD_REC * (size_t)nsteps, c->stream));
  B.nslots = nsteps;
  B.slot = 0;
  if (const double *last = bud_host_rec(B, ns, false)) {
    std::vector<double> keep(last, last + BUD_REC);
    B.recs.swap(keep);
    B.first = ns;
  } else B.recs.clear();
  return 0;
}
void budget_call_slot(blomgpu_ctx *c, int it) {
  if (c->bud) c->bud->slot = it;
}
int st_budget_instep(blomgpu_ctx *c, int ncall, int off) {
  if (!budget_on(c)) return 0;                                                   // :105
  BudgetState &B = *c->bud;
  if (ncall == 1 && B.slot > 0) return 0;                                        // the call 7 before it has written these numbers
  const DevView &h = c->h;
  double *rec = B.dev + (size_t)B.slot * BUD_REC;
  double *next = ncall == 7 && B.slot + 1 < B.nslots ? rec + BUD_REC : nullptr;
  TimeScope ts(c, "budget");
  if (c->tiling.multi()) {
    if (int rc = bud_sums_planes(c, ncall, off, rec)) return rc;
    if (next) HIPCHK(c, hipMemcpyAsync(next, rec + 6 * BUD_NQ, sizeof(double) * BUD_NQ, hipMemcpyDeviceToDevice, c->stream));
    return 0;
  }
  if (h.itdm != h.ii || h.jtdm != h.jj) return ctx_fail(c, "budget_sums: this context is one tile of a larger domain but no transport is attached");
  int nt = 0, chs = 0, nthr = 0;
  if (int rc = bud_ntq(c, &nt)) return rc;
  if (int rc = bud_rows_fit(c, "budget_sums")) return rc;
  bud_geometry(h, &chs, &nthr);
  const int nq = 2 + nt, sc = ncall == bud_sc_call(c) ? 1 : 0;
  const dim3 grid(h.jj, 1 + sc);
  const size_t lds = bud_lds_bytes(nq, chs);
  switch (nt) {
    case 0: hipLaunchKernelGGL(k_budget_rows<0>, grid, dim3(nthr), lds, c->stream, c->d, off, chs, B.rows); break;
    case 1: hipLaunchKernelGGL(k_budget_rows<1>, grid, dim3(nthr), lds, c->stream, c->d, off, chs, B.rows); break;
    case 2: hipLaunchKernelGGL(k_budget_rows<2>, grid, dim3(nthr), lds, c->stream, c->d, off, chs, B.rows); break;
    default: hipLaunchKernelGGL(k_budget_rows<3>, grid, dim3(nthr), lds, c->stream, c->d, off, chs, B.rows); break;
  }
  BudDst D;
  static const int qpos[4][BUD_NQ] = {{0, 1, -1, -1, -1}, {0, 1, 2, -1, -1}, {0, 1, 2, 3, -1}, {0, 1, 2, 3, 4}};
  for (int q = 0; q <= BUD_NQ; q++) D.pos[q] = D.next[q] = -1;
  for (int q = 0; q < nq; q++) { D.pos[q] = (ncall - 1) * BUD_NQ + qpos[nt][q]; D.next[q] = qpos[nt][q]; }
  if (sc) D.pos[nq] = BUD_SC;
  hipLaunchKernelGGL(k_budget_total, dim3(nq + sc), dim3(256), sizeof(double) * (size_t)h.jj, c->stream, B.rows, h.jj, D, rec, next);
  HIPCHK(c, hipGetLastError());
  return 0;
}
int st_budget_output_instep(blomgpu_ctx *c) {
  if (!budget_on(c)) return 0;                                                   // :207
  BudgetState &B = *c->bud;
  const DevView &h = c->h;
  double *rec = B.dev + (size_t)B.slot * BUD_REC;
  TimeScope ts(c, "budget_output");
  if (c->tiling.multi()) return bud_output_planes(c, rec);
  if (h.itdm != h.ii || h.jtdm != h.jj) return ctx_fail(c, "budget_output: this context is one tile of a larger domain but no transport is attached");
  int chs = 0, nthr = 0;
  if (int rc = bud_rows_fit(c, "budget_output")) return rc;
  bud_geometry(h, &chs, &nthr);
  const int nq = h.ntr >= 1 ? 3 : 2;
  hipLaunchKernelGGL(k_budget_rows2d, dim3(h.jj, nq), dim3(nthr), bud_lds_bytes(1, chs), c->stream, c->d, chs, B.rows);
  BudDst D;
  for (int q = 0; q <= BUD_NQ; q++) { D.pos[q] = q < nq ? BUD_SF + q : -1; D.next[q] = -1; }
  hipLaunchKernelGGL(k_budget_total, dim3(nq), dim3(256), sizeof(double) * (size_t)h.jj, c->stream, B.rows, h.jj, D, rec, (double *)nullptr);
  HIPCHK(c, hipGetLastError());
  return 0;
}
// a record's sums where budget_get finds them: calls 1..5 under the step's level n, calls 6 and 7 under its level m
static void bud_file_ctx(blomgpu_ctx *c, int step, const double *rec, int call0, int call1) {
  const int m = (step - 1) % 2 + 1, n = step % 2 + 1;
  for (int k = call0; k <= call1; k++)
    for (int q = 0; q < BUD_NQ; q++) c->budget[q][k - 1][(k <= 5 ? n : m) - 1] = rec[(k - 1) * BUD_NQ + q];
}
// the one copy of a call, in front of its last read-back of the error words ...
int budget_call_fetch(blomgpu_ctx *c) {
  if (!budget_on(c) || !c->bud || !c->bud->nslots) return 0;
  BudgetState &B = *c->bud;
  B.stage.resize((size_t)B.nslots * BUD_REC);
  HIPCHK(c, hipMemcpyAsync(B.stage.data(), B.dev, sizeof(double) * B.stage.size(), hipMemcpyDeviceToHost, c->stream));
  return 0;
}
// ... and behind it: steps ns + 1 .. ns + nslots
int budget_call_commit(blomgpu_ctx *c, int ns) {
  if (!budget_on(c) || !c->bud || !c->bud->nslots) return 0;
  BudgetState &B = *c->bud;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int s = 0; s < B.nslots; s++) {
    const double *src = B.stage.data() + (size_t)s * BUD_REC;
    memcpy(bud_host_rec(B, ns + 1 + s, true), src, sizeof(double) * BUD_REC);
    bud_file_ctx(c, ns + 1 + s, src, 1, 7);
  }
  B.nslots = 0;
  return 0;
}

// ---- a host that sequences the stages itself: the reference's util planes, the sums filed under the step c->h.P.nstep ---------------------
int st_budget_sums(blomgpu_ctx *c, int ncall, int n, int off) {
  if (!c->cnsvdi) return 0;                                                      // :105
  if (ncall < 1 || ncall > 7 || n < 1 || n > 2) return ctx_fail(c, "budget_sums: ncall in 1..7, n in 1..2");
  if (c->tiling.rccl) return ctx_fail(c, "budget_sums: not built for RCCL ranks");
  if (int rc = bud_state(c, 2)) return rc;
  BudgetState &B = *c->bud;
  if (int rc = bud_sums_planes(c, ncall, off, B.dev)) return rc;
  double got[BUD_NQ + 1] = {};
  HIPCHK(c, hipMemcpyAsync(got, B.dev + (ncall - 1) * BUD_NQ, sizeof(double) * BUD_NQ, hipMemcpyDeviceToHost, c->stream));
  const bool sc = ncall == bud_sc_call(c);
  if (sc) HIPCHK(c, hipMemcpyAsync(got + BUD_NQ, B.dev + BUD_SC, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int nt = 0;
  if (int rc = bud_ntq(c, &nt)) return rc;
  double *rec = bud_host_rec(B, c->h.P.nstep, true);
  for (int q = 0; q < BUD_NQ; q++) {
    if (q >= 2 && q - 1 > nt) continue;                                          // (a quantity the tracer set does not have stays as it is)
    c->budget[q][ncall - 1][n - 1] = rec[(ncall - 1) * BUD_NQ + q] = got[q];
  }
  if (sc) rec[BUD_SC] = got[BUD_NQ];
  return 0;
}
int st_budget_init(blomgpu_ctx *c) {
  if (!c->cnsvdi) return 0;                                                      // :80
  if (c->tiling.rccl) return ctx_fail(c, "budget_init: not built for RCCL ranks");
  if (int rc = bud_state(c, 2)) return rc;
  BudgetState &B = *c->bud;
  hipLaunchKernelGGL(k_budget_planes, plane_grid(c->h, 1, 64), dim3(64), 0, c->stream, c->d, 0, 3);
  if (int rc = bud_plane_sum(c, F_util1, B.dev)) return rc;
  HIPCHK(c, hipMemcpyAsync(&B.mass0, B.dev, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  B.have_mass0 = true;
  return 0;
}
int st_budget_output(blomgpu_ctx *c, int m) {
  (void)m;                                                                       // (the line of the step is blomgpu_budget_line's)
  if (!c->cnsvdi) return 0;                                                      // :207
  if (c->tiling.rccl) return ctx_fail(c, "budget_output: not built for RCCL ranks");
  if (int rc = bud_state(c, 2)) return rc;
  BudgetState &B = *c->bud;
  if (int rc = bud_output_planes(c, B.dev)) return rc;
  double got[3] = {0., 0., 0.};
  HIPCHK(c, hipMemcpyAsync(got, B.dev + BUD_SF, sizeof(double) * (c->h.ntr >= 1 ? 3 : 2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double *rec = bud_host_rec(B, c->h.P.nstep, true);
  for (int q = 0; q < 3; q++) rec[BUD_SF + q] = got[q];
  return 0;
}

// ---- records and lines -----------------------------------------------------------------------------------------------------------------
int budget_steps(blomgpu_ctx *c, int *first, int *count) {
  *first = c->bud ? c->bud->first : 0;
  *count = c->bud ? (int)(c->bud->recs.size() / BUD_REC) : 0;
  return 0;
}
int budget_mass0(blomgpu_ctx *c, double *mass0) {
  if (!c->bud || !c->bud->have_mass0) return ctx_fail(c, "blomgpu_budget_mass0: budget_init has not run (with cnsvdi = 1)");
  *mass0 = c->bud->mass0;
  return 0;
}
int budget_record(blomgpu_ctx *c, int nstep, double *rec) {
  const double *r = c->bud ? bud_host_rec(*c->bud, nstep, false) : nullptr;
  if (!r) return ctx_fail(c, "blomgpu_budget_record: no record of step " + std::to_string(nstep));
  memcpy(rec, r, sizeof(double) * BUD_REC);
  return 0;
}
// which of the six files the tracer set calls for (:231-268): bit 0 salbud, 1 tembud, 2 tkebud, 3 glsbud, 4 trcbud, 5 trcbudtot
int budget_files(blomgpu_ctx *c, int *mask) {
  int nt = 0;
  if (int rc = bud_ntq(c, &nt)) return rc;
  *mask = 3 | (nt >= 2 ? 4 : 0) | (nt >= 3 ? 8 : 0) | (nt >= 1 ? 48 : 0);
  return 0;
}
// the terms of one line of budget_output (:211-331) in the reference's order; file: 0 salbud 1 tembud 2 tkebud 3 glsbud 4 trcbud 5 trcbudtot
int budget_line(blomgpu_ctx *c, int nstep, int file, double *terms, int *nterms) {
  static const char *const names[6] = {"salbud", "tembud", "tkebud", "glsbud", "trcbud", "trcbudtot"};
  if (file < 0 || file > 5) return ctx_fail(c, "blomgpu_budget_line: file is 0 salbud, 1 tembud, 2 tkebud, 3 glsbud, 4 trcbud or 5 trcbudtot");
  int mask = 0;
  if (int rc = budget_files(c, &mask)) return rc;
  if (!(mask >> file & 1)) return ctx_fail(c, std::string("blomgpu_budget_line: the tracer set does not call for ") + names[file]);
  const double *a = c->bud ? bud_host_rec(*c->bud, nstep - 1, false) : nullptr, *b = c->bud ? bud_host_rec(*c->bud, nstep, false) : nullptr;
  if (!b) return ctx_fail(c, "blomgpu_budget_line: no record of step " + std::to_string(nstep));
  if (!a) return ctx_fail(c, "blomgpu_budget_line: step " + std::to_string(nstep) + " has no line: no record of step " + std::to_string(nstep - 1));
  if (!c->bud->have_mass0) return ctx_fail(c, "blomgpu_budget_line: budget_init has not run");
  const double mass0 = c->bud->mass0, grav = GRAV, spcifh = SPCIFH;
  static const int qof[6] = {0, 1, 3, 4, 2, 2};
  const int q = qof[file];
  double x[8];
  for (int k = 1; k <= 5; k++) x[k] = a[(k - 1) * BUD_NQ + q];
  for (int k = 6; k <= 7; k++) x[k] = b[(k - 1) * BUD_NQ + q];
  if (file == 5) {
    for (int k = 1; k <= 7; k++) terms[k - 1] = x[k] / mass0;
    *nterms = 7;
    return 0;
  }
  const double sc = a[BUD_SC], sf = a[BUD_SF], tf = a[BUD_SF + 1], trf = a[BUD_SF + 2];
  const int forced = c->h.P.vcoord_tag == 1 ? 4 : 3;              // the difference that carries the surface flux
  for (int d = 1; d <= 6; d++) {
    if (d != forced || file == 2 || file == 3) terms[d - 1] = (x[d + 1] - x[d]) / mass0;
    else if (file == 0) terms[d - 1] = (x[d + 1] - x[d] + (sf - sc) * grav) / mass0;
    else if (file == 1) terms[d - 1] = (x[d + 1] - x[d] + tf * grav / spcifh) / mass0;
    else terms[d - 1] = (x[d + 1] - x[d] + trf * grav) / mass0;
  }
  *nterms = 6;
  return 0;
}
