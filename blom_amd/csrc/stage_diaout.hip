// What diaout_iogrp (phy/mod_dia.F90:2330) forms from the accumulators before it writes them, on the device: diamer (:4004-4629) -- the
// overturning stream functions in density and in depth space and the meridional heat and salt transports, per latitude section and
// region --, diasec (:3814-4001) -- mass, heat and salt transport through named sections --, and the global sums and means
// (:2427-2588).  An output-time stage: blomgpu_dia_reduce runs it between the last step of a window and blomgpu_dia_finalize, it only
// reads accumulators, and nothing inside blomgpu_step knows of it.
//
// The 23 "msc" names have no accumulator: blomgpu_dia_select takes them and selects their sources (diaini :557, :559, :598-670).  The
// tables the reference reads from files (mer_orfile, mer_mifile :4026-4108; sec_sifile :3838-3866) are the caller's
// (blomgpu_dia_set_mertra, blomgpu_dia_set_sections; blom_amd/diasections.py reads the two text formats).
//
// The bits.  r is formed on the host in the reference's order: (.5*spcifh | .5*g2kg | .5) / ((grav*baclin)*real(nacc)).  Per section
// entry a running sum down the levels -- transports (:4188-4212) a(1)*r, + a(k)*r; density space (:4340-4371) the exclusive sum 0.,
// + r*a(k-1); depth space (:4492-4559) 0. | r*(a1 + .5*a2) | + r*(.5*a(ddm-1) + a(ddm)) | + (.5*r)*(a(k-1) + a(k)) in that branch order;
// diasec (:3903-3953) as the transports plus the ucum350 pair -- at the wet u | v points, 0. elsewhere.  Then per (section, level) a
// SERIAL sum over the entries in the table's order, one accumulator per ocean region o = oflg(i,j):
//   mflx_or(l,o) = (mflx_or(l,o) + real(uflg)*ucum) + real(vflg)*vcum     (:4227, :4384, :4572; tr(s) of :3970, :3976 likewise)
// and the sums over the ocean regions of a meridional region with the fill rules (:4235-4256, :4391-4408, :4578-4596).
//
// k_diaout_sections<kind>: one workgroup per (section, source pair), one launch per kind of name.  A PASS takes up to `ep` entries of the section, one per lane (a zonal
// section is contiguous in i: the 8-byte gathers of a level coalesce).  Inside a pass the levels go by in CHUNKS of `lc`: phase A, each
// lane advances its entry's running ucum / vcum (registers) over the chunk and stages the two addends of every level in LDS as
// [level in chunk][entry]; phase B, thread (level in chunk, ocean region) walks the pass's entries serially in LDS and carries its sum
// in an LDS array [level][ocean region] that lives across chunks and passes.  After the last pass thread (level, meridional region)
// forms the region sums and the fill rules and stores them.  A serial chain per (section, level, region), parallel over levels,
// regions, sections and source pairs: the reference's order without double atomics, which would not give it.  Nothing crosses HBM but
// the gathers and the results; all LDS is dynamic, the base 16-byte aligned and every carve a multiple of 16.
// Algorithmic bytes of a launch: 16 per entry and source level, 16 per entry for its table row.
#include "../../include/blomgpu.h"
#include "blomgpu_internal.h"
#include <cmath>
#include <cstring>

namespace {
constexpr double NF90_FILL_DOUBLE = 9.9692099683868690e+36;
enum { K_TR = 0, K_DENS = 1, K_DEPTH = 2, K_SEC = 3, K_GLB = 4 };   // what a name is: a transport, a stream function in density | depth space, a section transport, a global number
enum { R_MASS = 0, R_HEAT = 1, R_SALT = 2 };                      // the factor: .5 | .5*spcifh | .5*g2kg over (grav*baclin)*nacc
struct MscRow { const char *name; int kind, fac; const char *usrc, *vsrc; int line; };
// the order of the reference's allocate (:4113-4119), then diasec's three, then the global names in the order of :2427-2588's results
const MscRow g_msc[] = {
  {"mmflxl", K_DENS, R_MASS, "umfll", "vmfll", 4324}, {"mmftdl", K_DENS, R_MASS, "umfltdl", "vmfltdl", 4328},
  {"mmfsml", K_DENS, R_MASS, "umflsml", "vmflsml", 4332},
  {"mmflxd", K_DEPTH, R_MASS, "uflxlvl", "vflxlvl", 4476}, {"mmftdd", K_DEPTH, R_MASS, "umfltdlvl", "vmfltdlvl", 4480},
  {"mmfsmd", K_DEPTH, R_MASS, "umflsmlvl", "vmflsmlvl", 4484},
  {"mhflx", K_TR, R_HEAT, "utflx", "vtflx", 4144}, {"mhftd", K_TR, R_HEAT, "utfltd", "vtfltd", 4149},
  {"mhfsm", K_TR, R_HEAT, "utflsm", "vtflsm", 4154}, {"mhfld", K_TR, R_HEAT, "utflld", "vtflld", 4159},
  {"msflx", K_TR, R_SALT, "usflx", "vsflx", 4164}, {"msftd", K_TR, R_SALT, "usfltd", "vsfltd", 4169},
  {"msfsm", K_TR, R_SALT, "usflsm", "vsflsm", 4174}, {"msfld", K_TR, R_SALT, "usflld", "vsflld", 4179},
  {"masstr", K_SEC, R_MASS, "uflxlvl", "vflxlvl", 3884}, {"heattr", K_SEC, R_HEAT, "utflxlvl", "vtflxlvl", 3889},
  {"salttr", K_SEC, R_SALT, "usflxlvl", "vsflxlvl", 3894},
  {"massgs", K_GLB, 0, "dp", nullptr, 2458}, {"salnga", K_GLB, 0, "dp", "saln", 2524}, {"tempga", K_GLB, 0, "dp", "temp", 2557},
  {"volgs", K_GLB, 0, "dz", nullptr, 2491}, {"sssga", K_GLB, 0, "sss", nullptr, 2573}, {"sstga", K_GLB, 0, "sst", nullptr, 2586},
};
constexpr int NMSC = (int)(sizeof(g_msc) / sizeof(g_msc[0]));
static_assert(NMSC == 23, "the 23 msc names");
enum { M_MASSGS = 17, M_SALNGA, M_TEMPGA, M_VOLGS, M_SSSGA, M_SSTGA };
constexpr int KIND_MSC = 5;                       // what blomgpu_dia_name_msc reports for these rows
constexpr int DOUT_MAXREG = 32;                   // ocean regions | meridional regions at most: (levels per chunk) x (ocean regions) threads walk
constexpr int DOUT_NFLG = 20;                     // second extent of mer_regflg (phy/mod_dia.F90: mer_regflg(mer_nreg_max, 20))
constexpr int DOUT_T = 256;                       // lanes of a workgroup
constexpr int DOUT_LC = 8;                        // levels per chunk at most
constexpr int DOUT_MAXJOB = 14;                   // diamer's 14 source pairs (diasec's 3 go in a launch of their own)
struct alignas(16) Int4 { int x, y, z, w; };      // a table row: one 16-byte load
constexpr int DOUT_MAXLEV = 128;                  // kdm <= 120 for the classes, ddm <= 128 (stage_diaacc.hip)

// a set of sections on the device: section s holds the entries start[s] .. start[s+1]-1 of pts = (plane index, uflg, vflg, ocean region)
struct SecTab {
  const int *start, *pts;
  int nsec;
  // diamer's only: the sections' latitudes, the regions
  const double *mtlat, *minlat, *maxlat;
  const int *nflg, *regflg;
  int no, nm;
};
struct OutJob { int nsrc, nout; long long pu, pv, out; double r; };     // pu, pv: first element of the source pair in the accumulators
struct OutJobs {
  int n, ep, lc;               // jobs; entries per pass, levels per chunk
  int k350, equat;             // diasec: the level of :112 | :131, the 1-based section of the upper-350 m sums (-1: none)
  double w350;
  OutJob j[DOUT_MAXJOB];
};
__host__ __device__ inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }
// the carve of the dynamic LDS: su, sv [lc][ep]; sdep [ep]; sum [nout][no]; so [ep]; cnt [no]; deep [nout][no]
struct Carve { size_t su, sv, sdep, sum, so, cnt, deep, bytes; };
__host__ __device__ inline Carve carve_of(int ep, int lc, int nout, int no) {
  Carve C;
  size_t o = 0;
  C.su = o; o += up16(sizeof(double) * lc * ep);
  C.sv = o; o += up16(sizeof(double) * lc * ep);
  C.sdep = o; o += up16(sizeof(double) * ep);
  C.sum = o; o += up16(sizeof(double) * nout * no);
  C.so = o; o += up16(sizeof(int) * ep);
  C.cnt = o; o += up16(sizeof(int) * no);
  C.deep = o; o += up16(sizeof(int) * nout * no);
  C.bytes = o;
  return C;
}

template <int kind>
__global__ __launch_bounds__(DOUT_T) void k_diaout_sections(const DevView *__restrict__ Vp, const double *__restrict__ accp, const double *__restrict__ edgep,
                                                           const SecTab T, const OutJobs J, int lds_nout, int lds_no, double *__restrict__ outp) {
#ifdef BLOM_HOSTEMU
  char *smem = (char *)hostemu::dyn_lds();
#else
  extern __shared__ __attribute__((aligned(16))) char smem[];
#endif
  const DevView &V = *Vp;
  const OutJob &jb = J.j[blockIdx.y];
  const int l = blockIdx.x, tid = threadIdx.x;                    // (kind: what every job of the launch is)
  const int no = T.no, nout = jb.nout, nsrc = jb.nsrc, ep = J.ep, lc = J.lc;
  const Carve C = carve_of(ep, lc, lds_nout, lds_no);
  double *su = (double *)(smem + C.su), *sv = (double *)(smem + C.sv), *sdep = (double *)(smem + C.sdep), *sum = (double *)(smem + C.sum);
  int *so = (int *)(smem + C.so), *cnt = (int *)(smem + C.cnt), *deep = (int *)(smem + C.deep);
  gci_t start = global_ptr(T.start), pts = global_ptr(T.pts);
  gcd_t acc = global_ptr(accp), edge = global_ptr(edgep);
  const int e0 = start[l], nent = start[l + 1] - e0;
  const size_t np = V.nplane;
  const double r = jb.r, hr = .5 * r;                             // (.5*r is formed first, :4547)
  for (int x = tid; x < nout * no; x += DOUT_T) { sum[x] = 0.; deep[x] = 0; }      // mflx_or(l,o) = 0. (:4220, :4378, :4566); tr(s) = 0. (:3965)
  for (int x = tid; x < no; x += DOUT_T) cnt[x] = 0;
  __syncthreads();
  const bool staged = kind == K_DENS || kind == K_DEPTH;          // every level is an output; the others give one number after the last level
  for (int p0 = 0; p0 < nent; p0 += ep) {
    const int npass = nent - p0 < ep ? nent - p0 : ep;
    const bool on = tid < npass;
    int c = 0, uf = 0, vf = 0;
    bool wu = false, wv = false;
    if (on) {
      const Int4 q = ((const Int4 BLOM_GAS *)pts)[e0 + p0 + tid];
      c = q.x; uf = q.y; vf = q.z;
      so[tid] = q.w;
      const int msk = V.m[I_mpack][c];
      wu = (msk >> 1) & 1; wv = (msk >> 2) & 1;
      if (kind == K_DEPTH) sdep[tid] = V.f[F_depths][c];
    }
    gcd_t au_ = acc + (jb.pu + c), av_ = acc + (jb.pv + c);
    const double fu = (double)uf, fv = (double)vf;
    double ucum = 0., vcum = 0., up = 0., vp = 0., u350 = 0., v350 = 0.;      // (:4131-4137, :3869-3877: 0. wherever no wet point writes)
    for (int k0 = 0; k0 < nsrc; k0 += lc) {
      // phase A: the chunk's 2 lc gathers are requested together, then the running sums advance level by level
      double au[DOUT_LC], av[DOUT_LC];
#pragma unroll
      for (int u = 0; u < DOUT_LC; u++) {                        // (no lane predicate: a level behind the table is the last level again, a dry or
        if (u >= lc) break;                                      //  (uniform)
        const size_t o = (size_t)(k0 + u < nsrc ? k0 + u : nsrc - 1) * np;      //  idle lane reads a point it never uses -- all inside the accumulators)
        au[u] = au_[o];
        av[u] = av_[o];
      }
#pragma unroll
      for (int u = 0; u < DOUT_LC; u++) {
        if (u >= lc || k0 + u >= nsrc) break;
        const int k = k0 + u + 1;                                 // the reference's level
        const double a = au[u], b = av[u];
        if (kind == K_DENS) {                                     // :4340-4371
          if (wu) ucum = k == 1 ? 0. : ucum + r * up;
          if (wv) vcum = k == 1 ? 0. : vcum + r * vp;
        } else if (kind == K_DEPTH) {                             // :4492-4559, in the reference's branch order
          if (wu) ucum = k == 1 ? 0. : k == 2 ? r * (up + .5 * a) : k == nsrc ? ucum + r * (.5 * up + a) : ucum + hr * (up + a);
          if (wv) vcum = k == 1 ? 0. : k == 2 ? r * (vp + .5 * b) : k == nsrc ? vcum + r * (.5 * vp + b) : vcum + hr * (vp + b);
        } else {                                                  // :4188-4212 | :3903-3953
          if (wu) ucum = k == 1 ? a * r : ucum + a * r;
          if (wv) vcum = k == 1 ? b * r : vcum + b * r;
          if (kind == K_SEC && k >= 2) {
            if (k == J.k350 - 1) {
              if (wu) u350 = ucum;
              if (wv) v350 = vcum;
            } else if (k == J.k350) {
              if (wu) u350 = u350 + J.w350 * (ucum - u350);
              if (wv) v350 = v350 + J.w350 * (vcum - v350);
            }
          }
        }
        up = a; vp = b;
        if (staged && on) { su[u * ep + tid] = fu * ucum; sv[u * ep + tid] = fv * vcum; }
      }
      const bool last = k0 + lc >= nsrc;
      if (!staged && !last) continue;                             // (uniform)
      if (!staged && on) {
        const bool eq = kind == K_SEC && l + 1 == J.equat;        // :3966-3978
        su[tid] = (eq ? u350 : ucum) * fu; sv[tid] = (eq ? v350 : vcum) * fv;
      }
      __syncthreads();
      // phase B: thread (level in chunk, ocean region) walks the pass's entries in their order
      const int nl = staged ? (nsrc - k0 < lc ? nsrc - k0 : lc) : 1;
      if (tid < nl * no) {
        const int kq = tid / no, o = tid % no + 1, k = staged ? k0 + kq : 0;
        double s = sum[k * no + o - 1];
        int dp = deep[k * no + o - 1], n = 0;
        const double lo = kind == K_DEPTH ? edge[k] : 0.;         // depthslev_bnds(1,k)
        for (int e = 0; e < npass; e++)
          if (so[e] == o) {
            s = (s + su[kq * ep + e]) + sv[kq * ep + e];
            n++;
            if (kind == K_DEPTH && lo < sdep[e]) dp = 1;          // :4454: some entry of the region lies deeper than the level's upper bound
          }
        sum[k * no + o - 1] = s;
        deep[k * no + o - 1] = dp;
        if (kind == K_TR) cnt[o - 1] += n;                        // mcnt_or, :4229
      }
      __syncthreads();
    }
  }
  __syncthreads();
  gd_t out = global_ptr(outp) + jb.out;
  if (kind == K_SEC) {
    if (tid == 0) out[l] = sum[0];
    return;
  }
  // thread (level, meridional region): the sum over the region's ocean regions and the fill rules, into [mer_nreg][nout][lmax]
  const int nm = T.nm, lmax = T.nsec;
  const double lat = global_ptr(T.mtlat)[l];
  gci_t nflg = global_ptr(T.nflg), regflg = global_ptr(T.regflg);
  for (int x = tid; x < nout * nm; x += DOUT_T) {
    const int k = x / nm, m = x % nm;
    const bool all = regflg[m * DOUT_NFLG] == 0;
    const int n = all ? no : nflg[m];
    double s = 0.;
    int count = 0, dp = 0;
    for (int q = 0; q < n; q++) {
      const int o = all ? q + 1 : regflg[m * DOUT_NFLG + q];
      s = s + sum[k * no + o - 1];
      count += cnt[o - 1];
      dp |= deep[k * no + o - 1];
    }
    bool fill = lat < global_ptr(T.minlat)[m] || lat > global_ptr(T.maxlat)[m];
    if (kind == K_DEPTH && !dp) fill = true;                      // kmax(l,m) < k, :4449-4467, :4581
    if (kind == K_TR && count == 0) fill = true;                  // :4254
    out[((size_t)m * nout + k) * lmax + l] = fill ? NF90_FILL_DOUBLE : s;
  }
}

// the global sums' columns (:2429-2457 and its four repeats, :2564-2572, :2577-2585): util1 = a(1), + a(k) for k = 2..kk, then *scp2 at
// the owned wet p-points; 0. elsewhere (xcsum's mask leaves those out).  Up to six sources, a plane of `util` each.
struct ColJobs { int n; long long src[6]; int nlev[6]; };
__global__ __launch_bounds__(256) void k_diaout_columns(const DevView *__restrict__ Vp, const double *__restrict__ accp, const ColJobs J, double *__restrict__ utilp) {
  const DevView &V = *Vp;
  THREAD_IJ_NATURAL(V);
  const bool wet = i >= 1 && i <= V.ii && j >= 1 && j <= V.jj && (V.m[I_mpack][c] & 1);
  gcd_t acc = global_ptr(accp);
  gd_t util = global_ptr(utilp);
  const size_t np = V.nplane;
  const double scp2 = V.f[F_scp2][c];
  for (int q = 0; q < J.n; q++) {
    double s = 0.;
    if (wet) {
      gcd_t a = acc + (J.src[q] + c);
      s = a[0];
      for (int k0 = 1; k0 < J.nlev[q]; k0 += COLUMN_U) {
        double v[COLUMN_U];
#pragma unroll
        for (int u = 0; u < COLUMN_U; u++) v[u] = a[(size_t)(k0 + u < J.nlev[q] ? k0 + u : J.nlev[q] - 1) * np];
#pragma unroll
        for (int u = 0; u < COLUMN_U; u++)
          if (k0 + u < J.nlev[q]) s = s + v[u];
      }
      s = s * scp2;
    }
    util[(size_t)q * np + c] = s;
  }
}

// the six numbers from the sums, in the reference's order and with its dependencies (:2492, :2525, :2558, :2561, :2574, :2587): salnga and
// tempga divide by the UNSCALED massgs, which is scaled only afterwards.  idx[x]: the sum of dp, dz, saln, temp, sss, sst, or -1.
struct GlbJob { int idx[6]; long long out[6]; double rnacc, area; };   // out[x]: where massgs, salnga, tempga, volgs, sssga, sstga go, or -1
__global__ void k_diaout_globals(const double *__restrict__ sums, const GlbJob G, double *__restrict__ outp) {
  if (threadIdx.x || blockIdx.x) return;
  gd_t out = global_ptr(outp);
  double massgs = G.idx[0] >= 0 ? sums[G.idx[0]] : 0.;
  if (G.out[3] >= 0) out[G.out[3]] = G.rnacc * sums[G.idx[1]];
  if (G.out[1] >= 0) out[G.out[1]] = sums[G.idx[2]] / massgs;
  if (G.out[2] >= 0) out[G.out[2]] = sums[G.idx[3]] / massgs;
  if (G.out[0] >= 0) out[G.out[0]] = G.rnacc * massgs / GRAV;
  if (G.out[4] >= 0) out[G.out[4]] = G.rnacc * sums[G.idx[4]] / G.area;
  if (G.out[5] >= 0) out[G.out[5]] = G.rnacc * sums[G.idx[5]] / G.area;
}

// one table on the device: ints then doubles in one allocation
struct DevTab {
  int *ints = nullptr;
  double *dbls = nullptr;
  void release() {
    if (ints) (void)hipFree(ints);
    if (dbls) (void)hipFree(dbls);
    ints = nullptr; dbls = nullptr;
  }
};
}  // namespace

struct DiaOutState {
  // blomgpu_dia_set_mertra
  bool has_mer = false;
  int lmax = 0, no = 0, nm = 0;
  DevTab mer;
  SecTab mer_dev{};
  // blomgpu_dia_set_sections
  bool has_sec = false;
  int sec_num = 0, equat = -1;
  DevTab sec;
  SecTab sec_dev{};
  // blomgpu_dia_reduce: the results [name][...] on the device, where each selected name's lie and their shapes; the global sums' planes
  double *res = nullptr;
  size_t res_cap = 0;
  bool reduced = false;
  long long off[NMSC];
  int dims[NMSC][3];
  double *util = nullptr, *rows = nullptr;     // six planes; 6 jtdm row sums + 6 sums
};

namespace {
DiaOutState *state_of(blomgpu_ctx *c) {
  if (!c->diaout) c->diaout = new DiaOutState;
  return c->diaout;
}
template <class T> int to_device(blomgpu_ctx *c, T **dst, const std::vector<T> &src) {
  HIPCHK(c, hipMalloc((void **)dst, sizeof(T) * (src.size() ? src.size() : 1)));
  if (src.size()) HIPCHK(c, hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
  return 0;
}
// (i, j) 1-based global -> the plane index of a context that holds the whole domain
inline int plane_index(const DevView &h, int i, int j) { return (i + NBDY - 1) + h.ni * (j + NBDY - 1); }
bool whole_domain(const blomgpu_ctx *c) { return !c->tiling.multi() && c->h.itdm == c->h.ii && c->h.jtdm == c->h.jj; }
}  // namespace

int diaout_msc_index(const char *name) {
  for (int r = 0; r < NMSC; r++)
    if (!strcmp(name, g_msc[r].name)) return r;
  return -1;
}
void diaout_msc_sources(int row, std::vector<std::string> *names) {
  names->push_back(g_msc[row].usrc);
  if (g_msc[row].vsrc) names->push_back(g_msc[row].vsrc);
}
// the rows of blomgpu_dia_name_ext in their order, then the 23 msc names with kind 5
int diaout_name_msc(int index, char *buf, int cap, int *kind, int *grid) {
  static const int NROW_EXT = [] {                                // the length of stage_diaacc.hip's table, asked of its enumerator
    char b[32];
    int n = 0;
    while (dia_name_ext(n, b, 32, nullptr, nullptr) == 0) n++;
    return n;
  }();
  if (index < NROW_EXT) return dia_name_ext(index, buf, cap, kind, grid);
  if (index >= NROW_EXT + NMSC || !buf || cap < 2) return 1;
  snprintf(buf, cap, "%s", g_msc[index - NROW_EXT].name);
  if (kind) *kind = KIND_MSC;
  if (grid) *grid = 0;
  return 0;
}

void diaout_invalidate(blomgpu_ctx *c) { if (c->diaout) c->diaout->reduced = false; }
void diaout_free(blomgpu_ctx *c) {
  DiaOutState *D = c->diaout;
  if (!D) return;
  (void)hipStreamSynchronize(c->stream);
  D->mer.release();
  D->sec.release();
  if (D->res) (void)hipFree(D->res);
  if (D->util) (void)hipFree(D->util);
  if (D->rows) (void)hipFree(D->rows);
  delete D;
  c->diaout = nullptr;
}

// mer_orfile + mer_mifile as the caller read them (:4026-4108).  A point whose oflg <= 0 is dropped as :4070 does; what the reference
// stops for (:4076-4093) and what would leave its arrays (ldm, sdm :163-164; mflx_or(lmax,ocn_nreg)) is refused.
int diaout_set_mertra(blomgpu_ctx *c, int lmax, const double *mtlat, const int *nind, const int *pts, const int *oflg, int ocn_nreg,
                      int mer_nreg, const int *nflg, const int *regflg, const double *minlat, const double *maxlat) {
  const char *who = "blomgpu_dia_set_mertra: ";
  DiaOutState *D = state_of(c);
  if (lmax == 0 && !mtlat && !nind && !pts) {                     // NULL with count 0 clears the table
    (void)hipStreamSynchronize(c->stream);
    D->mer.release();
    D->has_mer = false;
    D->reduced = false;
    return 0;
  }
  if (lmax < 1 || !mtlat || !nind || !pts || !oflg || !nflg || !regflg || !minlat || !maxlat) return ctx_fail(c, std::string(who) + "null argument");
  const int itdm = c->h.itdm, jtdm = c->h.jtdm, ldm = itdm + jtdm;
  if (lmax > ldm) return ctx_fail(c, std::string(who) + "too many or too long sections! lmax = " + std::to_string(lmax) + " > itdm+jtdm = " + std::to_string(ldm));
  if (ocn_nreg < 1 || ocn_nreg > DOUT_MAXREG) return ctx_fail(c, std::string(who) + "ocn_nreg = " + std::to_string(ocn_nreg) + ": 1.." + std::to_string(DOUT_MAXREG) + " ocean regions");
  if (mer_nreg < 1 || mer_nreg > DOUT_MAXREG) return ctx_fail(c, std::string(who) + "mer_nreg = " + std::to_string(mer_nreg) + ": 1.." + std::to_string(DOUT_MAXREG) + " meridional regions");
  for (size_t x = 0; x < (size_t)itdm * jtdm; x++)
    if (oflg[x] > ocn_nreg) return ctx_fail(c, std::string(who) + "oflg(" + std::to_string(x % itdm + 1) + "," + std::to_string(x / itdm + 1) + ") = " + std::to_string(oflg[x]) + " > ocn_nreg = " + std::to_string(ocn_nreg));
  for (int m = 0; m < mer_nreg; m++) {
    const int *f = regflg + (size_t)m * DOUT_NFLG;
    if (f[0] == 0) continue;                                      // all ocean regions (:4242)
    if (nflg[m] < 1 || nflg[m] > DOUT_NFLG) return ctx_fail(c, std::string(who) + "mer_nflg(" + std::to_string(m + 1) + ") = " + std::to_string(nflg[m]) + ": 1.." + std::to_string(DOUT_NFLG) + " flags");
    for (int n = 0; n < nflg[m]; n++)
      if (f[n] < (n ? 1 : 0) || f[n] > ocn_nreg)
        return ctx_fail(c, std::string(who) + "mer_regflg(" + std::to_string(m + 1) + "," + std::to_string(n + 1) + ") = " + std::to_string(f[n]) + " outside 0..ocn_nreg = " + std::to_string(ocn_nreg) + " (0 as the first flag only)");
  }
  std::vector<int> ints, start(1, 0);
  const int *p = pts;
  for (int l = 0; l < lmax; l++) {
    if (nind[l] < 0) return ctx_fail(c, std::string(who) + "section " + std::to_string(l + 1) + " has a negative count");
    int kept = 0;
    for (int s = 0; s < nind[l]; s++, p += 4) {
      if (p[0] < 1 || p[0] > itdm || p[1] < 1 || p[1] > jtdm)
        return ctx_fail(c, std::string(who) + "indices out of range! section " + std::to_string(l + 1) + ": iind = " + std::to_string(p[0]) + " itdm = " + std::to_string(itdm) +
                           " jind = " + std::to_string(p[1]) + " jtdm = " + std::to_string(jtdm));
      const int o = oflg[(size_t)(p[1] - 1) * itdm + (p[0] - 1)];
      if (o <= 0) continue;                                       // :4070
      ints.insert(ints.end(), {plane_index(c->h, p[0], p[1]), p[2], p[3], o});
      kept++;
    }
    if (kept > ldm) return ctx_fail(c, std::string(who) + "too many or too long sections! section " + std::to_string(l + 1) + " keeps " + std::to_string(kept) + " > itdm+jtdm = " + std::to_string(ldm) + " points");
    start.push_back(start.back() + kept);
  }
  // [pts | start | nflg | regflg] and [mtlat | minlat | maxlat]
  const size_t o_start = ints.size(), o_nflg = o_start + start.size(), o_reg = o_nflg + mer_nreg;
  ints.insert(ints.end(), start.begin(), start.end());
  ints.insert(ints.end(), nflg, nflg + mer_nreg);
  ints.insert(ints.end(), regflg, regflg + (size_t)mer_nreg * DOUT_NFLG);
  std::vector<double> dbls(mtlat, mtlat + lmax);
  dbls.insert(dbls.end(), minlat, minlat + mer_nreg);
  dbls.insert(dbls.end(), maxlat, maxlat + mer_nreg);
  (void)hipSetDevice(c->device);
  DevTab T;
  if (to_device(c, &T.ints, ints) || to_device(c, &T.dbls, dbls)) { T.release(); return 1; }
  (void)hipStreamSynchronize(c->stream);
  D->mer.release();
  D->mer = T;
  D->has_mer = true;
  D->reduced = false;
  D->lmax = lmax; D->no = ocn_nreg; D->nm = mer_nreg;
  SecTab &S = D->mer_dev;
  S.pts = T.ints; S.start = T.ints + o_start; S.nflg = T.ints + o_nflg; S.regflg = T.ints + o_reg;
  S.mtlat = T.dbls; S.minlat = T.dbls + lmax; S.maxlat = T.dbls + lmax + mer_nreg;
  S.nsec = lmax; S.no = ocn_nreg; S.nm = mer_nreg;
  return 0;
}

// sec_sifile as the caller read it (:3838-3866); equat_sec: the 1-based section of the upper-350 m sums (:3849), -1 for none
int diaout_set_sections(blomgpu_ctx *c, int sec_num, const int *nsi, const int *pts, int equat_sec) {
  const char *who = "blomgpu_dia_set_sections: ";
  DiaOutState *D = state_of(c);
  if (sec_num == 0 && !nsi && !pts) {
    (void)hipStreamSynchronize(c->stream);
    D->sec.release();
    D->has_sec = false;
    D->reduced = false;
    return 0;
  }
  if (sec_num < 1 || !nsi || !pts) return ctx_fail(c, std::string(who) + "null argument");
  const int itdm = c->h.itdm, jtdm = c->h.jtdm, ldm = itdm + jtdm;
  if (sec_num > ldm) return ctx_fail(c, std::string(who) + "sec_num = " + std::to_string(sec_num) + " > itdm+jtdm = " + std::to_string(ldm));
  if (equat_sec != -1 && (equat_sec < 1 || equat_sec > sec_num))
    return ctx_fail(c, std::string(who) + "equat_sec = " + std::to_string(equat_sec) + ": a section 1.." + std::to_string(sec_num) + ", or -1 for none");
  if (equat_sec >= 1 && !dia_levels_kind(c))
    return ctx_fail(c, std::string(who) + "the upper-350 m sums of section " + std::to_string(equat_sec) + " need k350 and w350, which the reference has for its own two level tables only "
                       "(phy/mod_dia.F90:112-113, :131-132): the depth levels in force are a table of blomgpu_dia_set_levels");
  std::vector<int> ints, start(1, 0);
  const int *p = pts;
  for (int s = 0; s < sec_num; s++) {
    if (nsi[s] < 0 || nsi[s] > ldm) return ctx_fail(c, std::string(who) + "section " + std::to_string(s + 1) + " has " + std::to_string(nsi[s]) + " points: 0..itdm+jtdm = " + std::to_string(ldm));
    for (int n = 0; n < nsi[s]; n++, p += 4) {
      if (p[0] < 1 || p[0] > itdm || p[1] < 1 || p[1] > jtdm)
        return ctx_fail(c, std::string(who) + "indices out of range! section " + std::to_string(s + 1) + ": i = " + std::to_string(p[0]) + " itdm = " + std::to_string(itdm) +
                           " j = " + std::to_string(p[1]) + " jtdm = " + std::to_string(jtdm));
      ints.insert(ints.end(), {plane_index(c->h, p[0], p[1]), p[2], p[3], 1});
    }
    start.push_back(start.back() + nsi[s]);
  }
  const size_t o_start = ints.size();
  ints.insert(ints.end(), start.begin(), start.end());
  (void)hipSetDevice(c->device);
  DevTab T;
  if (to_device(c, &T.ints, ints)) { T.release(); return 1; }
  (void)hipStreamSynchronize(c->stream);
  D->sec.release();
  D->sec = T;
  D->has_sec = true;
  D->reduced = false;
  D->sec_num = sec_num; D->equat = equat_sec;
  SecTab &S = D->sec_dev;
  S = SecTab{};
  S.pts = T.ints; S.start = T.ints + o_start; S.nsec = sec_num; S.no = 1; S.nm = 1;
  return 0;
}

// diamer, diasec and the global sums for the selected msc names, on the context's stream; nothing waits for the device
int diaout_reduce(blomgpu_ctx *c) {
  const char *who = "blomgpu_dia_reduce: ";
  const unsigned msc = dia_msc_mask(c);
  if (!whole_domain(c))
    return ctx_fail(c, std::string(who) + "this context is a tile of a group or an RCCL rank: the sections and the sums span the whole domain (xcaget over tiles is not built)");
  if (!msc) return ctx_fail(c, std::string(who) + "no msc name is selected (blomgpu_dia_select)");
  if (dia_finalized(c))
    return ctx_fail(c, std::string(who) + "blomgpu_dia_finalize has run, and the level accumulators hold fill values: the reductions come in front of it (phy/mod_dia.F90:2366-2588), or after blomgpu_dia_reset");
  int nacc = 0;
  if (int rc = dia_nacc(c, &nacc)) return rc;
  if (nacc == 0) return ctx_fail(c, std::string(who) + "nacc = 0: no step has been accumulated, and the reference divides by nacc");
  DiaOutState *D = state_of(c);
  bool need_mer = false, need_sec = false, need_glb = false;
  for (int r = 0; r < NMSC; r++)
    if (msc >> r & 1) {
      need_mer |= g_msc[r].kind <= K_DEPTH; need_sec |= g_msc[r].kind == K_SEC; need_glb |= g_msc[r].kind == K_GLB;
      if (g_msc[r].kind <= K_DEPTH && !D->has_mer)
        return ctx_fail(c, std::string(who) + g_msc[r].name + " is selected, which needs the sections and regions of diamer (blomgpu_dia_set_mertra)");
      if (g_msc[r].kind == K_SEC && !D->has_sec)
        return ctx_fail(c, std::string(who) + g_msc[r].name + " is selected, which needs the sections of diasec (blomgpu_dia_set_sections)");
    }
  const DevView &h = c->h;
  const int kk = h.kk;
  int ddm = 0;
  const double *edges = dia_edges_dev(c, &ddm);
  const int lvk = dia_levels_kind(c);
  if (need_sec && D->equat >= 1 && !lvk)
    return ctx_fail(c, std::string(who) + "the upper-350 m sums of section " + std::to_string(D->equat) + " need k350 and w350, which the reference has for its own two level tables only "
                       "(phy/mod_dia.F90:112-113, :131-132): the depth levels in force are a table of blomgpu_dia_set_levels");
  if ((msc >> M_SSSGA & 3) && c->area <= 0.) return ctx_fail(c, std::string(who) + "sssga / sstga: the ocean area (mod_grid: area) has not been set");
  // where the results go
  size_t n = 0;
  for (int r = 0; r < NMSC; r++) {
    D->off[r] = -1;
    D->dims[r][0] = D->dims[r][1] = D->dims[r][2] = 0;
    if (!(msc >> r & 1)) continue;
    int *d = D->dims[r];
    switch (g_msc[r].kind) {
      case K_DENS: d[0] = D->nm; d[1] = kk; d[2] = D->lmax; break;
      case K_DEPTH: d[0] = D->nm; d[1] = ddm; d[2] = D->lmax; break;
      case K_TR: d[0] = D->nm; d[1] = D->lmax; d[2] = 1; break;
      case K_SEC: d[0] = D->sec_num; d[1] = d[2] = 1; break;
      default: d[0] = d[1] = d[2] = 1;
    }
    D->off[r] = (long long)n;
    n += (size_t)d[0] * d[1] * d[2];
  }
  const size_t o_massgs_hidden = n;                               // massgs where salnga | tempga want it and the name is not selected
  n++;
  (void)hipSetDevice(c->device);
  if (n > D->res_cap) {                                           // (the first reduce of a selection and table set; none afterwards)
    if (D->res) { (void)hipStreamSynchronize(c->stream); (void)hipFree(D->res); D->res = nullptr; D->res_cap = 0; }
    HIPCHK(c, hipMalloc((void **)&D->res, sizeof(double) * n));
    D->res_cap = n;
  }
  D->reduced = false;
  ctx_sync_view(c);
  const double rnacc = 1. / (double)nacc;                         // :2363
  if (need_mer || need_sec) {
    OutJobs J[4];                                                 // a launch per kind of name: the transports, the two stream functions, diasec's
    memset(J, 0, sizeof(J));
    for (OutJobs &j : J) {
      j.ep = c->diaout_entries; j.lc = c->diaout_levels;
      j.k350 = lvk == 70 ? 25 : 12; j.w350 = lvk == 70 ? .5 : 1.; // :112-113 | :131-132
      j.equat = D->equat;
    }
    const double den = (GRAV * h.P.baclin) * (double)nacc;
    const double *base = nullptr;
    int lds_nout[4] = {1, 1, 1, 1};
    for (int r = 0; r < NMSC; r++) {
      if (!(msc >> r & 1) || g_msc[r].kind > K_SEC) continue;
      const MscRow &m = g_msc[r];
      const double *pu = dia_plane_dev(c, m.usrc), *pv = dia_plane_dev(c, m.vsrc);
      if (!pu || !pv) return ctx_fail(c, std::string(who) + m.name + ": a source accumulator is not selected");
      if (!base) base = pu;
      const int w = m.kind;
      OutJob &jb = J[w].j[J[w].n++];
      jb.nsrc = m.kind == K_TR || m.kind == K_DENS ? kk : ddm;
      jb.nout = m.kind == K_DENS ? kk : m.kind == K_DEPTH ? ddm : 1;
      jb.r = (m.fac == R_HEAT ? .5 * SPCIFH : m.fac == R_SALT ? .5 * G2KG : .5) / den;
      jb.out = D->off[r];
      jb.pu = pu - base; jb.pv = pv - base;                       // (element offsets from one base pointer of the accumulators)
      if (jb.nout > DOUT_MAXLEV) return ctx_fail(c, std::string(who) + m.name + ": more than " + std::to_string(DOUT_MAXLEV) + " levels");
      if (jb.nout > lds_nout[w]) lds_nout[w] = jb.nout;
    }
    static const char *const label[4] = {"diaout_transports", "diaout_density", "diaout_depth", "diaout_diasec"};
    for (int w = 0; w < 4; w++) {
      if (!J[w].n) continue;
      const SecTab &T = w == K_SEC ? D->sec_dev : D->mer_dev;
      const Carve C = carve_of(J[w].ep, J[w].lc, lds_nout[w], T.no);
      TimeScope ts(c, label[w]);
      const dim3 grid(T.nsec, J[w].n);
      // (256 entries x 8 levels, 128 levels x 32 regions: 85 KB at most, of the 160 KB a workgroup can have; past 64 KB the kernel is told)
#define DOUT_LAUNCH(K)                                                                                                                    \
  if (C.bytes > 64 * 1024) (void)hipFuncSetAttribute((const void *)k_diaout_sections<K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)C.bytes); \
  hipLaunchKernelGGL((k_diaout_sections<K>), grid, dim3(DOUT_T), C.bytes, c->stream, c->d, base, edges, T, J[w], lds_nout[w], T.no, D->res)
      if (w == K_TR) { DOUT_LAUNCH(K_TR); }
      else if (w == K_DENS) { DOUT_LAUNCH(K_DENS); }
      else if (w == K_DEPTH) { DOUT_LAUNCH(K_DEPTH); }
      else { DOUT_LAUNCH(K_SEC); }
#undef DOUT_LAUNCH
      HIPCHK(c, hipGetLastError());
    }
  }
  if (need_glb) {
    if (!D->util) HIPCHK(c, hipMalloc((void **)&D->util, sizeof(double) * 6 * (size_t)h.nplane));
    if (!D->rows) HIPCHK(c, hipMalloc((void **)&D->rows, sizeof(double) * 6 * ((size_t)h.jtdm + 1)));
    // the sums the names ask for: dp (massgs, and salnga | tempga's divisor), dz, saln, temp, sss, sst
    static const char *const src[6] = {"dp", "dz", "saln", "temp", "sss", "sst"};
    const bool want[6] = {(msc >> M_MASSGS & 7) != 0, (msc >> M_VOLGS & 1) != 0, (msc >> M_SALNGA & 1) != 0, (msc >> M_TEMPGA & 1) != 0,
                          (msc >> M_SSSGA & 1) != 0, (msc >> M_SSTGA & 1) != 0};
    ColJobs Q;
    memset(&Q, 0, sizeof(Q));
    GlbJob G;
    const double *base = nullptr;
    for (int x = 0; x < 6; x++) {
      G.idx[x] = -1;
      if (!want[x]) continue;
      const double *p = dia_plane_dev(c, src[x]);
      if (!p) return ctx_fail(c, std::string(who) + src[x] + ": a source accumulator is not selected");
      if (!base) base = p;
      G.idx[x] = Q.n;
      Q.src[Q.n] = p - base; Q.nlev[Q.n] = x < 4 ? kk : 1;
      Q.n++;
    }
    const auto at = [&](int r) { return msc >> r & 1 ? D->off[r] : -1ll; };
    G.out[0] = at(M_MASSGS); G.out[1] = at(M_SALNGA); G.out[2] = at(M_TEMPGA); G.out[3] = at(M_VOLGS); G.out[4] = at(M_SSSGA); G.out[5] = at(M_SSTGA);
    if (G.out[0] < 0 && want[0]) G.out[0] = (long long)o_massgs_hidden;       // formed whenever salnga | tempga is selected, handed out only when selected itself
    G.rnacc = rnacc; G.area = c->area;
    {
      TimeScope ts(c, "diaout_columns");
      hipLaunchKernelGGL(k_diaout_columns, plane_grid(h), dim3(256), 0, c->stream, c->d, base, Q, D->util);
      HIPCHK(c, hipGetLastError());
    }
    const double *planes[6];
    const int *masks[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // ips
    for (int q = 0; q < Q.n; q++) planes[q] = D->util + (size_t)q * h.nplane;
    double *sums = D->rows + 6 * (size_t)h.jtdm;
    TimeScope ts(c, "diaout_xcsum");
    if (int rc = st_xcsum_batch(c, Q.n, planes, masks, D->rows, sums, false)) return rc;      // (not one of thermf's counted launches)
    hipLaunchKernelGGL(k_diaout_globals, dim3(1), dim3(64), 0, c->stream, sums, G, D->res);
    HIPCHK(c, hipGetLastError());
  }
  D->reduced = true;
  return 0;
}

int diaout_msc_get(blomgpu_ctx *c, const char *name, double *out, int cap, int *dims) {
  const char *who = "blomgpu_dia_msc_get: ";
  if (!name || !dims || (!out && cap > 0)) return ctx_fail(c, std::string(who) + "null argument");
  const int r = diaout_msc_index(name);
  if (r < 0) return ctx_fail(c, std::string(who) + "unknown msc name " + name);
  if (!(dia_msc_mask(c) >> r & 1)) return ctx_fail(c, std::string(who) + name + " is not selected");
  DiaOutState *D = c->diaout;
  if (!D || !D->reduced) return ctx_fail(c, std::string(who) + name + ": no blomgpu_dia_reduce since the selection, the tables or the accumulators were set");
  const size_t n = (size_t)D->dims[r][0] * D->dims[r][1] * D->dims[r][2];
  for (int x = 0; x < 3; x++) dims[x] = D->dims[r][x];
  if (cap == 0) return 0;                                         // the shape alone
  if ((size_t)(cap < 0 ? 0 : cap) < n) return ctx_fail(c, std::string(who) + name + " has " + std::to_string(n) + " values, cap = " + std::to_string(cap));
  HIPCHK(c, hipMemcpyAsync(out, D->res + D->off[r], sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}
