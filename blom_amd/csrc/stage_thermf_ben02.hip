// The surface forcing of the forced ocean-ice experiment (expcnf = 'ben02clim' / 'ben02syn' / 'single_column'; Bentsen & Drange 2002):
// sfcstr_ben02 and thermf_ben02, the one experiment family in which BLOM itself carries sea ice.
//
//   k_sfcstr_ben02          ben02/mod_sfcstr_ben02.F90:44-61: ficem, hicem with a halo of one (xctilr, in front of the kernel); taux at
//                           u-points and tauy at v-points, the wind stress and the ice stress weighted with facice
//   k_thermf_ben02_flux     ben02/mod_thermf_ben02.F90:124-598 per owned wet p-point: the slab ice / snow thermodynamics, lead freezing and
//                           lateral melt, the stores of the ice state and the five accumulations of asflux' averages, the runoff
//                           reservoir, fresh water / salt / heat fluxes, tracer fluxes, the relaxation towards SST and SSS (both vertical
//                           coordinates), the applied and the diagnosed relaxation fluxes, the age of the ice, the friction velocity --
//                           and the area weighted planes of every global sum that follows
//   st_xcsum_batch          :608, :629-630, :653: 1 + ntr' + 2 sums in two launches (halo.hip), left ON THE DEVICE
//   k_thermf_ben02_corr     :608-665: the corrections that need the sums
// so that thermf_ben02 is four launches up to 32 planes in the batch.  The per-step scalars (rnf_fac, sag_fac of :98-99 -- the routine's
// exp(-sagets*dt) is the host's; y, m1..m5, ntld of :103-113) are kernel arguments.  The kernel's own transcendentals are
// exp(-hotl/swal2) and hice**.28 (exp_libm, pow_libm).  swtfrz is the stand-alone driver's with inieos' coefficients for these
// experiments (drivers/nocoupler/mod_swtfrz.F, phy/mod_eos.F90:137-141).  asflux (ben02/mod_ben02.F90:1602-1918), which turns the
// accumulated averages into the fluxes this routine reads, stays the host's: its bulk transfer coefficients need log and atan.
// Roofline: HBM, ~60 two-dimensional planes (plus 2 kk + 2 (kk+1) levels under the hybrid coordinate); launch-bound at channel size.
#include "blomgpu_internal.h"
#include "ben02_constants.h"
#include "pow_libm.h"
#include "thermf_relax.h"
#include <cmath>

struct ThermfBen02Par {
  double trxday, srxday, trxdpt, srxdpt, trxlim, srxlim, xmi, sref, area, dt, y;
  double rnf_fac, sag_fac;       // :98-99
  double atf, btf, ctf;          // swtfrz
  double gls_c, gls_vk, gls_z;   // gls_cmu0**gls_p, vonKar**gls_n, Zos**(gls_n-1.) (phy/mod_tke.F90:36-58)
  int l1mi, l2mi, l3mi, l4mi, l5mi, m1, m2, m3, m4, m5, ntld;   // 1-based, as the reference's
  int use_gls, aptflx, apsflx, ditflx, disflx, srxbal, hybrid;
};

__global__ void k_sfcstr_ben02(const DevView *__restrict__ Vp) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii) return;
  gcd_t ficem = V.f[F_ficem], hicem = V.b[F_hicem];
  if (V.m[I_iu][c]) {
    const double facice = (ficem[c] + ficem[c - 1]) * fmin2(2., hicem[c] + hicem[c - 1]) * .25;
    V.f[F_taux][c] = V.f[F_ztx][c] * (1. - facice) + V.b[F_tauxice][c] * facice;
  }
  if (V.m[I_iv][c]) {
    const double facice = (ficem[c] + ficem[c - V.ni]) * fmin2(2., hicem[c] + hicem[c - V.ni]) * .25;
    V.f[F_tauy][c] = V.f[F_mty][c] * (1. - facice) + V.b[F_tauyice][c] * facice;
  }
}

__global__ void k_thermf_ben02_flux(const DevView *__restrict__ Vp, ThermfBen02Par T, int nn, int k1n) {
  const DevView &V = *Vp;
  THREAD_IJ_XCD(V);
  if (j < 1 || j > V.jj || i < 1 || i > V.ii || !V.m[I_ip][c]) return;
  const size_t np = V.nplane, o1 = c + (size_t)nn * np, o2 = o1 + np, okn = c + (size_t)(k1n - 1) * np;
  const int kk = V.kk, ntr = V.ntr;
  gcd_t dp = V.f[F_dp], temp = V.f[F_temp], saln = V.f[F_saln];
  const double p1 = V.f[F_p][c];
  const double dt = T.dt, cpsw = SPCIFH;
  // the ocean top layer, the mixed layer and the ice / snow state, :130-152
  const double dpotl = dp[okn];
  const double hotl = dpotl / ONEM;
  const double totl = temp[okn] + T0DEG;
  const double sotl = saln[okn];
  double fice = V.f[F_ficem][c], hice = V.b[F_hicem][c], hsnw = V.b[F_hsnwm][c], tsrf = V.b[F_tsrfm][c];
  const double fice0 = fice, hice0 = hice, hsnw0 = hsnw;
  const double tice_f = T.atf * sotl + T.btf + T.ctf * p1 + T0DEG;
  const double hice_min = V.f[F_plat][c] > 0. ? HICE_NHMN : HICE_SHMN;
  const double swa = V.f[F_swa][c], nsf = V.f[F_nsf][c], albw = V.b[F_albw][c];
  double alb, qsww, qnsw, tice;
  if (fice * hice < 1.e-5) {
    // at most a small amount of ice: melt the remainders of ice and snow, :161-176
    hice = 0.;
    hsnw = 0.;
    fice = 0.;
    alb = albw;
    qsww = swa;
    qnsw = nsf;
    tsrf = totl;
    tice = totl;
  } else {
    // thermodynamics of an ice slab, :184-293
    const double dfl = V.b[F_dfl][c], tsi = V.b[F_tsi][c], sop = V.f[F_sop][c];
    double albi, tsmlt;
    if (fice * hsnw > 1.e-3) {
      albi = tsrf > TSNW_M - .1 ? ALBS_M : ALBS_F;
      tsmlt = TSNW_M;
    } else {
      const double albi_h = .065 + .44 * pow_libm(hice, .28);
      albi = tsrf > TICE_M - .1 ? fmin2(ALBI_M, albi_h) : fmin2(ALBI_F, albi_h);
      tsmlt = TICE_M;
    }
    alb = albi * fice + albw * (1. - fice);
    const double qswi = swa * (1. - albi) / (1. - alb);
    qsww = swa * (1. - albw) / (1. - alb);
    double dh = sop * dt / RHOSNW;
    hsnw = hsnw + dh;
    const double qsnwf = dh * FUSS / dt;
    const double fcond = RKICE * RKSNW / (RKSNW * hice + RKICE * hsnw);
    double qdamp;
    if (fabs(fcond - dfl * (2. - fice)) < 1.e-3) {
      tsrf = tice_f + (qswi + nsf) / fcond;
      qnsw = nsf;
      qdamp = 0.;
    } else {
      tsrf = (qswi + nsf - dfl * (tsi + (1. - fice) * totl) + fcond * tice_f) / (fcond - dfl * (2. - fice));
      qnsw = nsf + dfl * fice * (totl - fmin2(tsrf, tsmlt));
      qdamp = dfl * (fmin2(tsrf, tsmlt) - tsi);
    }
    double qsmlt;
    if (tsrf > tsmlt) {
      tsrf = tsmlt;
      qsmlt = qswi + nsf + dfl * ((1. - fice) * (tsrf - totl) + tsrf - tsi) + fcond * (tice_f - tsrf);
    } else {
      qsmlt = 0.;
    }
    tice = tice_f - fcond * (tice_f - tsrf) * hice / RKICE;
    // heat flux from ocean to ice (Maykut and McPhee 1995) and the heat budget at the bottom of the ice
    const double qo2i = RHOWAT * cpsw * CWI * fmax2(V.b[F_ustari][c], .2e-2) * fmin2(tice_f - totl, 0.) + CUC * fmax2(tice_f - totl, 0.);
    const double qbot = -(fcond * (tice_f - tsrf)) - qo2i - qdamp + qsnwf;
    dh = -(qsmlt * dt / FUSS);
    if (hsnw + dh < 0.) {
      qsmlt = qsmlt - hsnw * FUSS / dt;
      hsnw = 0.;
    } else {
      qsmlt = 0.;
      hsnw = hsnw + dh;
    }
    hice = fmax2(0., hice - (qbot + qsmlt) * dt / FUSI);
    // snow to ice: aging, and flooding where the snow load exceeds the updrift of the ice
    hice = hice + hsnw * (1. - T.sag_fac) * RHOSNW / RHOICE;
    hsnw = hsnw * T.sag_fac;
    dh = (hsnw * RHOSNW - hice * (RHOWAT - RHOICE)) / RHOWAT;
    if (dh > 0.) {
      hice = hice + dh;
      hsnw = hsnw - dh * RHOICE / RHOSNW;
    }
  }
  // the open water fraction, :303-340
  const double swfac = 1. - V.f[F_swfc2][c] * exp_libm(-(hotl / V.f[F_swal2][c]));
  const double dtml = (swfac * qsww + qnsw) * 2. * dt / (cpsw * RHOWAT * hotl);
  if (totl + dtml < tice_f) {
    const double q = .5 * (tice_f - totl) * cpsw * RHOWAT * hotl / dt;
    const double volice = -((qsww + qnsw - q) * (1. - fice) * dt / FUSI);
    if (volice > EPSILT) {
      const double df = volice / hice_min;
      const double fnew = fmin2(FICE_MAX, fice + df);
      hice = (hice * fice + volice) / fnew;
      hsnw = hsnw * fice / fnew;
      fice = fnew;
    }
  } else if (swfac * qsww + qnsw > 0.) {
    fice = fice - (swfac * qsww + qnsw) * fice * dt / fmax2(hice * FUSI + hsnw * FUSS, EPSILT);
    if (fice < 0.) {
      fice = 0.;
      hice = 0.;
      hsnw = 0.;
    }
  }
  // the updated ice / snow state, :346-350; what asflux averages, :356-360
  V.f[F_ficem][c] = fice;
  V.b[F_hicem][c] = hice;
  V.b[F_hsnwm][c] = hsnw;
  V.b[F_tsrfm][c] = tsrf;
  V.b[F_ticem][c] = tice;
  V.b[F_alb][c] = alb;
  V.b[F_alb_tda][c] = V.b[F_alb_tda][c] + alb;
  V.b[F_tml_tda][c] = V.b[F_tml_tda][c] + totl;
  V.b[F_sml_tda][c] = V.b[F_sml_tda][c] + sotl;
  V.b[F_fice_tda][c] = V.b[F_fice_tda][c] + fice;
  V.b[F_tsi_tda][c] = V.b[F_tsi_tda][c] + tsrf;
  // fluxes of heat and salt to the ocean, :367-416
  const double dvi = hice * fice - hice0 * fice0;
  const double dvs = hsnw * fice - hsnw0 * fice0;
  double rnfres = V.b[F_rnfres][c] + V.b[F_rnfins][c];
  const double rnf = rnfres * T.rnf_fac;
  rnfres = rnfres * (1. - T.rnf_fac);
  V.f[F_rnf][c] = rnf;
  V.b[F_rnfres][c] = rnfres;
  const double fmltfz = -((dvi * RHOICE + dvs * RHOSNW) / dt);
  V.f[F_fmltfz][c] = fmltfz;
  const double fwflx = V.f[F_eva][c] + V.f[F_lip][c] + V.f[F_sop][c] + rnf + V.f[F_rfi][c] + fmltfz;
  const double sfl = -(SICE * dvi * RHOICE / dt * G2KG);
  V.f[F_sfl][c] = sfl;
  V.f[F_brnflx][c] = fmax2(0., -sotl * fmltfz * G2KG + sfl);
  const double vrtsfl = -sotl * fwflx * G2KG;
  WK2(V, S2_VRTSFL)[c] = vrtsfl;
  const double scp2 = V.f[F_scp2][c];
  gd_t util = V.f[F_thermf_util] + c;
  util[0] = -(T.sref * fwflx * G2KG + vrtsfl + V.f[F_salt_corr][c] * G2KG / (2. * dt)) * scp2;
  V.f[F_salt_corr][c] = 0.;
  const double hmltfz = (dvi * FUSI + dvs * FUSS) / dt;
  V.f[F_hmltfz][c] = hmltfz;
  V.f[F_surflx][c] = -(swa + nsf + hmltfz);
  V.f[F_sswflx][c] = -(qsww * (1. - fice0));
  // tracer fluxes (positive downwards), :423-451; and the area weighted plane of each tracer's global sum with the reset of its
  // correction (nothing up to :653 changes them)
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
    util[(size_t)q * np] = -(tf + *corr / (2. * dt)) * scp2;
    *corr = 0.;
    q++;
  }
  // relaxation fluxes, :458-578 (sstclm in kelvin)
  double pbot = p1;
  if (T.hybrid && (T.trxday > EPSILT || T.srxday > EPSILT)) {            // :477-481, :535-539
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
    double sstc = intp5(V.f[F_sstclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
    const double rice = intp5(V.f[F_ricclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
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
    const double sssc = intp5(V.f[F_sssclm] + c, np, T.l1mi, T.l2mi, T.l3mi, T.l4mi, T.l5mi, T.xmi);
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
  // age of the ice, :584-588; friction velocity, :594
  V.b[F_iagem][c] = fice * hice < 1.e-5 ? 0. : (V.b[F_iagem][c] + dt / 86400.) * (1. - fmax2(0., dvi) / (fice * hice));
  V.f[F_ustar][c] = fmin2(V.b[F_ustari][c], .8e-2) * fice0 + V.f[F_ustarw][c] * (1. - fice0);
}

// :608-665; sums[0] = the salt plane's sum, sums[1 .. ntr'] the tracers' in their order, sums[nq], sums[nq+1] = totsrp, totsrn
__global__ void k_thermf_ben02_corr(const DevView *__restrict__ Vp, ThermfBen02Par T, const double *__restrict__ sums, int nq) {
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
// The fields of the coupled experiment's lists that this experiment has too (ztx mty, the planes of the sums, the four 48-level arrays,
// ipwocn) keep their ids there: the declaration gives them names, and memory to all but the 48-level arrays (cesm_field).
static const struct { const char *name; int id; bool lazy; } kSharedReal[] = {
  {"ztx", F_ztx, false}, {"mty", F_mty, false}, {"thermf_util", F_thermf_util, false},
  {"tflxap", F_tflxap, true}, {"sflxap", F_sflxap, true}, {"tflxdi", F_tflxdi, true}, {"sflxdi", F_sflxdi, true},
};

// The declaration that the forced ocean-ice experiment's forcing exists.  The host uploads what asflux and the forcing readers leave
// (swa nsf dfl lip sop eva rfi rnfins ustarw tsi albw ztx mty, ustari tauxice tauyice, the climatologies, the ice state); every plane
// starts at zero.  Calling it again zeroes the diagnosed relaxation fluxes and their counts (phy/mod_idarlx.F90:89-114), nothing else.
int ben02_inifrc(blomgpu_ctx *c) {
  DevView &h = c->h;
  if (!ben02_expcnf(c->expcnf))
    return ctx_fail(c, "blomgpu_inifrc_ben02: expcnf = " + c->expcnf + " is not an experiment of mod_ben02 (ben02clim, ben02syn, single_column)");
  if (c->cesm_declared) return ctx_fail(c, "blomgpu_inifrc_ben02: this context has declared the coupled experiment's forcing (blomgpu_inifrc_cesm)");
  if (c->use_graph)
    return ctx_fail(c, "blomgpu_inifrc_ben02: the experiment's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  ctx_drop_graphs(c);
  if (!c->ben02_declared) {
    if (int rc = frc_alloc(c, &c->ben02_planes, NF_BEN02)) return rc;
    int k = 0;
#define X(name, lev) h.b[k] = c->ben02_planes + (size_t)k * h.nplane; c->real_ids[#name] = FID_BEN02 + k; k++;
    BLOM_BEN02_REAL_FIELDS(X)
#undef X
    for (const auto &s : kSharedReal) c->real_ids[s.name] = s.id;
    c->int_ids["ipwocn"] = I_ipwocn;
    c->ben02_declared = true;
    c->ntda = 0;
  }
  for (const auto &s : kSharedReal)
    if (!s.lazy)
      if (int rc = frc_alloc(c, &h.f[s.id], c->nlev_real[s.id])) return rc;
  if (!h.m[I_ipwocn]) {
    const size_t bytes = sizeof(int) * (size_t)h.nplane;
    HIPCHK(c, hipMalloc((void **)&h.m[I_ipwocn], bytes));
    HIPCHK(c, hipMemsetAsync(h.m[I_ipwocn], 0, bytes, c->stream));
  }
  if (int rc = frc_sum_buffers(c)) return rc;
  if (c->aptflx) if (int rc = frc_alloc(c, &h.f[F_tflxap], NLEV_RLX)) return rc;
  if (c->apsflx) if (int rc = frc_alloc(c, &h.f[F_sflxap], NLEV_RLX)) return rc;
  if (c->ditflx || c->disflx) {
    for (int &n : c->nflxdi) n = 0;
    for (int f : {(int)F_tflxdi, (int)F_sflxdi}) {
      if (!(f == F_tflxdi ? c->ditflx : c->disflx)) continue;
      if (int rc = frc_alloc(c, &h.f[f], NLEV_RLX)) return rc;
      HIPCHK(c, hipMemsetAsync(h.f[f], 0, sizeof(double) * (size_t)NLEV_RLX * h.nplane, c->stream));
    }
  }
  c->dirty = true;
  return 0;
}

// what asflux does before it leaves (ben02/mod_ben02.F90:1623-1624, :1701-1705): the five accumulated planes and their count to zero
int ben02_reset_tda(blomgpu_ctx *c) {
  if (!c->ben02_declared) return ctx_fail(c, "blomgpu_ben02_reset_tda: the forcing has not been declared (blomgpu_inifrc_ben02)");
  static_assert(F_tml_tda == F_tsi_tda + 1 && F_sml_tda == F_tsi_tda + 2 && F_alb_tda == F_tsi_tda + 3 && F_fice_tda == F_tsi_tda + 4,
                "the five accumulators are consecutive planes");
  HIPCHK(c, hipMemsetAsync(c->h.b[F_tsi_tda], 0, sizeof(double) * 5 * (size_t)c->h.nplane, c->stream));
  c->ntda = 0;
  return 0;
}

void ben02_free(blomgpu_ctx *c) {
  if (c->ben02_planes) (void)hipFree(c->ben02_planes);
  c->ben02_planes = nullptr;
}

// what the stages refuse before they launch anything
static int ben02_ready(blomgpu_ctx *c, const char *who) {
  if (!ben02_on(c)) return ctx_fail(c, std::string(who) + ": the forcing has not been declared (blomgpu_inifrc_ben02, expcnf = 'ben02clim' / 'ben02syn' / 'single_column')");
  if (c->use_graph)
    return ctx_fail(c, std::string(who) + ": the experiment's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  return 0;
}

int st_sfcstr_ben02(blomgpu_ctx *c) {
  if (int rc = ben02_ready(c, "sfcstr_ben02")) return rc;
  DevView &h = c->h;
  ctx_sync_view(c);
  TimeScope ts(c, "sfcstr");
  if (int rc = st_xctilr(c, h.f[F_ficem], 1, 1, 1, 1, 1)) return rc;        // :44-45 (halo_ps)
  if (int rc = st_xctilr(c, h.b[F_hicem], 1, 1, 1, 1, 1)) return rc;
  hipLaunchKernelGGL(k_sfcstr_ben02, plane_grid(h), dim3(256), 0, c->stream, c->d);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int st_thermf_ben02(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  (void)m; (void)n; (void)mm; (void)k1m;
  if (int rc = ben02_ready(c, "thermf_ben02")) return rc;
  DevView &h = c->h;
  static_assert(FUSS / FUSI - RHOSNW / RHOICE < EPSILT && RHOSNW / RHOICE - FUSS / FUSI < EPSILT,
                "thermf: check consistency between snow/ice densities and heat of fusion!");      // :85-93
  if (c->area <= 0.) return ctx_fail(c, "thermf_ben02: the ocean area (mod_grid: area) has not been set");
  if (c->nstep_in_day < 1 || h.P.nday_in_year < 1) return ctx_fail(c, "thermf_ben02: nstep_in_day and nday_in_year have not been set");
  ThermfBen02Par T;
  T.trxday = c->trxday; T.srxday = c->srxday; T.trxdpt = c->trxdpt; T.srxdpt = c->srxdpt; T.trxlim = c->trxlim; T.srxlim = c->srxlim;
  T.xmi = c->xmi; T.sref = c->sref; T.area = c->area; T.dt = h.P.baclin;
  T.rnf_fac = h.P.baclin / (double)(NRFETS * 86400);                                              // :98
  T.sag_fac = std::exp(-SAGETS * T.dt);                                                           // :99
  T.atf = -0.0547; T.btf = 0.; T.ctf = 0.;                                                        // phy/mod_eos.F90:137-141
  T.use_gls = h.P.itrtke >= 1 && h.P.gls ? 1 : 0;
  T.gls_c = std::pow(.527, 3.); T.gls_vk = std::pow(.4, -1.); T.gls_z = std::pow(.0002, -1. - 1.);
  T.l1mi = c->lmi[0]; T.l2mi = c->lmi[1]; T.l3mi = c->lmi[2]; T.l4mi = c->lmi[3]; T.l5mi = c->lmi[4];
  // time interpolation of the diagnosed relaxation fluxes, :103-113
  double y = ((double)(c->nday_of_year - 1) + (double)(h.P.nstep % c->nstep_in_day) / (double)c->nstep_in_day) * 48. / (double)h.P.nday_in_year;
  const int m3 = (int)y + 1;
  y = y - (double)(m3 - 1);
  if (m3 < 1 || m3 > NLEV_RLX) return ctx_fail(c, "thermf_ben02: nday_of_year lies outside the year");
  T.y = y;
  T.m3 = m3; T.m1 = (m3 + 45) % 48 + 1; T.m2 = (m3 + 46) % 48 + 1; T.m4 = m3 % 48 + 1; T.m5 = (m3 + 1) % 48 + 1;
  T.ntld = m3;
  T.aptflx = c->aptflx; T.apsflx = c->apsflx; T.ditflx = c->ditflx; T.disflx = c->disflx;
  T.srxbal = c->srxbal; T.hybrid = h.P.vcoord_tag != 1;
  const bool bal = c->srxday > EPSILT && c->srxbal;
  if (bal && c->tiling.multi()) return ctx_fail(c, "thermf_ben02: the balanced salinity relaxation (srxbal) is built for a single tile");
  if (c->aptflx) if (int rc = cesm_field(c, F_tflxap)) return rc;
  if (c->apsflx) if (int rc = cesm_field(c, F_sflxap)) return rc;
  if (c->ditflx) if (int rc = cesm_field(c, F_tflxdi)) return rc;
  if (c->disflx) if (int rc = cesm_field(c, F_sflxdi)) return rc;
  ctx_sync_view(c);
  if (c->ditflx || c->disflx) c->nflxdi[T.ntld - 1]++;                                           // :115
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
  // (the stage's timer, and one per part of it: tools/gpu_thermf_ben02_cost.py)
  TimeScope ts(c, "thermf");
  {
    TimeScope t1(c, "thermf_ben02_flux");
    hipLaunchKernelGGL(k_thermf_ben02_flux, plane_grid(h), dim3(256), 0, c->stream, c->d, T, nn, k1n);
    c->cesm_launches++;
  }
  {
    TimeScope t2(c, "thermf_ben02_sums");
    if (int rc = st_xcsum_batch(c, (int)planes.size(), planes.data(), masks.data(), c->cesm_rows, c->cesm_sums)) return rc;
  }
  {
    TimeScope t3(c, "thermf_ben02_corr");
    hipLaunchKernelGGL(k_thermf_ben02_corr, plane_grid(h), dim3(256), 0, c->stream, c->d, T, c->cesm_sums, nq);
    c->cesm_launches++;
  }
  HIPCHK(c, hipGetLastError());
  c->ntda++;                                                                                      // :671
  return 0;
}
