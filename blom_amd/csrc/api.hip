// C-ABI of libblomgpu.so: context, field registry, options, dispatcher, stepping.
// See include/blomgpu.h for the contract and the reference interfaces it mirrors.
#include "../../include/blomgpu.h"
#include "blomgpu_internal.h"
#include "pow_libm.h"
#include "sin_libm.h"
#include "atan2_libm.h"
#include <algorithm>
#include <cstring>
#include <string_view>

static thread_local std::string g_err;

int ctx_fail(blomgpu_ctx *c, const std::string &msg) {
  if (c) c->err = msg;
  g_err = msg;
  return 1;
}

void ctx_drop_graphs(blomgpu_ctx *c) {
  for (auto &g : c->step_graph)
    if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
  // an option switched after the warm-up may select kernels whose lazily allocated buffers / occupancy queries have
  // not run yet: a capture must not be the first execution of such a sequence, so the warm-up count restarts
  c->steps_warm = 0;
}

void ctx_sync_view(blomgpu_ctx *c) {
  if (!c->dirty) return;
  ctx_drop_graphs(c);
  (void)hipMemcpyAsync(c->d, &c->h, sizeof(DevView), hipMemcpyHostToDevice, c->stream);
  // the alternative views (blomgpu_internal.h): the same fields and parameters, momtum's own p / pu / pv / work space
  for (int v = 1; v < NVIEW; v++) {
    if (!c->dv[v]) continue;
    DevView &a = c->hv[v];
    a = c->h;
    a.wk = c->wk_mom;
    a.nwk = MF_NSLOT;
    if (v == VIEW_MOM_A) { a.f[F_pu] = c->pu_alt; a.f[F_pv] = c->pv_alt; }
    if (v == VIEW_MOM_B) a.f[F_p] = c->p_alt;
    (void)hipMemcpyAsync(c->dv[v], &a, sizeof(DevView), hipMemcpyHostToDevice, c->stream);
  }
  c->dirty = false;
}

// ---- the second stream of blomgpu_step's stage overlap (blomgpu_internal.h: blomgpu_ctx::overlap) -----------------------
bool ctx_overlap_on(const blomgpu_ctx *c) {
  // not while stage timers run (their HIP events bracket launches on the context's stream), not on the hybrid coordinates
  // (their sequence has its own second stream inside ale_regrid_remap)
  return c->overlap && c->seq.in_sequence && !c->timing && c->h.P.vcoord_tag == 1 && c->side != nullptr;
}
int ctx_side_fork(blomgpu_ctx *c, int ev) {
  HIPCHK(c, hipEventRecord(c->ev_side[ev], c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_side[ev], 0));
  return 0;
}
int ctx_side_done(blomgpu_ctx *c, int ev) {
  HIPCHK(c, hipEventRecord(c->ev_side[ev], c->side));
  return 0;
}
int ctx_side_join(blomgpu_ctx *c, int ev) {
  HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_side[ev], 0));
  return 0;
}

TimeScope::TimeScope(blomgpu_ctx *c_, const char *w, hipStream_t s) : c(c_), what(w), st(s ? s : c_->stream) {
  if (!c->timing) return;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, st);
}
TimeScope::~TimeScope() {
  if (!c->timing) return;
  (void)hipEventRecord(b, st);
  c->timers[what].pending.emplace_back(a, b);
}

// inieos, phy/mod_eos.F90:105-116
static void set_eos(Params &P) {
  const double a11 = 9.9985372432159340e+02, a12 = 1.0380621928183473e+01,
               a13 = 1.7073577195684715e+00, a14 = -3.6570490496333680e-02,
               a15 = -7.3677944503527477e-03, a16 = -3.5529175999643348e-03,
               b11 = 1.7083494994335439e-06, b12 = 7.1567921402953455e-09,
               b13 = 1.2821026080049485e-09, a21 = 1.0, a22 = 1.0316374535350838e-02,
               a23 = 8.9521792365142522e-04, a24 = -2.8438341552142710e-05,
               a25 = -1.1887778959461776e-05, a26 = -4.0163964812921489e-06,
               b21 = 1.1995545126831476e-09, b22 = 5.5234008384648383e-12,
               b23 = 8.4310335919950873e-13, alpha0 = ALPHA0;
  P.ap21 = a21 + b21 * P.pref;
  P.ap22 = a22 + b22 * P.pref;
  P.ap23 = a23 + b23 * P.pref;
  P.ap24 = a24;
  P.ap25 = a25;
  P.ap26 = a26;
  P.ap11 = a11 + b11 * P.pref - P.ap21 / alpha0;
  P.ap12 = a12 + b12 * P.pref - P.ap22 / alpha0;
  P.ap13 = a13 + b13 * P.pref - P.ap23 / alpha0;
  P.ap14 = a14 - P.ap24 / alpha0;
  P.ap15 = a15 - P.ap25 / alpha0;
  P.ap16 = a16 - P.ap26 / alpha0;
}

// the four wet masks of a point in one word (bit 0 ip, 1 iu, 2 iv, 3 iq): one load instead of four in the fused kernels
__global__ void k_pack_masks(const DevView *__restrict__ Vp) {
  const DevView &V = *Vp;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  V.m[I_mpack][t] = (V.m[I_ip][t] != 0) | (V.m[I_iu][t] != 0) << 1 | (V.m[I_iv][t] != 0) << 2 | (V.m[I_iq][t] != 0) << 3;
}
int ctx_pack_masks(blomgpu_ctx *c) {
  c->mom_aw_key = -1;              // (the viscous march's launch lists follow the masks: stage_momtum_fused.hip)
  ctx_sync_view(c);
  hipLaunchKernelGGL(k_pack_masks, plane_grid(c->h), dim3(256), 0, c->stream, c->d);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int ctx_err_words(blomgpu_ctx *c) {
  if (!c->err_dev) {
    HIPCHK(c, hipMalloc((void **)&c->err_dev, sizeof(int) * 8));
    HIPCHK(c, hipMemsetAsync(c->err_dev, 0, sizeof(int) * 8, c->stream));
  }
  return 0;
}

int ctx_check_errors(blomgpu_ctx *c) {
  if (blomgpu_ctx *G = bt_global_ctx(c))                   // RCCL tiles: the barotropic solver's words live in its own context
    if (ctx_check_errors(G)) { c->err = G->err; return 1; }
  if (c->ale && c->h.P.vcoord_tag != 1)
    if (int rc = ale_check_deferred(c)) return rc;
  if (!c->err_dev) return stepend_check_errors(c);
  int e[5] = {0, 0, 0, 0, 0};          // (word 3: convec's iteration limit, which the reference only prints: not an error)
  HIPCHK(c, hipMemcpyAsync(e, c->err_dev, sizeof(e), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // the words are only ever set by a failing kernel (zeroed at allocation): clear them once reported
  if (e[0] || e[1] || e[2] || e[4]) HIPCHK(c, hipMemsetAsync(c->err_dev, 0, sizeof(int) * 8, c->stream));
  if (e[0] & 2) return ctx_fail(c, "blom: diapfl: no convergence in implicit diffusion!");        // mod_diapfl.F90:520-530
  if (e[0] & 1) return ctx_fail(c, "blom: diapfl: no convergence in flux limit!");
  if (e[1] & 1) return ctx_fail(c, "blom: eddtra_gm_isopyc_bulkml: no convergence");              // mod_eddtra.F90:536-555
  if (e[1] & 2) return ctx_fail(c, "blom: eddtra_gm_isopyc_bulkml: flux bound violated");          // mod_eddtra.F90:640-660
  if (e[4]) return ctx_fail(c, "ndiff: a face found more neutral layers than its record space holds");
  if (e[2]) return ctx_fail(c, "barotp: a tile of the persistent substep kernel timed out waiting for its neighbours");
  return stepend_check_errors(c);                          // chkvar, the step's last call (phy/mod_chkvar.F90:77-141)
}

// an option that the cached ALE structures depend on has changed: report what the engine still holds of earlier steps (its deferred
// status, polled otherwise every check_period steps), then drop the structures
static int ale_reset(blomgpu_ctx *c) {
  if (!c->ale) return 0;
  const int rc = c->h.P.vcoord_tag != 1 ? ale_check_deferred(c) : 0;
  ale_free(c);
  return rc;
}

// ---- the option table ------------------------------------------------------------------------------------------------------
// One row per name that blomgpu_set_real / blomgpu_set_int / blomgpu_set_str accept: its kind (which entry point knows it), where
// the value lives, what setting it touches, and how it is checked.  The defaults and the comments of the values stand at the
// members (blomgpu_internal.h: Params, blomgpu_ctx).  Every setter drops the captured graphs, for unknown names too (KEEP_GRAPHS:
// the one exception).
enum OptKind { O_REAL, O_INT, O_BOOL, O_STR };      // O_BOOL: set through blomgpu_set_int and stored as v != 0
enum : unsigned {
  DIRTY = 1,        // a member of Params: the device view is uploaded again (context members are read by host code only)
  ALE_RESET = 2,    // the cached ALE structures depend on it
  READABLE = 4,     // blomgpu_get_real returns it
  KEEP_GRAPHS = 8,  // selects nothing a captured graph holds
};
struct Slot {       // the member a row names, with the member's own type
  double *d = nullptr; int *i = nullptr; bool *b = nullptr; std::string *s = nullptr;
  Slot(double &x) : d(&x) {}
  Slot(int &x) : i(&x) {}
  Slot(bool &x) : b(&x) {}
  Slot(std::string &x) : s(&x) {}
  void put(double v) const { if (d) *d = v; else if (i) *i = (int)v; else *b = v != 0; }
};
struct Opt {
  const char *name;
  OptKind kind;
  Slot (*at)(blomgpu_ctx *);          // nullptr: the value is checked and nothing is stored
  unsigned flags;
  const char *(*check)(double &v);    // clamps or scales v, or returns the refusal
  void (*after)(blomgpu_ctx *);       // what else follows from the new value
  // O_STR: what the refusal says in front of the value, and the accepted words with their codes (none: the string itself is stored)
  const char *refuse;
  struct { const char *word; int code; } words[5];
};
#define IN_P(m) [](blomgpu_ctx *c) { return Slot(c->h.P.m); }
#define IN_C(m) [](blomgpu_ctx *c) { return Slot(c->m); }
#define PR(nm) {#nm, O_REAL, IN_P(nm), DIRTY}
#define PRR(nm) {#nm, O_REAL, IN_P(nm), DIRTY | READABLE}
#define PI(nm) {#nm, O_INT, IN_P(nm), DIRTY}
#define CR(nm) {#nm, O_REAL, IN_C(nm), 0}
#define CI(nm) {#nm, O_INT, IN_C(nm), 0}
#define CB(nm) {#nm, O_BOOL, IN_C(nm), 0}
#define ONE_OR_TWO(msg) [](double &v) -> const char * { return v != 1 && v != 2 ? msg : nullptr; }
// (a declared context allocates the option's 48-level array when the option is switched on, outside the step: stage_thermf_cesm.hip)
#define RLX(nm, fid) {#nm, O_BOOL, IN_C(nm), 0, nullptr, [](blomgpu_ctx *c) { if (c->nm && frc_declared(c)) (void)cesm_field(c, fid); }}
#define LMI(n) {"l" #n "mi", O_INT, [](blomgpu_ctx *c) { return Slot(c->lmi[n - 1]); }, 0, \
                [](double &v) -> const char * { return v < 1 || v > 12 ? "blomgpu_set_int: l" #n "mi is a month, 1..12" : nullptr; }}
static const Opt g_opts[] = {
  // ---- reals ----
  PRR(baclin), PRR(batrop), PRR(delt1), PRR(dlt), PR(mdv2hi), PR(mdv2lo), PR(mdv4hi), PR(mdv4lo), PR(mdc2hi), PR(mdc2lo),
  PR(vsc2hi), PR(vsc2lo), PR(vsc4hi), PR(vsc4lo), PR(cbar), PR(cb), PR(cwbdts), PR(cwbdls), PR(wuv1), PR(wuv2), PR(wts1), PR(wts2),
  PRR(wbaro), PR(bdmc1), PR(bdmc2), PR(iwdfac), PR(nubmin), PR(vland),
  {"pref", O_REAL, IN_P(pref), DIRTY | READABLE, nullptr, [](blomgpu_ctx *c) { set_eos(c->h.P); }},
  CR(swamxd), CR(brine_mlbase_frac),                      // phy/mod_swabs.F90:179-183, phy/mod_forcing.F90:63
  // &DIFFUSION, as far as phy/mod_difest.F90's isopycnic routines read it (phy/mod_diffusion.F90:45-110)
  CR(egc), CR(eggam), CR(eglsmn), CR(egmndf), CR(egmxdf), CR(egidfq), CR(rhiscf), CR(ri0), CR(tkepf),
  {"bdml_logc", O_REAL, IN_C(bdml_logc), READABLE},
  // thermf: mod_forcing's namelist variables, mod_grid's area, mod_time's interpolation weight of the month
  CR(trxday), CR(srxday), CR(trxdpt), CR(srxdpt), CR(trxlim), CR(srxlim), CR(sref), {"area", O_REAL, IN_C(area), READABLE}, CR(xmi),
  // mod_mxlayr's and mod_niw's namelist variables (phy/mod_mxlayr.F90:58-68, phy/mod_niw.F90:38-45)
  CR(rm0), CR(rm5), CR(niwgf), CR(niwbf), CR(niwlf),
  // mixed layer restratification of eddtra_ale, phy/mod_eddtra.F90:53-94
  {"ce", O_REAL, IN_C(eddtra_ce), 0}, {"cl", O_REAL, IN_C(eddtra_cl), 0}, CR(tau_mlr), CR(tau_growing_hbl), CR(tau_decaying_hbl),
  CR(tau_growing_hml), CR(tau_decaying_hml), CR(lfmin), CR(mstar), CR(nstar), CR(wpup_min), CR(mlbl_max_ratio),
  CR(ale_regrid_nudge_ts), CR(ale_stab_fac_limit), CR(ale_dpvar_fac), CR(ale_smooth_diff_max),
  {"ale_dpmin_interior", O_REAL, IN_C(ale_dpmin_interior), 0,                        // [m], as in &ALE_REGRID_REMAP (:1352-1353)
   [](double &v) -> const char * { v = v * ONEM; return nullptr; }},
  // ---- integers ----
  {"nstep", O_INT, IN_P(nstep), 0},                       // host-side only (stage_cppm.hip): the device view is not touched
  PI(lstep), PI(nday_in_year), PI(itriag), PI(itrtke), PI(itrgls), PI(tkeadv), PI(tkeidf), PI(gls), PI(vcoord_tag), PI(ltedtp_opt),
  PI(bdmtyp), PI(iwdflg), PI(bdmldp), PI(allwet),
  CB(csdiag), CB(eddf2d), CB(edsprs), CB(edanis), CB(redi3d), CB(edfsmo), CB(rhsctp), CB(difest_live),
  {"edritp_opt", O_INT, IN_C(edritp_opt), 0, ONE_OR_TWO(" readnml_diffusion: edritp is unsupported!")},   // phy/mod_diffusion.F90:113-116
  {"edwmth_opt", O_INT, IN_C(edwmth_opt), 0, ONE_OR_TWO(" readnml_diffusion: edwmth is unsupported!")},
  {"full_physics", O_BOOL, IN_C(full_physics), 0, nullptr, [](blomgpu_ctx *c) { if (c->full_physics) c->live_slopes = true; }},
  // thermf: mod_forcing's switches (phy/mod_forcing.F90:43-47), mod_time's months of the interpolation, mod_ben02's ntda
  RLX(aptflx, F_tflxap), RLX(apsflx, F_sflxap), RLX(ditflx, F_tflxdi), RLX(disflx, F_sflxdi), CB(srxbal), LMI(1), LMI(2), LMI(3), LMI(4), LMI(5), CI(ntda),
  // (the stage timers select nothing: a step with them runs plain launches beside the graphs, which stay)
  {"timing", O_BOOL, IN_C(timing), KEEP_GRAPHS},
  CI(barotp_fused),
  {"barotp_tile", O_INT, IN_C(barotp_tile), 0, [](double &v) -> const char * {
     if (v == 0) return nullptr;
     for (const BtShape &s : kBtShapes) if (v == 100 * s.ti + s.tj) return nullptr;
     return "blomgpu_set_int: barotp_tile must be 0, 3216, 3208, 1608, 4016, 2616, 2615 or 4015"; }},
  CI(barotp_persist), CI(barotp_block), CI(barotp_overlap), CI(barotp_rimbuf), CI(barotp_arctic_fused), CI(barotp_arctic_persist),
  CI(eddtra_frozen), CI(pgf_uv_pair), CI(pgf_uv_ring), CI(pgf_reuse), CI(pgf_copy_fused), CI(kprof_sel), CI(mom_aw_split),
  CI(mom_force_aw), CI(convec_nsingle), CI(cmn_nslope_nb), CI(scan_reassoc),
  {"check_period", O_INT, IN_C(check_period), 0, [](double &v) -> const char * { if (v < 1) v = 1; return nullptr; }},
  CI(cnsvdi), CI(arctic_strips), CI(use_graph), CI(overlap), CI(phys_dag), CI(mom_early_at), CI(lean_fluxes), CI(tmsmt_fold),
  CI(tmsmt_ahead), CI(remap_fold), CI(remap_nfirst), CI(halo_overlap), CI(cmnfld1), CI(diapfl_du), CI(live_slopes),
  CI(momtum_bs), CI(momtum_lds_pad), CI(momtum_order), CI(momtum_chunks_a), CI(momtum_chunks_b), CI(diffus_shfl),
  {"ale_upper_bndr_ord", O_INT, IN_C(ale_upper_bndr_ord), ALE_RESET}, {"ale_lower_bndr_ord", O_INT, IN_C(ale_lower_bndr_ord), ALE_RESET},
  CI(ale_k_range_plevel), CI(ale_dktzu), CI(ale_dktzl),
  {"ale_density_pc_upper_bndr", O_BOOL, IN_C(ale_density_pc_upper), ALE_RESET},
  {"ale_density_pc_lower_bndr", O_BOOL, IN_C(ale_density_pc_lower), ALE_RESET},
  {"ale_tracer_pc_upper_bndr", O_BOOL, IN_C(ale_tracer_pc_upper), ALE_RESET},
  {"ale_tracer_pc_lower_bndr", O_BOOL, IN_C(ale_tracer_pc_lower), ALE_RESET},
  {"ale_velocity_pc_upper_bndr", O_BOOL, IN_C(ale_velocity_pc_upper), ALE_RESET},
  {"ale_velocity_pc_lower_bndr", O_BOOL, IN_C(ale_velocity_pc_lower), ALE_RESET},
  CB(ndiff_surface_align),
  {"ndiff_rec_per_face", O_INT, IN_C(ndiff_rec_per_face), ALE_RESET, [](double &v) -> const char * { if (v < 0) v = 0; return nullptr; }},
  // ---- strings: the reference's words, refused in the reference's words (blomgpu_set_str marks the view dirty for every name) ----
  {"expcnf", O_STR, IN_C(expcnf), 0},
  {"mlrttp", O_STR, IN_C(mlrttp), 0},                     // resolved (and refused) in mxlayr, phy/mod_mxlayr.F90:197-212
  {"mommth", O_STR, IN_P(mommth), DIRTY, nullptr, nullptr, " mommth = ", {{"enscon", 0}, {"enecon", 1}, {"enedis", 2}}},   // phy/mod_momtum.F90:815-820
  {"pgfmth", O_STR, IN_P(pgfmth), DIRTY, nullptr, nullptr, " pgfmth = ", {{"geopotential", 0}, {"dynamic enthalpy", 1}}},   // phy/mod_pgforc.F90:529-534
  {"advmth", O_STR, IN_P(advmth), DIRTY, nullptr, nullptr, " advmth = ", {{"remap", 0}, {"cppm", 1}}},                      // phy/mod_advect.F90:166-171
  {"bmcmth", O_STR, IN_P(bmcmth), DIRTY, nullptr, nullptr, " bmcmth = ", {{"uc", 0}, {"dluc", 1}}},                         // phy/mod_pbcor.F90:112-117
  {"eitmth", O_STR, IN_P(eitmth), DIRTY, nullptr, nullptr, " eitmth = ", {{"intdif", 1}, {"gm", 2}}},                       // phy/mod_diffusion.F90:316-327
  {"cppm_compatibility", O_STR, IN_C(cppm_compat), 0, nullptr, nullptr, " init_cppm: cppm_compatibility = ", {{"full", 1}, {"partial", 2}}},        // phy/mod_cppm.F90:2524-2535
  {"cppm_limiting", O_STR, IN_C(cppm_limiting), 0, nullptr, nullptr, " init_cppm: cppm_limiting = ", {{"monotonic", 1}, {"non_oscillatory", 2}}},   // phy/mod_cppm.F90:2536-2548
  // init_eddtra, phy/mod_eddtra.F90:1773-1806 (bod23: refused with isopyc_bulkml when the stage runs, :1787-1795)
  {"mlrmth", O_STR, IN_C(mlrmth), 0, nullptr, nullptr, " init_eddtra: mlrmth = ", {{"none", 0}, {"fox08", 1}, {"bod23", 2}}},
  {"vcoord_type", O_STR, IN_P(vcoord_tag), DIRTY, nullptr, nullptr, " readnml_vcoord: vcoord_type = ",                      // phy/mod_vcoord.F90:908-921
   {{"isopyc_bulkml", 1}, {"cntiso_hybrid", 2}, {"plevel", 3}}},
  // &ALE_REGRID_REMAP, phy/mod_ale_regrid_remap.F90:1185-1355 (readnml_ale_regrid_remap; same words, same refusals)
  {"ale_reconstruction_method", O_STR, IN_C(ale_method), 0, nullptr, nullptr, " readnml_ale_regrid_remap: reconstruction_method = ",
   {{"plm", 101}, {"ppm", 102}, {"pqm", 103}}},
  {"ale_regrid_method", O_STR, IN_C(ale_regrid_method), 0, nullptr, nullptr, " readnml_ale_regrid_remap: regrid_method = ", {{"direct", 1}, {"nudge", 2}}},   // :1323-1337
  {"ale_density_limiting", O_STR, nullptr, 0, nullptr, nullptr, " readnml_ale_regrid_remap: density_limiting = ", {{"monotonic", 0}}},
  // (the cached reconstruction structures hold the limiter)
  {"ale_tracer_limiting", O_STR, IN_C(ale_tracer_limiting), ALE_RESET, nullptr, nullptr, " readnml_ale_regrid_remap: tracer_limiting = ",
   {{"monotonic", 201}, {"non_oscillatory", 203}}},
  {"ale_velocity_limiting", O_STR, IN_C(ale_velocity_limiting), ALE_RESET, nullptr, nullptr, " readnml_ale_regrid_remap: velocity_limiting = ",
   {{"monotonic", 201}, {"non_oscillatory", 203}}},
};
// The coupled experiment's options (stage_thermf_cesm.hip), a table of their own behind the same setters: mod_cesm's smtfrc, nstep_in_cpl,
// l1ci, l2ci (cesm/mod_cesm.F90:55-103), mod_forcing's use_stream_relaxation, mod_time's nstep_in_day and nday_of_year (nstep and
// nday_in_year stand in the table above), and the A/B switch of thermf_cesm's sums.  blomgpu_option_name lists the table above only:
// its rows are pinned name by name (tests/test_option_table.py), and these names mean nothing until blomgpu_inifrc_cesm has been called.
// The forced ocean-ice experiment (stage_thermf_ben02.hip) needs nstep_in_day and nday_of_year of these, and none of its own.
static const Opt g_cesm_opts[] = {
  CB(smtfrc), CB(use_stream_relaxation), CI(nstep_in_cpl), CI(l1ci), CI(l2ci), CI(nstep_in_day), CI(nday_of_year), CI(cesm_single_sums),
};
// The end of blom_step (stage_stepend.hip), likewise a table of its own that blomgpu_option_name does not list: the clock (step_time),
// mod_swabs' swamth, jwtype, chlopt (phy/mod_swabs.F90:92-94; refused in iniswa's words), mod_forcing's sprfac and prfac
// (phy/mod_forcing.F90:48, :115), and chkvar.  A new swamth wants blomgpu_iniswa again; sprfac = 1 does what inivar_forcing does for it.
static const Opt g_stepend_opts[] = {
  CB(step_time), CB(chkvar), CI(jwtype), {"chlopt", O_STR, IN_C(chlopt), 0},
  {"swamth", O_STR, IN_C(swamth), 0, nullptr, nullptr, " iniswa: swamth = ",                               // phy/mod_swabs.F90:601-606
   {{"top-layer", SWA_TOP_LAYER}, {"jerlov", SWA_JERLOV}, {"chlorophyll_ma94", SWA_MA94}, {"chlorophyll_ohl03", SWA_OHL03}, {"spatial_frac_attlen", SWA_SPATIAL}}},
  {"sprfac", O_BOOL, IN_C(sprfac), 0, nullptr, [](blomgpu_ctx *c) { (void)stepend_set_sprfac(c); }},
  {"prfac", O_REAL, IN_C(prfac), READABLE},
};
// mod_budget inside blomgpu_step (stage_budget.hip), likewise unlisted: with cnsvdi = 1 (the listed table's) the step runs budget_sums'
// seven calls and budget_output's sums where blom_step has them and keeps a record per step
static const Opt g_budget_opts[] = {
  CI(budget_step),
};
// blomgpu_dia_reduce's section kernel (stage_diaout.hip), likewise unlisted: the entries of a section a pass takes and the levels a
// chunk stages, so that a small grid can cross both boundaries
static const Opt g_diaout_opts[] = {
  {"diaout_entries", O_INT, IN_C(diaout_entries), KEEP_GRAPHS, [](double &v) -> const char * {
     return v < 1 || v > 256 ? "blomgpu_set_int: diaout_entries is 1..256" : nullptr; }},
  {"diaout_levels", O_INT, IN_C(diaout_levels), KEEP_GRAPHS, [](double &v) -> const char * {
     return v < 1 || v > 8 ? "blomgpu_set_int: diaout_levels is 1..8" : nullptr; }},
};
#undef IN_P
#undef IN_C
#undef PR
#undef PRR
#undef PI
#undef CR
#undef CI
#undef CB
#undef ONE_OR_TWO
#undef LMI
#undef RLX
static const Opt *find_opt(std::string_view name, unsigned kinds) {      // kinds: bit per OptKind
  for (const Opt &o : g_opts)
    if (name == o.name && (kinds >> o.kind & 1)) return &o;
  for (const Opt &o : g_cesm_opts)
    if (name == o.name && (kinds >> o.kind & 1)) return &o;
  for (const Opt &o : g_stepend_opts)
    if (name == o.name && (kinds >> o.kind & 1)) return &o;
  for (const Opt &o : g_budget_opts)
    if (name == o.name && (kinds >> o.kind & 1)) return &o;
  for (const Opt &o : g_diaout_opts)
    if (name == o.name && (kinds >> o.kind & 1)) return &o;
  return nullptr;
}
// what the three setters share; `who` is the entry point's name in the messages
static int opt_lookup(blomgpu_ctx *c, const char *who, const char *name, unsigned kinds, const Opt **o) {
  if (!c || !name) return ctx_fail(c, std::string(who) + ": null argument");
  *o = find_opt(name, kinds);
  if (!*o || !((*o)->flags & KEEP_GRAPHS)) ctx_drop_graphs(c);
  return *o ? 0 : ctx_fail(c, std::string(who) + ": unknown option " + name);
}
static int set_number(blomgpu_ctx *c, const char *who, const char *name, unsigned kinds, double v) {
  const Opt *o;
  if (int rc = opt_lookup(c, who, name, kinds, &o)) return rc;
  if (o->kind == O_BOOL) v = v != 0;
  if (o->check)
    if (const char *refusal = o->check(v)) return ctx_fail(c, refusal);
  o->at(c).put(v);
  if (o->flags & DIRTY) c->dirty = true;
  if (o->after) o->after(c);
  return o->flags & ALE_RESET ? ale_reset(c) : 0;
}

// a (and b, unless nullptr) to the device, launch(grid, a, b, z) on the context's stream, z back
template <class Launch>
static int libm_probe(blomgpu_ctx *c, int n, const double *a, const double *b, double *z, const char *who, Launch launch) {
  if (n <= 0) return 0;
  double *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, sizeof(double) * 3 * (size_t)n));
  int rc = 0;
  if (hipMemcpyAsync(d, a, sizeof(double) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = 1;
  if (b && hipMemcpyAsync(d + n, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = 1;
  launch(dim3((n + 255) / 256), d, d + n, d + 2 * (size_t)n);
  if (hipMemcpyAsync(z, d + 2 * (size_t)n, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = 1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = 1;
  (void)hipFree(d);
  return rc ? ctx_fail(c, std::string(who) + ": copy or launch failed") : 0;
}

extern "C" {

const char *blomgpu_last_error(const blomgpu_ctx *ctx) {
  return ctx ? ctx->err.c_str() : g_err.c_str();
}

int blomgpu_create(const blomgpu_dims *d, blomgpu_ctx **out) {
  if (!d || !out) return ctx_fail(nullptr, "blomgpu_create: null argument");
  if (d->nbdy != NBDY) return ctx_fail(nullptr, "blomgpu_create: nbdy must be 4 (phy/mod_xc.F90:45)");
  if (d->idm < 1 || d->jdm < 1 || d->kdm < 3 || d->ntr < 0)
    return ctx_fail(nullptr, "blomgpu_create: bad dimensions");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return ctx_fail(nullptr, "blomgpu_create: no HIP device -- libblomgpu has no host fallback");
  if (d->device < 0 || d->device >= ndev) return ctx_fail(nullptr, "blomgpu_create: bad device ordinal");
  blomgpu_ctx *c = new blomgpu_ctx();
  c->device = d->device;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  DevView &h = c->h;
  memset(&h, 0, sizeof(h));
  h.ii = d->idm; h.jj = d->jdm; h.kk = d->kdm;
  h.ni = d->idm + 2 * NBDY; h.nj = d->jdm + 2 * NBDY; h.nplane = h.ni * h.nj;
  h.itdm = d->itdm; h.jtdm = d->jtdm; h.i0 = d->i0; h.j0 = d->j0; h.nreg = d->nreg; h.ntr = d->ntr;
  Params &P = h.P;
  // defaults of the reference's module variables (phy/mod_tmsmt.F90:46-51)
  P.wuv1 = .75; P.wuv2 = .125; P.wts1 = .875; P.wts2 = .0625; P.wbaro = .125;
  P.vland = 0.0; P.allwet = 1; P.vcoord_tag = 1; P.ltedtp_opt = 1; P.eitmth = 2;
  P.pref = 2000.e4;
  set_eos(P);
  const int K = d->kdm, NT = d->ntr > 0 ? d->ntr : 1;
  int id = 0;
#define X(name, lev)                                                                   \
  c->nlev_real[id] = (lev);                                                            \
  c->real_ids[#name] = id;                                                             \
  id++;
  BLOM_REAL_FIELDS(X)
#undef X
  // (the coupled experiment's fields: level counts only -- no name and no memory until blomgpu_inifrc_cesm)
#define X(name, lev) c->nlev_real[id++] = (lev);
  BLOM_CESM_REAL_FIELDS(X)
#undef X
  id = 0;
#define X(name, lev)                                                                   \
  c->nlev_int[id] = (lev);                                                             \
  c->int_ids[#name] = id;                                                              \
  id++;
  BLOM_INT_FIELDS(X)
#undef X
#define X(name, lev) c->nlev_int[id++] = (lev);
  BLOM_CESM_INT_FIELDS(X)
#undef X
  for (int f = 0; f < NF_BASE_REAL; f++) {
    size_t bytes = sizeof(double) * (size_t)c->nlev_real[f] * h.nplane;
    HIPCHK(c, hipMalloc((void **)&h.f[f], bytes));
    HIPCHK(c, hipMemsetAsync(h.f[f], 0, bytes, c->stream));
  }
  for (int f = 0; f < NF_BASE_INT; f++) {
    size_t bytes = sizeof(int) * (size_t)c->nlev_int[f] * h.nplane;
    HIPCHK(c, hipMalloc((void **)&h.m[f], bytes));
    HIPCHK(c, hipMemsetAsync(h.m[f], 0, bytes, c->stream));
  }
  h.nwk = wk_slots(d->ntr);
  HIPCHK(c, hipMalloc((void **)&h.wk, sizeof(double) * (size_t)h.nwk * K * h.nplane));
  HIPCHK(c, hipMemsetAsync(h.wk, 0, sizeof(double) * (size_t)h.nwk * K * h.nplane, c->stream));
  HIPCHK(c, hipMalloc((void **)&h.wk2d, sizeof(double) * (size_t)NWK2D * h.nplane));
  HIPCHK(c, hipMemsetAsync(h.wk2d, 0, sizeof(double) * (size_t)NWK2D * h.nplane, c->stream));
  HIPCHK(c, hipMalloc((void **)&c->d, sizeof(DevView)));
  // momtum's own work space and interface pressures + the second stream (blomgpu_internal.h: blomgpu_ctx::overlap)
  HIPCHK(c, hipMalloc((void **)&c->wk_mom, sizeof(double) * (size_t)MF_NSLOT * K * h.nplane));
  HIPCHK(c, hipMemsetAsync(c->wk_mom, 0, sizeof(double) * (size_t)MF_NSLOT * K * h.nplane, c->stream));
  for (double **pp : {&c->p_alt, &c->pu_alt, &c->pv_alt}) {
    HIPCHK(c, hipMalloc((void **)pp, sizeof(double) * (size_t)(K + 1) * h.nplane));
    HIPCHK(c, hipMemsetAsync(*pp, 0, sizeof(double) * (size_t)(K + 1) * h.nplane, c->stream));
  }
  for (int v = 1; v < NVIEW; v++) HIPCHK(c, hipMalloc((void **)&c->dv[v], sizeof(DevView)));
  HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
  for (auto &e : c->ev_side) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  c->dirty = true;
  ctx_sync_view(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  *out = c;
  // A/B aid: BLOMGPU_OPTS="name=int,name=int" sets kernel-variant options on every context of the process (so that a whole
  // test suite or bench run can be repeated with a variant: `BLOMGPU_OPTS=pgf_uv_ring=0 pytest -m gpu ...`); unknown names fail loudly
  if (const char *env = getenv("BLOMGPU_OPTS")) {
    std::string e(env);
    size_t pos = 0;
    while (pos < e.size()) {
      size_t end = e.find(',', pos);
      if (end == std::string::npos) end = e.size();
      const std::string item = e.substr(pos, end - pos);
      const size_t eq = item.find('=');
      if (eq != std::string::npos)
        if (int rc = blomgpu_set_int(c, item.substr(0, eq).c_str(), atoi(item.substr(eq + 1).c_str()))) return rc;
      pos = end + 1;
    }
  }
  return 0;
}

int blomgpu_destroy(blomgpu_ctx *c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  if (!c->stream_borrowed) (void)hipStreamSynchronize(c->stream);
  ctx_drop_graphs(c);
  for (int f = 0; f < NF_REAL; f++) (void)hipFree(c->h.f[f]);
  for (int f = 0; f < NF_INT; f++) (void)hipFree(c->h.m[f]);
  (void)hipFree(c->h.wk);
  (void)hipFree(c->h.wk2d);
  (void)hipFree(c->d);
  if (c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
  for (auto &e : c->ev_side) if (e) (void)hipEventDestroy(e);
  for (int v = 1; v < NVIEW; v++) if (c->dv[v]) (void)hipFree(c->dv[v]);
  if (c->mom_aw_dev) (void)hipFree(c->mom_aw_dev);
  if (c->side3) { (void)hipStreamSynchronize(c->side3); (void)hipStreamDestroy(c->side3); }
  for (auto &e : c->ev_side3) if (e) (void)hipEventDestroy(e);
  (void)hipFree(c->wk_mom); (void)hipFree(c->p_alt); (void)hipFree(c->pu_alt); (void)hipFree(c->pv_alt);
  if (c->tiling.rccl) (void)blomgpu_rccl_finalize(c);
  if (c->err_dev) (void)hipFree(c->err_dev);
  if (c->bt_flags) (void)hipFree(c->bt_flags);
  ale_free(c);
  dia_free(c);
  diaout_free(c);
  cesm_free(c);
  ben02_free(c);
  stepend_free(c);
  budget_free(c);
  if (c->ale_plevel) (void)hipFree(c->ale_plevel);
  if (c->arc_strip) (void)hipFree(c->arc_strip);
  if (c->xcsum_buf) (void)hipFree(c->xcsum_buf);
  if (c->xstream) (void)hipStreamDestroy(c->xstream);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (!c->stream_borrowed) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int blomgpu_sync(blomgpu_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->side) HIPCHK(c, hipStreamSynchronize(c->side));
  return 0;
}

int blomgpu_set_real(blomgpu_ctx *c, const char *name, double v) { return set_number(c, "blomgpu_set_real", name, 1u << O_REAL, v); }
int blomgpu_set_int(blomgpu_ctx *c, const char *name, int v) { return set_number(c, "blomgpu_set_int", name, 1u << O_INT | 1u << O_BOOL, v); }

int blomgpu_set_str(blomgpu_ctx *c, const char *name, const char *val) {
  const Opt *o = nullptr;
  const int rc = opt_lookup(c, "blomgpu_set_str", name, 1u << O_STR, &o);
  if (c) c->dirty = true;              // for every name it is called with, known or not
  if (rc) return rc;
  if (!val) return ctx_fail(c, "blomgpu_set_str: null argument");
  const std::string v(val);
  if (!o->words[0].word) { *o->at(c).s = v; return 0; }
  for (const auto &w : o->words)
    if (w.word && v == w.word) {
      if (o->at) o->at(c).put(w.code);
      if (o->at && o->at(c).i == &c->swamth) c->swa_ready = false;      // (blomgpu_iniswa once more)
      return o->flags & ALE_RESET ? ale_reset(c) : 0;
    }
  return ctx_fail(c, o->refuse + v + " is unsupported!");
}

int blomgpu_get_real(blomgpu_ctx *c, const char *name, double *v) {
  const std::string s(name);
  if (const Opt *o = find_opt(s, 1u << O_REAL))
    if (o->flags & READABLE) { *v = *o->at(c).d; return 0; }
  // which form of the barotropic substep kernel this context runs with its present options: 1 four substeps per hand-off
  // (k_bt_steps4, persistent), 2 the same kernel with a launch per four substeps, 0 the forms of stage_barotp_pair.hip's head
  if (s == "barotp_block_mode") { *v = bt_block_mode(c); return 0; }
  // ... and with which tile shape, 100 * ti + tj: a test that means to reach one instantiation of the kernel asserts both
  if (s == "barotp_shape") { *v = bt_shape_code(c); return 0; }
  // how many steps of this context blomgpu_step has replayed as HIP graphs / how many captures failed (a capture that fails leaves the
  // sequence on plain launches: correct, and a few per cent slower -- a caller that times steps wants to know)
  if (s == "graph_steps") { *v = c->graph_steps; return 0; }
  if (s == "graph_failures") { *v = c->graph_failures; return 0; }
  // how many steps blomgpu_step has run without keeping the heat and salt flux diagnostics current (flux_diag: all but the last two of a call)
  if (s == "flux_diag_steps_skipped") { *v = (double)c->flux_diag_skipped; return 0; }
  // thermf_cesm's correction of the virtual salt flux (cesm/mod_thermf_cesm.F90:342-343), from the sum the last thermf left on the device
  if (s == "thermf_cesm_launches") { *v = (double)c->cesm_launches; return 0; }      // (counted where they are issued, single tile)
  if (s == "thermf_ben02_launches") { *v = c->ben02_declared ? (double)c->cesm_launches : 0.; return 0; }   // (the same counter: one family a context)
  // the clock, while blomgpu_step keeps it (step_time = 1; stage_stepend.hip): what the last step's step_time left where the setters write
  if (c->step_time) {
    if (s == "xmi") { *v = c->xmi; return 0; }
    if (s == "nday_of_year") { *v = c->nday_of_year; return 0; }
    if (s.size() == 4 && s[0] == 'l' && s[1] >= '1' && s[1] <= '5' && s.compare(2, 2, "mi") == 0) { *v = c->lmi[s[1] - '1']; return 0; }
  }
  if (s == "sflxc") {
    if (!frc_declared(c)) return ctx_fail(c, "blomgpu_get_real: sflxc exists once blomgpu_inifrc_cesm has been called");
    double sum = 0.;
    HIPCHK(c, hipMemcpyAsync(&sum, c->cesm_sums, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *v = sum / c->area;
    return 0;
  }
  // diagnostic counters of mxlayr (stage_mxlayr.hip): columns whose iteration for the mixed layer depth ended at its limit since the last
  // query, named by the message the reference prints for such a column: "mxlayr_maxitr_detrain" = the first iteration
  // (phy/mod_mxlayr.F90:437-449, 'reached maxitr when detraining', :440; word 5), "mxlayr_maxitr_entrain" = the second
  // (:947-982, 'reached maxitr when entraining', :950; word 6).  (Until round 5 the two names were swapped.)
  if (s == "mxlayr_maxitr_entrain" || s == "mxlayr_maxitr_detrain") {
    *v = 0.;
    if (!c->err_dev) return 0;
    const int w = s == "mxlayr_maxitr_detrain" ? 5 : 6;
    int n = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&n, c->err_dev + w, sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemset(c->err_dev + w, 0, sizeof(int)));
    *v = n;
    return 0;
  }
  return ctx_fail(c, "blomgpu_get_real: unknown option " + s);
}

// the names of the option table in its order, with the entry point that sets each: kind 0 blomgpu_set_real, 1 blomgpu_set_int,
// 2 blomgpu_set_int (stored as v != 0), 3 blomgpu_set_str; non-zero past the end
int blomgpu_option_name(int index, char *buf, int cap, int *kind) {
  if (index < 0 || index >= (int)(sizeof(g_opts) / sizeof(g_opts[0])) || !buf || cap < 2) return 1;
  snprintf(buf, cap, "%s", g_opts[index].name);
  if (kind) *kind = g_opts[index].kind;
  return 0;
}

int blomgpu_field_info(blomgpu_ctx *c, const char *name, int *nlev, int *is_int) {
  auto it = c->real_ids.find(name);
  if (it != c->real_ids.end()) {
    *nlev = ctx_real_nlev(c, it->second);
    if (std::string(name) == "trc" || std::string(name) == "trcold")
      *nlev = c->h.ntr * (std::string(name) == "trc" ? 2 : 1) * c->h.kk;
    *is_int = 0;
    return 0;
  }
  auto jt = c->int_ids.find(name);
  if (jt != c->int_ids.end()) { *nlev = c->nlev_int[jt->second]; *is_int = 1; return 0; }
  return ctx_fail(c, std::string("unknown field ") + name);
}

// The device pointer of level lev0 (1-based) of a named real field, nlev levels of which must exist -- the one place where the entry points
// that take a field by name resolve it.  A 48-level array of the coupled experiment that has no memory yet gets it here (cesm_field).
static int real_levels(blomgpu_ctx *c, const char *who, const char *name, int lev0, int nlev, double **ptr) {
  if (!c || !name) return ctx_fail(c, std::string(who) + ": null argument");
  auto it = c->real_ids.find(name);
  if (it == c->real_ids.end()) return ctx_fail(c, std::string(who) + ": unknown field " + name);
  if (lev0 < 1 || nlev < 1 || lev0 - 1 + nlev > ctx_real_nlev(c, it->second))
    return ctx_fail(c, std::string(who) + ": levels out of range for field " + name + " (lev0 is 1-based)");
  if (int rc = cesm_field(c, it->second)) return rc;
  if (!ctx_real_ptr(c, it->second)) return ctx_fail(c, std::string(who) + ": field " + name + " has no memory");
  *ptr = ctx_real_ptr(c, it->second) + (size_t)(lev0 - 1) * c->h.nplane;
  return 0;
}

static int locate(blomgpu_ctx *c, const char *name, int nlev, void **ptr, size_t *bytes) {
  int nl, isint;
  if (blomgpu_field_info(c, name, &nl, &isint)) return 1;
  if (nlev < 1 || nlev > nl) return ctx_fail(c, std::string("bad level count for field ") + name);
  if (isint) {
    *ptr = c->h.m[c->int_ids[name]];
    *bytes = sizeof(int) * (size_t)nlev * c->h.nplane;
  } else {
    if (int rc = cesm_field(c, c->real_ids[name])) return rc;      // (a 48-level array of the coupled experiment, on first use)
    *ptr = ctx_real_ptr(c, c->real_ids[name]);
    *bytes = sizeof(double) * (size_t)nlev * c->h.nplane;
  }
  return 0;
}

int blomgpu_upload(blomgpu_ctx *c, const char *name, const void *host, int nlev) {
  void *p; size_t bytes;
  if (locate(c, name, nlev, &p, &bytes)) return 1;
  HIPCHK(c, hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const std::string s(name);
  if (s == "ip" || s == "iu" || s == "iv" || s == "iq") return ctx_pack_masks(c);
  return 0;
}

// one level (1-based) of a real field from a host plane: a coupling interval refreshes level l2ci of the _da pairs alone
int blomgpu_upload_level(blomgpu_ctx *c, const char *name, const void *host, int lev) {
  if (!host) return ctx_fail(c, "blomgpu_upload_level: null argument");
  double *base = nullptr;
  if (int rc = real_levels(c, "blomgpu_upload_level", name, lev, 1, &base)) return rc;
  HIPCHK(c, hipMemcpyAsync(base, host, sizeof(double) * (size_t)c->h.nplane, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int blomgpu_download(blomgpu_ctx *c, const char *name, void *host, int nlev) {
  void *p; size_t bytes;
  if (locate(c, name, nlev, &p, &bytes)) return 1;
  HIPCHK(c, hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int blomgpu_set_masks(blomgpu_ctx *c, const int *ip, const int *iu, const int *iv, const int *iq) {
  if (c) ctx_drop_graphs(c);
  return blomgpu_upload(c, "ip", ip, 1) || blomgpu_upload(c, "iu", iu, 1) ||
         blomgpu_upload(c, "iv", iv, 1) || blomgpu_upload(c, "iq", iq, 1);
}

int blomgpu_xctilr(blomgpu_ctx *c, const char *name, int lev0, int l1, int ld, int mh, int nh, int itype) {
  if (l1 < 1) return ctx_fail(c, "xctilr: level range outside field");
  double *base = nullptr;
  if (int rc = real_levels(c, "xctilr", name, lev0, ld, &base)) return rc;
  ctx_sync_view(c);
  return st_xctilr(c, base, l1, ld, mh, nh, itype);
}

int blomgpu_crc(blomgpu_ctx *c, const char *name, int lev0, int nlev, int itype, unsigned *crc) {
  double *base = nullptr;
  if (int rc = real_levels(c, "crc", name, lev0, nlev, &base)) return rc;
  ctx_sync_view(c);
  return st_crc(c, base, nlev, itype, crc);
}

int blomgpu_crc_strips(blomgpu_ctx *c, const char *name, int lev0, int nlev, int itype, unsigned *out, int cap, int *l0, int *ns) {
  double *base = nullptr;
  if (int rc = real_levels(c, "crc_strips", name, lev0, nlev, &base)) return rc;
  ctx_sync_view(c);
  return st_crc_strips(c, base, nlev, itype, out, cap, l0, ns);
}

// names of the registered fields, in registry order (reals first): lets a host scatter a whole state over tiles
int blomgpu_field_name(blomgpu_ctx *c, int index, char *buf, int cap) {
  const int nr = (int)c->real_ids.size(), ni = (int)c->int_ids.size();
  if (index < 0 || index >= nr + ni || cap < 2) return 1;
  const auto &m = index < nr ? c->real_ids : c->int_ids;
  // the index-th name in the order of the ids (which have gaps once blomgpu_inifrc_ben02 has named a part of the forcing lists)
  std::vector<std::pair<int, const std::string *>> byid;
  for (const auto &kv : m) byid.emplace_back(kv.second, &kv.first);
  std::sort(byid.begin(), byid.end());
  snprintf(buf, cap, "%s", byid[index < nr ? index : index - nr].second->c_str());
  return 0;
}

// settings of the reference's compile-time tracer switches that this library does not carry
static int check_tracer_options(blomgpu_ctx *c) {
  const Params &P = c->h.P;
  if (P.itrtke >= 1 && !P.tkeadv && P.advmth == 1)
    return ctx_fail(c, "cppm advects every tracer (phy/mod_cppm.F90 has no TKEADV switch): tkeadv = 0 only with advmth = 'remap'");
  if (P.itrtke >= 1 && (P.itrtke > c->h.ntr || P.itrgls > c->h.ntr || P.itrgls < 1))
    return ctx_fail(c, "itrtke / itrgls outside 1..ntr");
  return 0;
}
#define STAGE6(nm)                                                                         \
  int blomgpu_##nm(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {       \
    if (int rc = check_tracer_options(c)) return rc;                                       \
    ctx_sync_view(c);                                                                      \
    return st_##nm(c, m, n, mm, nn, k1m, k1n);                                             \
  }
STAGE6(init_fluxes) STAGE6(advect) STAGE6(pbcor1) STAGE6(pbcor2) STAGE6(diffus) STAGE6(pgforc)
STAGE6(momtum) STAGE6(barotp) STAGE6(eddtra) STAGE6(convec) STAGE6(updtrc) STAGE6(cmnfld2) STAGE6(cmnfld1)
int blomgpu_tmsmt1(blomgpu_ctx *c, int nn) { ctx_sync_view(c); return st_tmsmt1(c, nn); }
int blomgpu_tmsmt2(blomgpu_ctx *c, int m, int mm, int nn, int k1m) { ctx_sync_view(c); return st_tmsmt2(c, m, mm, nn, k1m); }
int blomgpu_initms(blomgpu_ctx *c, int mm) { ctx_sync_view(c); return st_initms(c, mm); }
int blomgpu_diapfl(blomgpu_ctx *c, int n, int nn, int k1n) { ctx_sync_view(c); return st_diapfl(c, n, nn, k1n); }
// diaacc (phy/mod_dia.F90:1092): the count of accumulated steps first (:1123-1125), then the accumulation (stage_diaacc.hip)
int blomgpu_diaacc(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  if (!dia_active(c)) return 0;
  ctx_sync_view(c);
  dia_count(c);
  return st_diaacc(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_dia_select(blomgpu_ctx *c, const char *names) { return dia_select(c, names); }
int blomgpu_dia_alarm(blomgpu_ctx *c, int alarm) { return dia_alarm(c, alarm); }
// on != 0: every step of a blomgpu_step call keeps the heat and salt flux diagnostics current, not only its last two
int blomgpu_keep_flux_diagnostics(blomgpu_ctx *c, int on) {
  if (!c) return ctx_fail(c, "blomgpu_keep_flux_diagnostics: null context");
  c->keep_flux_diag = on != 0;
  return 0;
}
int blomgpu_dia_nacc(blomgpu_ctx *c, int *nacc) { return dia_nacc(c, nacc); }
int blomgpu_dia_get(blomgpu_ctx *c, const char *name, double *out) { return dia_get(c, name, out); }
int blomgpu_dia_finalize(blomgpu_ctx *c) { return dia_finalize(c); }
int blomgpu_dia_reset(blomgpu_ctx *c) { return dia_reset(c); }
int blomgpu_dia_name(int index, char *buf, int cap, int *is_lyr, int *grid) { return dia_name(index, buf, cap, is_lyr, grid); }
int blomgpu_dia_set_levels(blomgpu_ctx *c, const double *bnds, int ddm) { return dia_set_levels(c, bnds, ddm); }
int blomgpu_dia_levels_levitus2x(blomgpu_ctx *c) { return dia_levels_levitus2x(c); }
int blomgpu_dia_get_levels(blomgpu_ctx *c, double *bnds, int cap, int *ddm) { return dia_get_levels(c, bnds, cap, ddm); }
int blomgpu_dia_name_all(int index, char *buf, int cap, int *kind, int *grid) { return dia_name_all(index, buf, cap, kind, grid); }
int blomgpu_dia_name_full(int index, char *buf, int cap, int *kind, int *grid) { return dia_name_full(index, buf, cap, kind, grid); }
int blomgpu_dia_name_ext(int index, char *buf, int cap, int *kind, int *grid) { return dia_name_ext(index, buf, cap, kind, grid); }
int blomgpu_dia_set_sigdia(blomgpu_ctx *c, const double *sigdia, int n) { return dia_set_sigdia(c, sigdia, n); }
int blomgpu_dia_get_sigdia(blomgpu_ctx *c, double *out, int cap, int *n) { return dia_get_sigdia(c, out, cap, n); }
// what diaout_iogrp forms from the accumulators at output time (stage_diaout.hip)
int blomgpu_dia_name_msc(int index, char *buf, int cap, int *kind, int *grid) { return diaout_name_msc(index, buf, cap, kind, grid); }
int blomgpu_dia_set_mertra(blomgpu_ctx *c, int lmax, const double *mtlat, const int *nind, const int *pts, const int *oflg, int ocn_nreg,
                           int mer_nreg, const int *nflg, const int *regflg, const double *minlat, const double *maxlat) {
  return c ? diaout_set_mertra(c, lmax, mtlat, nind, pts, oflg, ocn_nreg, mer_nreg, nflg, regflg, minlat, maxlat) : 1;
}
int blomgpu_dia_set_sections(blomgpu_ctx *c, int sec_num, const int *nsi, const int *pts, int equat_sec) {
  return c ? diaout_set_sections(c, sec_num, nsi, pts, equat_sec) : 1;
}
int blomgpu_dia_reduce(blomgpu_ctx *c) { return c ? diaout_reduce(c) : 1; }
int blomgpu_dia_msc_get(blomgpu_ctx *c, const char *name, double *out, int cap, int *dims) { return c ? diaout_msc_get(c, name, out, cap, dims) : 1; }
// sfcstr, phy/mod_sfcstr.F90:33-62: the surface stress of the idealised experiments is set at initialisation
// (or absent), so the stage is empty for them; the coupled/reanalysis branches live in modules that are
// not part of this path.
// xcsum of level `lev` (1-based) of a named field, mask by grid type as in xctilr/xccrc (p-grid: ips)
int blomgpu_xcsum(blomgpu_ctx *c, const char *name, int lev, int itype, double *sum) {
  double *base = nullptr;
  if (int rc = real_levels(c, "blomgpu_xcsum", name, lev, 1, &base)) return rc;
  ctx_sync_view(c);
  return st_xcsum(c, base, itype, sum);
}
// exp(), pow(), sin() and atan2() as the kernels evaluate them (exp_libm.h, pow_libm.h, sin_libm.h, atan2_libm.h), elementwise on
// host arrays: lets a caller check that the device returns the bits of its own libm (tests/test_exp_libm.py, test_pow_libm.py,
// test_sin_atan2_libm.py)
__global__ void k_exp_libm(int n, const double *x, double *y) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) y[t] = exp_libm(x[t]);
}
__global__ void k_pow_libm(int n, const double *x, const double *y, double *z) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) z[t] = pow_libm(x[t], y[t]);
}
__global__ void k_sin_libm(int n, const double *x, double *z) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) z[t] = sin_libm(x[t]);
}
__global__ void k_atan2_libm(int n, const double *y, const double *x, double *z) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) z[t] = atan2_libm(y[t], x[t]);
}
int blomgpu_exp(blomgpu_ctx *c, int n, const double *x, double *y) {
  return libm_probe(c, n, x, nullptr, y, "blomgpu_exp", [&](dim3 g, double *a, double *, double *z) { hipLaunchKernelGGL(k_exp_libm, g, dim3(256), 0, c->stream, n, a, z); });
}
int blomgpu_pow(blomgpu_ctx *c, int n, const double *x, const double *y, double *z) {
  return libm_probe(c, n, x, y, z, "blomgpu_pow", [&](dim3 g, double *a, double *b, double *r) { hipLaunchKernelGGL(k_pow_libm, g, dim3(256), 0, c->stream, n, a, b, r); });
}
int blomgpu_sin(blomgpu_ctx *c, int n, const double *x, double *z) {
  return libm_probe(c, n, x, nullptr, z, "blomgpu_sin", [&](dim3 g, double *a, double *, double *r) { hipLaunchKernelGGL(k_sin_libm, g, dim3(256), 0, c->stream, n, a, r); });
}
int blomgpu_atan2(blomgpu_ctx *c, int n, const double *y, const double *x, double *z) {
  return libm_probe(c, n, y, x, z, "blomgpu_atan2", [&](dim3 g, double *a, double *b, double *r) { hipLaunchKernelGGL(k_atan2_libm, g, dim3(256), 0, c->stream, n, a, b, r); });
}
int blomgpu_difest_isobml(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  (void)k1m; (void)k1n;
  ctx_sync_view(c);
  return st_difest_isobml(c, m, n, mm, nn);
}
int blomgpu_budget_sums(blomgpu_ctx *c, int ncall, int n, int nn) { ctx_sync_view(c); return st_budget_sums(c, ncall, n, nn); }
int blomgpu_budget_init(blomgpu_ctx *c) { ctx_sync_view(c); return st_budget_init(c); }
int blomgpu_budget_output(blomgpu_ctx *c, int m) { ctx_sync_view(c); return st_budget_output(c, m); }
int blomgpu_budget_steps(blomgpu_ctx *c, int *first, int *count) {
  if (!c || !first || !count) return ctx_fail(c, "blomgpu_budget_steps: null argument");
  return budget_steps(c, first, count);
}
int blomgpu_budget_mass0(blomgpu_ctx *c, double *mass0) { return budget_mass0(c, mass0); }
int blomgpu_budget_record(blomgpu_ctx *c, int nstep, double *rec) {
  if (!c || !rec) return ctx_fail(c, "blomgpu_budget_record: null argument");
  return budget_record(c, nstep, rec);
}
int blomgpu_budget_files(blomgpu_ctx *c, int *mask) {
  if (!c || !mask) return ctx_fail(c, "blomgpu_budget_files: null argument");
  return budget_files(c, mask);
}
int blomgpu_budget_line(blomgpu_ctx *c, int nstep, int file, double *terms, int *nterms) {
  if (!c || !terms || !nterms) return ctx_fail(c, "blomgpu_budget_line: null argument");
  return budget_line(c, nstep, file, terms, nterms);
}
// which: 0 sdp, 1 tdp, 2 trdp, 3 tkedp, 4 glsdp (phy/mod_budget.F90:50-59)
int blomgpu_budget_get(blomgpu_ctx *c, int which, int ncall, int n, double *v) {
  if (which < 0 || which > 4 || ncall < 1 || ncall > 7 || n < 1 || n > 2) return ctx_fail(c, "blomgpu_budget_get: index out of range");
  *v = c->budget[which][ncall - 1][n - 1];
  return 0;
}
int blomgpu_sfcstr(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  (void)m; (void)n; (void)mm; (void)nn; (void)k1m; (void)k1n;
  const std::string &e = c->expcnf;
  if (e == "noforcing" || e == "fuk95" || e == "channel") return 0;
  if (cesm_on(c)) return st_sfcstr_cesm(c);
  if (ben02_on(c)) return st_sfcstr_ben02(c);
  if (e == "cesm")
    return ctx_fail(c, " sfcstr: expcnf = " + e + " is not built on the device (sfcstr_cesm / sfcstr_ben02) until blomgpu_inifrc_cesm has been called");
  if (e == "ben02clim" || e == "ben02syn" || e == "single_column")
    return ctx_fail(c, " sfcstr: expcnf = " + e + " is not built on the device (sfcstr_cesm / sfcstr_ben02)");
  return ctx_fail(c, " sfcstr: expcnf = " + e + " is unsupported!");          // :54-60
}
int blomgpu_init_cppm(blomgpu_ctx *c) { ctx_sync_view(c); return st_init_cppm(c); }   // phy/mod_cppm.F90:2504
int blomgpu_mxlayr_tail(blomgpu_ctx *c, int nn, int k1n) { ctx_sync_view(c); return st_mxlayr_tail(c, nn, k1n); }
int blomgpu_thermf(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  if (cesm_on(c)) {
    if (int rc = check_tracer_options(c)) return rc;
    return st_thermf_cesm(c, m, n, mm, nn, k1m, k1n);
  }
  if (ben02_on(c)) {
    if (int rc = check_tracer_options(c)) return rc;
    return st_thermf_ben02(c, m, n, mm, nn, k1m, k1n);
  }
  if (c->expcnf == "cesm") return ctx_fail(c, "thermf: expcnf = cesm is not built on the device until blomgpu_inifrc_cesm has been called");
  ctx_sync_view(c);
  return st_thermf(c, m, n, mm, nn, k1m, k1n);
}
// The coupled experiment (expcnf = 'cesm').  blomgpu_inifrc_cesm is inifrc_cesm (cesm/mod_cesm.F90:175-200) and the declaration that the
// coupler's forcing exists; blomgpu_getfrc_cesm is getfrc_cesm (:202-263); blomgpu_cesm_nflxdi returns mod_forcing's nflxdi(48).
int blomgpu_inifrc_cesm(blomgpu_ctx *c) {
  if (!c) return ctx_fail(c, "blomgpu_inifrc_cesm: null argument");
  if (c->ben02_declared) return ctx_fail(c, "blomgpu_inifrc_cesm: this context has declared the forced ocean-ice experiment's forcing (blomgpu_inifrc_ben02)");
  return cesm_inifrc(c);
}
// The forced ocean-ice experiment (expcnf = 'ben02clim' / 'ben02syn' / 'single_column'; stage_thermf_ben02.hip).  blomgpu_inifrc_ben02
// declares that its forcing exists; blomgpu_ben02_ntda returns mod_ben02's ntda, the steps thermf_ben02 has accumulated into tsi_tda
// tml_tda sml_tda alb_tda fice_tda; blomgpu_ben02_reset_tda zeroes the five planes and the count, as asflux does when it has used them
// (ben02/mod_ben02.F90:1623-1624, :1701-1705).
int blomgpu_inifrc_ben02(blomgpu_ctx *c) { return c ? ben02_inifrc(c) : ctx_fail(c, "blomgpu_inifrc_ben02: null argument"); }
int blomgpu_ben02_ntda(blomgpu_ctx *c, int *n) {
  if (!c || !n) return ctx_fail(c, "blomgpu_ben02_ntda: null argument");
  *n = c->ntda;
  return 0;
}
int blomgpu_ben02_reset_tda(blomgpu_ctx *c) { return c ? ben02_reset_tda(c) : ctx_fail(c, "blomgpu_ben02_reset_tda: null argument"); }
int blomgpu_getfrc_cesm(blomgpu_ctx *c) { return st_getfrc_cesm(c); }
// The end of blom_step (stage_stepend.hip).  Each returns at once unless its option has declared it.
int blomgpu_iniswa(blomgpu_ctx *c) { return c ? stepend_iniswa(c) : ctx_fail(c, "blomgpu_iniswa: null argument"); }   // phy/mod_swabs.F90:216
int blomgpu_updswa(blomgpu_ctx *c) { return c ? st_updswa(c) : ctx_fail(c, "blomgpu_updswa: null argument"); }        // phy/mod_swabs.F90:611
int blomgpu_fwbbal(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {                                   // phy/mod_forcing.F90:361
  (void)m; (void)n; (void)mm; (void)nn; (void)k1m; (void)k1n;
  return c ? st_fwbbal(c) : ctx_fail(c, "blomgpu_fwbbal: null argument");
}
int blomgpu_chkvar(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {                                   // phy/mod_chkvar.F90:77
  (void)m; (void)n; (void)mm; (void)k1m; (void)k1n;
  return c ? st_chkvar(c, nn) : ctx_fail(c, "blomgpu_chkvar: null argument");
}
int blomgpu_cesm_nflxdi(blomgpu_ctx *c, int *out) {
  if (!c || !out) return ctx_fail(c, "blomgpu_cesm_nflxdi: null argument");
  for (int k = 0; k < 48; k++) out[k] = c->nflxdi[k];
  return 0;
}
// xcsum of the levels lev0 .. lev0 + nlev - 1 (1-based) of a named field at once, through the kernels thermf_cesm's sums take
// (halo.hip: st_xcsum_batch); mask: "ips", or the name of an integer field whose points equal to 1 are summed
int blomgpu_xcsum_batch(blomgpu_ctx *c, const char *name, int lev0, int nlev, const char *mask, double *sums) {
  if (!c || !name || !mask || !sums) return ctx_fail(c, "blomgpu_xcsum_batch: null argument");
  double *base = nullptr;
  if (int rc = real_levels(c, "blomgpu_xcsum_batch", name, lev0, nlev, &base)) return rc;
  ctx_sync_view(c);
  const int *mk = nullptr;
  if (std::string(mask) != "ips") {
    auto jt = c->int_ids.find(mask);
    if (jt == c->int_ids.end() || c->nlev_int[jt->second] != 1) return ctx_fail(c, std::string("blomgpu_xcsum_batch: unknown mask ") + mask);
    mk = c->h.m[jt->second];
  }
  std::vector<const double *> planes;
  std::vector<const int *> masks(nlev, mk);
  for (int q = 0; q < nlev; q++) planes.push_back(base + (size_t)q * c->h.nplane);
  double *dev = nullptr;
  HIPCHK(c, hipMalloc((void **)&dev, sizeof(double) * (size_t)nlev * (c->h.jtdm + 1)));
  int rc = st_xcsum_batch(c, nlev, planes.data(), masks.data(), dev + nlev, dev);
  if (!rc && hipMemcpyAsync(sums, dev, sizeof(double) * nlev, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = 1;
  if (hipStreamSynchronize(c->stream) != hipSuccess) rc = 1;
  (void)hipFree(dev);
  return rc ? (c->err.empty() ? ctx_fail(c, "blomgpu_xcsum_batch: copy or launch failed") : 1) : 0;
}
int blomgpu_mxlayr(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) { ctx_sync_view(c); return st_mxlayr(c, m, n, mm, nn, k1m, k1n); }
int blomgpu_ale_regrid_remap(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {   // phy/mod_ale_regrid_remap.F90:1486
  ctx_sync_view(c);
  return st_ale_regrid_remap(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_ale_remap_diazlv(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {   // phy/mod_ale_regrid_remap.F90:1986
  ctx_sync_view(c);
  return st_ale_remap_diazlv(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_cmnfld_bfsqi_ale(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {  // phy/mod_cmnfld_routines.F90:352
  ctx_sync_view(c);
  return st_cmnfld_bfsqi_ale(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_ale_forcing(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {  // phy/mod_ale_forcing.F90:45
  ctx_sync_view(c);
  return st_ale_forcing(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_ale_vdifft(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {   // phy/mod_ale_vdiff.F90:50
  ctx_sync_view(c);
  return st_ale_vdifft(c, m, n, mm, nn, k1m, k1n);
}
int blomgpu_ale_vdiffm(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {   // phy/mod_ale_vdiff.F90:245
  ctx_sync_view(c);
  return st_ale_vdiffm(c, m, n, mm, nn, k1m, k1n);
}
// 1-D module arrays of the reference: "plevel" (kdm pressure levels of vcoord_type = 'plevel', phy/mod_vcoord.F90:99)
int blomgpu_set_vector(blomgpu_ctx *c, const char *name, const double *v, int nv) {
  if (!c || !name || !v) return ctx_fail(c, "blomgpu_set_vector: null argument");
  const std::string s(name);
  if (s == "plevel") {
    if (nv != c->h.kk) return ctx_fail(c, " readnml_vcoord: number of plevel values does not match vertical dimension!");   // :965
    if (!c->ale_plevel) HIPCHK(c, hipMalloc((void **)&c->ale_plevel, sizeof(double) * nv));
    HIPCHK(c, hipMemcpy(c->ale_plevel, v, sizeof(double) * nv, hipMemcpyHostToDevice));
    return 0;
  }
  return ctx_fail(c, "blomgpu_set_vector: unknown array " + s);
}

int blomgpu_halo_cmnfld2(blomgpu_ctx *c, int n) {     // phy/mod_cmnfld_routines.F90:1171-1196
  ctx_sync_view(c);
  const int kk = c->h.kk;
  {
    double *ptrs[2] = {c->h.f[F_temp], c->h.f[F_saln]};
    const int nl[2] = {2 * kk, 2 * kk}, it[2] = {1, 1};
    if (st_xctilr_multi(c, 2, ptrs, nl, 3, 3, it)) return 1;
  }
  return st_kfpla_halo(c, n);                         // kfpla(:,:,n) halo through util1, :1176-1196
}
// the halo updates of difest_lateral_hybrid (which = 0, phy/mod_difest.F90:826-831) and difest_vertical_hybrid (which = 1,
// :877-878): the routines need CVMix and are not built, their halo updates are what momtum and ale_vdiffm rely on
int blomgpu_halo_difest_hyb(blomgpu_ctx *c, int which, int k1n) {
  ctx_sync_view(c);
  const int kk = c->h.kk;
  const size_t np = c->h.nplane;
  if (which == 0) {
    double *ptrs[6] = {c->h.f[F_u], c->h.f[F_v], c->h.f[F_ubflxs_p], c->h.f[F_vbflxs_p], c->h.f[F_pbu], c->h.f[F_pbv]};
    const int nl[6] = {2 * kk, 2 * kk, 2, 2, 2, 2}, it[6] = {13, 14, 13, 14, 3, 4};
    return st_xctilr_multi(c, 6, ptrs, nl, 2, 2, it);
  }
  double *ptrs[2] = {c->h.f[F_u] + (size_t)(k1n - 1) * np, c->h.f[F_v] + (size_t)(k1n - 1) * np};
  const int nl[2] = {kk, kk}, it[2] = {13, 14};
  return st_xctilr_multi(c, 2, ptrs, nl, 1, 1, it);
}

int blomgpu_halo_difest(blomgpu_ctx *c, int nn) {     // phy/mod_difest.F90:750-772
  ctx_sync_view(c);
  const int kk = c->h.kk;
  {
    double *ptrs[6] = {c->h.f[F_u], c->h.f[F_v], c->h.f[F_ubflxs_p], c->h.f[F_vbflxs_p], c->h.f[F_pbu], c->h.f[F_pbv]};
    const int nl[6] = {2 * kk, 2 * kk, 2, 2, 2, 2}, it[6] = {13, 14, 13, 14, 3, 4};
    if (st_xctilr_multi(c, 6, ptrs, nl, 2, 2, it)) return 1;
  }
  // interface pressure out to ii+3 for remap (:761-772) -- unless st_cmnfld2 has done it in front of its kernels on the second stream
  if (c->seq.pscan_done_ahead) { c->seq.pscan_done_ahead = false; return 0; }
  return launch_pscan(c, nn, -2, 3);
}

// Everything blomgpu_stage accepts: X(name, the call of its entry point), the reference's stages and the pseudo-stages that stand for
// parts of them.  (blom_amd/stepper.py keeps its own lists of these names.)
#define STAGE_ARGS blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n
#define ALL6 c, m, n, mm, nn, k1m, k1n
#define BLOM_STAGES(X)                                                                                                          \
  X(init_fluxes, blomgpu_init_fluxes(ALL6)) X(tmsmt1, blomgpu_tmsmt1(c, nn)) X(tmsmt2, blomgpu_tmsmt2(c, m, mm, nn, k1m))        \
  X(initms, blomgpu_initms(c, mm)) X(advect, blomgpu_advect(ALL6)) X(pbcor1, blomgpu_pbcor1(ALL6)) X(pbcor2, blomgpu_pbcor2(ALL6)) \
  X(diffus, blomgpu_diffus(ALL6)) X(pgforc, blomgpu_pgforc(ALL6)) X(momtum, blomgpu_momtum(ALL6)) X(convec, blomgpu_convec(ALL6))  \
  X(sfcstr, blomgpu_sfcstr(ALL6)) X(updtrc, blomgpu_updtrc(ALL6)) X(diapfl, blomgpu_diapfl(c, n, nn, k1n))                        \
  X(barotp, blomgpu_barotp(ALL6)) X(eddtra, blomgpu_eddtra(ALL6)) X(init_cppm, blomgpu_init_cppm(c))                              \
  X(halo_cmnfld2, blomgpu_halo_cmnfld2(c, n)) X(cmnfld2, blomgpu_cmnfld2(ALL6)) X(cmnfld1, blomgpu_cmnfld1(ALL6))                 \
  X(halo_difest, blomgpu_halo_difest(c, nn)) X(difest_isobml_pre, (ctx_sync_view(c), st_difest_isobml_pre(c, m, n, mm, nn)))      \
  X(difest_isobml, blomgpu_difest_isobml(ALL6)) X(niw_ke_tendency, (ctx_sync_view(c), st_niw_ke_tendency(c, m, mm)))              \
  X(halo_difest_hyb, blomgpu_halo_difest_hyb(c, 0, k1n)) X(halo_difest_vert, blomgpu_halo_difest_hyb(c, 1, k1n))                  \
  X(mxlayr_tail, blomgpu_mxlayr_tail(c, nn, k1n)) X(mxlayr, blomgpu_mxlayr(ALL6)) X(thermf, blomgpu_thermf(ALL6))                 \
  X(ale_regrid_remap, blomgpu_ale_regrid_remap(ALL6)) X(ale_forcing, blomgpu_ale_forcing(ALL6))                                   \
  X(cmnfld_bfsqi_ale, blomgpu_cmnfld_bfsqi_ale(ALL6)) X(ale_vdifft, blomgpu_ale_vdifft(ALL6)) X(ale_vdiffm, blomgpu_ale_vdiffm(ALL6)) \
  X(diaacc, blomgpu_diaacc(ALL6)) X(ale_remap_diazlv, blomgpu_ale_remap_diazlv(ALL6)) X(getfrc_cesm, blomgpu_getfrc_cesm(c)) \
  X(updswa, blomgpu_updswa(c)) X(fwbbal, blomgpu_fwbbal(ALL6)) X(chkvar, blomgpu_chkvar(ALL6))                                    \
  /* mod_budget's calls by their number (phy/mod_blom_step.F90:96-230: 1..5 on level n, 6 and 7 on level m) and budget_output (:245) */ \
  X(budget_sums1, blomgpu_budget_sums(c, 1, n, nn)) X(budget_sums2, blomgpu_budget_sums(c, 2, n, nn))                           \
  X(budget_sums3, blomgpu_budget_sums(c, 3, n, nn)) X(budget_sums4, blomgpu_budget_sums(c, 4, n, nn))                           \
  X(budget_sums5, blomgpu_budget_sums(c, 5, n, nn)) X(budget_sums6, blomgpu_budget_sums(c, 6, m, mm))                           \
  X(budget_sums7, blomgpu_budget_sums(c, 7, m, mm)) X(budget_output, blomgpu_budget_output(c, m))
enum StageId {
#define X(nm, call) S_##nm,
  BLOM_STAGES(X)
#undef X
  NSTAGE
};
static const struct Stage { const char *name; StageId id; int (*entry)(STAGE_ARGS); } g_stages[NSTAGE] = {
#define X(nm, call) {#nm, S_##nm, [](STAGE_ARGS) -> int { return call; }},
  BLOM_STAGES(X)
#undef X
};

int blomgpu_stage(blomgpu_ctx *c, const char *stage, int m, int n, int mm, int nn, int k1m, int k1n) {
  const std::string_view s(stage);
  for (const Stage &st : g_stages)
    if (s == st.name) return st.entry(ALL6);
  return ctx_fail(c, "blomgpu_stage: unknown stage " + std::string(s));
}

// Stage sequence of one baroclinic step, phy/mod_blom_step.F90:89-253 (hot path only).
static int step_sequence(STAGE_ARGS) {
  static const StageId seq[] = {S_init_fluxes, S_tmsmt1, S_halo_cmnfld2, S_halo_difest, S_eddtra, S_advect, S_pbcor1, S_diffus, S_pgforc,
                                S_momtum, S_convec, S_diapfl, S_mxlayr_tail, S_updtrc, S_barotp, S_pbcor2, S_tmsmt2};
  // the other vertical coordinates (phy/mod_blom_step.F90:126-233 with vcoord_tag /= vcoord_isopyc_bulkml), as far as built:
  // blom_amd/stepper.py HYBRID_STAGES says what is left out and why
  static const StageId seq_ale[] = {S_init_fluxes, S_tmsmt1, S_ale_regrid_remap, S_cmnfld2, S_halo_difest_hyb, S_eddtra, S_advect,
                                    S_pbcor1, S_diffus, S_pgforc, S_momtum, S_cmnfld_bfsqi_ale, S_ale_forcing, S_halo_difest_vert,
                                    S_ale_vdifft, S_ale_vdiffm, S_updtrc, S_barotp, S_pbcor2, S_tmsmt2, S_cmnfld1};
  const auto stage = [&](StageId id) { return g_stages[id].entry(ALL6); };
  const bool ale = c->h.P.vcoord_tag != 1;
  // The coupled experiment, once its forcing is declared (stage_thermf_cesm.hip): getfrc_cesm behind init_fluxes (phy/mod_blom_step.F90:116),
  // sfcstr in front of pgforc (:163), and under the hybrid coordinates thermf behind momtum (:188; the isopycnic full-physics
  // sequence has its thermf already).  None of the three touches the flux arrays the lean init_fluxes leaves for advect, and none
  // reads or writes what the second stream holds at that point: the viscous chain of momtum reads no wind stress (k_mom_cor_march
  // does, behind pgforc), and thermf_cesm beside diapfl's momentum mixing reads p, dp, temp, saln, trc and writes surface planes only
  // (tools/kernel_rw_sets.py: k_diapfl_momentum / k_diapfl_dpudpv write u, v, dpu, dpv).
  // The forced ocean-ice experiment, once declared (stage_thermf_ben02.hip), has no getfrc stage on the device (asflux is the host's); its
  // sfcstr and thermf stand where the coupled experiment's do, and read and write the same arrays of the step plus planes of their own.
  // updswa (stage_stepend.hip) behind getfrc (:122) whenever a chlorophyll method is declared, for every expcnf: it writes the four band
  // planes and chl10 only, which nothing between the lean init_fluxes and advect touches (thermf and ale_forcing read them, far behind),
  // and nothing runs on the second stream at that point (tools/kernel_rw_sets.py: k_updswa).
  const bool cesm = cesm_on(c), ben02 = ben02_on(c), frc = cesm || ben02, swa = swa_chlorophyll(c);
  c->seq = StepState{};
  c->seq.defer_checks = c->seq.in_sequence = true;
  {
    // the one way out of the sequence, whichever return takes it
    struct Leave {
      blomgpu_ctx *c;
      bool failed = true;
      ~Leave() {
        c->seq.defer_checks = c->seq.in_sequence = false;
        if (failed) c->tmsmt1_done_ahead = false;
      }
    } leave{c};
    // mod_budget (option budget_step with cnsvdi; stage_budget.hip): budget_sums' calls by their number where blom_step has them (:96,
    // :132/:156, :159/:177, :183/:205, :215, :224, :230), each behind the last writer of dp, temp, saln, trc of its level on the context's
    // stream.  What runs on the second stream beside them writes none of the four (momtum's viscous chain: its own work space; diapfl's
    // momentum mixing: u, v, dpu, dpv) but for what raises updtrc_on_side -- updtrc's ideal-age step (a tracer that can be tracer 1) and,
    // with phys_dag bit 8, mxlayr's copy-back clamp (saln and the tracers) -- which call 5 joins (tests/test_budget_sets.py).  pbcor2 stores its
    // level m itself with the option on (stage_pbcor_tile.hip), so that call 6 reads it where the reference does.
    const auto bud = [&](int ncall) { return st_budget_instep(c, ncall, ncall <= 5 ? nn : mm); };
    if (int rc = bud(1)) return rc;                                         // :96 (blomgpu_step has advanced the clock already: the sums read no clock scalar)
    if (ale) {
      for (const StageId st : seq_ale) {
        if (c->tmsmt1_done_ahead && st == S_tmsmt1) { c->tmsmt1_done_ahead = false; continue; }
        if (c->eddtra_frozen && st == S_eddtra) continue;
        if (frc && st == S_pgforc)
          if (int rc = stage(S_sfcstr)) return rc;
        if (int rc = stage(st)) return rc;
        if (const int ncall = st == S_ale_regrid_remap ? 2 : st == S_diffus ? 3 : st == S_ale_vdiffm ? 4 : st == S_updtrc ? 5 : st == S_pbcor2 ? 6 : st == S_tmsmt2 ? 7 : 0)
          if (int rc = bud(ncall)) return rc;
        if (cesm && st == S_init_fluxes)
          if (int rc = stage(S_getfrc_cesm)) return rc;
        if (swa && st == S_init_fluxes)
          if (int rc = stage(S_updswa)) return rc;
        if (frc && st == S_momtum)
          if (int rc = stage(S_thermf)) return rc;
      }
    } else for (const StageId st : seq) {
      // live_slopes: cmnfld2 (the halo updates plus buoyancy frequency and neutral slopes) in place of its halo part alone
      StageId run = c->live_slopes && st == S_halo_cmnfld2 ? S_cmnfld2 : st;
      // full_physics (blom_amd/stepper.py FULL_STAGES): the built part of difest_isobml, thermf and mxlayr in place of the two
      // pseudo-stages that stood in for them
      if (c->full_physics && st == S_halo_difest) run = c->difest_live ? S_difest_isobml : S_difest_isobml_pre;
      if (c->full_physics && st == S_mxlayr_tail) {
        if (int rc = stage(S_thermf)) return rc;
        run = S_mxlayr;
      }
      // eddtra_frozen: the eddy-induced fluxes umfltd.. stay as uploaded (the reference build of the oracle has no mod_eddtra;
      // tests pin advect/remap on non-zero fluxes this way)
      if (c->eddtra_frozen && st == S_eddtra) continue;
      // the step before this one, in the same call, has done this step's tmsmt1 in its tmsmt2
      if (c->tmsmt1_done_ahead && st == S_tmsmt1) { c->tmsmt1_done_ahead = false; continue; }
      // The lean init_fluxes zeroes only the ring the tile kernel of remap does not store (stage_simple.hip): until advect has run, every
      // other plane of uflx .. vsflx (m) holds the PREVIOUS step's fluxes.  Only stages known not to touch them may run in between.
      if (c->seq.fluxes_lean) {
        bool allowed = false;
        for (const StageId ok : {S_tmsmt1, S_halo_cmnfld2, S_cmnfld2, S_halo_difest, S_difest_isobml, S_difest_isobml_pre, S_eddtra, S_advect})
          allowed = allowed || run == ok;
        if (!allowed)
          return ctx_fail(c, std::string("blomgpu_step: stage ") + g_stages[run].name + " between the lean init_fluxes and advect: the flux arrays of level m are not zeroed (set lean_fluxes = 0)");
      }
      // what an earlier stage left running on the second stream and this stage needs (st_mxlayr waits for diapfl's momentum mixing itself)
      if ((c->seq.diapfl_mom_on_side && run != S_mxlayr) || (c->seq.updtrc_on_side && st == S_pbcor2)) {
        const int ev = c->seq.diapfl_mom_on_side ? 7 : 9;
        c->seq.diapfl_mom_on_side = c->seq.updtrc_on_side = false;
        if (ctx_side_done(c, ev) || ctx_side_join(c, ev)) return 1;
      }
      if (frc && st == S_pgforc)
        if (int rc = stage(S_sfcstr)) return rc;
      if (int rc = stage(run)) return rc;
      if (const int ncall = st == S_diffus ? 2 : st == S_convec ? 3 : st == S_diapfl ? 4 : st == S_updtrc ? 5 : st == S_pbcor2 ? 6 : st == S_tmsmt2 ? 7 : 0) {
        if (ncall == 5 && budget_on(c) && c->seq.updtrc_on_side) {        // k_idlage_step may write tracer 1, k_mxl_clamp writes saln and the tracers
          c->seq.updtrc_on_side = false;
          if (ctx_side_done(c, 9) || ctx_side_join(c, 9)) return 1;
        }
        if (int rc = bud(ncall)) return rc;
      }
      if (cesm && st == S_init_fluxes)
        if (int rc = stage(S_getfrc_cesm)) return rc;
      if (swa && st == S_init_fluxes)
        if (int rc = stage(S_updswa)) return rc;
      // cmnfld2's kernels still alone on the second stream (frozen diffusivities: difest_isobml did not wait for them): eddtra reads the slopes
      if (st == S_halo_difest && c->seq.cmn_on_side) {
        c->seq.cmn_on_side = false;
        if (ctx_side_done(c, 4) || ctx_side_join(c, 4)) return 1;
      }
      // momtum's viscous chain starts here, on the second stream (stage_momtum.hip: st_momtum_early) -- or behind a later stage
      // (option mom_early_at: nothing up to pgforc writes what the chain reads)
      static const StageId early_at[] = {S_halo_difest, S_eddtra, S_advect, S_pbcor1, S_diffus};
      if (st == early_at[c->mom_early_at < 0 || c->mom_early_at > 4 ? 0 : c->mom_early_at])
        if (int rc = st_momtum_early(c, m, n, mm, nn)) return rc;
    }
    leave.failed = false;
  }
  // (outside the sequence: nothing is handed to it and it defers nothing)
  if (!ale && (c->cmnfld1 || c->full_physics))
    if (int rc = stage(S_cmnfld1)) return rc;                               // phy/mod_blom_step.F90:233
  // diaacc (:239) with a selection: on the context's stream, behind everything the step put on the second one (the last of it
  // is joined in front of pbcor2).  Its sources are arrays of the finished step; the tmsmt1 that tmsmt_ahead folded into tmsmt2
  // wrote *old arrays only (diavfl reads dpold: with its group selected nothing is folded, blomgpu_step).  blomgpu_step counts the step (a capture passes here without executing)
  if (dia_active(c))
    if (int rc = st_diaacc(ALL6)) return rc;
  // fwbbal (:242) and chkvar (:252), each only where its option has declared it (stage_stepend.hip); chkvar leaves its words on the
  // device for blomgpu_step's check, like every stage of the sequence
  if (c->sprfac)
    if (int rc = st_fwbbal(c)) return rc;
  if (int rc = st_budget_output_instep(c)) return rc;                       // :245
  if (c->chkvar) {
    c->seq.defer_checks = true;
    const int rc = st_chkvar(c, nn);
    c->seq.defer_checks = false;
    return rc;
  }
  return 0;
}
#undef ALL6
#undef STAGE_ARGS

// A step is ~100 kernel launches, and on the smaller grids most of them are shorter than the time it takes to launch
// them.  The sequence depends on the step only through the parity of the time levels, so it is captured from the stream
// for both parities at once (after two plain steps: work buffers are allocated on first use) and replayed as HIP graphs.
// Single tile only (the RCCL transport and the in-process tile groups synchronise on the host); not while stage timers run.
int blomgpu_step(blomgpu_ctx *c, int *nstep, int nsteps) {
  const int kk = c->h.kk;
  if (int rc = dia_step_check(c)) return rc;
  if (cesm_on(c) && c->use_graph)
    return ctx_fail(c, "blomgpu_step: the coupled experiment's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  if (ben02_on(c) && c->use_graph)
    return ctx_fail(c, "blomgpu_step: the forced ocean-ice experiment's per-step scalars are kernel arguments, which a captured graph would freeze (set use_graph = 0)");
  if (int rc = stepend_step_check(c)) return rc;
  // mod_budget (stage_budget.hip): the records of this call's steps on the device; one copy brings them back in front of the last check
  const int ns0 = *nstep;
  if (int rc = budget_call_begin(c, ns0, nsteps)) return rc;
  // (the stage entries outside this call keep the flux diagnostics current, whichever way it returns)
  struct FluxDiagBack { blomgpu_ctx *c; ~FluxDiagBack() { c->flux_diag = true; } } flux_diag_back{c};
  // the row test walks the selection: once per call, the selection cannot change inside it
  const bool flux_diag_lazy = !c->keep_flux_diag && c->h.P.vcoord_tag == 1 && !dia_reads_flux_diag(c);
  for (int it = 0; it < nsteps; it++) {
    const int ns = *nstep;
    const int m = ns % 2 + 1, n = (ns + 1) % 2 + 1;
    const int mm = (m - 1) * kk, nn = (n - 1) * kk, k1m = 1 + mm, k1n = 1 + nn;
    c->h.P.nstep = ns + 1;                             // read by host code only: no upload of the view for it
    // step_time (phy/mod_time.F90:182-219; stage_stepend.hip): the day of the year and the interpolation scalars of this step, where the
    // setters put them -- context members that host code reads, no upload of the view either
    if (c->step_time)
      if (int rc = stepend_step_time(c, ns + 1)) return rc;
    ctx_sync_view(c);
    budget_call_slot(c, it);
    // (not while diavfl's group is selected: its dp(km) - dpold(km) needs the dpold the PREVIOUS step's tmsmt1 left, and the fold
    // would have tmsmt2 overwrite it in front of diaacc.  The cost of the launch it brings back: DESIGN 3.13)
    c->tmsmt1_ahead = !c->use_graph && !c->csdiag && it < nsteps - 1 && c->tmsmt_ahead && !dia_reads_dpold(c);
    // The heat and salt flux diagnostics (blomgpu_internal.h: flux_diag) are kept current only by the steps that can leave something
    // observable in them.  The caller sees them when the call has returned, on both time levels: level m of the last step is written in
    // that step; its level n was written one step earlier (eddtra, remap, pbcor1, diffus under level m there) and by the last step's
    // pbcor2.  Every older value is zeroed (k_init_fluxes_ring) or assigned (remap's tile kernel, eddtra, diffus' *flld) under the same
    // constant masks before it could be seen.  So all but the last two steps skip, unless something reads the arrays every step:
    // csdiag's checksums, a diaacc row -- or the launches are a captured graph's, the same in every step.  The hybrid-coordinate
    // sequence writes these arrays inside fused kernels (eddtra_ale, ndiff) and keeps today's form.
    c->flux_diag = !(flux_diag_lazy && !c->use_graph && !c->csdiag && it < nsteps - 2);
    // (the hybrid-coordinate sequence too: the engine's status of ale_regrid_remap stays on the device until the check below)
    // (nor a budgeted step: its record changes every step)
    bool graph = c->use_graph && !c->timing && !c->tiling.multi() && c->steps_warm >= 2 && !budget_on(c);
    hipGraphExec_t &ge = c->step_graph[ns & 1];
    if (graph && !ge) {
      // Capture; nothing executes while capturing, so on any failure the step is simply run with plain launches.  Both parities are
      // captured at once -- this step's sequence, then the next step's (time levels swapped) -- so that a caller's warm-up of four
      // steps from rest (the time step changes after the first: the view is uploaded again and the count restarts) leaves nothing but replays
      // to the steps after it.  A capture that fails after it began (a buffer allocated on first
      // use inside it) is tried again two plain steps later, three times at most; a stream that cannot capture at all is not asked again.
      bool began = false;
      auto capture = [&](hipGraphExec_t &out, int m_, int n_, int nstep_) {
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
        began = true;
        c->h.P.nstep = nstep_;
        const int mm_ = (m_ - 1) * kk, nn_ = (n_ - 1) * kk;
        const int rc = step_sequence(c, m_, n_, mm_, nn_, 1 + mm_, 1 + nn_);
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        bool ok = rc == 0 && e == hipSuccess && g != nullptr;
        if (ok && hipGraphInstantiate(&out, g, nullptr, nullptr, 0) != hipSuccess) { out = nullptr; ok = false; }
        if (g) (void)hipGraphDestroy(g);
        return ok;
      };
      bool ok = capture(ge, m, n, ns + 1);
      hipGraphExec_t &ge2 = c->step_graph[(ns + 1) & 1];
      if (ok && !ge2 && !capture(ge2, n, m, ns + 2)) ge2 = nullptr;          // (left to its own step)
      c->h.P.nstep = ns + 1;
      if (!ok) {
        (void)hipGetLastError();
        c->err.clear();
        if (!began || ++c->graph_failures >= 3) c->use_graph = 0;           // plain launches from now on
        else c->steps_warm = 0;
        graph = false;
      }
    }
    if (graph) { HIPCHK(c, hipGraphLaunch(ge, c->stream)); c->graph_steps++; }
    else if (int rc = step_sequence(c, m, n, mm, nn, k1m, k1n)) { c->tmsmt1_done_ahead = false; return rc; }
    if (!c->flux_diag) c->flux_diag_skipped++;
    dia_count(c);                                          // nacc_phy, phy/mod_dia.F90:1123-1125
    c->steps_done++;
    c->steps_warm++;
    // the stages' error words are sticky: one read-back (a host synchronisation) per check_period steps (every step with
    // csdiag or stage timing, where the reference's stop-in-the-failing-step matters) and at the end of the call
    const int period = (c->csdiag || c->timing) ? 1 : c->check_period;
    if (it == nsteps - 1)
      if (int rc = budget_call_fetch(c)) return rc;
    if (it == nsteps - 1 || (it + 1) % period == 0)
      if (int rc = ctx_check_errors(c)) {
        const int first = ns + 1 - (it % period);
        c->err += " (raised in one of the steps nstep = " + std::to_string(first) + ".." + std::to_string(ns + 1) + ")";
        c->tmsmt1_done_ahead = false;
        return rc;
      }
    const double delt2 = c->h.P.baclin + c->h.P.baclin;      // phy/mod_blom_step.F90:300
    if (c->h.P.delt1 != delt2) { c->h.P.delt1 = delt2; c->dirty = true; }   // changes after the first step only
    *nstep = ns + 1;
  }
  return budget_call_commit(c, ns0);
}

// debug (builds with -DBT_PROFILE only record anything): host == nullptr allocates and zeroes nwords of timestamps for the
// persistent barotp kernel, otherwise copies them back
int blomgpu_dbg_bt_prof(blomgpu_ctx *c, long long *host, int nwords) {
  if (!host) {
    if (c->bt_prof) (void)hipFree(c->bt_prof);
    HIPCHK(c, hipMalloc((void **)&c->bt_prof, sizeof(long long) * nwords));
    HIPCHK(c, hipMemset(c->bt_prof, 0, sizeof(long long) * nwords));
    return 0;
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, c->bt_prof, sizeof(long long) * nwords, hipMemcpyDeviceToHost));
  return 0;
}

// debug: per-wavefront phase timestamps of the column kernels that carry KPROF marks (library built with -DBLOM_KPROF: tools/probes;
// the production build records nothing): host == nullptr allocates and zeroes nwords, otherwise copies them back.  The kernels
// bound-check their slot against the stored size.
int blomgpu_dbg_kprof(blomgpu_ctx *c, long long *host, int nwords) {
  if (!host) {
    if (c->kprof) (void)hipFree(c->kprof);
    c->kprof = nullptr; c->kprof_words = 0;
    if (nwords <= 0) return 0;
    HIPCHK(c, hipMalloc((void **)&c->kprof, sizeof(long long) * nwords));
    HIPCHK(c, hipMemset(c->kprof, 0, sizeof(long long) * nwords));
    c->kprof_words = nwords;
    return 0;
  }
  if (!c->kprof || nwords > c->kprof_words) return ctx_fail(c, "blomgpu_dbg_kprof: no buffer of that size");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(host, c->kprof, sizeof(long long) * nwords, hipMemcpyDeviceToHost));
  return 0;
}

int blomgpu_timer_reset(blomgpu_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (auto &kv : c->timers) {
    for (auto &ev : kv.second.pending) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    kv.second = KTimer();
  }
  return 0;
}

int blomgpu_timer_get(blomgpu_ctx *c, const char *what, double *ms_total, int *launches) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  KTimer &t = c->timers[what];
  for (auto &ev : t.pending) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.first, ev.second);
    t.ms += ms;
    t.launches++;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  t.pending.clear();
  *ms_total = t.ms;
  *launches = t.launches;
  return 0;
}

}  // extern "C"
