// The map of the shared work space (DevView::wk, DevView::wk2d; blomgpu_internal.h): every slot name of the library, so that the next
// free slot, every sharing and every hand-over between two stages can be read in one place.  A stage owns its slots from its first kernel
// to its last unless the line says otherwise; stages on the context's stream follow each other, so two families may use the same numbers.
// What runs BESIDE another stage inside blomgpu_step must not: those relations are written out below and asserted.
// tools/kernel_rw_sets.py resolves the names through this file (tests/test_side_by_side_sets.py, tests/test_shared_definitions.py).
#pragma once

// ==== wk2d: NWK2D single planes, WK2(V, slot) ============================================================================================
#define NWK2D 48
//   0  S2_PBFACO    tmsmt2: pb / sum of dpold; k_tmsmt2_fac -> k_tmsmt2
//      S2_REMAP_PM  = 0 on purpose.  remap: the smallest bottom pressure of the nine points around; k_adv_pbmin -> the remap kernels.  Never live together: advect has long
//                   ended when tmsmt2 -- the last stage of a step -- starts on the same stream
//   1  S2_PBFACN    tmsmt2: pb / sum of dp(n); k_tmsmt2_fac -> k_tmsmt2
//      S2_PBUT      = 1 on purpose.  pbcor (bmcmth = dluc): min of pb at the u-point; k_pbc_total -> the tile kernel of the same pbcor
//                   call.  Never live together: tmsmt2 follows pbcor2 on the same stream
//   2  S2_PBVT      pbcor: the same at the v-point
//   3  S2_DRAG      momtum: bottom drag; k_mom_drag -> the Coriolis march (stage_momtum.hip, stage_momtum_fused.hip)
//   4  S2_QUM       momtum: FOUR planes 4..7 -- the barotropic part of utotm vtotm utotn vtotn; k_mom_qplanes -> the fused kernels
//   8  S2_VRTSFL    thermf and thermf_cesm: the reference's local array vrtsfl; flux kernel -> correction kernel
//   9  S2_PBFACM    tmsmt2: pb / p(kk+1) of pbcor2's folded column pass (StepState::pbcor2_dp_in_wk)
//  10  S2_BVFBOT    difest_isobml: k_dfi_vert_a -> k_dfi_vert_b
//  11  S2_EXPB      difest_isobml: exp(pbot / q); likewise
// (no comment inside an enum of this file: tools/kernel_rw_sets.py splits the members at the commas)
enum Wk2dSlot {
  S2_PBFACO = 0, S2_REMAP_PM = S2_PBFACO, S2_PBFACN = 1, S2_PBUT = S2_PBFACN, S2_PBVT = 2, S2_DRAG = 3, S2_QUM = 4, S2_VRTSFL = 8,
  S2_PBFACM = 9, S2_BVFBOT = 10, S2_EXPB = 11, S2_NEXT_FREE = 12
};
static_assert(S2_QUM + 4 == S2_VRTSFL && S2_NEXT_FREE <= NWK2D, "momtum's four planes end in front of thermf's; the planes fit");

// ==== wk: nwk fields of kk levels each, WK(V, slot) ======================================================================================
// how many there are (blomgpu_create); the stages' run-time "work space too small" checks compare with DevView::nwk
constexpr int wk_slots(int ntr) { return 32 + 5 * (ntr > 0 ? ntr : 1); }

// ---- cppm (stage_cppm.hip), inside advect with advmth = cppm; ntl = 2 + ntr transported quantities (T, S, tracers)
enum { CP_HM = 0, CP_HF, CP_HPC0, CP_HPC1, CP_HPC2, CP_TE };      // CP_TE + nt: one per transported quantity
#define CP_HTF(ntl) (CP_TE + (ntl))
#define CP_TPC0(ntl) (CP_TE + 2 * (ntl))
#define CP_TPC1(ntl) (CP_TE + 3 * (ntl))
#define CP_TPC2(ntl) (CP_TE + 4 * (ntl))
#define CP_NSLOT(ntl) (CP_TE + 5 * (ntl))

// ---- remap (remap_common.h, stage_advect.hip, stage_remap_tile.hip), inside advect with advmth = remap.  RG_*: the numbering of the
// limited gradients (rows of the tile kernel's LDS array today); RF_* behind them: the flux planes, tile kernel -> k_remap_update (lean_fluxes = 0)
enum { RG_DX = 0, RG_DY, RG_TX, RG_TY, RG_TD, RG_SX, RG_SY, RG_SD };
#define RG_TRX(nt) (8 + 3 * (nt))
#define RG_TRY(nt) (9 + 3 * (nt))
#define RG_TRD(nt) (10 + 3 * (nt))
#define F_BASE(ntr) (8 + 3 * (ntr))
#define RF_DU(ntr) (F_BASE(ntr) + 0)
#define RF_DV(ntr) (F_BASE(ntr) + 1)
#define RF_TU(ntr) (F_BASE(ntr) + 2)
#define RF_TV(ntr) (F_BASE(ntr) + 3)
#define RF_SU(ntr) (F_BASE(ntr) + 4)
#define RF_SV(ntr) (F_BASE(ntr) + 5)
#define RF_TRU(ntr, nt) (F_BASE(ntr) + 6 + 2 * (nt))
#define RF_TRV(ntr, nt) (F_BASE(ntr) + 7 + 2 * (nt))
// ---- the hand-over remap -> pbcor1 (remap_fold, StepState::remap_handed_over): k_remap_tile<.., FOLD = true> leaves the new dp, T, S and
// advected tracers of level kn in the slots of the flux planes, which nothing uses then; live from advect to pbcor1's tile kernel
#define R_BASE(ntr) (8 + 3 * (ntr))
#define R_DP(ntr) (R_BASE(ntr) + 0)
#define R_T(ntr) (R_BASE(ntr) + 1)
#define R_S(ntr) (R_BASE(ntr) + 2)
#define R_TR(ntr, nt) (R_BASE(ntr) + 3 + (nt))
static_assert(F_BASE(3) == R_BASE(3) && F_BASE(0) == R_BASE(0), "R_DP.. reuse the flux planes' slots");

// ---- the new state of pbcor's tile kernel (stage_pbcor_tile.hip), and two hand-overs under the same names: pbcor1 -> diffus (S, T, tracers:
// StepState::pbcor1_handed_over, stage_diffus.hip) and pbcor2 -> tmsmt2 (pbcor2_handed_over, with pbcor2_dp_in_wk also dp; stage_simple.hip)
enum { N_DP = 0, N_S = 1, N_T = 2 };
#define N_TR(nt) (3 + (nt))
// R_* is read while N_* is written by the same kernel (k_pbc_tile, from_remap): the two families must not overlap
static_assert(R_BASE(0) > N_TR(0) - 1 && R_BASE(64) > N_TR(64 - 1), "remap's hand-over lies behind pbcor's new state");

// ---- difest_isobml (stage_difest_iso.hip), from k_dfi_uv2 to k_dfi_lateral / k_dfi_smooth
enum { DF_DU2 = 0, DF_DV2, DF_BVFSQ, DF_BVF, DF_EGR, DF_ANISOK, DF_SM1, DF_SM2, DF_NUB, DF_NSLOT };

// ---- cmnfld2 (stage_cmnfld.hip).  Inside blomgpu_step k_cmn_bfsqf runs on the second stream BESIDE difest_isobml's kernels (phys_dag bit 1):
// its slot lies behind theirs.  CM_GAM_ALE: the hybrid coordinate's kernel (st_cmnfld_bfsqi_ale), on the context's stream
enum { CM_DELP = 0, CM_BFSQ, CM_SLS2, CM_GAM_ALE, CM_GAM = DF_NSLOT, CM_NSLOT };
static_assert(CM_GAM >= DF_NSLOT, "cmnfld2 beside difest_isobml: no common slot");

// ---- eddtra (stage_eddtra.hip): per component (u: 0.., v: ED_NSLOT..); mfl needs kk + 1 levels and borrows the first level of the next slot
enum { ED_MFL = 0, ED_SPARE, ED_DLM, ED_DLP, ED_NSLOT };
// ---- eddtra_ale (stage_eddtra_ale.hip): the arrays of a column inside the kernel's wavefront-major layout of wk (not WK slots)
enum { EA_PUV = 0, EA_GM, EA_SM, EA_MFL, EA_DLM, EA_DLP, EA_NARR };
// ---- diapfl (stage_diapfl.hip): per component of the momentum mixing, k_diapfl_column3 -> k_diapfl_momentum
enum { U_GTD = 0, U_NSLOT };
// ---- diapfl's column kernel (stage_diapfl_col3.hip): the values of a level in its wavefront-major layout of wk (not WK slots)
enum { D3_SU = 0, D3_SL, D3_FCU, D3_FCL, D3_FMAX, D3_H, D3_R, D3_T, D3_F, D3_FT, D3_GTD, D3_NSLOT };
// ---- convec (stage_convec.hip): the remapped velocity column, u then v; k_convec_velocity only
enum { CV_UN = 0 };
// ---- pgforc with pgfmth = dynamic enthalpy (stage_pgforc.hip): k_pgf_dynh_col -> k_pgf_dynh_uv
enum { DH_POT = 0, DH_POTPB, DH_A, DH_T, DH_ALPR, DH_NSLOT };
// ---- ale_vdifft / ale_vdiffm (stage_ale_vdiff.hip): the tridiagonal solver's gam, for T | u and for S | v; inside one kernel
enum { VD_GAM0 = 0, VD_GAM1 };
// ---- momtum's fused kernels (stage_momtum_fused.hip): these index momtum's OWN work space wk_mom (the views VIEW_MOM_*), not wk: the
// viscous chain runs beside the stages between difest and momtum
enum { MF_VISU = 0, MF_VISV, MF_UM, MF_UN, MF_VM, MF_VN, MF_NSLOT };

// ---- every stage's demand fits into wk_slots(ntr): the slot behind a stage's last one, as the stage's run-time check states it
constexpr int wk_need_cppm(int ntr) { return CP_NSLOT(2 + ntr); }
constexpr int wk_need_remap(int ntr) { return ntr > 0 ? RF_TRV(ntr, ntr - 1) + 1 : RF_SV(ntr) + 1; }
constexpr int wk_need_handover(int ntr) { return R_TR(ntr, ntr); }
constexpr int wk_need_pbcor(int ntr) { return N_TR(ntr); }
constexpr int wk_max(int a, int b) { return a > b ? a : b; }
constexpr int wk_need_fixed() {
  return wk_max(wk_max(wk_max(DF_NSLOT, CM_NSLOT), wk_max(2 * ED_NSLOT, 2 * EA_NARR + 3)),
                wk_max(wk_max(2 * U_NSLOT, D3_NSLOT), wk_max(wk_max(CV_UN + 2, DH_NSLOT), VD_GAM1 + 1)));
}
constexpr bool wk_fits(int ntr) {
  return wk_need_cppm(ntr) <= wk_slots(ntr) && wk_need_remap(ntr) <= wk_slots(ntr) && wk_need_handover(ntr) <= wk_slots(ntr) &&
         wk_need_pbcor(ntr) <= wk_slots(ntr) && wk_need_fixed() <= wk_slots(ntr);
}
static_assert(wk_fits(0) && wk_fits(1) && wk_fits(3) && wk_fits(24) && wk_fits(64), "a stage's slots do not fit into wk_slots(ntr)");
