// diaacc: the time-mean diagnostics of phy/mod_dia.F90 accumulated on the device (phy/mod_blom_step.F90:239).
//
// The reference's accumulators are `acc = acc + fld*w` (acch2d :5182, acclyr :5471), `acc = max(acc, fld)` (maxh2d :5285) and
// `acc = acc + fld*fld` (sqh2d :5409) at the owned points i = 1..ii, j = 1..jj where the grid's own mask is set, starting from
// `inival*mask` over the whole padded plane (inih2d :5001, inilyr :5055).  No bit depends on an order of summation, there is no
// halo and no communication: pure streaming read-modify-write, HBM-bound.
//
// The selected accumulators live in ONE allocation [slot][level][padded plane] in the model's plane layout.  A step launches
// k_diaacc twice: once over (plane, level) for all selected layer accumulators, once over the plane for the 2-D ones.  One thread
// per point and level; it loads its masks (mpack) once, each weight dp / dpu / dpv (km) and each shared source ub / vb (m) once,
// and then walks the slot table -- a table of ints in the kernel arguments, fetched with scalar loads in a
// wave-uniform loop -- DIA_U slots at a time: all loads of the group are issued before its stores.
// Algorithmic bytes per launch: (2 n_acc + n_distinct_sources) F.
//
// The z-level (Levitus) accumulators -- diazlv (:4737-4993) + acclvl (:5709-5781), called per layer from diaacc (:2000-2053,
// :2119-2168, :2222-2271) -- are k_dialvl further down: one thread per column of a grid, one launch per grid with a selected name.
// Under cntiso_hybrid / plevel four of them -- templvl salnlvl uvellvl vvellvl -- are not diaacc's (:1944, :2059, :2174): stage_ale.hip remaps
// the step's vertical reconstructions onto the levels and adds them to these slots (dia_hybrid_slots), at the start or at the end of a step
// as the output alarm the host declares says (dia_alarm; phy/mod_ale_regrid_remap.F90:1524-1531, :2014-2017).
//
// The mass fluxes binned into the diagnostic density classes sigdia (:1368-1538) are k_diasig at the end of the kernels: one thread
// per column of the u- or v-grid, the classes' bins of the step in LDS.  The first family that communicates: the one-point halo of
// sigint is exchanged in front of it (:1392).
//
// The vertical mass flux and its square, on the layers and on the depth levels (diavfl, :4633-4733, called at :2279), are k_diavfl_lyr
// and k_diavfl_lvl: the first family that reads a neighbour of a source, that exchanges accumulators between tiles (uflxlvl, vflxlvl,
// :4681-4684), and that needs the dpold of the previous step (api.hip keeps tmsmt1 unfolded while it is selected).
//
// The diagnostics diaacc derives from the step's water column before it accumulates them -- sbot tbot (:1251-1294), t20d t17d
// (:1296-1366), the Levitus-82 mixed layer depth mldl82 with its minimum, maximum and square (:1706, :1755, :1758, :1773; the field is
// cmnfld1's, stage_cmnfld.hip) -- are k_diacol; the layer potential vorticity pair avdsg dpvor (:1203-1249) is k_diapv.
#include "../../include/blomgpu.h"
#include "blomgpu_internal.h"
#include <cstring>

namespace {
enum { G_P = 0, G_U = 1, G_V = 2 };                 // the grid = the bit of mpack that masks it
enum { OP_SUM = 0, OP_MAX = 1, OP_SQ = 2, OP_LVL = 3, OP_LVLFLX = 4, OP_CLS = 5,     // acclvl with diazlv's weights | weightsflx; the density classes
       OP_VFL = 6, OP_OLD = 7,      // diavfl's own rows, and the two level slots it keeps last step's uflxlvl / vflxlvl in: no table-driven launch touches them
       OP_COL = 8, OP_PV = 9 };     // k_diacol's and k_diapv's rows: likewise
// what a row of k_diacol is (DiaRow::src of an OP_COL row): the two bottom values, the two isotherm depths, mldl82 summed | min | max | squared
enum { C_SBOT = 0, C_TBOT, C_T20D, C_T17D, C_ML, C_MLMN, C_MLMX, C_MLSQ, C_N };
enum { W_NONE = 0, W_DP = 1, W_DPU = 2, W_DPV = 3 };       // weight (km); also: the register a source is taken from
enum { A_NONE = 0, A_UB = 1, A_VB = 2, A_PLANE = 3, A_ONEM = 4 };   // fld = src + ub(m) | src + vb(m) | src + a second plane | src*onem
// the level of the source that the reference passes (0-based plane of the field; a layer row adds its layer)
enum { LV_0, LV_M, LV_N, LV_KK, LV_MM, LV_NN, LV_TKE, LV_GLS };
enum { SRC_DPML = -1 };                             // dpml as :1148-1171 forms it
// (SPVAL: -spval is the inival of maxbld (:5948) and mldl82mx (:5901), +spval of mldl82mn (:5900))
constexpr double DPBOT = ONEM;                      // phy/mod_dia.F90:196
constexpr double EPSIL = 1.e-11, NF90_FILL_DOUBLE = 9.9692099683868690e+36;   // finlyr, :6126, :6140
constexpr double SIGEPS = 1.e-9;                    // phy/mod_dia.F90:1120
constexpr double DZEPS = 1e1 * EPSILP, DPEPS = 1e5 * EPSILP, FLXEPS = 1e5 * EPSILP;   // diazlv, :4760-4762

// One row per accumulator; the name is the reference's ACC_* suffix in lower case, `line` the call in phy/mod_dia.F90.
struct DiaRow { const char *name; int lyr, grid, op, src, lev, wgt, aux, line; };   // lyr: 0 2-D, 1 kk layers, 2 ddm depth levels, 3 kk density classes
#define H2D(nm, g, f, lv, ln) {#nm, 0, g, OP_SUM, f, lv, W_NONE, A_NONE, ln}
#define LYR(nm, g, f, lv, w, ln) {#nm, 1, g, OP_SUM, f, lv, w, A_NONE, ln}
#define LVF(nm, g, f, ln) {#nm, 2, g, OP_LVLFLX, f, LV_NN, W_NONE, A_NONE, ln}
#define LVP(nm, f, lv, ln) {#nm, 2, G_P, OP_LVL, f, lv, W_NONE, A_NONE, ln}
#define CLS(nm, g, f, ln) {#nm, 3, g, OP_CLS, f, LV_NN, W_NONE, A_NONE, ln}
#define VFL(nm, kind, g, op, f, ln) {#nm, kind, g, op, f, LV_NN, W_NONE, A_NONE, ln}
#define COL(nm, what, ln) {#nm, 0, G_P, OP_COL, what, LV_0, W_NONE, A_NONE, ln}
const DiaRow g_rows[] = {
  // ---- acch2d, :1547-1745 ----
  H2D(ub, G_U, F_ub, LV_M, 1547), H2D(ubflxs, G_U, F_ubflxs, LV_N, 1550), H2D(taux, G_U, F_taux, LV_0, 1556),
  H2D(vb, G_V, F_vb, LV_M, 1565), H2D(vbflxs, G_V, F_vbflxs, LV_N, 1568), H2D(tauy, G_V, F_tauy, LV_0, 1574),
  H2D(psrf, G_P, F_p, LV_0, 1583), H2D(pbot, G_P, F_p, LV_KK, 1586), H2D(sealv, G_P, F_z, LV_0, 1589),
  H2D(sigmx, G_P, F_sigma, LV_MM, 1592), H2D(swa, G_P, F_swa, LV_0, 1616), H2D(nsf, G_P, F_nsf, LV_0, 1619),
  H2D(hmltfz, G_P, F_hmltfz, LV_0, 1625), H2D(lip, G_P, F_lip, LV_0, 1631), H2D(sop, G_P, F_sop, LV_0, 1634),
  H2D(eva, G_P, F_eva, LV_0, 1637), H2D(fmltfz, G_P, F_fmltfz, LV_0, 1640), H2D(sfl, G_P, F_sfl, LV_0, 1643),
  H2D(rnfflx, G_P, F_rnf, LV_0, 1649), H2D(rfiflx, G_P, F_rfi, LV_0, 1652), H2D(ustar, G_P, F_ustar, LV_0, 1655),
  H2D(ustar3, G_P, F_ustar3, LV_0, 1658), H2D(idkedt, G_P, F_idkedt, LV_0, 1661), H2D(mtkeus, G_P, F_mtkeus, LV_0, 1667),
  H2D(mtkeni, G_P, F_mtkeni, LV_0, 1670), H2D(mtkebf, G_P, F_mtkebf, LV_0, 1673), H2D(mtkers, G_P, F_mtkers, LV_0, 1676),
  H2D(mtkepe, G_P, F_mtkepe, LV_0, 1679), H2D(mtkeke, G_P, F_mtkeke, LV_0, 1682), H2D(sss, G_P, F_saln, LV_MM, 1691),
  H2D(sst, G_P, F_temp, LV_MM, 1694), H2D(bld, G_P, SRC_DPML, LV_0, 1703), H2D(surflx, G_P, F_surflx, LV_0, 1718),
  H2D(salflx, G_P, F_salflx, LV_0, 1721), H2D(surrlx, G_P, F_surrlx, LV_0, 1724), H2D(salrlx, G_P, F_salrlx, LV_0, 1727),
  H2D(brnflx, G_P, F_brnflx, LV_0, 1730), H2D(brnpd, G_P, F_pbrnda, LV_0, 1733),
  // ---- maxh2d, :1752 ----
  {"maxbld", 0, G_P, OP_MAX, SRC_DPML, LV_0, W_NONE, A_NONE, 1752},
  // ---- sqh2d, :1780-1786 ----
  {"slvsq", 0, G_P, OP_SQ, F_z, LV_0, W_NONE, A_NONE, 1780}, {"ssssq", 0, G_P, OP_SQ, F_saln, LV_MM, W_NONE, A_NONE, 1783},
  {"sstsq", 0, G_P, OP_SQ, F_temp, LV_MM, W_NONE, A_NONE, 1786},
  // ---- acclyr, :1793-1913 (uvel = u(km) + ub(m), :1173-1186; vvel likewise) ----
  {"uvel", 1, G_U, OP_SUM, F_u, LV_MM, W_DPU, A_UB, 1793}, LYR(dpu, G_U, F_dpu, LV_MM, W_NONE, 1796),
  LYR(uflx, G_U, F_uflx, LV_NN, W_NONE, 1799), LYR(utflx, G_U, F_utflx, LV_NN, W_NONE, 1802), LYR(usflx, G_U, F_usflx, LV_NN, W_NONE, 1805),
  LYR(umfltd, G_U, F_umfltd, LV_NN, W_NONE, 1808), LYR(umflsm, G_U, F_umflsm, LV_NN, W_NONE, 1811),
  LYR(utfltd, G_U, F_utfltd, LV_NN, W_NONE, 1814), LYR(utflsm, G_U, F_utflsm, LV_NN, W_NONE, 1817),
  LYR(utflld, G_U, F_utflld, LV_NN, W_NONE, 1820), LYR(usfltd, G_U, F_usfltd, LV_NN, W_NONE, 1823),
  LYR(usflsm, G_U, F_usflsm, LV_NN, W_NONE, 1826), LYR(usflld, G_U, F_usflld, LV_NN, W_NONE, 1829),
  {"vvel", 1, G_V, OP_SUM, F_v, LV_MM, W_DPV, A_VB, 1832}, LYR(dpv, G_V, F_dpv, LV_MM, W_NONE, 1835),
  LYR(vflx, G_V, F_vflx, LV_NN, W_NONE, 1838), LYR(vtflx, G_V, F_vtflx, LV_NN, W_NONE, 1841), LYR(vsflx, G_V, F_vsflx, LV_NN, W_NONE, 1844),
  LYR(vmfltd, G_V, F_vmfltd, LV_NN, W_NONE, 1847), LYR(vmflsm, G_V, F_vmflsm, LV_NN, W_NONE, 1850),
  LYR(vtfltd, G_V, F_vtfltd, LV_NN, W_NONE, 1853), LYR(vtflsm, G_V, F_vtflsm, LV_NN, W_NONE, 1856),
  LYR(vtflld, G_V, F_vtflld, LV_NN, W_NONE, 1859), LYR(vsfltd, G_V, F_vsfltd, LV_NN, W_NONE, 1862),
  LYR(vsflsm, G_V, F_vsflsm, LV_NN, W_NONE, 1865), LYR(vsflld, G_V, F_vsflld, LV_NN, W_NONE, 1868),
  LYR(saln, G_P, F_saln, LV_MM, W_DP, 1871), LYR(temp, G_P, F_temp, LV_MM, W_DP, 1874), LYR(dp, G_P, F_dp, LV_MM, W_NONE, 1877),
  LYR(dz, G_P, F_dz, LV_0, W_NONE, 1880), LYR(bfsq, G_P, F_bfsql, LV_0, W_DP, 1883), LYR(difint, G_P, F_difint, LV_0, W_DP, 1886),
  LYR(difiso, G_P, F_difiso, LV_0, W_DP, 1889), LYR(difdia, G_P, F_difdia, LV_0, W_DP, 1893),
  LYR(tke, G_P, F_trc, LV_TKE, W_DP, 1909), LYR(gls_psi, G_P, F_trc, LV_GLS, W_DP, 1913),
  // ---- acclvl on the u-grid, :2010-2054 (isopyc_bulkml; :1955-1996 otherwise, without uvellvl) ----
  {"uvellvl", 2, G_U, OP_LVL, F_u, LV_MM, W_NONE, A_UB, 2010}, LVF(uflxlvl, G_U, F_uflx, 2013), LVF(utflxlvl, G_U, F_utflx, 2017),
  LVF(usflxlvl, G_U, F_usflx, 2021), LVF(umfltdlvl, G_U, F_umfltd, 2025), LVF(umflsmlvl, G_U, F_umflsm, 2029),
  LVF(utfltdlvl, G_U, F_utfltd, 2033), LVF(utflsmlvl, G_U, F_utflsm, 2037), LVF(utflldlvl, G_U, F_utflld, 2041),
  LVF(usfltdlvl, G_U, F_usfltd, 2045), LVF(usflsmlvl, G_U, F_usflsm, 2049), LVF(usflldlvl, G_U, F_usflld, 2053),
  // ---- the v-grid, :2125-2169 (:2070-2111 otherwise, without vvellvl) ----
  {"vvellvl", 2, G_V, OP_LVL, F_v, LV_MM, W_NONE, A_VB, 2125}, LVF(vflxlvl, G_V, F_vflx, 2128), LVF(vtflxlvl, G_V, F_vtflx, 2132),
  LVF(vsflxlvl, G_V, F_vsflx, 2136), LVF(vmfltdlvl, G_V, F_vmfltd, 2140), LVF(vmflsmlvl, G_V, F_vmflsm, 2144),
  LVF(vtfltdlvl, G_V, F_vtfltd, 2148), LVF(vtflsmlvl, G_V, F_vtflsm, 2152), LVF(vtflldlvl, G_V, F_vtflld, 2156),
  LVF(vsfltdlvl, G_V, F_vsfltd, 2160), LVF(vsflsmlvl, G_V, F_vsflsm, 2164), LVF(vsflldlvl, G_V, F_vsflld, 2168),
  // ---- the p-grid, :2233-2271 (:2185-2217 otherwise, without salnlvl and templvl) ----
  LVP(salnlvl, F_saln, LV_MM, 2233), LVP(templvl, F_temp, LV_MM, 2236), LVP(bfsqlvl, F_bfsql, LV_0, 2239),
  LVP(difintlvl, F_difint, LV_0, 2242), LVP(difisolvl, F_difiso, LV_0, 2245), LVP(difdialvl, F_difdia, LV_0, 2248),
  LVP(tkelvl, F_trc, LV_TKE, 2264), LVP(gls_psilvl, F_trc, LV_GLS, 2267), LVP(dzlvl, F_dz, LV_0, 2271),
  // ---- the density classes, :1368-1538: acclyr of the step's bins.  Enumerated by blomgpu_dia_name_all only ----
  CLS(umfll, G_U, F_uflx, 1457), CLS(umfltdl, G_U, F_umfltd, 1461), CLS(umflsml, G_U, F_umflsm, 1465),
  CLS(vmfll, G_V, F_vflx, 1530), CLS(vmfltdl, G_V, F_vmfltd, 1534), CLS(vmflsml, G_V, F_vmflsm, 1538),
  // ---- diavfl, :4633-4733: the vertical mass flux and its square on the layers and on the depth levels; one group (diaini :615-618,
  // :644-647, :673-680).  Then ACC_UFLXOLD / ACC_VFLXOLD (:1921-1942), slots of the group that no name selects.  Enumerated by
  // blomgpu_dia_name_full only ----
  VFL(wflx, 1, G_P, OP_VFL, F_uflx, 4667), VFL(wflx2, 1, G_P, OP_VFL, F_uflx, 4669),
  VFL(wflxlvl, 2, G_P, OP_VFL, F_uflx, 4722), VFL(wflx2lvl, 2, G_P, OP_VFL, F_uflx, 4724),
  VFL(uflxold, 2, G_U, OP_OLD, F_uflx, 1928), VFL(vflxold, 2, G_V, OP_OLD, F_vflx, 1934),
  // ---- the column-derived diagnostics (k_diacol): acch2d :1697-1715, minh2d :1755, maxh2d :1758, sqh2d :1773 of fields that diaacc
  // (:1251-1366) and cmnfld1 (phy/mod_cmnfld_routines.F90:933-995) form from the step's column; then the layer pair of :1203-1249
  // (k_diapv; acclyr :1244, :1247), one group (diaini :681-682).  Enumerated by blomgpu_dia_name_ext only ----
  COL(sbot, C_SBOT, 1697), COL(tbot, C_TBOT, 1700), COL(t20d, C_T20D, 1712), COL(t17d, C_T17D, 1715),
  COL(mldl82, C_ML, 1706), COL(mldl82mn, C_MLMN, 1755), COL(mldl82mx, C_MLMX, 1758), COL(mldl82sq, C_MLSQ, 1773),
  {"avdsg", 1, G_P, OP_PV, F_absvor, LV_0, W_NONE, A_NONE, 1244}, {"dpvor", 1, G_P, OP_PV, F_dpvor, LV_0, W_NONE, A_NONE, 1247},
};
#undef COL
#undef H2D
#undef LYR
#undef LVF
#undef LVP
#undef CLS
#undef VFL
constexpr int NROW = (int)(sizeof(g_rows) / sizeof(g_rows[0]));
constexpr int NROW_CLS = 6, NROW_VFL = 6, NROW_COL = 10;
constexpr int NROW_FULL = NROW - NROW_COL;         // blomgpu_dia_name_full stops in front of the column-derived rows,
constexpr int NROW_ALL = NROW_FULL - NROW_VFL;     // blomgpu_dia_name_all in front of diavfl's,
constexpr int NROW_NAMED = NROW_ALL - NROW_CLS;    // blomgpu_dia_name in front of the class rows
constexpr int KIND_INTERNAL = 4;                   // what blomgpu_dia_name_full reports for uflxold / vflxold: ddm levels, selected by the group only

// depthslev_bnds as its ddm + 1 edges: bnds(1,d) = edge[d-1], bnds(2,d) = edge[d] (:119-128; with LEVITUS2X :142-159)
const double g_edges35[] = {0., 5., 15., 25., 40., 62.5, 87.5, 112.5, 137.5, 175., 225., 275., 350., 450., 550., 650., 750., 850., 950., 1050.,
  1150., 1250., 1350., 1450., 1625., 1875., 2250., 2750., 3250., 3750., 4250., 4750., 5250., 5750., 6250., 8000.};
const double g_edges70[] = {0., 2.5, 7.5, 12.5, 17.5, 22.5, 27.5, 35., 45., 56.2, 68.8, 81.2, 93.8, 106.2, 118.8, 131.2, 143.8, 162.5, 187.5,
  212.5, 237.5, 262.5, 287.5, 325., 375., 425., 475., 525., 575., 625., 675., 725., 775., 825., 875., 925., 975., 1025., 1075., 1125.,
  1175., 1225., 1275., 1325., 1375., 1425., 1475., 1562.5, 1687.5, 1812.5, 1937.5, 2125., 2375., 2625., 2875., 3125., 3375., 3625.,
  3875., 4125., 4375., 4625., 4875., 5125., 5375., 5625., 5875., 6125., 6375., 6625., 8000.};
static_assert(sizeof(g_edges35) == 36 * sizeof(double) && sizeof(g_edges70) == 71 * sizeof(double), "ddm = 35 | 70");

int find_row(const std::string &name) {
  for (int r = 0; r < NROW; r++)
    if (name == g_rows[r].name) return r;
  return -1;
}
}  // namespace

// the selection of a context (blomgpu_dia_select) and its accumulators
struct DiaState {
  std::vector<int> rows;        // the selected rows in the table's order: 2-D slots first, then the layer slots
  std::vector<int> plane0;      // first plane of each slot in `acc`
  size_t nplanes = 0;
  double *acc = nullptr;
  int nacc = 0;                 // nacc_phy, :1123-1125
  bool needs_z = false;         // a selected row reads z or dz (cmnfld1's output)
  int ddm = 0;                  // levels of a depth-level slot; 0: none selected.  Their ddm + 1 edges lie behind the last plane of `acc`
  double *edges() const { return acc + nplanes * np; }
  int ncls = 0;                 // selected density-class slots; their kk class densities lie behind the edges
  bool vfl = false;             // diavfl's group is selected: wflx wflx2 wflxlvl wflx2lvl uflx vflx uflxlvl vflxlvl uflxold vflxold
  bool col = false, ml82 = false, pv = false;   // a row of k_diacol is selected; one of mldl82 mldl82mn mldl82mx mldl82sq; avdsg dpvor
  unsigned msc = 0;             // the selected msc names (stage_diaout.hip: bit = its row there); they have no slot, their sources have
  bool finalized = false;       // blomgpu_dia_finalize has run since the last initialisation: the level rows hold fill values
  double *sigdia() const { return edges() + (ddm ? ddm + 1 : 0); }
  size_t np = 0;
  int slot_of(int row) const {
    for (size_t s = 0; s < rows.size(); s++)
      if (rows[s] == row) return (int)s;
    return -1;
  }
};

// ---- the slot table a launch carries ------------------------------------------------------------------------------------------
#define DIA_MAXSLOT 42         // the larger of the table's 2-D (42) and layer (36) row counts
#ifndef DIA_U
#define DIA_U 4                // slots whose loads are in flight together
#endif
// per slot: [0] source field, [1] source plane (of layer 1), [2] second plane's field, [3] its plane, [4] code, [5] first plane of the
// slot in the allocation.  code = grid | op << 2 | weight << 4 | aux << 6 | source register << 9 (W_*: the source IS that weight)
struct DiaTab {
  int n, need;                 // need: bit 0 dp, 1 dpu, 2 dpv (km), 3 ub, 4 vb (m) are loaded
  int lyr, mlev;               // 1: blockIdx.y is the layer; m - 1
  int d[DIA_MAXSLOT][6];
};

__global__ __launch_bounds__(256) void k_diaacc(const DevView *__restrict__ Vp, double *__restrict__ accp, const DiaTab T, int mm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj) return;          // owned points only: min(ii, il*) on the u-grid too (:5209)
  const int msk = V.m[I_mpack][t] & 7;
  if (!msk) return;
  const int k = T.lyr ? (int)by : 0;
  const size_t np = V.nplane, c = t, okm = c + (size_t)(mm + k) * np;
  gd_t acc = global_ptr(accp);
  // each weight and each shared source once per point
  const double wdp = (T.need & 1) && (msk & 1) ? V.f[F_dp][okm] : 0.;
  const double wdpu = (T.need & 2) && (msk & 2) ? V.f[F_dpu][okm] : 0.;
  const double wdpv = (T.need & 4) && (msk & 4) ? V.f[F_dpv][okm] : 0.;
  const double sub = (T.need & 8) && (msk & 2) ? V.f[F_ub][c + (size_t)T.mlev * np] : 0.;
  const double svb = (T.need & 16) && (msk & 4) ? V.f[F_vb][c + (size_t)T.mlev * np] : 0.;
  for (int s0 = 0; s0 < T.n; s0 += DIA_U) {                     // wave-uniform
    double a[DIA_U], v[DIA_U], x[DIA_U];
    size_t oa[DIA_U];
    bool on[DIA_U];
#pragma unroll
    for (int u = 0; u < DIA_U; u++) {
      const int s = s0 + u < T.n ? s0 + u : T.n - 1;             // (uniform; the table is read inside its bounds)
      const int code = T.d[s][4];
      on[u] = s0 + u < T.n && ((msk >> (code & 3)) & 1);
      oa[u] = c + ((size_t)T.d[s][5] + k) * np;
      a[u] = v[u] = x[u] = 0.;
      if (on[u]) {
        a[u] = acc[oa[u]];
        if (!((code >> 9) & 3)) v[u] = V.f[T.d[s][0]][c + ((size_t)T.d[s][1] + k) * np];
        if (((code >> 6) & 7) == A_PLANE) x[u] = V.f[T.d[s][2]][c + (size_t)T.d[s][3] * np];
      }
    }
    // (selects on wave-uniform codes, no branches: the group's arithmetic is straight-line code between its loads and its stores)
    double r[DIA_U];
#pragma unroll
    for (int u = 0; u < DIA_U; u++) {
      const int s = s0 + u < T.n ? s0 + u : T.n - 1, code = T.d[s][4];
      const int op = (code >> 2) & 3, wg = (code >> 4) & 3, aux = (code >> 6) & 7, sr = (code >> 9) & 3;
      double f = sr == W_DP ? wdp : sr == W_DPU ? wdpu : sr == W_DPV ? wdpv : v[u];
      // fld = u(km) + ub(m) (:1180) | v(km) + vb(m) (:1195) | dp(1+mm) + dp(2+mm) (:1155) | OBLdepth*onem (:1165)
      f = aux == A_UB ? f + sub : aux == A_VB ? f + svb : aux == A_PLANE ? f + x[u] : aux == A_ONEM ? f * ONEM : f;
      const double w = wg == W_DP ? wdp : wg == W_DPU ? wdpu : wdpv;
      // acc + fld*fld (:5454) | acc + fld*wghts (:5266, :5513) | acc + fld (:5256, :5500) | max(acc, fld) (:5330) as amdflang lowers it
      const double add = op == OP_SQ ? f * f : wg ? f * w : f;
      r[u] = op == OP_MAX ? fmax2(a[u], f) : a[u] + add;
    }
#pragma unroll
    for (int u = 0; u < DIA_U; u++)
      if (on[u]) acc[oa[u]] = r[u];
  }
}

// inih2d / inilyr (:5001-5113): inival*mask over the WHOLE padded plane (so land is -0.0 under maxbld's -spval, +0.0 under mldl82mn's +spval)
#define DIA_MAXINI 136
static_assert(NROW <= DIA_MAXINI, "k_dia_init carries one entry per selected row");
struct DiaIni { int n; int d[DIA_MAXINI][3]; };                 // per slot: first plane, levels, grid | inival << 2 (0: 0., 1: -spval, 2: +spval)
__global__ __launch_bounds__(256) void k_dia_init(const DevView *__restrict__ Vp, double *__restrict__ accp, const DiaIni T) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x, k = by;
  if (t >= V.nplane) return;
  const int msk = V.m[I_mpack][t];
  gd_t acc = global_ptr(accp);
  for (int s = 0; s < T.n; s++) {
    if (k >= T.d[s][1]) continue;
    const int iv = T.d[s][2] >> 2;
    const double inival = iv == 1 ? -SPVAL : iv == 2 ? SPVAL : 0.;
    acc[(size_t)t + ((size_t)T.d[s][0] + k) * V.nplane] = inival * (double)((msk >> (T.d[s][2] & 3)) & 1);
  }
}

// finlyr (:6114-6185) in place: acc / wgt where wgt > epsil, else nf90_fill_double; one (slot, weight slot) pair per launch
__global__ __launch_bounds__(256) void k_dia_finlyr(const DevView *__restrict__ Vp, double *__restrict__ accp, int pa, int pw, int grid) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x, k = by;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj || !((V.m[I_mpack][t] >> grid) & 1)) return;
  gd_t acc = global_ptr(accp);
  const size_t oa = (size_t)t + ((size_t)pa + k) * V.nplane, ow = (size_t)t + ((size_t)pw + k) * V.nplane;
  const double w = acc[ow], a = acc[oa];
  acc[oa] = w > EPSIL ? a / w : NF90_FILL_DOUBLE;
}

// ---- the depth levels: diazlv + acclvl ------------------------------------------------------------------------------------------
// One thread per column of grid G (owned points with the grid's mask bit, as above; the reference's extra u-column ii+1 and v-row
// jj+1 are the neighbour tile's and never written to a file).  Sweep 1 is the column's total thickness (:4806-4816 | :4839-4849 |
// :4872-4882), sweep 2 walks the layers with the reference's own loop over the levels (:4915-4927 | :4940-4953 | :4966-4979): the
// carried ind1, `cycle`, `exit`, the comparisons non-strict on p and strict on u / v.  zbot(k) = sum(1..k)*bath/sum(1..kk) with the
// sum in k order (:4819-4830: the product first; zbot(kk) is rescaled last, so every layer divides by the unscaled total).
// A grid's slots (<= 12) are dealt to blockIdx.y four at a time.  The accumulators of ONE level -- the one the lane is in -- live in
// registers for the thread's slots: a one-entry cache keyed by the level, loaded when the lane enters a level, stored when it leaves.  So every element gets its additions in ascending k
// starting from the value in memory, is read and written once a step, and a u / v layer that re-enters the level above because a
// bound EQUALS its top (it adds fld*0 there) finds that level's values in memory again.
// Algorithmic bytes per grid: (2 n_acc ddm + (n_src + 2) kk) planes.
#define LVL_MAXSLOT 12
#define DIA_MAXLEV 128
struct LvlTab {
  int n, ddm, mlev;            // slots, levels, m - 1
  int tfld, cfld, clev;        // thickness dp | dpu | dpv (at mm); the condition's field and first plane: dp (mm) | uflx | vflx (nn)
  int d[LVL_MAXSLOT][4];       // source field, plane of its layer 1, bit 0: weightsflx, bit 1: + ub | vb (m), first plane of the slot
};

#define LVL_NS 4               // slots of a thread: a grid's slots are dealt to blockIdx.y in groups of four
#define LVL_KB 2               // layers ahead whose sources are in flight (3: 142 VGPRs on u / v)
template <int G>
__global__ __launch_bounds__(256) void k_dialvl(const DevView *__restrict__ Vp, double *__restrict__ accp, const double *__restrict__ edgep, const LvlTab T, int mm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj) return;
  if (!((V.m[I_mpack][t] >> G) & 1)) return;
  const size_t np = V.nplane, c = t;
  const int kk = V.kk, ddm = T.ddm;
  const int s0 = (int)by * LVL_NS, ns = T.n - s0 < LVL_NS ? T.n - s0 : LVL_NS;      // wave-uniform
  gd_t acc = global_ptr(accp);
  gcd_t edge = global_ptr(edgep);                                 // bnds(1,d) = edge[d-1], bnds(2,d) = edge[d]
  gcd_t th = V.f[T.tfld] + (c + (size_t)mm * np), cs = V.f[T.cfld] + (c + (size_t)T.clev * np);
  // pbath | ubath | vbath, :1078-1088
  double bath = V.f[F_depths][c];
  if (G == G_U) bath = fmin2(bath, V.f[F_depths][c - 1]);
  if (G == G_V) bath = fmin2(bath, V.f[F_depths][c - V.ni]);
  // sweep 1: zbot(kk) before the rescaling
  double tot = 0.;
  for (int k0 = 0; k0 < kk; k0 += COLUMN_U) {
    double v[COLUMN_U];
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++) v[u] = th[(size_t)(k0 + u < kk ? k0 + u : kk - 1) * np];
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++)
      if (k0 + u < kk) {
        const double x = G == G_P ? v[u] : fmax2(v[u], DPEPS);
        tot = k0 + u == 0 ? x : tot + x;
      }
  }
  // sweep 2.  A slot's source and accumulators are a wave-uniform pointer plus the lane's offset.
  gcd_t sp[LVL_NS];
  gd_t ap[LVL_NS];
  int flx = 0, aux = 0;
#pragma unroll
  for (int s = 0; s < LVL_NS; s++) {
    const int q = s0 + (s < ns ? s : 0);
    sp[s] = V.f[T.d[q][0]] + (size_t)T.d[q][1] * np;
    ap[s] = acc + (size_t)T.d[q][3] * np;
    if (s < ns && (T.d[q][2] & 1)) flx |= 1 << s;
    if (s < ns && (T.d[q][2] & 2)) aux |= 1 << s;
  }
  const double sub = aux ? V.f[G == G_V ? F_vb : F_ub][c + (size_t)T.mlev * np] : 0.;      // uvel = u(km) + ub(m), :1180; vvel :1195
  // a: the level the lane is in (dc); an: the level below it (dn), requested when the lane entered dc, behind the store that the
  // entry issued -- so a lane that steps back one level (the u / v equality case) and forward again reads what it stored
  double a[LVL_NS], an[LVL_NS];
#pragma unroll
  for (int s = 0; s < LVL_NS; s++) a[s] = an[s] = 0.;
  double run = 0., ztop = 0.;
  int ind1 = 0, dc = -1, dn = -1;
  // the sources of the next LVL_KB layers wait in a queue of registers: layer k + LVL_KB is requested at the top of layer k
  double thq[LVL_KB], csq[LVL_KB], fq[LVL_KB][LVL_NS];
#pragma unroll
  for (int u = 0; u < LVL_KB; u++) {
    const size_t o = (size_t)(u < kk ? u : kk - 1) * np;
    thq[u] = th[o];
    csq[u] = cs[o];
#pragma unroll
    for (int s = 0; s < LVL_NS; s++) fq[u][s] = s < ns ? sp[s][c + o] : 0.;
  }
  for (int k = 0; k < kk; k++) {
    {
      const double thk = thq[0], csk = csq[0];
      double f[LVL_NS];
#pragma unroll
      for (int s = 0; s < LVL_NS; s++) f[s] = (aux >> s) & 1 ? fq[0][s] + sub : fq[0][s];
#pragma unroll
      for (int u = 0; u + 1 < LVL_KB; u++) {
        thq[u] = thq[u + 1];
        csq[u] = csq[u + 1];
#pragma unroll
        for (int s = 0; s < LVL_NS; s++) fq[u][s] = fq[u + 1][s];
      }
      {
        const size_t o = (size_t)(k + LVL_KB < kk ? k + LVL_KB : kk - 1) * np;
        thq[LVL_KB - 1] = th[o];
        csq[LVL_KB - 1] = cs[o];
#pragma unroll
        for (int s = 0; s < LVL_NS; s++)
          if (s < ns) fq[LVL_KB - 1][s] = sp[s][c + o];
      }
      const double x = G == G_P ? thk : fmax2(thk, DPEPS);
      run = k == 0 ? x : run + x;
      const double zbot = run * bath / tot;
      if (G == G_P ? csk > DPEPS : fabs(csk) > FLXEPS) {
        for (int d = ind1; d < ddm; d++) {
          const double lo = edge[d], hi = edge[d + 1];
          if (G == G_P ? hi <= ztop : hi < ztop) { ind1 = d + 1; continue; }
          if (G == G_P ? lo >= zbot : lo > zbot) break;
          if (d != dc) {
            const size_t od = c + (size_t)d * np;
            if (dc >= 0) {
#pragma unroll
              for (int s = 0; s < LVL_NS; s++)
                if (s < ns) ap[s][c + (size_t)dc * np] = a[s];
            }
            if (d == dn) {
#pragma unroll
              for (int s = 0; s < LVL_NS; s++) a[s] = an[s];
            } else {
#pragma unroll
              for (int s = 0; s < LVL_NS; s++)
                if (s < ns) a[s] = ap[s][od];
            }
            dc = d;
            dn = d + 1 < ddm ? d + 1 : -1;
            if (dn >= 0) {
#pragma unroll
              for (int s = 0; s < LVL_NS; s++)
                if (s < ns) an[s] = ap[s][od + np];
            }
          }
          const double r = fmin2(zbot, hi) - fmax2(ztop, lo);
          const double w = r / fmax2(DZEPS, fmin2(bath, hi) - lo);           // r/dlev(d), :4776-4789, :4924-4926 | :4951 | :4977
          const double wf = G == G_P ? 0. : r / (zbot - ztop);               // weightsflx, :4952 | :4978
#pragma unroll
          for (int s = 0; s < LVL_NS; s++)
            if (s < ns) a[s] = a[s] + f[s] * (G != G_P && ((flx >> s) & 1) ? wf : w);     // acclvl, :5741 | :5754 | :5767
        }
      }
      ztop = zbot;
    }
  }
  if (dc >= 0) {
#pragma unroll
    for (int s = 0; s < LVL_NS; s++)
      if (s < ns) ap[s][c + (size_t)dc * np] = a[s];
  }
}

// msklvl (:6659-6738): at EVERY owned point, wet or not, the levels behind kmax -- the last one whose upper bound lies above the
// bottom (of the shallower of the two p-points on u / v) -- become nf90_fill_double.  The bounds increase, so level d is kept
// exactly when bath > bnds(1,d).
struct MskTab { int n, ddm; int d[3 * LVL_MAXSLOT][2]; };         // per slot: first plane, grid
__global__ __launch_bounds__(256) void k_dia_msklvl(const DevView *__restrict__ Vp, double *__restrict__ accp, const double *__restrict__ edgep, const MskTab T) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x, d = by;
  if (t >= V.nplane || d >= T.ddm) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj) return;
  gd_t acc = global_ptr(accp);
  const double lo = global_ptr(edgep)[d], dep = V.f[F_depths][t];
  const double bath[3] = {dep, fmin2(dep, V.f[F_depths][t - 1]), fmin2(dep, V.f[F_depths][t - V.ni])};
  for (int s = 0; s < T.n; s++) {
    const double b = T.d[s][1] == G_P ? bath[0] : T.d[s][1] == G_U ? bath[1] : bath[2];
    if (!(b > lo)) acc[(size_t)t + ((size_t)T.d[s][0] + d) * V.nplane] = NF90_FILL_DOUBLE;
  }
}

// ---- the density classes: :1368-1538 ---------------------------------------------------------------------------------------------
// sigint at the owned p-points under isopyc_bulkml (:1372-1390): sigma(k1m) | .5*(sigma(km-1) + sigma(km)); nothing elsewhere
__global__ __launch_bounds__(256) void k_diasig_int(const DevView *__restrict__ Vp, int mm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x, k = by;
  if (t >= V.nplane || k >= V.kk) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj || !(V.m[I_mpack][t] & 1)) return;
  gcd_t sg = V.f[F_sigma] + ((size_t)t + (size_t)(mm + k) * V.nplane);
  gd_t si = V.f[F_sigint];
  const double lo = sg[0];
  const double up = sg[k ? -(ptrdiff_t)V.nplane : 0];
  si[(size_t)t + (size_t)k * V.nplane] = k == 0 ? lo : .5 * (up + lo);
}

// One thread per owned, masked column of grid G (u | v), one wave per block, one slot per blockIdx.y (a grid has <= 3): the kk bins
// of the step (tmp3d, :1394 | :1467) live in LDS as [bin][lane] -- every lane has its own bank pair, and the bin is the lane's own
// kup.  The class densities sit in LDS beside them.  KCAP >= kk fixes the static LDS of an instance: (KCAP*64 + KCAP) doubles.
// The walk is :1398-1453 | :1471-1526 line for line: kup carried down the column from 2, the two-branch search with its exits, the
// klo search against sigdia(klo) + sigeps, q = 1/(sigmax - sigmin), three pieces or the whole flux.  Then acclyr (:5500): acc =
// acc + tmp for ALL k.  sigup of layer k + 1 is siglo of layer k (the same two loads, the same operations) and is carried; the
// interface pair and the flux of the next DSG_KB layers are requested ahead.
// Algorithmic bytes per grid: (2 + n_sel + 2 n_sel) kk planes; the dealing re-reads sigint per slot: (2 n_sel + n_sel + 2 n_sel).
#define DSG_KB 2
#define DSG_W 64
#define DSG_MAXK 120
struct SigTab { int n; int d[3][3]; };            // per slot: source field, plane of its layer 1 (nn), first plane of the slot
template <int G, int KCAP>
__global__ __launch_bounds__(DSG_W) void k_diasig(const DevView *__restrict__ Vp, double *__restrict__ accp, const double *__restrict__ sigdiap, const SigTab T) {
  __shared__ double bins[KCAP * DSG_W], sd[KCAP];
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int lane = threadIdx.x, t = bx * DSG_W + lane;
  const int kk = V.kk;
  for (int k = lane; k < kk && k < KCAP; k += DSG_W) sd[k] = global_ptr(sigdiap)[k];
  __syncthreads();
  bool on = t < V.nplane && (int)by < T.n && kk <= KCAP;
  if (on) {
    const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
    on = i >= 1 && i <= V.ii && j >= 1 && j <= V.jj && ((V.m[I_mpack][t] >> G) & 1);
  }
  if (!on) return;
  const size_t np = V.nplane, c = t, cn = c - (G == G_U ? (size_t)1 : (size_t)V.ni);   // the western | southern p-point
  gcd_t sg = V.f[F_sigint];
  gcd_t src = V.f[T.d[by][0]] + (c + (size_t)T.d[by][1] * np);
  gd_t acc = global_ptr(accp) + (c + (size_t)T.d[by][2] * np);
  double *bin = bins + lane;
  for (int k = 0; k < kk; k++) bin[k * DSG_W] = 0.;                 // tmp3d(:,:,:) = 0.
  double a0 = sg[c], b0 = sg[cn];
  double aq[DSG_KB], bq[DSG_KB], fq[DSG_KB];
#pragma unroll
  for (int u = 0; u < DSG_KB; u++) {
    const size_t o = (size_t)(1 + u < kk ? 1 + u : kk - 1) * np;
    aq[u] = sg[c + o];
    bq[u] = sg[cn + o];
    fq[u] = src[(size_t)(u < kk ? u : kk - 1) * np];
  }
  int kup = 2;
  for (int k = 0; k < kk; k++) {
    const double a1 = aq[0], b1 = bq[0], f = fq[0];
#pragma unroll
    for (int u = 0; u + 1 < DSG_KB; u++) { aq[u] = aq[u + 1]; bq[u] = bq[u + 1]; fq[u] = fq[u + 1]; }
    {
      const size_t o = (size_t)(k + 1 + DSG_KB < kk ? k + 1 + DSG_KB : kk - 1) * np;
      aq[DSG_KB - 1] = sg[c + o];
      bq[DSG_KB - 1] = sg[cn + o];
      fq[DSG_KB - 1] = src[(size_t)(k + DSG_KB < kk ? k + DSG_KB : kk - 1) * np];
    }
    const double sigup = .5 * (b0 + a0), siglo = .5 * (b1 + a1);   // :1406-1407 | :1479-1480 (level min(kk, k+1): the queue clamps)
    a0 = a1;
    b0 = b1;
    const double sigmin = fmin2(sigup, siglo), sigmax = fmax2(sigup, siglo);
    // sigdia(x) = sd[x - 1]; kup, klo are the reference's 1-based indices
    if (sigmin > sd[kup - 2]) {
      while (sigmin > sd[kup - 1]) {
        if (kup == kk) break;
        kup++;
      }
    } else {
      for (;;) {
        if (kup == 2) break;
        if (sigmin > sd[kup - 2]) break;
        kup--;
      }
    }
    int klo = kup;
    while (sigmax > sd[klo - 1] + SIGEPS) {
      if (klo == kk) break;
      klo++;
    }
    if (kup < klo) {
      const double q = 1. / (sigmax - sigmin);
      double w = (sd[kup - 1] - sigmin) * q;
      bin[(kup - 2) * DSG_W] = bin[(kup - 2) * DSG_W] + w * f;
      for (int kt = kup; kt <= klo - 2; kt++) {
        w = (sd[kt] - sd[kt - 1]) * q;
        bin[(kt - 1) * DSG_W] = bin[(kt - 1) * DSG_W] + w * f;
      }
      w = (sigmax - sd[klo - 2]) * q;
      bin[(klo - 2) * DSG_W] = bin[(klo - 2) * DSG_W] + w * f;
    } else {
      bin[(kup - 2) * DSG_W] = bin[(kup - 2) * DSG_W] + f;
    }
  }
  // acclyr, op 0 (:5500): every class, touched or not
  for (int k0 = 0; k0 < kk; k0 += COLUMN_U) {
    double v[COLUMN_U];
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++) v[u] = acc[(size_t)(k0 + u < kk ? k0 + u : kk - 1) * np];
#pragma unroll
    for (int u = 0; u < COLUMN_U; u++)
      if (k0 + u < kk) acc[(size_t)(k0 + u) * np] = v[u] + bin[(k0 + u) * DSG_W];
  }
}

template <int G>
static void launch_diasig(blomgpu_ctx *c, DiaState *S, const SigTab &T) {
  const int kk = c->h.kk;
  const dim3 grid = plane_grid(c->h, T.n, DSG_W);
  if (kk <= 32) hipLaunchKernelGGL((k_diasig<G, 32>), grid, dim3(DSG_W), 0, c->stream, c->d, S->acc, S->sigdia(), T);
  else if (kk <= 56) hipLaunchKernelGGL((k_diasig<G, 56>), grid, dim3(DSG_W), 0, c->stream, c->d, S->acc, S->sigdia(), T);
  else hipLaunchKernelGGL((k_diasig<G, DSG_MAXK>), grid, dim3(DSG_W), 0, c->stream, c->d, S->acc, S->sigdia(), T);
}

// ---- the vertical mass flux: diavfl, :4633-4733 -------------------------------------------------------------------------------------
// Both kernels: one thread per owned wet p-column, i on the lanes, the sources of the next VFL_KB layers | levels requested ahead in
// a queue of registers, every accumulator element read and written once.
// k_diavfl_lyr (:4647-4676): wflx carried from k = kk up to k = 1,
//   wflx = wflx - (uflx(i+1,kn) - uflx(i,kn) + vflx(j+1,kn) - vflx(j,kn)) - (dp(km) - dpold(km))*scp2      (km in the last term, as written)
// evaluated left to right, then acc(k) = acc(k) + wflx and acc2(k) = acc2(k) + wflx**2 (a product).  uflx(ii+1) and vflx(jj+1) are
// halo values that the step leaves equal to the neighbour's owned ones.
// Algorithmic bytes: (4 + 4) kk planes (uflx, vflx, dp, dpold -- a face is read by the two columns it separates and comes from memory
// once; two accumulators read and written).
#define VFL_KB 2
__global__ __launch_bounds__(256) void k_diavfl_lyr(const DevView *__restrict__ Vp, double *__restrict__ accp, int pw, int pw2, int mm, int nn) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj || !(V.m[I_mpack][t] & 1)) return;
  const size_t np = V.nplane, c = t, ni = V.ni;
  const int kk = V.kk;
  gcd_t uf = V.f[F_uflx] + (c + (size_t)nn * np), vf = V.f[F_vflx] + (c + (size_t)nn * np);
  gcd_t dp = V.f[F_dp] + (c + (size_t)mm * np), dpo = V.f[F_dpold] + (c + (size_t)mm * np);
  gd_t a1 = global_ptr(accp) + (c + (size_t)pw * np), a2 = global_ptr(accp) + (c + (size_t)pw2 * np);
  const double scp2 = V.f[F_scp2][c];
  double ue[VFL_KB], uw[VFL_KB], vn[VFL_KB], vs[VFL_KB], dn[VFL_KB], dold[VFL_KB], q1[VFL_KB], q2[VFL_KB];
#pragma unroll
  for (int u = 0; u < VFL_KB; u++) {
    const size_t o = (size_t)(kk - 1 - u > 0 ? kk - 1 - u : 0) * np;
    ue[u] = uf[o + 1]; uw[u] = uf[o]; vn[u] = vf[o + ni]; vs[u] = vf[o];
    dn[u] = dp[o]; dold[u] = dpo[o]; q1[u] = a1[o]; q2[u] = a2[o];
  }
  double wflx = 0.;
  for (int k = kk - 1; k >= 0; k--) {
    const double e = ue[0], w = uw[0], n_ = vn[0], s_ = vs[0], d = dn[0], dd = dold[0], x1 = q1[0], x2 = q2[0];
#pragma unroll
    for (int u = 0; u + 1 < VFL_KB; u++) {
      ue[u] = ue[u + 1]; uw[u] = uw[u + 1]; vn[u] = vn[u + 1]; vs[u] = vs[u + 1];
      dn[u] = dn[u + 1]; dold[u] = dold[u + 1]; q1[u] = q1[u + 1]; q2[u] = q2[u + 1];
    }
    {
      const size_t o = (size_t)(k - VFL_KB > 0 ? k - VFL_KB : 0) * np;       // (layer 0 again at the end: in bounds, unused)
      ue[VFL_KB - 1] = uf[o + 1]; uw[VFL_KB - 1] = uf[o]; vn[VFL_KB - 1] = vf[o + ni]; vs[VFL_KB - 1] = vf[o];
      dn[VFL_KB - 1] = dp[o]; dold[VFL_KB - 1] = dpo[o];
      if (k - VFL_KB >= 0) { q1[VFL_KB - 1] = a1[o]; q2[VFL_KB - 1] = a2[o]; }
    }
    wflx = (wflx - (((e - w) + n_) - s_)) - (d - dd) * scp2;
    const size_t ok = (size_t)k * np;
    a1[ok] = x1 + wflx;
    a2[ok] = x2 + wflx * wflx;
  }
}

// k_diavfl_lvl (:4693-4730): ucum(i), ucum(i+1), vcum(j), vcum(j+1) carried from d = ddm up to 1, each ucum = ucum + uflxlvl(d) -
// uflxold(d) where the face's iu | iv is set (the loops over isu / isv to ii+1 | jj+1) and 0 otherwise; then
//   q = -(ucum(i+1) - ucum(i) + vcum(j+1) - vcum(j)),  acc(d) = acc(d) + q,  acc2(d) = acc2(d) + q**2.
// A column forms its eastern and northern neighbours' face sums itself: the same operations on the same values in the same
// order, so the bits agree with what the neighbour forms.  The faces at ii+1 | jj+1 are the halo the exchange in front of the
// launch gave uflxlvl | vflxlvl, and the halo the copy in front of the level launches took along into uflxold | vflxold.
// Algorithmic bytes: (4 + 4) ddm planes.
__global__ __launch_bounds__(256) void k_diavfl_lvl(const DevView *__restrict__ Vp, double *__restrict__ accp, int pu, int pv, int puo, int pvo, int pw, int pw2, int ddm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj) return;
  const int mc = V.m[I_mpack][t];
  if (!(mc & 1)) return;
  const size_t np = V.nplane, c = t, ni = V.ni;
  const bool bw = (mc >> G_U) & 1, be = (V.m[I_mpack][t + 1] >> G_U) & 1, bs = (mc >> G_V) & 1, bn = (V.m[I_mpack][t + V.ni] >> G_V) & 1;
  gd_t acc = global_ptr(accp);
  gcd_t un = acc + (c + (size_t)pu * np), uo = acc + (c + (size_t)puo * np), vn = acc + (c + (size_t)pv * np), vo = acc + (c + (size_t)pvo * np);
  gd_t a1 = acc + (c + (size_t)pw * np), a2 = acc + (c + (size_t)pw2 * np);
  double une[VFL_KB], unw[VFL_KB], uoe[VFL_KB], uow[VFL_KB], vnn[VFL_KB], vns[VFL_KB], von[VFL_KB], vos[VFL_KB], q1[VFL_KB], q2[VFL_KB];
#pragma unroll
  for (int u = 0; u < VFL_KB; u++) {
    const size_t o = (size_t)(ddm - 1 - u > 0 ? ddm - 1 - u : 0) * np;
    une[u] = un[o + 1]; unw[u] = un[o]; uoe[u] = uo[o + 1]; uow[u] = uo[o];
    vnn[u] = vn[o + ni]; vns[u] = vn[o]; von[u] = vo[o + ni]; vos[u] = vo[o];
    q1[u] = a1[o]; q2[u] = a2[o];
  }
  double ucw = 0., uce = 0., vcs = 0., vcn = 0.;
  for (int d = ddm - 1; d >= 0; d--) {
    const double ne = une[0], nw = unw[0], oe = uoe[0], ow = uow[0], nn_ = vnn[0], ns = vns[0], on = von[0], os = vos[0], x1 = q1[0], x2 = q2[0];
#pragma unroll
    for (int u = 0; u + 1 < VFL_KB; u++) {
      une[u] = une[u + 1]; unw[u] = unw[u + 1]; uoe[u] = uoe[u + 1]; uow[u] = uow[u + 1];
      vnn[u] = vnn[u + 1]; vns[u] = vns[u + 1]; von[u] = von[u + 1]; vos[u] = vos[u + 1];
      q1[u] = q1[u + 1]; q2[u] = q2[u + 1];
    }
    {
      const size_t o = (size_t)(d - VFL_KB > 0 ? d - VFL_KB : 0) * np;
      une[VFL_KB - 1] = un[o + 1]; unw[VFL_KB - 1] = un[o]; uoe[VFL_KB - 1] = uo[o + 1]; uow[VFL_KB - 1] = uo[o];
      vnn[VFL_KB - 1] = vn[o + ni]; vns[VFL_KB - 1] = vn[o]; von[VFL_KB - 1] = vo[o + ni]; vos[VFL_KB - 1] = vo[o];
      if (d - VFL_KB >= 0) { q1[VFL_KB - 1] = a1[o]; q2[VFL_KB - 1] = a2[o]; }
    }
    ucw = bw ? (ucw + nw) - ow : ucw;
    uce = be ? (uce + ne) - oe : uce;
    vcs = bs ? (vcs + ns) - os : vcs;
    vcn = bn ? (vcn + nn_) - on : vcn;
    const double q = -(((uce - ucw) + vcn) - vcs);
    const size_t od = (size_t)d * np;
    a1[od] = x1 + q;
    a2[od] = x2 + q * q;
  }
}

// ---- the column-derived diagnostics: :1251-1366, and the mldl82 family ---------------------------------------------------------------
// k_diacol: one thread per owned wet p-column, i on the lanes, ONE downward pass over the layers for the names that are selected
// (wave-uniform flags: T.p[x] < 0 skips name x and the loads only it needs).  p(kk+1) first; p(k+1), temp, saln and dp of the next
// COL_KB layers wait in a queue of registers; z and dz are read behind the pass, at the two layers an interpolation needs and nowhere
// else.  Every value is added straight into its slot: no temporary plane.
//   sbot, tbot (:1264-1292): q = max(0., p(k+1) - max(p(kk+1) - dpbot, p(k))); the sums start at 0. and take all kk terms in
//     ascending k, those with q = 0. too; then *(1./dps) where dps > onemm, the layer-1 value otherwise.
//   t20d, t17d (:1301-1325 | :1337-1361): kup moves on the layers with dp(km) > onecm and temp(km) > T only, the walk ends at the
//     first layer with dp(km) > onecm and temp(km) <= T (k = 1: 0.; never: z(kk+1); otherwise the interpolation between the centres
//     of kup and k with tlo = min(temp(km), tup - epsilp)).  The reference leaves kup undefined when the walk ends at k > 1 with
//     nothing but massless layers above: here kup = 1 then (no case of this library has a massless top layer).
//   mldl82 mldl82mn mldl82mx mldl82sq (:1706, :1755, :1758, :1773): acc + fld, min(acc, fld), max(acc, fld), acc + fld*fld of the
//     device field mldl82 that cmnfld1 left (stage_cmnfld.hip; under isopyc_bulkml st_cmnfld1 forms it for these four names only).
// Algorithmic bytes: ((sbot | tbot: 2) + (t20d | t17d: 1) + 1 (temp)) kk planes + p(kk+1) + <= 4 planes of z / dz + mldl82 + 2 n_acc.
#define COL_KB 2
struct ColTab { int p[C_N]; };                // first plane of each name's slot, -1: not selected
__global__ __launch_bounds__(256) void k_diacol(const DevView *__restrict__ Vp, double *__restrict__ accp, const ColTab T, int mm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x;
  if (t >= V.nplane) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj || !(V.m[I_mpack][t] & 1)) return;
  const size_t np = V.nplane, c = t;
  const int kk = V.kk;
  gd_t acc = global_ptr(accp);
  const bool bot = T.p[C_SBOT] >= 0 || T.p[C_TBOT] >= 0, iso = T.p[C_T20D] >= 0 || T.p[C_T17D] >= 0;       // wave-uniform
  if (bot || iso) {
    gcd_t p = V.f[F_p] + c, z = V.f[F_z] + c, dz = V.f[F_dz] + c;
    gcd_t temp = V.f[F_temp] + (c + (size_t)mm * np), saln = V.f[F_saln] + (c + (size_t)mm * np), dp = V.f[F_dp] + (c + (size_t)mm * np);
    const double plim = bot ? p[(size_t)kk * np] - DPBOT : 0.;          // p(kk+1) - dpbot
    double pk = bot ? p[0] : 0.;
    double pq[COL_KB], tq[COL_KB], sq[COL_KB], dq[COL_KB];
#pragma unroll
    for (int u = 0; u < COL_KB; u++) {
      const size_t o = (size_t)(u < kk ? u : kk - 1) * np;
      tq[u] = temp[o];
      pq[u] = bot ? p[o + np] : 0.;
      sq[u] = bot ? saln[o] : 0.;
      dq[u] = iso ? dp[o] : 0.;
    }
    double sb = 0., tb = 0., dps = 0., s1 = 0., t1 = 0.;
    // the two walks: ke = 0 while the walk goes on, else the layer it ended at (1-based); kup, tup as the reference carries them
    int ke20 = 0, ke17 = 0, ku20 = 1, ku17 = 1;
    double tu20 = 0., tu17 = 0., te20 = 0., te17 = 0.;
    for (int k = 0; k < kk; k++) {
      const double pk1 = pq[0], tk = tq[0], sk = sq[0], dk = dq[0];
#pragma unroll
      for (int u = 0; u + 1 < COL_KB; u++) { pq[u] = pq[u + 1]; tq[u] = tq[u + 1]; sq[u] = sq[u + 1]; dq[u] = dq[u + 1]; }
      {
        const size_t o = (size_t)(k + COL_KB < kk ? k + COL_KB : kk - 1) * np;
        tq[COL_KB - 1] = temp[o];
        if (bot) { pq[COL_KB - 1] = p[o + np]; sq[COL_KB - 1] = saln[o]; }
        if (iso) dq[COL_KB - 1] = dp[o];
      }
      if (k == 0) { s1 = sk; t1 = tk; tu20 = tu17 = tk; }
      if (bot) {
        const double q = fmax2(0., pk1 - fmax2(plim, pk));
        sb = sb + sk * q;
        tb = tb + tk * q;
        dps = dps + q;
        pk = pk1;
      }
      if (iso && dk > ONECM) {
        if (!ke20) {
          if (tk > 20.) { ku20 = k + 1; tu20 = tk; }
          else { ke20 = k + 1; te20 = tk; }
        }
        if (!ke17) {
          if (tk > 17.) { ku17 = k + 1; tu17 = tk; }
          else { ke17 = k + 1; te17 = tk; }
        }
      }
    }
    if (bot) {
      if (dps > ONEMM) {
        const double q = 1. / dps;
        sb = sb * q;
        tb = tb * q;
      } else {
        sb = s1;
        tb = t1;
      }
      if (T.p[C_SBOT] >= 0) { const size_t o = c + (size_t)T.p[C_SBOT] * np; acc[o] = acc[o] + sb; }
      if (T.p[C_TBOT] >= 0) { const size_t o = c + (size_t)T.p[C_TBOT] * np; acc[o] = acc[o] + tb; }
    }
#pragma unroll
    for (int w = 0; w < 2; w++) {
      const int slot = T.p[w ? C_T17D : C_T20D];
      if (slot < 0) continue;
      const int ke = w ? ke17 : ke20, ku = w ? ku17 : ku20;
      const double tx = w ? 17. : 20., tup = w ? tu17 : tu20, te = w ? te17 : te20;
      double d;
      if (ke == 1) d = 0.;
      else if (ke == 0) d = z[(size_t)kk * np];
      else {
        const double zup = z[(size_t)(ku - 1) * np] + .5 * dz[(size_t)(ku - 1) * np];
        const double zlo = z[(size_t)(ke - 1) * np] + .5 * dz[(size_t)(ke - 1) * np];
        const double tlo = fmin2(te, tup - EPSILP);
        d = (zup * (tlo - tx) + zlo * (tx - tup)) / (tlo - tup);
      }
      const size_t o = c + (size_t)slot * np;
      acc[o] = acc[o] + d;
    }
  }
  if (T.p[C_ML] >= 0 || T.p[C_MLMN] >= 0 || T.p[C_MLMX] >= 0 || T.p[C_MLSQ] >= 0) {
    const double f = V.f[F_mldl82][c];
    if (T.p[C_ML] >= 0) { const size_t o = c + (size_t)T.p[C_ML] * np; acc[o] = acc[o] + f; }                 // acch2d, :5256
    if (T.p[C_MLMN] >= 0) { const size_t o = c + (size_t)T.p[C_MLMN] * np; acc[o] = fmin2(acc[o], f); }       // minh2d, :5392
    if (T.p[C_MLMX] >= 0) { const size_t o = c + (size_t)T.p[C_MLMX] * np; acc[o] = fmax2(acc[o], f); }       // maxh2d, :5330
    if (T.p[C_MLSQ] >= 0) { const size_t o = c + (size_t)T.p[C_MLSQ] * np; acc[o] = acc[o] + f * f; }         // sqh2d, :5454
  }
}

// k_diapv (:1208-1247): one thread per owned wet p-point and layer.  The corner masks min(1, iu + iv) from the mask bits of the
// point and of its eastern and northern neighbours; dsig in its three cases with the .5* outside the max; the corner sums left to
// right, every product with a 0/1 mask performed (a q-point momtum never wrote holds spval, and spval*0. is +0.); absvor and dpvor
// at plane k, not km: momtum writes planes 1..kk of their 2*kdm.  Then acclyr (:5500), unweighted.
// Algorithmic bytes: (3 + 4) kk planes (absvor, dpvor: a q-point is read by the four p-points around it and comes from memory
// once; sigma: a thread reads up to three planes, each plane once from memory; two accumulators read and written).
__global__ __launch_bounds__(256) void k_diapv(const DevView *__restrict__ Vp, double *__restrict__ accp, int pa, int pd, int mm) {
  const DevView &V = *Vp;
  unsigned bx, by;
  xcd_block(bx, by);
  const int t = bx * blockDim.x + threadIdx.x, k = by;            // k: 0-based layer
  if (t >= V.nplane || k >= V.kk) return;
  const int i = t % V.ni - (NBDY - 1), j = t / V.ni - (NBDY - 1);
  if (i < 1 || i > V.ii || j < 1 || j > V.jj) return;
  const int mc = V.m[I_mpack][t];
  if (!(mc & 1)) return;
  const size_t np = V.nplane, c = t, ni = V.ni;
  const int kk = V.kk;
  const int iuw = (mc >> G_U) & 1, iue = (V.m[I_mpack][t + 1] >> G_U) & 1, ivs = (mc >> G_V) & 1, ivn = (V.m[I_mpack][t + V.ni] >> G_V) & 1;
  const double sw = (double)(iuw | ivs), se = (double)(iue | ivs), nw = (double)(iuw | ivn), ne = (double)(iue | ivn);     // min(1, iu + iv)
  gcd_t sg = V.f[F_sigma] + (c + (size_t)mm * np);
  gcd_t av = V.f[F_absvor] + (c + (size_t)k * np), dv = V.f[F_dpvor] + (c + (size_t)k * np);
  gd_t a1 = global_ptr(accp) + (c + ((size_t)pa + k) * np), a2 = global_ptr(accp) + (c + ((size_t)pd + k) * np);
  const double x1 = a1[0], x2 = a2[0];
  const double a00 = av[0], a10 = av[1], a01 = av[ni], a11 = av[ni + 1];
  const double d00 = dv[0], d10 = dv[1], d01 = dv[ni], d11 = dv[ni + 1];
  const double s2 = sg[kk > 1 ? np : 0];                                  // sigma(2+mm)
  double dsig;
  if (k + 1 <= 2) dsig = fmax2(0., s2 - sg[0]);
  else if (k + 1 == kk) dsig = fmax2(0., sg[(size_t)k * np] - fmax2(sg[(size_t)(k - 1) * np], s2));
  else dsig = .5 * fmax2(0., sg[(size_t)(k + 1) * np] - fmax2(sg[(size_t)(k - 1) * np], s2));
  const double f1 = (((a00 * sw + a10 * se) + a01 * nw) + a11 * ne) * dsig;
  const double f2 = ((d00 * sw + d10 * se) + d01 * nw) + d11 * ne;
  a1[0] = x1 + f1;
  a2[0] = x2 + f2;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
// inifld's initial values (:5864-5960): -spval under a maximum, +spval under a minimum, 0. otherwise
static int ini_of(const DiaRow &r) {
  if (r.op == OP_MAX || (r.op == OP_COL && r.src == C_MLMX)) return 1;
  if (r.op == OP_COL && r.src == C_MLMN) return 2;
  return 0;
}

static int dia_init(blomgpu_ctx *c, DiaState *S) {
  DiaIni T;
  T.n = 0;
  int maxlev = 1;
  for (size_t s = 0; s < S->rows.size(); s++) {
    const DiaRow &r = g_rows[S->rows[s]];
    const int nl = r.lyr == 2 ? S->ddm : r.lyr ? c->h.kk : 1;          // (kk for the layers and the density classes)
    T.d[T.n][0] = S->plane0[s]; T.d[T.n][1] = nl; T.d[T.n][2] = r.grid | ini_of(r) << 2;
    T.n++;
    if (nl > maxlev) maxlev = nl;
  }
  S->nacc = 0;
  S->finalized = false;
  if (!T.n) return 0;
  ctx_sync_view(c);
  hipLaunchKernelGGL(k_dia_init, plane_grid(c->h, maxlev), dim3(256), 0, c->stream, c->d, S->acc, T);
  HIPCHK(c, hipGetLastError());
  return 0;
}

void dia_free(blomgpu_ctx *c) {
  if (!c->dia) return;
  (void)hipStreamSynchronize(c->stream);
  if (c->dia->acc) (void)hipFree(c->dia->acc);
  delete c->dia;
  c->dia = nullptr;
}

bool dia_active(const blomgpu_ctx *c) { return c->dia != nullptr; }
// diavfl reads dpold(km) as the previous step's tmsmt1 left it: blomgpu_step must not fold this step's tmsmt1 into its tmsmt2
bool dia_reads_dpold(const blomgpu_ctx *c) { return c->dia && c->dia->vfl; }
// A selected row accumulates one of the heat and salt flux diagnostics that eddtra, diffus and pbcor keep current for diaacc alone
// (blomgpu_step, flux_diag): by the table's source column, whatever the row's kind (layers, depth levels, classes).  An OP_COL
// row's src is a C_* code, not a field.
bool dia_reads_flux_diag(const blomgpu_ctx *c) {
  if (!c->dia) return false;
  for (int r : c->dia->rows) {
    if (g_rows[r].op == OP_COL) continue;
    for (int f : {F_utflx, F_usflx, F_vtflx, F_vsflx, F_utfltd, F_usfltd, F_vtfltd, F_vsfltd, F_utflld, F_usflld, F_vtflld, F_vsflld})
      if (g_rows[r].src == f) return true;
  }
  return false;
}
// the accumulators as a halo update sees them (xctilr of uflxlvl / vflxlvl inside diavfl): base and number of doubles in whole planes
// one of mldl82 mldl82mn mldl82mx mldl82sq is selected: cmnfld1 forms mldl82 under isopyc_bulkml too (phy/mod_cmnfld_routines.F90:1109-1113)
bool dia_reads_mldl82(const blomgpu_ctx *c) { return c->dia && c->dia->ml82; }
double *dia_acc_span(const blomgpu_ctx *c, size_t *n) {
  if (!c->dia) return nullptr;
  *n = c->dia->nplanes * c->dia->np;
  return c->dia->acc;
}
void dia_count(blomgpu_ctx *c) { if (c->dia) c->dia->nacc++; }

// z and dz are cmnfld1's: a step that does not run it would accumulate whatever the arrays hold
static bool reads_z(const DiaRow &r) {     // z or dz directly, or through mldl82 (:950-976) and the isotherms' interpolation (:1318-1321)
  if (r.op == OP_COL) return r.src != C_SBOT && r.src != C_TBOT;
  return r.op < OP_VFL && (r.src == F_z || r.src == F_dz);
}
static bool hybrid_remapped(int r) {       // the level rows the hybrid coordinate forms inside ale_regrid_remap (:1944, :2059, :2174 leave them out)
  const std::string nm = g_rows[r].name;
  return nm == "uvellvl" || nm == "vvellvl" || nm == "salnlvl" || nm == "templvl";
}

int dia_step_check(blomgpu_ctx *c) {
  if (c->dia && c->dia->ncls && c->h.P.vcoord_tag == 3)
    return ctx_fail(c, "blomgpu_step: a density-class accumulator is selected, which reads sigint; vcoord_type = 'plevel' never writes it");
  if (c->dia && c->h.P.vcoord_tag != 1 && c->dia_alarm < 0)
    for (int r : c->dia->rows)
      if (hybrid_remapped(r))
        return ctx_fail(c, std::string("blomgpu_step: ") + g_rows[r].name + " is selected, which cntiso_hybrid / plevel form inside ale_regrid_remap while the output alarm is 0 "
                           "and in ale_remap_diazlv when it is 1 (phy/mod_ale_regrid_remap.F90:1524-1531, :2014-2017): the output alarm has not been declared (blomgpu_dia_alarm)");
  if (!c->dia || !c->dia->needs_z) return 0;
  if (c->h.P.vcoord_tag != 1 || c->cmnfld1 || c->full_physics) return 0;
  std::string names;
  for (int r : c->dia->rows)
    if (reads_z(g_rows[r])) names += std::string(names.empty() ? "" : " ") + g_rows[r].name;
  return ctx_fail(c, "blomgpu_step: the selected accumulators " + names + " read z / dz, which this step sequence does not compute (set cmnfld1 = 1 or full_physics = 1)");
}

int dia_select(blomgpu_ctx *c, const char *names) {
  if (!names) return ctx_fail(c, "blomgpu_dia_select: null argument");
  std::vector<char> want(NROW, 0);
  const std::string all(names);
  size_t pos = 0;
  bool any = false;
  unsigned msc = 0;
  std::vector<std::string> nms;
  while (pos < all.size()) {
    while (pos < all.size() && (all[pos] == ' ' || all[pos] == ',' || all[pos] == '\t' || all[pos] == '\n')) pos++;
    size_t end = pos;
    while (end < all.size() && !(all[end] == ' ' || all[end] == ',' || all[end] == '\t' || all[end] == '\n')) end++;
    if (end == pos) break;
    const std::string tok = all.substr(pos, end - pos);
    pos = end;
    // an msc name (diaout_iogrp's reductions, stage_diaout.hip) selects its sources as diaini does (:557, :559, :598-670)
    const int mi = diaout_msc_index(tok.c_str());
    if (mi >= 0) msc |= 1u << mi;
    if (mi >= 0) diaout_msc_sources(mi, &nms);
    else nms.push_back(tok);
  }
  for (const std::string &nm : nms) {
    const int r = find_row(nm);
    if (r < 0) return ctx_fail(c, "blomgpu_dia_select: unknown accumulator " + nm);
    if (g_rows[r].op == OP_OLD)
      return ctx_fail(c, "blomgpu_dia_select: " + nm + " is a slot of diavfl's group (ACC_UFLXOLD / ACC_VFLXOLD), selected with wflx wflx2 wflxlvl wflx2lvl and not by name");
    if (g_rows[r].lev == LV_TKE && c->h.P.itrtke < 1)
      return ctx_fail(c, "blomgpu_dia_select: " + nm + " needs the TKE tracers (itrtke >= 1, phy/mod_dia.F90:1907)");
    if (g_rows[r].lev == LV_GLS && !(c->h.P.itrtke >= 1 && c->h.P.gls && c->h.P.itrgls >= 1))
      return ctx_fail(c, "blomgpu_dia_select: " + nm + " needs the two-equation closure (itrtke >= 1, gls = 1)");
    if ((g_rows[r].lev == LV_TKE || g_rows[r].lev == LV_GLS) && (c->h.P.itrtke > c->h.ntr || c->h.P.itrgls > c->h.ntr))
      return ctx_fail(c, "blomgpu_dia_select: " + nm + ": itrtke / itrgls outside 1..ntr");
    if (c->h.P.vcoord_tag != 1 && hybrid_remapped(r) && c->dia_alarm < 0)
      return ctx_fail(c, "blomgpu_dia_select: " + nm + " is formed inside ale_regrid_remap under cntiso_hybrid / plevel (phy/mod_dia.F90:1944, :2059, :2174 leave it out), "
                         "at the start or at the end of a step as the output alarm says (phy/mod_ale_regrid_remap.F90:1524-1531, :2014-2017): the output alarm has not been declared (blomgpu_dia_alarm)");
    if (g_rows[r].lyr == 3) {
      if (c->dia_sigdia.empty())
        return ctx_fail(c, "blomgpu_dia_select: " + nm + " needs the diagnostic density classes sigdia (blomgpu_dia_set_sigdia)");
      if (c->h.P.vcoord_tag == 3)
        return ctx_fail(c, "blomgpu_dia_select: " + nm + " reads sigint, which vcoord_type = 'plevel' never writes (phy/mod_vcoord.F90:1059: it stays spval)");
      if ((int)c->dia_sigdia.size() != c->h.kk || c->h.kk < 2 || c->h.kk > DSG_MAXK)
        return ctx_fail(c, "blomgpu_dia_select: " + nm + ": the density classes need 2 <= kdm <= " + std::to_string(DSG_MAXK) + " and a sigdia of kdm values");
    }
    want[r] = 1;
    any = true;
  }
  // diaini's dependencies (:598-608): a dp-weighted row needs dp, uvel needs dpu, vvel needs dpv
  for (int r = 0; r < NROW; r++)
    if (want[r] && g_rows[r].wgt) want[find_row(g_rows[r].wgt == W_DP ? "dp" : g_rows[r].wgt == W_DPU ? "dpu" : "dpv")] = 1;
  // diavfl's group (diaini :615-618, :644-647, :673-680): any of its four names selects all four, the fluxes and the level fluxes
  // they are formed from, and the two slots that keep last step's level fluxes
  bool vfl = false;
  for (int r = 0; r < NROW; r++) vfl = vfl || (want[r] && g_rows[r].op == OP_VFL);
  if (vfl) {
    for (int r = 0; r < NROW; r++)
      if (g_rows[r].op == OP_VFL || g_rows[r].op == OP_OLD) want[r] = 1;
    for (const char *nm : {"uflx", "vflx", "uflxlvl", "vflxlvl"}) want[find_row(nm)] = 1;
  }
  // avdsg and dpvor come as a pair (diaini :681-682)
  if (want[find_row("avdsg")] || want[find_row("dpvor")]) want[find_row("avdsg")] = want[find_row("dpvor")] = 1;
  // z and dz are cmnfld1's: the names that need them are refused here already where the step sequence would not run it
  if (c->h.P.vcoord_tag == 1 && !c->cmnfld1 && !c->full_physics)
    for (int r = 0; r < NROW; r++)
      if (want[r] && g_rows[r].op == OP_COL && reads_z(g_rows[r]))
        return ctx_fail(c, std::string("blomgpu_dia_select: ") + g_rows[r].name + " reads z / dz, which this step sequence does not compute (set cmnfld1 = 1 or full_physics = 1)");
  DiaState *S = nullptr;
  if (any) {
    S = new DiaState;
    S->vfl = vfl;
    S->msc = msc;
    int n2d = 0, nly = 0, nlv = 0;
    for (int r = 0; r < NROW; r++)
      if (want[r] && g_rows[r].lyr == 2) nlv++;
    const std::vector<double> edges = c->dia_edges.empty() ? std::vector<double>(g_edges35, g_edges35 + 36) : c->dia_edges;
    S->np = c->h.nplane;
    S->ddm = nlv ? (int)edges.size() - 1 : 0;
    for (int pass = 0; pass < 4; pass++)
      for (int r = 0; r < NROW; r++)
        if (want[r] && g_rows[r].lyr == pass) {
          S->rows.push_back(r);
          S->plane0.push_back((int)S->nplanes);
          S->nplanes += pass == 2 ? S->ddm : pass ? c->h.kk : 1;
          if (pass < 2 && g_rows[r].op < OP_VFL) (pass ? nly : n2d)++;          // (the slots a launch of k_diaacc carries)
          if (pass == 3) S->ncls++;
          if (reads_z(g_rows[r])) S->needs_z = true;
          if (g_rows[r].op == OP_COL) { S->col = true; if (g_rows[r].src >= C_ML) S->ml82 = true; }
          if (g_rows[r].op == OP_PV) S->pv = true;
        }
    if (n2d > DIA_MAXSLOT || nly > DIA_MAXSLOT) { delete S; return ctx_fail(c, "blomgpu_dia_select: more slots than a launch carries"); }
    (void)hipSetDevice(c->device);
    // (the edges of the depth levels lie behind the last plane, the density classes behind them)
    if (hipMalloc((void **)&S->acc, sizeof(double) * (S->nplanes * (size_t)c->h.nplane + (S->ddm ? S->ddm + 1 : 0) + (S->ncls ? c->h.kk : 0))) != hipSuccess) {
      (void)hipGetLastError();
      const size_t mb = sizeof(double) * S->nplanes * (size_t)c->h.nplane >> 20;
      delete S;
      return ctx_fail(c, "blomgpu_dia_select: no device memory for " + std::to_string(mb) + " MB of accumulators");
    }
    if (S->ddm && hipMemcpy(S->edges(), edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(S->acc);
      delete S;
      return ctx_fail(c, "blomgpu_dia_select: the depth levels could not be copied to the device");
    }
    if (S->ncls && hipMemcpy(S->sigdia(), c->dia_sigdia.data(), sizeof(double) * c->dia_sigdia.size(), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(S->acc);
      delete S;
      return ctx_fail(c, "blomgpu_dia_select: the density classes could not be copied to the device");
    }
    if (dia_init(c, S)) { (void)hipFree(S->acc); delete S; return 1; }
  }
  dia_free(c);                       // the previous selection goes only now that the new one stands
  c->dia = S;
  diaout_invalidate(c);
  ctx_drop_graphs(c);
  return 0;
}

int dia_reset(blomgpu_ctx *c) {                                                  // inifld, :5864
  diaout_invalidate(c);
  return c->dia ? dia_init(c, c->dia) : 0;
}

// what stage_diaout.hip reads of a selection: the msc names, the count, whether finalize has run, the depth levels on the device,
// and the first plane of a selected accumulator
unsigned dia_msc_mask(const blomgpu_ctx *c) { return c->dia ? c->dia->msc : 0u; }
bool dia_finalized(const blomgpu_ctx *c) { return c->dia && c->dia->finalized; }
const double *dia_edges_dev(const blomgpu_ctx *c, int *ddm) {
  *ddm = c->dia ? c->dia->ddm : 0;
  return *ddm ? c->dia->edges() : nullptr;
}
int dia_levels_kind(const blomgpu_ctx *c) {       // 35: the table of :111-128, 70: LEVITUS2X, 0: a table of the caller's
  const std::vector<double> &e = c->dia_edges;
  if (e.empty() || (e.size() == 36 && !memcmp(e.data(), g_edges35, sizeof(g_edges35)))) return 35;
  return e.size() == 71 && !memcmp(e.data(), g_edges70, sizeof(g_edges70)) ? 70 : 0;
}
const double *dia_plane_dev(const blomgpu_ctx *c, const char *name) {
  const int r = find_row(name), s = r >= 0 && c->dia ? c->dia->slot_of(r) : -1;
  return s < 0 ? nullptr : c->dia->acc + (size_t)c->dia->plane0[s] * c->dia->np;
}

// alarm_phy(1) (phy/mod_dia.F90: diaout_alarms) as the host declares it.  Under cntiso_hybrid / plevel it decides where templvl salnlvl
// uvellvl vvellvl take their sample: inside ale_regrid_remap while it is 0 (phy/mod_ale_regrid_remap.F90:1524-1531), in ale_remap_diazlv
// when it is 1 (:2014-2017).  A captured step sequence holds the launches of one value: a change drops the graphs, as a selection does.
int dia_alarm(blomgpu_ctx *c, int alarm) {
  if (alarm != 0 && alarm != 1) return ctx_fail(c, "blomgpu_dia_alarm: alarm = " + std::to_string(alarm) + ": alarm_phy is 0 or 1");
  if (c->dia_alarm == alarm) return 0;
  c->dia_alarm = alarm;
  ctx_drop_graphs(c);
  return 0;
}

bool dia_hybrid_slots(const blomgpu_ctx *c, DiaHyb *Z) {
  const DiaState *S = c->dia;
  if (!S || !S->ddm || c->h.P.vcoord_tag == 1) return false;
  const auto plane = [&](const char *nm) { const int s = S->slot_of(find_row(nm)); return s < 0 ? -1 : S->plane0[s]; };
  Z->ddm = S->ddm; Z->acc = S->acc; Z->edges = S->edges();
  Z->temp = plane("templvl"); Z->saln = plane("salnlvl"); Z->uvel = plane("uvellvl"); Z->vvel = plane("vvellvl");
  return Z->temp >= 0 || Z->saln >= 0 || Z->uvel >= 0 || Z->vvel >= 0;
}

int dia_nacc(blomgpu_ctx *c, int *nacc) {
  if (!nacc) return ctx_fail(c, "blomgpu_dia_nacc: null argument");
  *nacc = c->dia ? c->dia->nacc : 0;
  return 0;
}

int dia_get(blomgpu_ctx *c, const char *name, double *out) {
  if (!name || !out) return ctx_fail(c, "blomgpu_dia_get: null argument");
  const int r = find_row(name), s = r >= 0 && c->dia ? c->dia->slot_of(r) : -1;
  if (r < 0) return ctx_fail(c, std::string("blomgpu_dia_get: unknown accumulator ") + name);
  if (s < 0) return ctx_fail(c, std::string("blomgpu_dia_get: accumulator ") + name + " is not selected");
  const size_t np = c->h.nplane, nl = g_rows[r].lyr == 2 ? c->dia->ddm : g_rows[r].lyr ? c->h.kk : 1;
  HIPCHK(c, hipMemcpyAsync(out, c->dia->acc + (size_t)c->dia->plane0[s] * np, sizeof(double) * nl * np, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return 0;
}

int dia_name_ext(int index, char *buf, int cap, int *kind, int *grid) {
  if (index < 0 || index >= NROW || !buf || cap < 2) return 1;
  snprintf(buf, cap, "%s", g_rows[index].name);
  if (kind) *kind = g_rows[index].op == OP_OLD ? KIND_INTERNAL : g_rows[index].lyr;
  if (grid) *grid = g_rows[index].grid;
  return 0;
}

// (the rows up to diavfl's: where the table ended before the column-derived rows)
int dia_name_full(int index, char *buf, int cap, int *kind, int *grid) { return index >= NROW_FULL ? 1 : dia_name_ext(index, buf, cap, kind, grid); }

// (the rows up to the density classes: where the table ended before diavfl's)
int dia_name_all(int index, char *buf, int cap, int *kind, int *grid) { return index >= NROW_ALL ? 1 : dia_name_full(index, buf, cap, kind, grid); }

// (the 2-D, layer and depth-level rows: where the table ended before the density classes)
int dia_name(int index, char *buf, int cap, int *is_lyr, int *grid) { return index >= NROW_NAMED ? 1 : dia_name_all(index, buf, cap, is_lyr, grid); }

// finlyr for the weighted layer pairs of :2597-2611; the table holds no weighted 2-D row (finh2d's are the ice fields, :2591-2594)
int dia_finalize(blomgpu_ctx *c) {
  DiaState *S = c->dia;
  if (!S) return 0;
  ctx_sync_view(c);
  for (size_t s = 0; s < S->rows.size(); s++) {
    const DiaRow &r = g_rows[S->rows[s]];
    if (r.lyr != 1 || !r.wgt) continue;
    const int ws = S->slot_of(find_row(r.wgt == W_DP ? "dp" : r.wgt == W_DPU ? "dpu" : "dpv"));
    hipLaunchKernelGGL(k_dia_finlyr, plane_grid(c->h, c->h.kk), dim3(256), 0, c->stream, c->d, S->acc, S->plane0[s], S->plane0[ws], r.grid);
  }
  // finlyr(ACC_AVDSG, ACC_DPVOR, 'p'), :2608: avdsg / dpvor where dpvor > epsil; dpvor itself stays
  if (S->pv)
    hipLaunchKernelGGL(k_dia_finlyr, plane_grid(c->h, c->h.kk), dim3(256), 0, c->stream, c->d, S->acc, S->plane0[S->slot_of(find_row("avdsg"))],
                       S->plane0[S->slot_of(find_row("dpvor"))], (int)G_P);
  // msklvl for every depth-level slot (:2642-2679)
  MskTab M;
  M.n = 0; M.ddm = S->ddm;
  for (size_t s = 0; s < S->rows.size(); s++)
    if (g_rows[S->rows[s]].lyr == 2 && g_rows[S->rows[s]].op != OP_OLD) { M.d[M.n][0] = S->plane0[s]; M.d[M.n][1] = g_rows[S->rows[s]].grid; M.n++; }   // (wflxlvl, wflx2lvl on p: :2676-2677)
  if (M.n) hipLaunchKernelGGL(k_dia_msklvl, plane_grid(c->h, S->ddm), dim3(256), 0, c->stream, c->d, S->acc, S->edges(), M);
  HIPCHK(c, hipGetLastError());
  S->finalized = true;               // blomgpu_dia_reduce is refused from here until a reset or a new selection
  return 0;
}

// ---- the depth levels (blomgpu_dia_set_levels): ddm + 1 edges kept in the context, copied to the device with a selection ----------
static bool dia_has_levels(const blomgpu_ctx *c) { return c->dia && c->dia->ddm; }

int dia_set_levels(blomgpu_ctx *c, const double *bnds, int ddm) {
  if (dia_has_levels(c)) return ctx_fail(c, "blomgpu_dia_set_levels: a depth-level accumulator is selected; deselect the *lvl names first");
  if (!bnds && ddm == 0) { c->dia_edges.clear(); return 0; }             // back to the 35 levels of :111-128
  if (!bnds || ddm < 1) return ctx_fail(c, "blomgpu_dia_set_levels: bounds and ddm >= 1, or NULL and 0 for the default table");
  if (ddm > DIA_MAXLEV) return ctx_fail(c, "blomgpu_dia_set_levels: ddm = " + std::to_string(ddm) + ": at most " + std::to_string(DIA_MAXLEV) + " levels");
  for (int d = 0; d < ddm; d++) {
    if (!(bnds[2 * d + 1] > bnds[2 * d])) return ctx_fail(c, "blomgpu_dia_set_levels: the bounds of level " + std::to_string(d + 1) + " are not increasing");
    if (d + 1 < ddm && bnds[2 * d + 1] != bnds[2 * d + 2])
      return ctx_fail(c, "blomgpu_dia_set_levels: levels " + std::to_string(d + 1) + " and " + std::to_string(d + 2) + " are not contiguous (bnds[d][1] == bnds[d+1][0])");
  }
  c->dia_edges.assign(1, bnds[0]);
  for (int d = 0; d < ddm; d++) c->dia_edges.push_back(bnds[2 * d + 1]);
  return 0;
}

int dia_levels_levitus2x(blomgpu_ctx *c) {                                 // LEVITUS2X, :130-159
  if (dia_has_levels(c)) return ctx_fail(c, "blomgpu_dia_levels_levitus2x: a depth-level accumulator is selected; deselect the *lvl names first");
  c->dia_edges.assign(g_edges70, g_edges70 + 71);
  return 0;
}

int dia_get_levels(blomgpu_ctx *c, double *bnds, int cap, int *ddm) {
  if (!ddm) return ctx_fail(c, "blomgpu_dia_get_levels: null argument");
  const double *e = c->dia_edges.empty() ? g_edges35 : c->dia_edges.data();
  *ddm = c->dia_edges.empty() ? 35 : (int)c->dia_edges.size() - 1;
  for (int d = 0; bnds && d < *ddm && d < cap; d++) { bnds[2 * d] = e[d]; bnds[2 * d + 1] = e[d + 1]; }
  return 0;
}

// ---- the density classes (blomgpu_dia_set_sigdia): kk values kept in the context, copied to the device with a selection -----------
int dia_set_sigdia(blomgpu_ctx *c, const double *sigdia, int n) {
  const bool selected = c->dia && c->dia->ncls;
  const char *held = "blomgpu_dia_set_sigdia: a density-class accumulator is selected; deselect the class names first";
  if (!sigdia && n == 0) {
    if (selected) return ctx_fail(c, held);
    c->dia_sigdia.clear();
    return 0;
  }
  if (!sigdia || n != c->h.kk) return ctx_fail(c, "blomgpu_dia_set_sigdia: sigdia and n == kdm = " + std::to_string(c->h.kk) + ", or NULL and 0 to clear the table");
  for (int k = 0; k < n; k++)
    if (!(sigdia[k] - sigdia[k] == 0.)) return ctx_fail(c, "blomgpu_dia_set_sigdia: sigdia(" + std::to_string(k + 1) + ") is not finite");
  if (selected) return ctx_fail(c, held);
  c->dia_sigdia.assign(sigdia, sigdia + n);        // otherwise as given: the reference checks nothing (phy/mod_vcoord.F90:978-1005, :1103)
  return 0;
}

int dia_get_sigdia(blomgpu_ctx *c, double *out, int cap, int *n) {
  if (!n) return ctx_fail(c, "blomgpu_dia_get_sigdia: null argument");
  *n = (int)c->dia_sigdia.size();
  for (int k = 0; out && k < *n && k < cap; k++) out[k] = c->dia_sigdia[k];
  return 0;
}

// the accumulation of one step (without the count: blomgpu_diaacc and blomgpu_step add it, a graph capture must not)
int st_diaacc(blomgpu_ctx *c, int m, int n, int mm, int nn, int k1m, int k1n) {
  (void)k1m; (void)k1n;
  DiaState *S = c->dia;
  if (!S) return 0;
  const DevView &h = c->h;
  // the density classes, in the reference's position (:1368-1538, in front of acch2d): sigint at the owned points under isopyc_bulkml
  // (cntiso_hybrid: what ale_regrid_remap left, stage_ale.hip), its one-point halo, then one launch per grid with a selected name
  if (S->ncls) {
    if (h.P.vcoord_tag == 3) return ctx_fail(c, "diaacc: a density-class accumulator is selected, which reads sigint; vcoord_type = 'plevel' never writes it");
    if (h.P.vcoord_tag == 1) {
      TimeScope ts(c, "diasig_int");
      hipLaunchKernelGGL(k_diasig_int, plane_grid(h, h.kk), dim3(256), 0, c->stream, c->d, mm);
      HIPCHK(c, hipGetLastError());
    }
    if (int rc = st_xctilr(c, h.f[F_sigint], 1, h.kk, 1, 1, 1)) return rc;          // xctilr(sigint,1,kk, 1,1, halo_ps), :1392
    for (int g = G_U; g <= G_V; g++) {
      SigTab T;
      T.n = 0;
      memset(T.d, 0, sizeof(T.d));
      for (size_t s = 0; s < S->rows.size(); s++) {
        const DiaRow &r = g_rows[S->rows[s]];
        if (r.lyr != 3 || r.grid != g) continue;
        int *d = T.d[T.n++];
        d[0] = r.src; d[1] = nn; d[2] = S->plane0[s];
      }
      if (!T.n) continue;
      TimeScope ts(c, g == G_U ? "diasig_u" : "diasig_v");
      if (g == G_U) launch_diasig<G_U>(c, S, T);
      else launch_diasig<G_V>(c, S, T);
      HIPCHK(c, hipGetLastError());
    }
  }
  // the layer potential vorticity pair, in the reference's position (:1203-1249)
  const auto plane_of = [&](const char *nm) { return (size_t)S->plane0[S->slot_of(find_row(nm))]; };
  if (S->pv) {
    TimeScope ts(c, "diapv");
    hipLaunchKernelGGL(k_diapv, plane_grid(h, h.kk), dim3(256), 0, c->stream, c->d, S->acc, (int)plane_of("avdsg"), (int)plane_of("dpvor"), mm);
    HIPCHK(c, hipGetLastError());
  }
  // the column-derived 2-D diagnostics (:1251-1366) and the mldl82 family, in front of the 2-D accumulation
  if (S->col) {
    ColTab T;
    for (int x = 0; x < C_N; x++) T.p[x] = -1;
    for (size_t s = 0; s < S->rows.size(); s++)
      if (g_rows[S->rows[s]].op == OP_COL) T.p[g_rows[S->rows[s]].src] = S->plane0[s];
    TimeScope ts(c, "diacol");
    hipLaunchKernelGGL(k_diacol, plane_grid(h), dim3(256), 0, c->stream, c->d, S->acc, T, mm);
    HIPCHK(c, hipGetLastError());
  }
  for (int pass = 1; pass >= 0; pass--) {
    DiaTab T;
    T.n = 0; T.need = 0; T.lyr = pass; T.mlev = m - 1;
    for (size_t s = 0; s < S->rows.size(); s++) {
      const DiaRow &r = g_rows[S->rows[s]];
      if (r.lyr != pass || r.op >= OP_VFL) continue;
      int src = r.src, aux = r.aux, f2 = 0, l2 = 0, lev = 0, sreg = 0;
      switch (r.lev) {
        case LV_0: lev = 0; break;
        case LV_M: lev = m - 1; break;
        case LV_N: lev = n - 1; break;
        case LV_KK: lev = h.kk; break;
        case LV_MM: lev = mm; break;
        case LV_NN: lev = nn; break;
        case LV_TKE: lev = (h.P.itrtke - 1) * 2 * h.kk + mm; break;       // trc(:,:,k1m,itrtke)
        case LV_GLS: lev = (h.P.itrgls - 1) * 2 * h.kk + mm; break;
      }
      if (src == SRC_DPML) {
        if (h.P.vcoord_tag == 1) { src = F_dp; lev = mm; aux = A_PLANE; f2 = F_dp; l2 = mm + 1; }      // :1155
        else { src = F_OBLdepth; lev = 0; aux = A_ONEM; }                                              // :1165
      }
      if (pass && lev == mm && (src == F_dp || src == F_dpu || src == F_dpv)) sreg = src == F_dp ? W_DP : src == F_dpu ? W_DPU : W_DPV;
      if (r.wgt) T.need |= 1 << (r.wgt - 1);
      if (sreg) T.need |= 1 << (sreg - 1);
      if (aux == A_UB) T.need |= 8;
      if (aux == A_VB) T.need |= 16;
      int *d = T.d[T.n++];
      d[0] = src; d[1] = lev; d[2] = f2; d[3] = l2;
      d[4] = r.grid | r.op << 2 | r.wgt << 4 | aux << 6 | sreg << 9;
      d[5] = S->plane0[s];
    }
    if (!T.n) continue;
    TimeScope ts(c, pass ? "diaacc_lyr" : "diaacc_h2d");
    hipLaunchKernelGGL(k_diaacc, plane_grid(h, pass ? h.kk : 1), dim3(256), 0, c->stream, c->d, S->acc, T, mm);
  }
  // diavfl's group, part 1 (:1921-1942, in front of the level launches): uflxold = uflxlvl, vflxold = vflxlvl -- the whole padded
  // planes, so that the halo column and row of the last exchange go along (the reference copies out to ii+1 | jj+1)
  if (S->vfl) {
    TimeScope ts(c, "diavfl_copy");
    const size_t nb = sizeof(double) * (size_t)S->ddm * S->np;
    HIPCHK(c, hipMemcpyAsync(S->acc + plane_of("uflxold") * S->np, S->acc + plane_of("uflxlvl") * S->np, nb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S->acc + plane_of("vflxold") * S->np, S->acc + plane_of("vflxlvl") * S->np, nb, hipMemcpyDeviceToDevice, c->stream));
  }
  // the depth levels: one launch per grid that has a selected name, in the reference's order u, v, p
  static const int order[3] = {G_U, G_V, G_P};
  for (int o = 0; S->ddm && o < 3; o++) {
    const int g = order[o];
    LvlTab T;
    T.n = 0; T.ddm = S->ddm; T.mlev = m - 1;
    T.tfld = g == G_P ? F_dp : g == G_U ? F_dpu : F_dpv;
    T.cfld = g == G_P ? F_dp : g == G_U ? F_uflx : F_vflx;
    T.clev = g == G_P ? mm : nn;
    for (size_t s = 0; s < S->rows.size(); s++) {
      const DiaRow &r = g_rows[S->rows[s]];
      if (r.lyr != 2 || r.grid != g || r.op >= OP_VFL) continue;
      if (h.P.vcoord_tag != 1 && hybrid_remapped(S->rows[s])) continue;      // :1944, :2059, :2174 leave them out: stage_ale.hip forms them
      int *d = T.d[T.n++];
      d[0] = r.src;
      d[1] = r.lev == LV_MM ? mm : r.lev == LV_NN ? nn : r.lev == LV_TKE ? (h.P.itrtke - 1) * 2 * h.kk + mm : r.lev == LV_GLS ? (h.P.itrgls - 1) * 2 * h.kk + mm : 0;
      d[2] = (r.op == OP_LVLFLX ? 1 : 0) | (r.aux != A_NONE ? 2 : 0);
      d[3] = S->plane0[s];
    }
    if (!T.n) continue;
    for (int s = T.n; s < LVL_MAXSLOT; s++) T.d[s][0] = T.d[s][1] = T.d[s][2] = T.d[s][3] = 0;
    TimeScope ts(c, g == G_P ? "dialvl_p" : g == G_U ? "dialvl_u" : "dialvl_v");
    const dim3 grid = plane_grid(h, (T.n + LVL_NS - 1) / LVL_NS);
    if (g == G_P) hipLaunchKernelGGL((k_dialvl<G_P>), grid, dim3(256), 0, c->stream, c->d, S->acc, S->edges(), T, mm);
    else if (g == G_U) hipLaunchKernelGGL((k_dialvl<G_U>), grid, dim3(256), 0, c->stream, c->d, S->acc, S->edges(), T, mm);
    else hipLaunchKernelGGL((k_dialvl<G_V>), grid, dim3(256), 0, c->stream, c->d, S->acc, S->edges(), T, mm);
  }
  HIPCHK(c, hipGetLastError());
  // diavfl's group, part 2 (:2279 -> :4633-4733), behind every other accumulation of the step
  if (S->vfl) {
    {
      TimeScope ts(c, "diavfl_lyr");
      hipLaunchKernelGGL(k_diavfl_lyr, plane_grid(h), dim3(256), 0, c->stream, c->d, S->acc, (int)plane_of("wflx"), (int)plane_of("wflx2"), mm, nn);
      HIPCHK(c, hipGetLastError());
    }
    {
      TimeScope ts(c, "diavfl_xctilr");
      if (int rc = st_xctilr(c, S->acc + plane_of("uflxlvl") * S->np, 1, S->ddm, 1, 1, 13)) return rc;      // halo_uv, :4681
      if (int rc = st_xctilr(c, S->acc + plane_of("vflxlvl") * S->np, 1, S->ddm, 1, 1, 14)) return rc;      // halo_vv, :4683
    }
    TimeScope ts(c, "diavfl_lvl");
    hipLaunchKernelGGL(k_diavfl_lvl, plane_grid(h), dim3(256), 0, c->stream, c->d, S->acc, (int)plane_of("uflxlvl"), (int)plane_of("vflxlvl"),
                       (int)plane_of("uflxold"), (int)plane_of("vflxold"), (int)plane_of("wflxlvl"), (int)plane_of("wflx2lvl"), S->ddm);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}
