"""Stage sequencing of one baroclinic step of the dynamical core.

Mirrors the order of phy/mod_blom_step.F90:96-253 for the isopyc_bulkml branch,
restricted to the stages of the hot path and the ones sitting between them
(SURVEY.md 8a/8f).  convec (phy/mod_blom_step.F90:174, between momtum and diapfl) is part of it.  Stages whose
reference modules need netCDF/CVMix (cmnfld, difest, mxlayr, thermf) are not part of the sequence: diffusivities and isopycnal slopes stay frozen.  eddtra is
part of it; the reference build used as oracle cannot contain it (mod_eddtra needs mod_difest ->
CVMix), so a backend without it skips it -- with zero slopes nslpx/nslpy, which is what the
reference-pinned cases use, eddtra's result is exactly the zero fluxes that backend keeps.
"""
from .hostinit import step_indices

DYNCORE_STAGES = ("init_fluxes", "tmsmt1", "halo_cmnfld2", "halo_difest", "eddtra", "advect", "pbcor1",
                  "diffus", "pgforc", "momtum", "convec", "diapfl", "mxlayr_tail", "updtrc", "barotp", "pbcor2",
                  "tmsmt2")
OPTIONAL_STAGES = ("eddtra",)
# halo_cmnfld2 / halo_difest : the xctilr calls of phy/mod_cmnfld_routines.F90:1171-1172 and
#   phy/mod_difest.F90:750-755 (the stages themselves are out of scope, their halo updates
#   are not: advect and momtum read those halos).
# mxlayr_tail : phy/mod_mxlayr.F90:1266-1310, halo of dp at the new level + dpu/dpv.


# Config 2 "full blom_step" as far as it is built: cmnfld2 on the live state, the part of difest_isobml in front
# of the diffusivity estimates (halos, interface pressure, ustar3, niw_ke_tendency: "difest_isobml_pre"), thermf and mxlayr in
# place of the mxlayr_tail pseudo-stage, cmnfld1 at the end -- the order of phy/mod_blom_step.F90:126-233 for isopyc_bulkml.
# Still frozen: the diffusivities themselves (difest_common/vertical/lateral_iso need CVMix at module level).
FULL_STAGES = tuple({"halo_cmnfld2": "cmnfld2", "halo_difest": "difest_isobml_pre"}.get(s, s) for s in DYNCORE_STAGES
                    if s != "mxlayr_tail")
FULL_STAGES = FULL_STAGES[:FULL_STAGES.index("diapfl") + 1] + ("thermf", "mxlayr") + FULL_STAGES[FULL_STAGES.index("diapfl") + 1:] + ("cmnfld1",)

# ... and with the diffusivity estimates of difest_isobml live (difest_common_iso, difest_vertical_iso, difest_lateral_iso; the device
# option difest_live): the whole routine in place of its front part
FULL_STAGES_LIVE = tuple("difest_isobml" if s == "difest_isobml_pre" else s for s in FULL_STAGES)

# diaacc (phy/mod_blom_step.F90:239): the time-mean diagnostics of the accumulators selected with BlomGpu.dia_select.  Part of no
# list above: a host that steps stage by stage appends it (stages=FULL_STAGES + DIAG_STAGES); BlomGpu.step runs it by itself
# whenever a selection exists.
DIAG_STAGES = ("diaacc",)
# ale_remap_diazlv (phy/mod_blom_step.F90:271-273; cntiso_hybrid / plevel only): the end-of-step sample of templvl salnlvl uvellvl
# vvellvl on an output step.  Part of no step: the host calls it after the step while its output alarm (BlomGpu.dia_alarm) is 1.
DIAG_OUTPUT_STAGES = ("ale_remap_diazlv",)

STAGES_FROZEN_EDDY_FLUXES = tuple(s for s in DYNCORE_STAGES if s != "eddtra")    # umfltd.. stay as uploaded

# The step of the other vertical coordinates (vcoord_type = 'cntiso_hybrid' or 'plevel'), phy/mod_blom_step.F90:126-233, as far
# as it is built: ale_regrid_remap in front, the ALE column physics (cmnfld_bfsqi_ale, ale_forcing, ale_vdifft, ale_vdiffm) in
# place of convec / diapfl / mxlayr, cmnfld1 at the end (the mixed layer depth ale_forcing reads).  Left out, as their modules
# need CVMix: difest_lateral_hybrid, difest_vertical_hybrid (the diffusivities, the non-local fractions and the boundary layer
# depth stay as uploaded); thermf (the surface fluxes stay as uploaded).  eddtra runs its ALE form (eddtra_ale).
# halo_difest_hyb / halo_difest_vert: the xctilr calls of the two routines that are left out (phy/mod_difest.F90:826-831, :877-878).
HYBRID_STAGES = ("init_fluxes", "tmsmt1", "ale_regrid_remap", "cmnfld2", "halo_difest_hyb", "eddtra", "advect", "pbcor1", "diffus", "pgforc",
                 "momtum", "cmnfld_bfsqi_ale", "ale_forcing", "halo_difest_vert", "ale_vdifft", "ale_vdiffm", "updtrc", "barotp",
                 "pbcor2", "tmsmt2", "cmnfld1")

# The coupled experiment (expcnf = 'cesm'), once BlomGpu.inifrc_cesm has declared the coupler's forcing: getfrc_cesm behind init_fluxes
# (phy/mod_blom_step.F90:116), sfcstr in front of pgforc (:163), and thermf at :188 -- which the full-physics tuples hold already and the
# hybrid step gains (behind momtum: the reference calls it in front of cmnfld_bfsqi_ale).  The dynamical core runs the first two only.
def _cesm(stages, thermf_after=None):
    out = []
    for s in stages:
        if s == "pgforc":
            out.append("sfcstr")
        out.append(s)
        if s == "init_fluxes":
            out.append("getfrc_cesm")
        if s == thermf_after:
            out.append("thermf")
    return tuple(out)


DYNCORE_STAGES_CESM = _cesm(DYNCORE_STAGES)
FULL_STAGES_CESM = _cesm(FULL_STAGES)
FULL_STAGES_LIVE_CESM = _cesm(FULL_STAGES_LIVE)
HYBRID_STAGES_CESM = _cesm(HYBRID_STAGES, thermf_after="momtum")


# The forced ocean-ice experiment (expcnf = 'ben02clim' / 'ben02syn' / 'single_column'), once BlomGpu.inifrc_ben02 has declared its forcing:
# sfcstr in front of pgforc and thermf at phy/mod_blom_step.F90:188, as above; no getfrc stage (asflux stays on the host).
def _ben02(stages, thermf_after=None):
    return tuple(s for s in _cesm(stages, thermf_after) if s != "getfrc_cesm")


DYNCORE_STAGES_BEN02 = _ben02(DYNCORE_STAGES)
FULL_STAGES_BEN02 = _ben02(FULL_STAGES)
FULL_STAGES_LIVE_BEN02 = _ben02(FULL_STAGES_LIVE)
HYBRID_STAGES_BEN02 = _ben02(HYBRID_STAGES, thermf_after="momtum")


# The end of blom_step, once its options declare it (BlomGpu.set "swamth" + iniswa, "sprfac", "chkvar"): updswa behind getfrc
# (phy/mod_blom_step.F90:122), fwbbal behind diaacc (:242), chkvar last (:252).  Each stage returns at once unless declared, so the tuples
# may carry all three.  step_time (:99) is the host's in a stage-by-stage step (stepend_ref.step_time restates it; BlomGpu.step does it
# itself with the option "step_time").
def with_step_end(stages):
    out = []
    for s in stages:
        out.append(s)
        if s == ("getfrc_cesm" if "getfrc_cesm" in stages else "init_fluxes"):
            out.append("updswa")
    return tuple(out) + ("fwbbal", "chkvar")


FULL_STAGES_LIVE_END = with_step_end(FULL_STAGES_LIVE)
FULL_STAGES_LIVE_CESM_END = with_step_end(FULL_STAGES_LIVE_CESM)
HYBRID_STAGES_CESM_END = with_step_end(HYBRID_STAGES_CESM)
FULL_STAGES_LIVE_BEN02_END = with_step_end(FULL_STAGES_LIVE_BEN02)
HYBRID_STAGES_BEN02_END = with_step_end(HYBRID_STAGES_BEN02)


# mod_budget's conservation diagnostics (phy/mod_budget.F90; the option cnsvdi): budget_sums' seven calls as pseudo-stages budget_sums1..7
# where blom_step has them (phy/mod_blom_step.F90:96, :132/:156, :159/:177, :183/:205, :215, :224, :230) and budget_output behind fwbbal and
# in front of chkvar (:245).  Each returns at once unless cnsvdi is set.  BlomGpu.step places them itself with the option "budget_step".
def with_budget(stages):
    hybrid = "ale_regrid_remap" in stages
    behind = {("ale_regrid_remap" if hybrid else "diffus"): 2, ("diffus" if hybrid else "convec"): 3, ("ale_vdiffm" if hybrid else "diapfl"): 4,
              "updtrc": 5, "pbcor2": 6, "tmsmt2": 7}
    out = ["budget_sums1"]
    for s in stages:
        if s == "chkvar":
            out.append("budget_output")
        out.append(s)
        if s in behind:
            out.append("budget_sums%d" % behind[s])
    if "chkvar" not in stages:
        out.append("budget_output")
    return tuple(out)


def dyncore_step(be, nstep, baclin, stages=DYNCORE_STAGES, hook=None):
    """Advance backend `be` from step count nstep to nstep+1.  `hook(stage, sextuple)` is
    called before each stage (tests use it to snapshot stage inputs)."""
    six = step_indices(nstep, be.kdm)
    be.set("nstep", nstep + 1)               # step_time, phy/mod_blom_step.F90:99
    for st in stages:
        if st in OPTIONAL_STAGES and not getattr(be, "has_stage", lambda s: True)(st):
            continue
        if hook is not None:
            hook(st, six)
        be.stage(st, *six)
    be.set("delt1", baclin + baclin)         # phy/mod_blom_step.F90:300
    return nstep + 1
