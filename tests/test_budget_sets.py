"""mod_budget's in-step kernels (blom_amd/csrc/stage_budget.hip) against what blomgpu_step has on its second stream where they run, in
the style of tests/test_side_by_side_sets.py and on the same parser (tools/kernel_rw_sets.py): a budget launch reads dp temp saln trc
(and scp2, salt_corr, the surface fluxes) and writes no field of the model, so it needs every WRITER of those arrays behind it on the
context's stream and nothing beside it that writes them.  Checked on the sources, before a race has to be caught by bytes."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_rw_sets import rw_sets  # noqa: E402

CSRC = os.path.join(ROOT, "blom_amd", "csrc")
BUD, DIA, MOM, FUS, SIM, MXL = ("stage_budget.hip", "stage_diapfl.hip", "stage_momtum.hip", "stage_momtum_fused.hip", "stage_simple.hip",
                                "stage_mxlayr.hip")
IN_STEP = [(BUD, "k_budget_rows"), (BUD, "k_budget_rows2d"), (BUD, "k_budget_total")]

# (name, budget kernels, kernels that may be running on the second stream at that place of the step)
WINDOWS = [
    ("calls 2 and 3 beside momtum's viscous chain (forked behind difest, joined inside momtum: call 2 sits between)",
     IN_STEP[:1] + IN_STEP[2:], [(MOM, "k_mom_pscan"), (MOM, "k_mom_pupv"), (FUS, "k_mom_classify"), (FUS, "k_mom_visc_march")]),
    ("calls 3 and 4 beside diapfl's momentum mixing (phys_dag bit 2)",
     IN_STEP[:1] + IN_STEP[2:], [(DIA, "k_diapfl_momentum"), (DIA, "k_diapfl_dpudpv")]),
]


def sets(chain):
    r, w = set(), set()
    for f, k in chain:
        rr, ww = rw_sets(os.path.join(CSRC, f), k)
        r |= rr | ww
        w |= ww
    return r, w


@pytest.mark.parametrize("name,budget,side", WINDOWS, ids=[w[0].split(" (")[0] for w in WINDOWS])
def test_budget_launches_share_no_written_array_with_the_second_stream(name, budget, side):
    rb, wb = sets(budget)
    rs, ws = sets(side)
    assert rs, "no array found: the parser lost the kernels of the second stream"
    clash = (ws & rb) | (wb & rs)
    assert not clash, f"{name}: {sorted(clash)} written on one side and touched on the other"


def test_in_step_budget_kernels_read_the_budgeted_arrays_and_write_no_field():
    r, w = sets(IN_STEP)
    assert {"F_dp", "F_temp", "F_saln", "F_trc", "F_scp2", "F_salt_corr", "F_salflx", "F_salrlx", "F_surflx", "F_surrlx", "F_trflx"} <= r
    assert not w, sorted(w)
    # the form of the tile groups and of a stage-by-stage host goes through the reference's util planes, and only those
    _, wp = rw_sets(os.path.join(CSRC, BUD), "k_budget_planes")
    assert wp == {"F_util1", "F_util2", "F_util3", "F_util4"}


def test_what_raises_updtrc_on_side_is_a_conflict_that_call_5_joins():
    """Two kernels can be on the second stream behind updtrc, both under the flag updtrc_on_side: k_idlage_step (phys_dag bit 4) writes a
    tracer that can be tracer 1, k_mxl_clamp (bit 8, stage_mxlayr.hip) writes saln and the tracers.  The check must see both conflicts,
    both launches must raise the flag, and step_sequence must record and wait for event 9 in front of call 5 for the flag alone -- not for
    the ideal-age case only."""
    r, _ = sets(IN_STEP)
    _, w = rw_sets(os.path.join(CSRC, SIM), "k_idlage_step")
    assert "F_trc" in (w & r)
    _, w = rw_sets(os.path.join(CSRC, MXL), "k_mxl_clamp")
    assert {"F_saln", "F_trc"} <= (w & r), sorted(w)
    for f, kernel in ((SIM, "k_idlage_step"), (MXL, "k_mxl_clamp")):
        src = open(os.path.join(CSRC, f)).read()
        at = src.index("hipLaunchKernelGGL(" + kernel)
        assert "updtrc_on_side = true" in src[at:at + 400], kernel
    api = open(os.path.join(CSRC, "api.hip")).read()
    at = api.index("if (ncall == 5 && budget_on(c) && c->seq.updtrc_on_side) {")
    body = api[at:at + 400]
    assert body.index("ctx_side_done(c, 9)") < body.index("ctx_side_join(c, 9)") < body.index("bud(ncall)")
