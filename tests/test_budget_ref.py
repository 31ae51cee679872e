"""tests/budget_ref.py, the numpy restatement of mod_budget's planes, against the compiled reference (oracle/_ref/<cfg>/libblomref.so):
budget_sums (phy/mod_budget.F90:95-196) leaves its column sums in util1..util4 -- tracer 1's in util1 over the salt's, the salt
correction's product over that at the call that carries it -- and every plane it leaves is compared with array_equal at the points the
routine writes.  chan_s_tk2 is the build with -DGLS: util4.  CPU only; the yardstick of tests/test_gpu_budget.py."""
import numpy as np
import pytest

from blom_amd import hostinit
from blom_amd.cases import make_case
from blom_amd.stepper import dyncore_step
import budget_ref as R

CFGS = ["chan_s", "box_s", "fuk95", "tri_s", "chan_s_tke", "tri_s_tke", "chan_s_tk2"]


@pytest.mark.parametrize("cfg", CFGS)
def test_restated_planes_equal_what_the_compiled_budget_sums_leaves(cfg):
    from oracle.refblom import get_ref_backend, have_ref
    if not have_ref(cfg):
        pytest.skip(f"oracle/_ref/{cfg}/libblomref.so not built")
    case = make_case(cfg)
    ref = get_ref_backend(cfg, case.depth)
    hostinit.init_state(ref, case)
    for nm, a in R.seeded_forcing(case, ref.ntr).items():
        ref.put(nm, a)
    nstep = 0
    for _ in range(2):
        nstep = dyncore_step(ref, nstep, case.params["baclin"])
    nt = R.tracer_set(ref.ntr, case.params)
    assert nt == {"chan_s_tke": 2, "tri_s_tke": 2, "chan_s_tk2": 3}.get(cfg, nt) and (nt >= 1) == (ref.ntr >= 1)
    sel = R.owned(ref.masks["ip"], case.idm, case.jdm)
    util = lambda k: R.planes_of(ref, "util%d" % k, case.idm, case.jdm)[0]
    ref.set("cnsvdi", 1)
    try:
        for n in (1, 2):
            off = (n - 1) * case.kdm
            for ncall in (2, 5):
                for k in range(1, 5):
                    ref.put("util%d" % k, np.full(sel.shape, -7.5)[None])
                ref.budget_sums(ncall, n, off)
                mine = R.column_planes(ref, case, off, nt)
                left = {2: "tdp"}
                if nt >= 2:
                    left[3] = "tkedp"
                if nt >= 3:
                    left[4] = "glsdp"
                for k, nm in left.items():
                    assert np.array_equal(util(k)[sel], mine[nm][sel]) and mine[nm][sel].any(), (cfg, ncall, n, nm)
                    assert (util(k)[~sel] == -7.5).all()
                for k in range(2, 5):
                    if k not in left:
                        assert (util(k) == -7.5).all(), (cfg, k)
                if ncall == 5:
                    want = R.salt_corr_plane(ref, case)
                elif nt >= 1:
                    want = mine["trdp"]
                else:
                    want = mine["sdp"]
                assert np.array_equal(util(1)[sel], want[sel]) and want[sel].any(), (cfg, ncall, n)
                assert (util(1)[~sel] == -7.5).all()
    finally:
        ref.set("cnsvdi", 0)


def test_lines_restated_on_numbers_worked_by_hand():
    """the six differences and where the forcing term goes (phy/mod_budget.F90:214-220, :274-280), on numbers whose terms are exact"""
    prev, cur = R.new_record(), R.new_record()
    prev["sdp"][:5] = [1.0, 3.0, 6.0, 10.0, 15.0]
    cur["sdp"][5:] = [21.0, 28.0]
    prev.update(sc=0.5, sf=1.5)
    iso = R.line_terms(prev, cur, 2.0, "salbud", True)
    hyb = R.line_terms(prev, cur, 2.0, "salbud", False)
    f = (1.5 - 0.5) * R.GRAV
    assert iso == [1.0, 1.5, 2.0, (5.0 + f) / 2.0, 3.0, 3.5]
    assert hyb == [1.0, 1.5, (4.0 + f) / 2.0, 2.5, 3.0, 3.5]
    prev["trdp"][:5] = [2.0, 4.0, 6.0, 8.0, 10.0]
    cur["trdp"][5:] = [12.0, 14.0]
    assert R.line_terms(prev, cur, 2.0, "trcbudtot") == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    assert R.files_of(0) == ["salbud", "tembud"] and R.files_of(2) == ["salbud", "tembud", "tkebud", "trcbud", "trcbudtot"]
    assert R.files_of(3) == list(R.FILES)
