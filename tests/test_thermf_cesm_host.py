"""The coupled experiment's surface forcing, what can be checked without a device: thermf_cesm's kernels share no written array with
diapfl's momentum mixing, beside which blomgpu_step runs them (option phys_dag bit 2; tools/kernel_rw_sets.py on the
sources), the stepper's tuples hold the reference's order (phy/mod_blom_step.F90:108-207), the header, the Python mirror and the Fortran
module name the same new entry points, and the numpy restatement's xcsum and time interpolation do what the reference's text says."""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_rw_sets import rw_sets  # noqa: E402
import thermf_cesm_ref as R  # noqa: E402

CSRC = os.path.join(ROOT, "blom_amd", "csrc")


def test_thermf_cesm_shares_no_written_array_with_diapfls_momentum_mixing():
    def touched(chain):
        r, w = set(), set()
        for f, k in chain:
            rr, ww = rw_sets(os.path.join(CSRC, f), k)
            assert rr | ww, (f, k, "no array found: the parser lost the kernel")
            r |= rr | ww
            w |= ww
        return r, w
    rs, ws = touched([("stage_diapfl.hip", "k_diapfl_momentum"), ("stage_diapfl.hip", "k_diapfl_dpudpv")])
    # (the batched sums in between take their planes as pointers: thermf_util, util2, util3 -- all in the flux kernel's set)
    rm, wm = touched([("stage_thermf_cesm.hip", "k_thermf_cesm_flux"), ("stage_thermf_cesm.hip", "k_thermf_cesm_corr")])
    # the parser files a store through a helper's pointer argument under the reads: everything the forcing kernels touch counts as written
    assert {"F_t_rs_nonloc", "F_s_rs_nonloc", "F_thermf_util", "F_surflx", "F_p", "F_dp", "F_temp"} <= rm
    masks = {"I_ip", "I_iu", "I_iv", "I_iq"}
    clash = ((ws & rm) | (rm & rs & (wm | {"F_t_rs_nonloc", "F_s_rs_nonloc"}))) - masks
    assert not clash, sorted(clash)
    assert ws == {"F_u", "F_v", "F_dpu", "F_dpv"}
    # momtum's viscous chain may be on the second stream while sfcstr writes the wind stress: the chain's kernel reads none
    r, w = rw_sets(os.path.join(CSRC, "stage_momtum_fused.hip"), "k_mom_visc_march")
    assert not ({"F_taux", "F_tauy"} & (r | w))


def test_stepper_tuples_hold_the_reference_order():
    from blom_amd import stepper as S
    for base, cesm in ((S.DYNCORE_STAGES, S.DYNCORE_STAGES_CESM), (S.FULL_STAGES, S.FULL_STAGES_CESM),
                       (S.FULL_STAGES_LIVE, S.FULL_STAGES_LIVE_CESM), (S.HYBRID_STAGES, S.HYBRID_STAGES_CESM)):
        assert tuple(s for s in cesm if s not in ("getfrc_cesm", "sfcstr") and not (s == "thermf" and "thermf" not in base)) == base
        assert cesm[cesm.index("init_fluxes") + 1] == "getfrc_cesm" and cesm[cesm.index("pgforc") - 1] == "sfcstr"
    assert "thermf" not in S.DYNCORE_STAGES_CESM
    h = S.HYBRID_STAGES_CESM
    assert h.index("momtum") < h.index("thermf") < h.index("cmnfld_bfsqi_ale") < h.index("ale_forcing")
    f = S.FULL_STAGES_CESM
    assert f.index("diapfl") < f.index("thermf") < f.index("mxlayr") and f.count("thermf") == 1


def test_the_three_interfaces_name_the_same_entry_points():
    hdr = open(os.path.join(ROOT, "include", "blomgpu.h")).read()
    py = open(os.path.join(ROOT, "blom_amd", "gpu.py")).read()
    f90 = open(os.path.join(ROOT, "blom_amd", "fortran", "mod_blomgpu.F90")).read()
    for nm in ("blomgpu_inifrc_cesm", "blomgpu_getfrc_cesm", "blomgpu_cesm_nflxdi", "blomgpu_upload_level"):
        assert re.search(r"\b%s\s*\(" % nm, hdr) and nm in py and ("name='%s'" % nm) in f90, nm
    assert "blomgpu_xcsum_batch" in hdr and "blomgpu_xcsum_batch" in py
    api = open(os.path.join(CSRC, "api.hip")).read()
    for opt in "smtfrc nstep_in_cpl l1ci l2ci use_stream_relaxation nstep_in_day nday_of_year".split():
        assert "(%s)" % opt in api, opt


def test_restated_xcsum_takes_the_reference_order():
    rng = np.random.default_rng(1)
    idm, jdm = 23, 7
    a = rng.standard_normal((jdm + 8, idm + 8)) * 10.0 ** rng.integers(-8, 8, (jdm + 8, idm + 8))
    m = (rng.random((jdm + 8, idm + 8)) > 0.3).astype(np.int32)
    rows = []
    for j in range(jdm):                                   # phy/mod_xc.F90:4116-4161, loop for loop
        s8 = 0.0
        for i1 in range(0, idm, 9):
            s8p = 0.0
            for i in range(i1, min(i1 + 9, idm)):
                if m[4 + j, 4 + i] == 1:
                    s8p = s8p + a[4 + j, 4 + i]
            s8 = s8 + s8p
        rows.append(s8)
    want = rows[0]
    for r in rows[1:]:
        want = want + r
    assert R.xcsum(a, m, idm, jdm) == want
    rows[-1] = 0.0
    seam = rows[0]
    for r in rows[1:]:
        seam = seam + r
    assert R.xcsum(a, m, idm, jdm, skip_seam=True) == seam


def test_restated_scalars():
    o = dict(smtfrc=1, nstep=6, nstep_in_cpl=4)
    w1, w2 = R.weights(o)
    assert w1 == 0.5 * (1.0 + math.cos(2 * 3.1415926536 / 4)) and w2 == 1.0 - w1
    assert R.weights(dict(smtfrc=0)) == (0.0, 1.0)
    y, m = R.time_of_year(dict(nday_of_year=1, nstep=3, nstep_in_day=4, nday_in_year=24))
    assert (y, m) == (0.5, (48, 1, 2, 3, 4))
    y, m = R.time_of_year(dict(nday_of_year=365, nstep=0, nstep_in_day=4, nday_in_year=365))
    assert m == (46, 47, 48, 1, 2) and 0.0 <= y < 1.0
    # phy/mod_intp1d.F90:29-52: the cubic through equal values is that value up to the rounding of its coefficients' sums
    assert abs(R.intp1d(2.0, 2.0, 2.0, 2.0, 2.0, 0.37) - 2.0) < 4.0e-15
    assert R.intp1d(0.0, 1.0, 0.0, 0.0, 0.0, 0.0) == -1.0 / 7.0 * 0.0 + 9.0 / 14 * 1.0


def test_the_fortran_wrappers_are_linked_into_the_host_program():
    """tests/hostemu's blom_dyncore_hostemu is built from mod_blomgpu.F90: a binary linked from the module as it stands names the new
    entry points among its undefined dynamic symbols, and is no older than the module"""
    f90 = os.path.join(ROOT, "blom_amd", "fortran", "mod_blomgpu.F90")
    exe = os.path.join(ROOT, "tests", "hostemu", "blom_dyncore_hostemu")
    import pytest
    if not os.path.exists(exe):
        pytest.skip("tests/hostemu/blom_dyncore_hostemu not built")
    blob = open(exe, "rb").read()
    for nm in (b"blomgpu_inifrc_cesm", b"blomgpu_getfrc_cesm", b"blomgpu_cesm_nflxdi", b"blomgpu_upload_level"):
        assert nm in blob, nm
    assert os.path.getmtime(exe) >= os.path.getmtime(f90)
