"""The forced ocean-ice experiment's surface forcing, what can be checked without a device: thermf_ben02's kernels share no written array
with diapfl's momentum mixing, beside which blomgpu_step runs them (option phys_dag bit 2; tools/kernel_rw_sets.py on
the sources), the stepper's tuples hold the reference's order (phy/mod_blom_step.F90:108-207), the header, the Python mirror and the
Fortran module name the same new entry points, the parameters of mod_thdysi are stated once, and the synthetic forcing is deterministic."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_rw_sets import rw_sets  # noqa: E402
import thermf_ben02_ref as R  # noqa: E402

CSRC = os.path.join(ROOT, "blom_amd", "csrc")
BEN02 = "stage_thermf_ben02.hip"


def touched(chain):
    r, w = set(), set()
    for f, k in chain:
        rr, ww = rw_sets(os.path.join(CSRC, f), k)
        assert rr | ww, (f, k, "no array found: the parser lost the kernel")
        r |= rr | ww
        w |= ww
    return r, w


def test_thermf_ben02_shares_no_written_array_with_diapfls_momentum_mixing():
    rs, ws = touched([("stage_diapfl.hip", "k_diapfl_momentum"), ("stage_diapfl.hip", "k_diapfl_dpudpv")])
    # (the batched sums in between take their planes as pointers: thermf_util, util2, util3 -- all in the flux kernel's set)
    rm, wm = touched([(BEN02, "k_thermf_ben02_flux"), (BEN02, "k_thermf_ben02_corr")])
    assert {"F_t_rs_nonloc", "F_s_rs_nonloc", "F_thermf_util", "F_surflx", "F_p", "F_dp", "F_temp", "F_ficem", "F_hicem", "F_fice_tda",
            "F_rnfres", "F_iagem", "F_plat", "F_swal2"} <= rm
    # what the flux kernel stores through V.f / V.b is seen as written
    assert {"F_ficem", "F_hicem", "F_hsnwm", "F_tsrfm", "F_ticem", "F_alb", "F_alb_tda", "F_tml_tda", "F_sml_tda", "F_fice_tda", "F_tsi_tda",
            "F_rnf", "F_rnfres", "F_fmltfz", "F_sfl", "F_brnflx", "F_hmltfz", "F_surflx", "F_sswflx", "F_surrlx", "F_salrlx", "F_iagem", "F_ustar",
            "F_salflx", "F_salt_corr"} <= wm
    masks = {"I_ip", "I_iu", "I_iv", "I_iq"}
    # what the pair writes the forcing kernels do not touch; what the pair touches they do not write (the parser files a store through a
    # helper's pointer argument under the reads: the two arrays rs_walk fills count as written)
    clash = ((ws & rm) | (rm & rs & (wm | {"F_t_rs_nonloc", "F_s_rs_nonloc"}))) - masks
    assert not clash, sorted(clash)
    assert ws == {"F_u", "F_v", "F_dpu", "F_dpv"}
    # momtum's viscous chain may be on the second stream while sfcstr writes the wind stress and the halos of ficem, hicem
    r, w = rw_sets(os.path.join(CSRC, "stage_momtum_fused.hip"), "k_mom_visc_march")
    rk, wk = rw_sets(os.path.join(CSRC, BEN02), "k_sfcstr_ben02")
    assert wk == {"F_taux", "F_tauy"} and {"F_ficem", "F_hicem", "F_ztx", "F_mty", "F_tauxice", "F_tauyice"} <= rk
    assert not ({"F_taux", "F_tauy", "F_ficem", "F_hicem"} & (r | w))


def test_stepper_tuples_hold_the_reference_order():
    from blom_amd import stepper as S
    for base, ben in ((S.DYNCORE_STAGES, S.DYNCORE_STAGES_BEN02), (S.FULL_STAGES, S.FULL_STAGES_BEN02),
                      (S.FULL_STAGES_LIVE, S.FULL_STAGES_LIVE_BEN02), (S.HYBRID_STAGES, S.HYBRID_STAGES_BEN02)):
        assert tuple(s for s in ben if s != "sfcstr" and not (s == "thermf" and "thermf" not in base)) == base
        assert ben[ben.index("pgforc") - 1] == "sfcstr" and "getfrc_cesm" not in ben
    assert "thermf" not in S.DYNCORE_STAGES_BEN02
    h = S.HYBRID_STAGES_BEN02
    assert h.index("momtum") < h.index("thermf") < h.index("cmnfld_bfsqi_ale") < h.index("ale_forcing")
    f = S.FULL_STAGES_BEN02
    assert f.index("diapfl") < f.index("thermf") < f.index("mxlayr") and f.count("thermf") == 1


def test_the_three_interfaces_name_the_same_entry_points():
    hdr = open(os.path.join(ROOT, "include", "blomgpu.h")).read()
    py = open(os.path.join(ROOT, "blom_amd", "gpu.py")).read()
    f90 = open(os.path.join(ROOT, "blom_amd", "fortran", "mod_blomgpu.F90")).read()
    api = open(os.path.join(CSRC, "api.hip")).read()
    for nm in ("blomgpu_inifrc_ben02", "blomgpu_ben02_ntda", "blomgpu_ben02_reset_tda"):
        assert re.search(r"\bint\s+%s\s*\(" % nm, hdr) and re.search(r"\bint %s\(" % nm, api) and nm in py and ("name='%s'" % nm) in f90, nm
    for ref in ("ben02/mod_thermf_ben02.F90:65-703", "ben02/mod_sfcstr_ben02.F90:35-72", "ben02/mod_thdysi.F90:60-78"):
        assert ref in hdr, ref
    for nm in ("inifrc_ben02", "gpu_ben02_ntda", "gpu_ben02_reset_tda"):
        assert re.search(r"public ::.*\b%s\b" % nm, f90) and re.search(r"subroutine %s\(" % nm, f90), nm


def test_the_fortran_wrappers_are_linked_into_the_host_program():
    """tests/hostemu's blom_dyncore_hostemu is built from mod_blomgpu.F90: the module as it stands compiles, and the library it is
    linked against exports the new entry points"""
    import ctypes
    import pytest
    lib = os.path.join(ROOT, "tests", "hostemu", "libblomgpu_hostemu.so")
    exe = os.path.join(ROOT, "tests", "hostemu", "blom_dyncore_hostemu")
    if not (os.path.exists(lib) and os.path.exists(exe)):
        pytest.skip("tests/hostemu not built")
    so = ctypes.CDLL(lib)
    for nm in ("blomgpu_inifrc_ben02", "blomgpu_ben02_ntda", "blomgpu_ben02_reset_tda"):
        assert hasattr(so, nm), nm
    assert os.path.getmtime(exe) >= os.path.getmtime(os.path.join(ROOT, "blom_amd", "fortran", "mod_blomgpu.F90"))


def test_the_parameters_of_the_slab_are_stated_once():
    """ben02/mod_thdysi.F90:60-78 and ben02/mod_ben02.F90:119, :216 in ben02_constants.h, with the reference's values; no other file of
    the library defines one of the names, and the restatement holds the same numbers"""
    import glob
    want = dict(ALBI_F=.70, ALBI_M=.60, ALBS_F=.85, ALBS_M=.75, RHOICE=906., RHOSNW=330., RKICE=2.04, RKSNW=.31, FUSI=3.02e8, FUSS=1.10e8,
                FICE_MAX=.995, TICE_M=273.05, TSNW_M=273.15, HICE_NHMN=.50, HICE_SHMN=.30, SAGETS=2.e-7, SICE=6., CWI=0.006, CUC=1.e3, RHOWAT=1024.,
                NRFETS=7)
    text = open(os.path.join(CSRC, "ben02_constants.h")).read()
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"constexpr (?:double|int) (\w+) = ([-+.\de]+);", text)}
    assert got == want
    for nm, v in want.items():
        assert getattr(R, nm) == v, nm
    for path in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")):
        if os.path.basename(path) == "ben02_constants.h":
            continue
        src = re.sub(r"//[^\n]*", "", open(path).read())
        for nm in want:
            assert not re.search(r"\b(?:double|int|define)\s+%s\b" % nm, src), (os.path.basename(path), nm)
    assert (R.ATF, R.BTF, R.CTF) == (-0.0547, 0.0, 0.0)


def test_the_synthetic_forcing_is_deterministic_and_complete():
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    case = make_case("chan_s_tke")
    a, b, c = hostinit.ben02_forcing(case, seed=3), hostinit.ben02_forcing(case, seed=3), hostinit.ben02_forcing(case, seed=4)
    assert set(hostinit.BEN02_FLUXES + hostinit.BEN02_ICE + ["plat", "ipwocn", "sstclm", "ricclm", "sssclm", "tflxap", "sflxap"]) <= set(a)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["nsf"], c["nsf"])
    assert (a["plat"] > 0).any() and (a["plat"] < 0).any() and (a["ficem"] == 0).any() and (a["ficem"] == 1).any()
    assert all(v.shape[1:] == (case.jdm + 8, case.idm + 8) for v in a.values())
