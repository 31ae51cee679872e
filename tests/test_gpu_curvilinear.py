"""The parity suites on a curvilinear grid with a varying Coriolis parameter.

Every other GPU test runs on a uniform Cartesian f-plane: all of scpx ... scvy are one constant, corioq = coriop everywhere.  There a
kernel that reads scuy where scvy is meant, a neighbour one point off, scp2 for scu2, corioq at the wrong corner, a tile that received
the wrong window of the grid arrays or a fold that mirrors a metric the wrong way produces the bits of the correct code.  Here the same
helpers run on blom_amd.cases.warped_grid (make_case(..., grid="warped" | "warped_eq")): each metric array its own smooth function at
its own staggered location, +-30 %, aspect ratio 0.7, f varying in i and j and -- warped_eq -- changing sign inside the domain
(tests/test_curvilinear_grid.py checks the grids themselves and that every metric array but scq2 is read).  Every comparison is ==.

The tests call the helpers and test functions of the other files inside `with on_grid(...)` (tests/curvilinear.py: make_case then builds
the named grid for them); nothing is restated here.  Small cases only
(20x24x6 to 84x40x6).  What this does not cover: full-size grids, and the real tnx2v1 / tnx1v4 grid files (poles inside land, cells
down to a few km) -- the full-size tests remain on the uniform grid.

diaacc and dialvl have no case here: their restated reference loops (tests/test_gpu_diaacc.py, tests/test_gpu_dialvl.py) read no grid
field -- the accumulators are sums and maxima of state arrays on the model's own points; scp2 enters only the ocean area, a scalar the
tiled tests hand over."""
import numpy as np
import pytest

from blom_amd import hostinit
from blom_amd.stepper import dyncore_step
from curvilinear import on_grid

pytestmark = pytest.mark.gpu
SKIP = {"util1", "util2", "util3", "util4"}            # scratch planes shared between stages


# ---- stage by stage against the compiled reference (test_gpu_stage_parity) -------------------------------------------------------
@pytest.mark.parametrize("cfg,grid", [("chan_s", "warped"), ("box_s", "warped"), ("tri_s", "warped"), ("chan_s_tke", "warped"),
                                      ("tri_s_tke", "warped"), ("chan_s", "warped_eq"), ("tri_s_tke", "warped_eq")])
def test_stage_parity(cfg, grid):
    from test_gpu_stage_parity import _run, GPU_STAGES
    with on_grid(grid):
        _run(cfg, 4, GPU_STAGES)


def test_stage_parity_with_eddy_fluxes_and_many_tracers():
    from test_gpu_stage_parity import _run, GPU_STAGES
    with on_grid("warped"):
        _run("chan_s_tke", 4, GPU_STAGES, eddy=True, ntr=11)


@pytest.mark.parametrize("cfg", ["chan_s", "box_s"])
def test_stage_parity_option_variants(cfg):
    from test_gpu_stage_parity import _run, GPU_STAGES
    from blom_amd.cases import make_case
    try:
        with on_grid("warped"):
            _run(cfg, 3, GPU_STAGES, mommth="enedis", pgfmth="dynamic enthalpy", bmcmth="dluc")
    finally:                        # the reference instance is shared between tests: back to the defaults
        from oracle.refblom import get_ref_backend
        case = make_case(cfg)
        hostinit.init_state(get_ref_backend(cfg, case.depth), case)


@pytest.mark.parametrize("cfg,nsteps", [("chan_s_tke", 40), ("tri_s_tke", 24)])
def test_freerun_device_resident(cfg, nsteps):
    from test_gpu_stage_parity import _freerun_device
    with on_grid("warped"):
        _freerun_device(cfg, nsteps, 0.0, False)


# ---- cppm: the coefficient tables come from scpx and scpy ------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["chan_s", "tri_s"])
def test_advect_cppm_stage_parity(cfg):
    from test_gpu_cppm import test_advect_cppm_stage_parity as check
    with on_grid("warped"):
        check(cfg, 6, "full", "non_oscillatory")


# ---- eddtra and cmnfld against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["chan_s", "tri_s"])
def test_eddtra_matches_restatement(cfg, monkeypatch):
    import test_gpu_eddtra

    def bigrid(case):               # test_gpu_eddtra's own has no case with an arctic patch and does not ask for one
        nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
        return nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq)
    monkeypatch.setattr(test_gpu_eddtra, "_bigrid", bigrid)
    with on_grid("warped"):
        test_gpu_eddtra.test_eddtra_matches_restatement(cfg, "gm", 5e-3)


@pytest.mark.parametrize("cfg", ["chan_s", "tri_s"])
def test_cmnfld2_matches_restatement_in_a_free_run(cfg):
    from test_gpu_cmnfld import test_cmnfld2_matches_restatement_in_a_free_run as check
    with on_grid("warped"):
        check(cfg)


# ---- the reference's real modules behind stand-ins -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,opts,grid", [("chan_s_tke", "noresm", "warped"), ("tri_s_tke", "noresm", "warped"), ("box_s", "noresm", "warped"),
                                           ("chan_s_tke", "shear", "warped"), ("tri_s_tke", "shear", "warped"), ("box_s", "shear", "warped"),
                                           # |coriop| guards and the sign of f
                                           ("chan_s_tke", "noresm", "warped_eq"), ("chan_s_tke", "shear", "warped_eq")])
def test_full_step_with_live_diffusivities(cfg, opts, grid):
    from test_xcheck_difest import _live_step_check, OPT_SHEAR
    with on_grid(grid):
        _live_step_check(cfg, 6, hostinit.DIFEST_NORESM if opts == "noresm" else OPT_SHEAR)


@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s"])
def test_rhsctp_acts_on_the_layer_interface_diffusivities(cfg):
    """betafp of the warped grid crosses the size at which the topographic Rhines scale takes over (a fifth of init_difest's betatp): the
    test's own bar -- rhsctp changes more than 5 % of difint -- holds on this grid"""
    from test_xcheck_difest import test_rhsctp_acts_on_the_layer_interface_diffusivities as check
    with on_grid("warped"):
        check(cfg)


def test_device_mxlayr_equals_the_real_module():
    from test_xcheck_mxlayr import _mxlayr_check
    with on_grid("warped"):
        _mxlayr_check("tri_s_tke", 3, "default")


def test_device_thermf_equals_the_real_module():
    from test_xcheck_thermf import test_device_thermf_equals_the_real_module as check
    with on_grid("warped"):
        check("chan_s_tke", 3, True)


def test_device_eddtra_equals_the_real_mod_eddtra():
    from test_xcheck_eddtra import test_device_eddtra_equals_the_real_mod_eddtra as check
    with on_grid("warped"):
        check("box_s", "gm", 5e-3)


def test_device_ale_regrid_remap_equals_the_real_module(tmp_path):
    from test_xcheck_ale import _ale_regrid_remap_check
    with on_grid("warped"):
        _ale_regrid_remap_check("tri_s", 3, 0.3, "nudge", tmp_path)


def test_device_eddtra_ale_equals_the_real_module():
    from test_xcheck_eddtra_ale import test_device_eddtra_ale_equals_the_real_module as check
    with on_grid("warped"):
        check("chan_s", "direct", 4, 1e-2, 7, "bod23")


def test_hybrid_step_equals_the_reference_stage_sequence(tmp_path):
    from test_xcheck_hybrid_step import _hybrid_step_check
    with on_grid("warped"):
        _hybrid_step_check("tri_s", "remap", "direct", "cntiso_hybrid", 4, tmp_path)


# ---- kernel variants identical to each other, and to the C restatement (chan_b, tri_m: several 26x16 barotp tiles and 32x8 remap
# tiles; no reference build at these sizes) ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_runs():
    """the C restatement's free run of a case on the warped grid, computed once"""
    from blom_amd.cases import make_case
    from oracle.coracle import COracle
    cache = {}

    def run(cfg, nsteps):
        if (cfg, nsteps) not in cache:
            case = make_case(cfg, grid="warped")
            nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
            orc = COracle(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))
            hostinit.init_state(orc, case)
            ns = 0
            for _ in range(nsteps):
                ns = dyncore_step(orc, ns, case.params["baclin"])
            J, I = slice(4, 4 + case.jdm), slice(4, 4 + case.idm)
            cache[cfg, nsteps] = {nm: orc.get(nm)[..., J, I].copy() for nm in ("dp", "temp", "saln", "u", "v", "pb", "ub", "vb", "uflx", "vflx", "trc")}
        return cache[cfg, nsteps]
    return run


@pytest.mark.parametrize("cfg,nsteps", [("chan_b", 6), ("tri_m", 6)])
def test_variants_bit_identical_and_equal_to_the_c_restatement(cfg, nsteps, oracle_runs):
    """the default kernels (k_bt_steps4 walking a whole phase on chan_b, the persistent pair kernel with the arctic patch on tri_m) against
    one kernel per equation, one launch per pair, four substeps per hand-off, one launch per four substeps and graph replay -- and the
    free run against the C restatement's (pinned on the compiled reference on this grid by tests/test_oracle_vs_reference.py)"""
    from test_gpu_variants import _run
    with on_grid("warped"):
        base = _run(cfg, nsteps)
    assert np.isfinite(base["ub"]).all() and np.abs(base["ub"]).max() > 0.0
    others = [dict(barotp_fused=0, barotp_persist=0), dict(barotp_persist=0), dict(barotp_fused=0), dict(use_graph=1)]
    others += [dict(barotp_arctic_persist=0)] if cfg == "tri_m" else [dict(barotp_block=0), dict(barotp_block=2)]
    for opts in others:
        with on_grid("warped"):
            b = _run(cfg, nsteps, **opts)
        bad = [nm for nm in base if nm not in SKIP and base[nm].tobytes() != b[nm].tobytes()]
        assert not bad, (opts, bad)
    want = oracle_runs(cfg, nsteps)
    nj, ni = want["dp"].shape[-2:]
    bad = [nm for nm, a in want.items() if not np.array_equal(a, base[nm][..., 4:4 + nj, 4:4 + ni], equal_nan=True)]
    assert not bad, bad


@pytest.mark.parametrize("cfg,nsteps", [("chan_b_tke", 4), ("tri_m_tke", 4)])
def test_physics_stages_side_by_side_on_the_second_stream(cfg, nsteps):
    from test_gpu_variants import test_physics_stages_side_by_side_on_the_second_stream as check
    with on_grid("warped"):
        check(cfg, nsteps, True)


# ---- tiles: where a wrong window of the grid becomes visible --------------------------------------------------------------------
@pytest.mark.parametrize("cfg,npx,npy", [("chan_s", 2, 2), ("tri_s", 4, 2), ("tri_s+strips", 2, 2)])
def test_tiles_match_single_tile(cfg, npx, npy):
    from test_gpu_tiles import test_tiles_match_single_tile as check
    with on_grid("warped"):
        check(cfg, npx, npy)


def test_unequal_tiles_match_single_tile():
    from test_gpu_tiles import test_unequal_tiles_match_single_tile as check
    with on_grid("warped"):
        check("tri_s", (6, 6, 6, 6), (11, 9))


def test_ragged_tiles_match_single_tile():
    from test_gpu_ragged_tiles import _run_group
    with on_grid("warped"):
        _run_group("chan_3x2_gap_row_does_not_wrap")


def test_rccl_transport_single_rank_equals_single_tile():
    from test_gpu_tiles import test_rccl_transport_single_rank_equals_single_tile as check
    with on_grid("warped"):
        check()


@pytest.mark.parametrize("live", [False, True])
def test_full_physics_step_on_tiles_matches_single_tile(live, monkeypatch):
    import test_gpu_tiles
    # betafp is not among the fields that test hands to its tiles for live diffusivities: zero everywhere on the f-plane, not here
    monkeypatch.setattr(test_gpu_tiles, "DFE_IN", test_gpu_tiles.DFE_IN + ["betafp"])
    with on_grid("warped"):
        test_gpu_tiles.test_full_physics_step_on_tiles_matches_single_tile("tri_s_tke", 2, 2, live)


# ---- the Fortran host ------------------------------------------------------------------------------------------------------------
# (named so that the host emulation run of this file leaves them out like tests/test_gpu_fortran_host.py: the host program links the real library)
def test_gpu_fortran_host_matches_python_driver(tmp_path):
    """a state file written from the warped chan_s: the Fortran host reads the grid from it like any other field"""
    from test_gpu_fortran_host import test_fortran_driver_matches_python_driver as check
    with on_grid("warped"):
        check(tmp_path)


def test_gpu_fortran_host_one_rank_with_a_1x1_table(tmp_path):
    import os
    from test_gpu_fortran_spmd import test_one_rank_with_a_1x1_table_matches_the_single_context as check, EXE
    if not os.path.exists(EXE):
        pytest.skip("Fortran driver not built")
    with on_grid("warped"):
        check(tmp_path, EXE, "chan_s", False)
