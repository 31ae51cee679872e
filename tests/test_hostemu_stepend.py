"""The end of blom_step on the CPU: the checks of tests/test_gpu_stepend.py (whose functions run here unchanged) on the device library
compiled for the host (tests/hostemu) -- the clock of step_time, k_swa_fill, k_updswa, k_fwbbal_*, k_chkvar and the step around them
against the numpy restatement of tests/stepend_ref.py, with the branch counts that keep the checks from passing on untaken branches.
Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_stepend as t
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = EMU
    h._LIB = EMU
    yield t
    g.LIB_PATH = old
    h._LIB = oldh


def test_step_time_restated():
    import test_gpu_stepend as t
    t.check_clock()


def test_restated_updswa_reaches_every_branch_and_a_hundred_table_entries():
    """the restatement alone, on chan_b's plane: every count positive, at least 100 distinct lookup indices"""
    import numpy as np
    import stepend_ref as R
    from blom_amd.cases import make_case
    case = make_case("chan_b")
    nj, ni = case.jdm + 8, case.idm + 8
    sel = np.zeros((nj, ni), bool)
    sel[4:-4, 4:-4] = True
    for method in ("chlorophyll_ma94", "chlorophyll_ohl03"):
        seen = {}
        s = {nm: np.zeros((1, nj, ni)) for nm in R.BANDS + ("chl10",)}
        s["chl10c"] = R.log10_chl(R.synthetic_chl(nj, ni))
        assert s["chl10c"].min() < -2.0 and s["chl10c"].max() > 1.0
        assert all(not np.array_equal(s["chl10c"][a], s["chl10c"][b]) for a in range(12) for b in range(a))
        R.updswa(s, method, (11, 12, 1, 2, 3), 0.3, sel, seen=seen)
        assert not R.missing(seen, method), seen
        if method == "chlorophyll_ohl03":
            assert len(seen["indices"]) >= 100, len(seen["indices"])


@needs_emu
@pytest.mark.parametrize("method", ["top-layer", "jerlov", "chlorophyll_ma94", "chlorophyll_ohl03", "spatial_frac_attlen"])
def test_updswa_on_the_host_emulation(emu_lib, method):
    if method.startswith("chlorophyll"):
        emu_lib.check_updswa_not_vacuous("chan_s_tke", method)
    else:
        emu_lib.check_updswa("chan_s_tke", method)


@needs_emu
@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke", "chan_b"])
def test_updswa_closed_box_arctic_patch_and_long_rows_on_the_host_emulation(emu_lib, cfg):
    seen = emu_lib.check_updswa_not_vacuous(cfg, "chlorophyll_ohl03")
    if cfg == "chan_b":
        assert len(seen["indices"]) >= 100
    emu_lib.check_updswa_not_vacuous(cfg, "chlorophyll_ma94")


@needs_emu
def test_updswa_warped_grid_and_hybrid_coordinate_on_the_host_emulation(emu_lib):
    emu_lib.check_updswa_not_vacuous("chan_s_tke", "chlorophyll_ohl03", grid="warped_eq")
    emu_lib.check_updswa_not_vacuous("chan_s", "chlorophyll_ma94", hybrid=True)


@needs_emu
def test_swabs_refusals_on_the_host_emulation(emu_lib):
    emu_lib.check_swabs_refusals()


@needs_emu
@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke", "chan_b"])
def test_fwbbal_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_fwbbal(cfg)


@needs_emu
def test_fwbbal_warped_grid_and_hybrid_coordinate_on_the_host_emulation(emu_lib):
    emu_lib.check_fwbbal("chan_s_tke", grid="warped_eq")
    emu_lib.check_fwbbal("chan_s", hybrid=True)


@needs_emu
@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_fwbbal_tiles_on_the_host_emulation(emu_lib, npx, npy):
    emu_lib.check_fwbbal_tiles(npx, npy)


@needs_emu
def test_chkvar_on_the_host_emulation(emu_lib):
    emu_lib.check_chkvar("chan_s_tke")
    assert emu_lib.check_chkvar("box_s") > 0
    emu_lib.check_chkvar("chan_s", hybrid=True)
    emu_lib.check_chkvar_tile()


@needs_emu
@pytest.mark.parametrize("config", ["cesm", "cesm_hybrid"])
def test_one_call_of_n_steps_equals_n_calls_on_the_host_emulation(emu_lib, config):
    emu_lib.check_interval(config, calls=(1, 2, 3))      # (N = 1..5 on the device; here the day's, month's and year's end of the fourth step)


@needs_emu
def test_refusals_and_names_on_the_host_emulation(emu_lib):
    emu_lib.check_refusals()


@needs_emu
@pytest.mark.parametrize("hybrid", [False, True])
def test_step_equals_the_stages_of_the_steppers_tuple_on_the_host_emulation(emu_lib, hybrid):
    emu_lib.check_staged(hybrid)
