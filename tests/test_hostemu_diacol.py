"""The column-derived diagnostics on the CPU: the checks of tests/test_gpu_diacol.py (whose functions run here unchanged) on the device
library compiled for the host (tests/hostemu) -- k_diacol, k_diapv and k_cmn_mldl82<DIAG> inside blomgpu_step against
phy/mod_dia.F90:1203-1366 and phy/mod_cmnfld_routines.F90:943-984 restated in numpy, the conditions that keep the checks from passing
on zeros, the prepared columns that take every outcome of the isotherm walk, the interface and its refusals, finalisation, reset, the
untouched accumulators and model state, tiles, the graph option, the hybrid coordinate, the warped grid, and absvor / dpvor against
the compiled reference.  Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

_EMU_RUNS = {}


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_diacol as t
    old, oldh, runs = g.LIB_PATH, h._LIB, t._RUNS
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._RUNS = _EMU_RUNS                               # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._RUNS = runs


@needs_emu
@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke"])
def test_step_accumulates_what_the_reference_loops_would_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_step_accumulates(cfg)
    emu_lib.check_not_vacuous(cfg)


@needs_emu
def test_warped_grid_on_the_host_emulation(emu_lib):
    emu_lib.check_step_accumulates("chan_s_tke", "warped_eq")


@needs_emu
def test_prepared_columns_on_the_host_emulation(emu_lib):
    emu_lib.check_prepared_columns()


@needs_emu
def test_interface_on_the_host_emulation(emu_lib):
    emu_lib.check_interface()


@needs_emu
def test_independence_finalize_reset_on_the_host_emulation(emu_lib):
    emu_lib.check_independence_finalize_reset()


@needs_emu
@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_on_the_host_emulation(emu_lib, monkeypatch, npx, npy):
    emu_lib.check_tiles(monkeypatch, npx, npy)


@needs_emu
def test_graph_option_on_the_host_emulation(emu_lib):
    """(the emulation cannot capture: the step falls back to plain launches, the count and the bytes must hold all the same)"""
    emu_lib.check_graph_replay(expect_replays=False)


@needs_emu
def test_hybrid_coordinate_on_the_host_emulation(emu_lib):
    emu_lib.check_hybrid()


@needs_emu
@pytest.mark.parametrize("cfg,grid", [("chan_s", None), ("box_s", None), ("tri_s", None), ("chan_s", "warped_eq")])
def test_absvor_and_dpvor_equal_the_compiled_reference_on_the_host_emulation(emu_lib, cfg, grid):
    emu_lib.check_pin(cfg, grid)
