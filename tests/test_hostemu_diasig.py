"""The density-class mass fluxes on the CPU: the checks of tests/test_gpu_diasig.py (whose functions run here unchanged) on the device
library compiled for the host (tests/hostemu) -- k_diasig inside blomgpu_step against :1398-1453 | :1471-1526 restated in numpy, sigint
and its halo, the coverage of the search, the interface and its refusals, finalisation, reset, the untouched accumulators and model
state, tiles, the graph option, the hybrid coordinate.  Byte for byte, where there is no GPU.  The restatement's own sanity check needs
no library at all."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

_EMU_RUNS, _EMU_TABLES = {}, {}


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_diasig as t
    old, oldh, runs, tabs = g.LIB_PATH, h._LIB, t._RUNS, t._TABLES
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._RUNS, t._TABLES = _EMU_RUNS, _EMU_TABLES       # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._RUNS, t._TABLES = runs, tabs


def test_restatement_conserves_the_flux_and_its_weights_sum_to_one():
    import test_gpu_diasig as t
    t.check_restatement_conserves()


@needs_emu
@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke"])
def test_step_accumulates_what_the_reference_loops_would_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_step_accumulates(cfg)
    emu_lib.check_coverage(cfg)


@needs_emu
def test_interface_and_refusals_on_the_host_emulation(emu_lib):
    emu_lib.check_interface()


@needs_emu
def test_independence_finalize_reset_on_the_host_emulation(emu_lib):
    emu_lib.check_independence_finalize_reset()


@needs_emu
def test_tiles_on_the_host_emulation(emu_lib, monkeypatch):
    emu_lib.check_tiles(monkeypatch)


@needs_emu
def test_graph_option_on_the_host_emulation(emu_lib):
    """(the emulation cannot capture: the step falls back to plain launches, the count and the bytes must hold all the same)"""
    emu_lib.check_graph_replay(expect_replays=False)


@needs_emu
def test_hybrid_coordinate_on_the_host_emulation(emu_lib):
    emu_lib.check_hybrid()
