"""The depth-level accumulators on the CPU: the checks of tests/test_gpu_dialvl.py (whose functions run here unchanged) on the device
library compiled for the host (tests/hostemu) -- k_dialvl inside blomgpu_step against diazlv / acclvl / msklvl restated in numpy, the
coverage of the walk, a bound equal to an interface, the level tables, refusals, finalisation, reset, the untouched layer
accumulators and model state, tiles.  Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

_EMU_RUNS = {}


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_dialvl as t
    old, oldh, runs = g.LIB_PATH, h._LIB, t._RUNS
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._RUNS = _EMU_RUNS                 # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._RUNS = runs


@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke"])
def test_step_accumulates_what_the_reference_loops_would_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_step_accumulates(cfg)
    emu_lib.check_coverage(cfg)
    emu_lib.check_finalize(cfg)


def test_a_bound_equal_to_an_interface_on_the_host_emulation(emu_lib):
    emu_lib.check_equality_case()


def test_set_levels_on_the_host_emulation(emu_lib):
    emu_lib.check_set_levels()


def test_refusals_on_the_host_emulation(emu_lib):
    emu_lib.check_refusals()


def test_reset_and_independence_on_the_host_emulation(emu_lib):
    emu_lib.check_reset_and_independence()


def test_graph_option_on_the_host_emulation(emu_lib):
    """(the emulation cannot capture: the step falls back to plain launches, the count and the bytes must hold all the same)"""
    emu_lib.check_graph_replay(expect_replays=False)


def test_tiles_on_the_host_emulation(emu_lib, monkeypatch):
    emu_lib.check_tiles(monkeypatch)
