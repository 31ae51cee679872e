"""diaacc's kernels on the CPU: the checks of tests/test_gpu_diaacc.py (whose functions run here unchanged) on the device library
compiled for the host (tests/hostemu) -- the accumulation inside blomgpu_step against the reference's loops restated in numpy,
finalisation, reset, selection semantics, the untouched model state, tiles.  Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_diaacc as t
    old, oldh, runs = g.LIB_PATH, h._LIB, t._RUNS
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._RUNS = _EMU_RUNS                 # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._RUNS = runs


_EMU_RUNS = {}


@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke"])
def test_step_accumulates_what_the_reference_loops_would_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_step_accumulates(cfg)
    emu_lib.check_not_zeros(cfg)
    emu_lib.check_finalize(cfg)


def test_dynamical_core_alone_on_the_host_emulation(emu_lib):
    emu_lib.check_dyncore_only()


def test_reset_and_untouched_state_on_the_host_emulation(emu_lib):
    emu_lib.check_reset()
    emu_lib.check_no_trace()


def test_selection_semantics_on_the_host_emulation(emu_lib):
    emu_lib.check_selection_semantics()


def test_graph_option_on_the_host_emulation(emu_lib):
    """(the emulation cannot capture: the step falls back to plain launches, the count and the bytes must hold all the same)"""
    emu_lib.check_graph_replay(expect_replays=False)


def test_tiles_on_the_host_emulation(emu_lib):
    emu_lib.check_tiles()
