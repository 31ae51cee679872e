"""templvl salnlvl uvellvl vvellvl under the hybrid coordinates on the CPU: the checks of tests/test_gpu_dia_hybrid.py (whose functions run
here unchanged) on the device library compiled for the host (tests/hostemu) -- the reference's window against the restated glue around the
reference's own mod_hor3map, the coverage of the remap, the alarm's gating, refusals, tiles, neutral diffusion and many tracers, the graph
option (which falls back to plain launches here), reset and independence.  Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

_EMU_STATES, _EMU_RUNS = {}, {}


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_dia_hybrid as t
    old, oldh, states, runs = g.LIB_PATH, h._LIB, t._STATES, t._RUNS
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._STATES, t._RUNS = _EMU_STATES, _EMU_RUNS        # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._STATES, t._RUNS = states, runs


def test_window_on_the_host_emulation(emu_lib):
    for key in emu_lib.CASES + [emu_lib.FUK95]:
        emu_lib.check_window(key)


def test_short_table_on_the_host_emulation(emu_lib):
    for key in emu_lib.CASES:
        emu_lib.check_short_table(key)


def test_coverage_on_the_host_emulation(emu_lib):
    emu_lib.check_coverage()


def test_gating_on_the_host_emulation(emu_lib):
    emu_lib.check_gating()


def test_refusals_on_the_host_emulation(emu_lib):
    emu_lib.check_refusals()


@pytest.mark.parametrize("cfg,npx,npy,vcoord,method", [("chan_s", 2, 1, "cntiso_hybrid", "nudge"), ("chan_s", 1, 2, "plevel", "direct"),
                                                       ("tri_s", 2, 2, "cntiso_hybrid", "nudge")])
def test_tiles_on_the_host_emulation(emu_lib, cfg, npx, npy, vcoord, method):
    emu_lib.check_tiles(cfg, npx, npy, vcoord, method)


def test_neutral_diffusion_and_many_tracers_on_the_host_emulation(emu_lib):
    emu_lib.check_window(emu_lib.NEUTRAL)
    emu_lib.check_window(emu_lib.MANY)


def test_graph_option_on_the_host_emulation(emu_lib):
    """(the emulation cannot capture: the steps fall back to plain launches, the bytes must hold all the same)"""
    emu_lib.check_graph_option(expect_replays=False)


def test_reset_and_two_contexts_on_the_host_emulation(emu_lib):
    emu_lib.check_reset_and_independence()
