"""The skipped heat and salt flux passes on the CPU: the checks of tests/test_gpu_lazy_flux_diag.py (whose functions run here
unchanged) on the device library compiled for the host (tests/hostemu) -- one call of N steps against N calls of one step, the
diaacc selections, the off-switch, csdiag, the graph option, tiles.  Byte for byte, where there is no GPU.  (The emulation cannot
capture a graph: with use_graph = 1 the step falls back to plain launches in its third step, and a call of four steps still may not
skip.)"""
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
    import test_gpu_lazy_flux_diag as t
    old, oldh, runs = g.LIB_PATH, h._LIB, t._RUNS
    g.LIB_PATH = EMU
    h._LIB = EMU
    t._RUNS = _EMU_RUNS                 # runs of the emulation are shared among these tests only
    yield t
    g.LIB_PATH = old
    h._LIB = oldh
    t._RUNS = runs


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", ["chan_s_tke", "tri_s_tke", "box_s"])
def test_one_call_of_n_steps_on_the_host_emulation(emu_lib, cfg, full, n):
    emu_lib.check_one_call(cfg, full, n)


@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", ["chan_s_tke", "tri_s_tke", "box_s"])
def test_selections_on_the_host_emulation(emu_lib, cfg, full):
    emu_lib.check_selection(cfg, full, emu_lib.FLUX_ROWS, 0)
    emu_lib.check_selection(cfg, full, emu_lib.OTHER_ROWS, 2)


@pytest.mark.parametrize("how", ["keep", "csdiag", "use_graph"])
@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", ["chan_s_tke", "tri_s_tke", "box_s"])
def test_what_keeps_every_step_whole_on_the_host_emulation(emu_lib, cfg, full, how):
    emu_lib.check_never_skips(cfg, full, how)


def test_tiles_on_the_host_emulation(emu_lib):
    emu_lib.check_tiles()
