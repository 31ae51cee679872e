"""mod_budget inside blomgpu_step on the CPU: the checks of tests/test_gpu_budget.py (whose functions run here unchanged) on the device
library compiled for the host (tests/hostemu) -- k_budget_rows, k_budget_rows2d, k_budget_total, the plane path of the tile groups, the
records and the lines, == against the reference's sums.  The rehearsal where there is no GPU; the emulation says nothing about
wavefronts or the order of two streams."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_budget as t
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = EMU
    h._LIB = EMU
    yield t
    g.LIB_PATH = old
    h._LIB = oldh


@pytest.mark.parametrize("cfg", ["chan_s", "tri_s_tke", "chan_s_tk2"])
def test_records_and_lines_equal_the_reference_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_records(cfg)


@pytest.mark.parametrize("cfg", ["chan_s@583x9x3_tke", "tri_s@31x12x3"])
def test_row_shapes_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_records(cfg, which="c", nsteps=2)


@pytest.mark.parametrize("config", ["full", "hybrid"])
def test_placement_on_the_host_emulation(emu_lib, config):
    emu_lib.check_placement(config)


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_on_the_host_emulation(emu_lib, npx, npy):
    emu_lib.check_tiles(npx, npy)


def test_off_refusals_and_graphs_on_the_host_emulation(emu_lib):
    emu_lib.check_off_and_refusals()


def test_coupled_context_on_the_host_emulation(emu_lib):
    emu_lib.check_coupled()
