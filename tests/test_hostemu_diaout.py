"""diamer, diasec and the global sums on the CPU: the checks of tests/test_gpu_diaout.py (whose functions run here unchanged) on the
device library compiled for the host (tests/hostemu) -- k_diaout_sections, k_diaout_columns and the batched xcsum against
phy/mod_dia.F90:4004-4629, :3814-4001 and :2427-2588 restated in numpy, the passes and chunks of the section kernel, both level tables
of the equatorial section, the fill below the bottom, the names that rest under isopyc_bulkml, the interface and its refusals, a tile
of a group.  Byte for byte, where there is no GPU."""
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
    import test_gpu_diaout as t
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
def test_reduce_gives_what_the_restated_routines_give_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_reduce(cfg)


@needs_emu
def test_reduce_on_the_warped_grid_on_the_host_emulation(emu_lib):
    emu_lib.check_reduce("chan_s_tke", grid="warped")


@needs_emu
def test_depth_space_holds_fill_below_the_bottom_on_the_host_emulation(emu_lib):
    emu_lib.check_fill_below_the_bottom()


@needs_emu
def test_passes_and_chunks_on_the_host_emulation(emu_lib):
    emu_lib.check_chunks_and_passes()


@needs_emu
def test_equatorial_section_on_both_level_tables_on_the_host_emulation(emu_lib):
    emu_lib.check_equatorial_tables()


@needs_emu
def test_resting_names_move_under_the_hybrid_coordinate_on_the_host_emulation(emu_lib):
    emu_lib.check_resting_names_under_the_hybrid_coordinate()


@needs_emu
def test_interface_and_refusals_on_the_host_emulation(emu_lib):
    emu_lib.check_interface()


@needs_emu
def test_a_tile_of_a_group_refuses_on_the_host_emulation(emu_lib):
    emu_lib.check_tile_refuses()
