"""The surface forcing of the coupled experiment on the CPU: the checks of tests/test_gpu_thermf_cesm.py (whose functions run here
unchanged) on the device library compiled for the host (tests/hostemu) -- k_getfrc_cesm, k_sfcstr_cesm, k_thermf_cesm_flux,
k_thermf_cesm_corr and the batched sums against the numpy restatement of cesm/mod_cesm.F90, cesm/mod_sfcstr_cesm.F90 and
cesm/mod_thermf_cesm.F90, the conditions that keep the checks from passing on untaken branches, the step against the stepper's tuples,
and the interface.  Byte for byte, where there is no GPU."""
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_thermf_cesm as t
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = EMU
    h._LIB = EMU
    yield t
    g.LIB_PATH = old
    h._LIB = oldh


@needs_emu
@pytest.mark.parametrize("optname", ["clim", "stream", "off", "ap", "di", "srxbal"])
def test_stages_equal_the_restated_routines_on_the_host_emulation(emu_lib, optname):
    emu_lib.check_not_vacuous("chan_s_tke", optname)


@needs_emu
@pytest.mark.parametrize("optname", ["clim", "stream", "di"])
def test_hybrid_coordinate_on_the_host_emulation(emu_lib, optname):
    emu_lib.check_not_vacuous("chan_s", optname, hybrid=True)


@needs_emu
@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke"])
def test_closed_box_and_arctic_seam_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_stage(cfg, "srxbal")


@needs_emu
def test_generic_length_scale_on_the_host_emulation(emu_lib):
    emu_lib.check_stage("chan_s_tk2", "clim")


@needs_emu
def test_warped_grid_on_the_host_emulation(emu_lib):
    emu_lib.check_stage("chan_s_tke", "clim", grid="warped_eq")


@needs_emu
def test_batched_sums_on_the_host_emulation(emu_lib):
    emu_lib.check_batch_second_round()
    emu_lib.check_stage("chan_s", "clim", ntr=24, presteps=2)


@needs_emu
@pytest.mark.parametrize("hybrid", [False, True])
def test_step_equals_the_stages_on_the_host_emulation(emu_lib, hybrid):
    emu_lib.check_step(hybrid)


@needs_emu
@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_on_the_host_emulation(emu_lib, npx, npy):
    emu_lib.check_tiles(npx, npy)


@needs_emu
def test_step_and_tiles_on_the_warped_grid_on_the_host_emulation(emu_lib):
    emu_lib.check_step_warped()
    emu_lib.check_tiles_warped()


@needs_emu
@pytest.mark.parametrize("cfg", ["chan_s", "box_s"])
def test_undeclared_context_against_the_golden_checksums_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_undeclared_golden(cfg)


@needs_emu
def test_named_entry_points_on_arrays_without_memory_on_the_host_emulation(emu_lib):
    emu_lib.check_unallocated_fields()


@needs_emu
def test_interface_on_the_host_emulation(emu_lib):
    emu_lib.check_interface()


@needs_emu
def test_device_equals_the_real_module_on_the_host_emulation(emu_lib):
    """tests/test_thermf_cesm_golden.py's device half: the reference's compiled thermf_cesm, nine option sets"""
    import test_thermf_cesm_golden as gold
    assert len(gold.FIXTURES) == 9
    for name in gold.FIXTURES:
        gold.check_device(name)
