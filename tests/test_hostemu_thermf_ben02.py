"""The surface forcing of the forced ocean-ice experiment on the CPU: the checks of tests/test_gpu_thermf_ben02.py (whose functions run
here unchanged) on the device library compiled for the host (tests/hostemu) -- k_sfcstr_ben02, k_thermf_ben02_flux, k_thermf_ben02_corr
and the batched sums against the numpy restatement of ben02/mod_sfcstr_ben02.F90 and ben02/mod_thermf_ben02.F90, the branch counts that
keep the checks from passing on untaken branches, the step against the stepper's tuples, tiles, the accumulators and the interface.
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
    import test_gpu_thermf_ben02 as t
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = EMU
    h._LIB = EMU
    yield t
    g.LIB_PATH = old
    h._LIB = oldh


@needs_emu
@pytest.mark.parametrize("optname", ["clim", "off", "ap", "di", "srxbal"])
def test_stages_equal_the_restated_routines_on_the_host_emulation(emu_lib, optname):
    emu_lib.check_not_vacuous("chan_s_tke", optname)


@needs_emu
@pytest.mark.parametrize("optname", ["clim", "di"])
def test_hybrid_coordinate_on_the_host_emulation(emu_lib, optname):
    emu_lib.check_not_vacuous("chan_s", optname, hybrid=True)


@needs_emu
@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke", "chan_b"])
def test_closed_box_arctic_seam_and_long_rows_on_the_host_emulation(emu_lib, cfg):
    emu_lib.check_stage(cfg, "srxbal")


@needs_emu
def test_generic_length_scale_on_the_host_emulation(emu_lib):
    emu_lib.check_stage("chan_s_tk2", "clim")


@needs_emu
def test_warped_grid_on_the_host_emulation(emu_lib):
    emu_lib.check_not_vacuous("chan_s_tke", "clim", grid="warped_eq")


@needs_emu
def test_24_tracers_on_the_host_emulation(emu_lib):
    emu_lib.check_stage("chan_s", "clim", ntr=24, presteps=2)


@needs_emu
@pytest.mark.parametrize("hybrid", [False, True])
def test_step_equals_the_stages_on_the_host_emulation(emu_lib, hybrid):
    emu_lib.check_step(hybrid)


@needs_emu
def test_ntda_and_the_accumulated_planes_on_the_host_emulation(emu_lib):
    emu_lib.check_ntda()


@needs_emu
@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_on_the_host_emulation(emu_lib, npx, npy):
    emu_lib.check_tiles(npx, npy)


@needs_emu
def test_interface_on_the_host_emulation(emu_lib):
    emu_lib.check_interface()
