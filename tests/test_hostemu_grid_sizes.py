"""The device kernels on the CPU (tests/test_hostemu_kernels.py) at grid sizes no family of blom_amd.cases has: the kernels pick
tile shapes, ragged last tiles and k chunks by idm, jdm, kdm, and the families' sizes leave some of them unreached -- a last
32 x 8 tile 1 or 31 wide, 1 or 7 high, k = 3, 7, 9, 16, 17 against chunks of 8, barotp's blocked form on 26 x 15 tiles.  The
free run of the emulated kernels against the C restatement (size-generic C, pinned on the compiled reference at the built sizes by
tests/test_oracle_vs_reference.py), ==.  tests/test_gpu_grid_sizes.py makes these comparisons, and more, on the device; the
emulation runs neither the persistent forms nor real wavefronts."""
import os

import numpy as np
import pytest

from blom_amd.cases import make_case
from blom_amd import hostinit
from blom_amd.stepper import dyncore_step
from test_hostemu_kernels import EMU, emu_lib, _run          # noqa: F401  (emu_lib is a fixture)

pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

FIELDS = ("dp", "temp", "saln", "u", "v", "pb", "ub", "vb", "uflx", "vflx", "trc")


def c_restatement_run(case, nsteps):
    from oracle.coracle import COracle
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    orc = COracle(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))
    hostinit.init_state(orc, case)
    ns = 0
    for _ in range(nsteps):
        ns = dyncore_step(orc, ns, case.params["baclin"])
    return orc


def assert_interior_equal(case, orc, new):
    J, I = slice(4, 4 + case.jdm), slice(4, 4 + case.idm)
    for nm in FIELDS:
        a, b = orc.get(nm)[..., J, I], new[nm][..., J, I]
        assert np.array_equal(a, b, equal_nan=True), (case.name, nm)
    assert np.isfinite(new["u"][..., J, I]).all() and np.abs(new["u"]).max() > 0.0


def shape_with(cfg, **opts):
    """(barotp_shape, barotp_block_mode) of a context of this case with these options"""
    from blom_amd.gpu import BlomGpu
    case = make_case(cfg)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))
    try:
        for k, v in opts.items():
            gpu.set(k, v)
        return int(gpu.get_real("barotp_shape")), int(gpu.get_real("barotp_block_mode"))
    finally:
        gpu.close()


# what each size reaches: tests/test_gpu_grid_sizes.py, DESIGN.md 4
@pytest.mark.parametrize("cfg", ["chan_s@5x5x3", "chan_s@33x17x3", "chan_s@63x23x7", "box_s@35x39x16", "tri_s@58x31x17_tke",
                                 "per_s@33x33x9"])
def test_current_kernels_equal_the_c_restatement_at_this_size(emu_lib, cfg):
    nsteps = 3
    case, new = _run(cfg, nsteps)
    assert case.name == cfg
    assert_interior_equal(case, c_restatement_run(case, nsteps), new)


@pytest.mark.parametrize("cfg", ["chan_s@20x37x3", "chan_s@58x53x3", "chan_s@20x261x3_tke"])
def test_blocked_barotp_on_15_row_tiles_equals_the_c_restatement(emu_lib, cfg):
    """k_bt_steps4<26,15>, the default barotp kernel of a non-arctic domain whose jj leaves a 26 x 16 tiling a last row lower than
    the blocked form's rim: 1 x 3 tiles with a last row of 7; 3 x 4 tiles, the last column exactly as wide as the rim across the
    periodic seam; 1 x 18 tiles.  With one launch per four substeps, the form the emulation can run."""
    nsteps = 3
    assert shape_with(cfg, barotp_block=2) == (2615, 2)
    case, new = _run(cfg, nsteps, barotp_block=2)
    assert_interior_equal(case, c_restatement_run(case, nsteps), new)


def test_more_density_classes_than_the_kernel_holds_are_refused(emu_lib):
    import test_gpu_grid_sizes as t
    t.check_class_cap()
