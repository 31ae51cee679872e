"""TEST INFRASTRUCTURE: runs the helpers and test functions of the other test files, unchanged, on a curvilinear grid.

Those helpers build their own case (make_case(cfg, ...)) and know nothing of grids.  Inside `with on_grid("warped")` make_case gives
them blom_amd.cases.warped_grid (blom_amd.cases.default_grid), and the two helpers that would start from a committed fixture
(tests/golden/chan_s_init.npz, box_s_init.npz: the uniform f-plane) get the same fields from make_case instead."""
import contextlib

from blom_amd import hostinit
from blom_amd.cases import default_grid, make_case
from parity import STATE_FIELDS, GRID_FIELDS, INT_FIELDS


def init_from_make_case(cfg):
    """(masks, fields) as parity.load_golden_init returns them, initialised by hostinit.init_state on the library blom_amd.gpu.LIB_PATH names"""
    from blom_amd.gpu import BlomGpu
    case = make_case(cfg)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    be = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(be, case)
    fields = {nm: be.get(nm) for nm in STATE_FIELDS + GRID_FIELDS + INT_FIELDS if be.has_field(nm)}
    be.close()
    return masks, fields


@contextlib.contextmanager
def on_grid(grid):
    import test_gpu_fortran_host
    import test_gpu_tiles
    users = (test_gpu_tiles, test_gpu_fortran_host)
    saved = [m.load_golden_init for m in users]
    with default_grid(grid):
        for m in users:
            m.load_golden_init = init_from_make_case
        try:
            yield
        finally:
            for m, f in zip(users, saved):
                m.load_golden_init = f
