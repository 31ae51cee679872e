"""The host-emulation suites on the curvilinear test grids (blom_amd.cases.warped_grid: every metric array its own function of i and
j, f varying and -- warped_eq -- changing sign).  On the uniform f-plane a kernel that reads the wrong metric array, a neighbour one
point off or f at the wrong corner, a rank given the wrong window of the grid or a fold that mirrors a metric the wrong way leaves the
bits of the correct code; here it does not.  The helpers and test functions of the other files run unchanged inside
`with on_grid(...)` (tests/curvilinear.py)."""
import os

import pytest

from curvilinear import on_grid

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
EXE = os.path.join(HERE, "hostemu", "blom_dyncore_hostemu")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    old = g.LIB_PATH
    g.LIB_PATH = EMU
    yield
    g.LIB_PATH = old


@pytest.mark.parametrize("cfg,ntr,grid", [("chan_s", None, "warped"), ("box_s", None, "warped"), ("tri_s", None, "warped"), ("chan_s_tke", 11, "warped"),
                                          ("tri_s_tke", 6, "warped"), ("chan_s", None, "warped_eq"), ("tri_s", None, "warped_eq")])
def test_current_kernels_equal_the_c_restatement(emu_lib, cfg, ntr, grid):
    from test_hostemu_kernels import test_current_kernels_equal_the_c_restatement as check
    with on_grid(grid):
        check(None, cfg, ntr)


@pytest.mark.parametrize("cfg,nsteps,grid", [("chan_s", 4, "warped_eq"), ("per_s", 3, "warped"), ("chan_b", 3, "warped")])
def test_barotp_forms_agree(emu_lib, cfg, nsteps, grid):
    """the pair kernel and k_bt_steps4 (rim points identified with their home points: the grid's halos must be exact copies of the
    interior for that) against one kernel per equation"""
    import test_hostemu_kernels as t
    with on_grid(grid):
        t.test_pair_kernel_equals_one_kernel_per_equation(None, cfg, nsteps)
        t.test_four_substeps_per_tile_launch_equal_one_kernel_per_equation(None, cfg, nsteps)


@pytest.mark.parametrize("cfg,isizes,jsizes,kw", [
    ("chan_s", (10, 10), (12, 12), dict()),                                   # 2 x 2
    ("tri_s", (6, 6, 6, 6), (11, 9), dict()),                                 # unequal tiles under the arctic fold
    ("tri_s", (12, 12), (11, 9), dict(cppm=True)),                            # the coefficient tables come from scpx and scpy
    ("chan_s_tke", (10, 10), (13, 11), dict(bt_global=True, full=True)),      # the full physics step, ocean area from scp2
], ids=["2x2", "unequal", "cppm", "full_physics"])
def test_rccl_ranks_match_single_tile(emu_lib, cfg, isizes, jsizes, kw):
    from test_hostemu_multirank import _run_case
    with on_grid("warped"):
        _run_case(cfg, isizes, jsizes, **kw)


def test_ragged_rccl_ranks_match_single_tile(emu_lib):
    """every rank's window of the metric arrays taken by the table of a land-eliminated layout: the row with an interior gap that does
    not wrap"""
    from test_hostemu_ragged import _check_case
    with on_grid("warped"):
        _check_case("chan_3x2_gap_row_does_not_wrap")


@pytest.mark.skipif(not os.path.exists(EXE), reason="tests/hostemu/blom_dyncore_hostemu not built")
def test_fortran_host_ranks_match_single_tile(emu_lib, tmp_path):
    """the state file holds the warped grid: every process of the Fortran host takes its own window of the metric arrays"""
    from test_fortran_spmd_host import run_tiled
    with on_grid("warped"):
        run_tiled(tmp_path, "chan_s", (10, 10), (12, 12))
