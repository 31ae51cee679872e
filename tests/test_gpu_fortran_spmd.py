"""`program blom_dyncore` with a tile table on the GPU (tests/test_fortran_spmd_host.py runs the same on the host
emulation with up to 8 processes).  One rank with a 1x1 patch.input takes the whole tiled path on the device -- the tile
context, the global context of the replicated barotropic solve, the RCCL communicator (of one rank: the checksum's
messages go to the rank itself) and blomgpu_rccl_crc -- and must print the checksums of the Python-driven single-context
run.  Two ranks need two GPUs (RCCL refuses two ranks on one device): skipped on a machine with one."""
import os

import pytest

from test_fortran_spmd_host import run_tiled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "blom_amd", "lib", "blom_dyncore")


@pytest.fixture()
def exe():
    if not os.path.exists(EXE):
        pytest.skip("Fortran driver not built")
    return EXE


@pytest.mark.parametrize("cfg,full", [("chan_s", False), ("chan_s_tke", True)])
def test_one_rank_with_a_1x1_table_matches_the_single_context(tmp_path, exe, cfg, full):
    from blom_amd.cases import make_case
    case = make_case(cfg)
    run_tiled(tmp_path, cfg, (case.idm,), (case.jdm,), nsteps=4, full=full, timeout=300, exe=exe, emulated=False)


def test_two_ranks_on_two_gpus_match_the_single_context(tmp_path, exe):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("two ranks need two GPUs (RCCL refuses two ranks on one device)")
    run_tiled(tmp_path, "chan_s", (10, 10), (24,), nsteps=4, timeout=300, exe=exe, local_rank=lambda r: r, emulated=False)
