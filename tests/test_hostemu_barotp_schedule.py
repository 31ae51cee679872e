"""tests/test_gpu_barotp_schedule.py's checks on the host emulation (tests/hostemu), which has no persistent form: one kernel per
equation, one launch per substep pair (32 x 16 tiles: the emulation reports no CUs) and the blocked kernel with one launch per four
substeps.  All seven phase lengths of that file's table on the one-tile cases, the shortest phase and the longest even one on the
cases of several tiles."""
import os

import pytest

import test_gpu_barotp_schedule as sched
from test_hostemu_kernels import EMU, emu_lib          # noqa: F401  (emu_lib is a fixture)

pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")

PAIRS, BLOCKED = ({}, 0), (dict(barotp_block=2), 2)
CASES = [(cfg, lstep, forms) for cfg, forms in (("chan_s", [PAIRS, BLOCKED]), ("tri_s", [PAIRS])) for lstep in (2, 4, 6, 8, 46, 48, 52)]
CASES += [(cfg, lstep, forms) for cfg, forms in (("chan_b", [PAIRS, BLOCKED]), ("tri_m", [PAIRS])) for lstep in (2, 52)]


@pytest.mark.parametrize("cfg,lstep,forms", CASES, ids=["%s-%d" % (c, l) for c, l, _ in CASES])
def test_every_form_equals_one_kernel_per_equation_at_this_lstep(emu_lib, cfg, lstep, forms):
    sched.check_forms_at_this_lstep(cfg, lstep, forms)


ALL_ON = dict(barotp_fused=1, barotp_persist=1, barotp_block=1)
EQUATIONS = (dict(ALL_ON, barotp_fused=0, barotp_persist=0), (3216, 0))
PLAIN_SEGMENTS = [EQUATIONS, (dict(ALL_ON), (3216, 0)), (dict(ALL_ON, barotp_block=2), (2616, 2)), (dict(ALL_ON), (3216, 0)), EQUATIONS]
ARCTIC_SEGMENTS = [EQUATIONS, (dict(ALL_ON), (3216, 0)), EQUATIONS, (dict(ALL_ON), (3216, 0))]


@pytest.mark.parametrize("cfg,segments", [("chan_s", PLAIN_SEGMENTS), ("chan_b", PLAIN_SEGMENTS), ("tri_s", ARCTIC_SEGMENTS)],
                         ids=["chan_s", "chan_b", "tri_s"])
def test_one_context_runs_one_form_after_another(emu_lib, cfg, segments):
    sched.check_forms_switched_in_one_context(cfg, segments)
