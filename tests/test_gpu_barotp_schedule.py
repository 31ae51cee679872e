"""barotp's host drivers at phase lengths no family of blom_amd.cases has.  Every family runs lstep = 50 or 30, so every barotropic
phase has an odd number of substeps (25 or 15), and the code that walks a phase -- an odd substep together with the even one behind
it unless the phase ends in between, the lone substeps around the arctic form's persistent launch, the blocked form's four substeps
per hand-off with a remainder -- never meets an even phase or a phase of one substep.  Here lstep is this file's own choice:

  lstep  substeps per phase  what it reaches
      2                   1  single-substep phases; zero pairs in the arctic bracket
      4                   2  even phase, no lone substeps
      6                   3  odd phase; total 15 = 3 blocks of 4, plus 3
      8                   4  exactly one block of four per phase
     46                  23  odd phase; remainder 3
     48                  24  no lone substeps; total 120 = 30 blocks of 4
     52                  26  even phase; remainder 2

baclin, batrop, lstep, dlt (and the first step's delt1 = baclin) are overridden together, as cases.default_params derives them; dlt stays
the families' 18 s, so the runs are stable.  The bar is ==: every form against one kernel per equation over every array, that form
against the C restatement on the interior.  tests/test_hostemu_barotp_schedule.py runs the check_* functions on the host emulation, with
the forms that has and all seven values; the device runs the forms of DESIGN.md 3.3 at four of them."""
import pytest

from blom_amd.cases import make_case
from test_gpu_grid_sizes import _device_run, _assert_equals_the_c_restatement, _assert_same_bytes

pytestmark = pytest.mark.gpu

DLT = 18.0
NSTEPS = 3
EQUATIONS = dict(barotp_fused=0, barotp_persist=0)


def case_with_lstep(cfg, lstep):
    baclin = DLT * lstep
    case = make_case(cfg, baclin=baclin, batrop=DLT, lstep=lstep, dlt=DLT, delt1=baclin)
    assert case.params["lstep"] == lstep and case.params["dlt"] == case.params["baclin"] / lstep
    return case


def check_forms_at_this_lstep(cfg, lstep, variants):
    """variants: (options, barotp_block_mode the context must report in front of the run, or None).  Three steps in every form; the
    equation form's run, made once, is what all of them are compared with, and is itself compared with the C restatement."""
    case = case_with_lstep(cfg, lstep)
    _, eq = _device_run(case, [(EQUATIONS, NSTEPS)])
    _assert_equals_the_c_restatement(case, NSTEPS, eq)          # (also: ub finite and non-zero)
    for opts, mode in variants:
        shapes, got = _device_run(case, [(opts, NSTEPS)])
        if mode is not None:
            assert shapes[0][1] == mode, (cfg, lstep, opts, shapes)
        _assert_same_bytes(case, eq, got, (lstep, opts))


def check_forms_switched_in_one_context(cfg, segments):
    """segments: (options, (barotp_shape, barotp_block_mode) expected in front of the segment).  One context runs two steps per segment;
    the forms share the completion counts, their epochs and the buffer-set bookkeeping of the context.  Against the same number of steps
    with one kernel per equation throughout."""
    case = make_case(cfg)
    shapes, got = _device_run(case, [(opts, 2) for opts, _ in segments])
    assert shapes == [sh for _, sh in segments], (cfg, shapes)
    _, eq = _device_run(case, [(EQUATIONS, 2 * len(segments))])
    _assert_same_bytes(case, eq, got, "forms switched")


# ---- on the device -------------------------------------------------------------------------------------------------------------------
LSTEPS = (2, 6, 48, 52)
# chan_s: one tile; chan_b: 4 x 3 tiles of 26 x 16, ragged, periodic seam
PLAIN = [({}, 1), (dict(barotp_block=0), 0), (dict(barotp_block=2), 2), (dict(barotp_persist=0), 0)]
# tri_m: 3 x 3 tiles with the arctic patch: the persistent launch bracketed by lone substeps, and one launch per pair
ARCTIC = [({}, 0), (dict(barotp_arctic_persist=0), 0)]


@pytest.mark.parametrize("lstep", LSTEPS)
@pytest.mark.parametrize("cfg,variants", [("chan_s", PLAIN), ("chan_b", PLAIN), ("tri_m", ARCTIC)], ids=["chan_s", "chan_b", "tri_m"])
def test_every_form_equals_one_kernel_per_equation_at_this_lstep(cfg, variants, lstep):
    check_forms_at_this_lstep(cfg, lstep, variants)


ALL_ON = dict(barotp_fused=1, barotp_persist=1, barotp_block=1, barotp_arctic_persist=1)
# the shapes are those of the selection rule on 256 CUs (tests/test_gpu_grid_sizes.py): 16 x 8 for the pairs of these small domains
PLAIN_SEGMENTS = [(dict(ALL_ON, barotp_fused=0, barotp_persist=0), (1608, 0)),      # one kernel per equation
                  (dict(ALL_ON, barotp_persist=0), (1608, 0)),                      # one launch per pair
                  (dict(ALL_ON), (2616, 1)),                                        # blocked, persistent
                  (dict(ALL_ON, barotp_block=0), (2616, 0)),                        # one persistent launch per phase
                  (dict(ALL_ON, barotp_persist=0), (1608, 0)),
                  (dict(ALL_ON, barotp_fused=0, barotp_persist=0), (1608, 0))]
ARCTIC_SEGMENTS = [(dict(ALL_ON, barotp_fused=0, barotp_persist=0), (1608, 0)),
                   (dict(ALL_ON, barotp_arctic_persist=0), (1608, 0)),              # one launch per pair
                   (dict(ALL_ON), (2616, 0)),                                       # the arctic form of the persistent phase
                   (dict(ALL_ON, barotp_persist=0), (1608, 0)),
                   (dict(ALL_ON, barotp_fused=0, barotp_persist=0), (1608, 0))]


@pytest.mark.parametrize("cfg,segments", [("chan_s", PLAIN_SEGMENTS), ("chan_b", PLAIN_SEGMENTS), ("tri_m", ARCTIC_SEGMENTS)],
                         ids=["chan_s", "chan_b", "tri_m"])
def test_one_context_runs_one_form_after_another(cfg, segments):
    check_forms_switched_in_one_context(cfg, segments)
