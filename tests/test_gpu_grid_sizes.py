"""The kernels at grid sizes of this file's own choosing.  Every other parity test takes idm, jdm, kdm from the table of families
in blom_amd.cases, and the kernels choose their code by exactly those numbers: barotp its tile shape and form from ii, jj, the
topology and the CU count; remap, pbcor, diffus, tmsmt2 cut the plane into 32 x 8 tiles; the column kernels walk k in chunks of 8,
6 or 4.  The sizes here reach what the families leave out (the tables below say which size reaches what).

The reference throughout is the C restatement (oracle.coracle.COracle) at the same sizes: size-generic C, pinned on the compiled
reference at the built sizes by tests/test_oracle_vs_reference.py.  The bar is ==.  Every test of a barotp shape first asserts the
shape and form the context is about to run (blomgpu_get_real "barotp_shape", "barotp_block_mode"; the expected values are those of
the selection rule on 256 CUs): on another device, or after a change of the rule, it fails saying that it no longer reaches its
kernel instead of passing on another one.  Also here, on the other GPU test files' own checks: the 15-row barotp tiles forced through
barotp_tile, and k_diasig's instantiation for more than 56 layers.  tests/test_hostemu_grid_sizes.py runs a part of this on the CPU."""
import numpy as np
import pytest

from blom_amd.cases import make_case
from blom_amd import hostinit
from blom_amd.stepper import dyncore_step
from parity import copy_state, diff_report, fmt_report, STATE_FIELDS, INT_FIELDS
import test_gpu_diasig as diasig
import test_gpu_variants as variants
from test_gpu_diaacc import dyncore_context
from test_gpu_stage_parity import GPU_STAGES, SCRATCH, TOL

pytestmark = pytest.mark.gpu

FREE_FIELDS = ("dp", "temp", "saln", "u", "v", "pb", "ub", "vb", "uflx", "vflx", "trc")
SKIP = {"util1", "util2", "util3", "util4"}          # scratch planes shared between stages


def _masks(case):
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    return nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq)


def _c_restatement(case):
    from oracle.coracle import COracle

    class Tracked(COracle):
        """remembers the time step dyncore_step and init_state hand it: the device stage needs the same one"""
        delt1 = None

        def set(self, name, v):
            if name == "delt1":
                self.delt1 = v
            return super().set(name, v)

    nreg, masks = _masks(case)
    orc = Tracked(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(orc, case)
    return orc


# ---- a. stage by stage ------------------------------------------------------------------------------------------------------------
def run_stages_against(ref, case, nsteps, stages, delt1):
    """The loop of tests/test_gpu_stage_parity.py::_run (same field list, same tolerances table, same report) on a backend handed in, so
    that it can be one the compiled reference has no build for: `ref`, initialised, is stepped through the stage sequence; in front of every
    stage of `stages` its whole state goes to a device context, the stage runs there, and behind it every array both sides hold is
    compared, halos included.  delt1(): the time step the backend is about to use.  A failure names step, stage, field and first cell."""
    from blom_amd.gpu import BlomGpu
    from blom_amd.stepper import DYNCORE_STAGES
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, ref.ntr, ref.nreg, ref.masks)
    for nm, v in case.params.items():
        if not nm.endswith("0"):
            gpu.set(nm, v)
    failures = []
    pending = {}
    nstep = [0]

    def check():
        if "st" in pending:
            st = pending.pop("st")
            rtol, atol = TOL.get(st, (0.0, 0.0))
            fields = [f for f in STATE_FIELDS + INT_FIELDS if f not in SCRATCH]
            bad = diff_report(ref, gpu, fields=fields, rtol=rtol, atol=atol)
            if bad:
                failures.append(f"step {nstep[0] + 1} stage {st}:\n" + fmt_report(bad))

    def hook(st, six):
        check()
        if st not in stages:
            return
        copy_state(ref, gpu)
        gpu.set("nstep", nstep[0] + 1)
        gpu.set("delt1", delt1())
        gpu.stage(st, *six)
        pending["st"] = st

    for _ in range(nsteps):
        new = dyncore_step(ref, nstep[0], case.params["baclin"], hook=hook, stages=DYNCORE_STAGES)
        check()
        nstep[0] = new
    gpu.close()
    assert not failures, "\n".join(failures[:40])


# family, sizes, ntr: what the size reaches
STAGE_SIZES = [
    ("chan_s@5x5x3", None),            # a domain barely wider than the halo; the smallest kdm
    ("chan_s@33x17x3", None),          # last 32 x 8 tile 1 wide and 1 high; the periodic seam beside a 1-wide tile
    ("chan_s@63x23x7", None),          # last tile 31 wide, 7 high; k = one chunk less one
    ("chan_s@64x16x8", None),          # exact tile multiples, the seam on a tile edge; k = exactly one chunk
    ("chan_s@97x9x3", None),           # four tile columns over two tile rows, the second row 1 high
    ("box_s@35x39x16", None),          # closed walls, island; two exact k chunks
    ("box_s@35x39x24_tke", 24),        # three exact chunks; six tracer batches of the tile kernels
    ("chan_s@27x31x24_tke", 11),       # barotp's last tile column 1 wide: the blocked form must decline; three tracer batches
    ("per_s@33x33x9", None),           # doubly periodic; k remainder 1
    ("fuk95@59x21x9", None),           # walls in i (nreg = 4); k remainder 1
    ("tri_s@58x31x17_tke", None),      # arctic patch; two chunks + 1
    ("tri_s@53x37x9", None),           # arctic patch with a last tile 21 wide / 5 high over k remainder 1
    # arctic patch with a last tile 1 wide / 6 high; an odd idm, where the point i = (idm + 1) / 2 of the seam row is its own mirror image on
    # the v-grid and changes its sign at every halo update (phy/mod_xc.F90:4348-4351) -- the persistent barotp kernel used to do that once
    ("tri_s@65x22x3", None),
]


@pytest.mark.parametrize("cfg,ntr", STAGE_SIZES, ids=[c for c, _ in STAGE_SIZES])
def test_stage_parity_at_this_size(cfg, ntr):
    """tests/test_gpu_stage_parity.py's loop with the C restatement as the backend: three steps, in front of every stage of
    GPU_STAGES the restatement's whole state goes to the device, the stage runs there, and every array both sides hold is compared,
    halos included"""
    case = make_case(cfg, ntr=ntr)
    assert case.name == cfg
    orc = _c_restatement(case)
    run_stages_against(orc, case, 3, GPU_STAGES, lambda: orc.delt1)


# ---- b. barotp's shapes, free run -------------------------------------------------------------------------------------------------
def _device_run(case, segments):
    """A fresh context stepped through `segments`, a list of (options, nsteps): the options are set in front of each segment.
    Returns the (barotp_shape, barotp_block_mode) in front of each segment and every STATE_FIELDS array after the last."""
    from blom_amd.gpu import BlomGpu
    nreg, masks = _masks(case)
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    try:
        hostinit.init_state(gpu, case)
        ns, shapes = 0, []
        for opts, nsteps in segments:
            for k, v in opts.items():
                gpu.set(k, v)
            shapes.append((int(gpu.get_real("barotp_shape")), int(gpu.get_real("barotp_block_mode"))))
            assert gpu.step(ns, nsteps) == ns + nsteps
            ns += nsteps
        return shapes, {nm: gpu.get(nm) for nm in STATE_FIELDS if gpu.has_field(nm)}
    finally:
        gpu.close()


def _assert_equals_the_c_restatement(case, nsteps, got):
    orc = _c_restatement(case)
    ns = 0
    for _ in range(nsteps):
        ns = dyncore_step(orc, ns, case.params["baclin"])
    J, I = slice(4, 4 + case.jdm), slice(4, 4 + case.idm)
    for nm in FREE_FIELDS:
        a, b = orc.get(nm)[..., J, I], got[nm][..., J, I]
        ne = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert not ne.any(), f"{case.name} after {nsteps} steps: {nm} differs from the C restatement in {int(ne.sum())} cells, first at (k,j,i) = {tuple(int(x) + 1 for x in np.argwhere(ne)[0])}"
    assert np.isfinite(got["ub"][..., J, I]).all() and np.abs(got["ub"]).max() > 0.0


def _assert_same_bytes(case, a, b, what):
    bad = [nm for nm in a if nm not in SKIP and a[nm].tobytes() != b[nm].tobytes()]
    assert not bad, (case.name, what, bad)


# size, steps, the (shape, form) the default options give on 256 CUs: the kernel that is
SHAPE_SIZES = [
    ("chan_s@20x37x3", 6, (2615, 1)),      # k_bt_steps4<26,15>: 1 x 3 tiles, last row 7
    ("chan_s@58x53x3", 6, (2615, 1)),      # the same over 3 x 4 tiles; the last column exactly BT4_RH wide across the periodic seam
    ("box_s@33x53x8", 6, (2615, 1)),       # the same with walls and land
    ("chan_s@31x47x5", 6, (2616, 0)),      # last column 5 < BT4_RH: the blocked form declines, persistent pair form
    ("tri_s@64x37x3", 6, (2615, 0)),       # k_bt_steps<true,26,15> with the arctic mirror, small
    ("tri_s@65x22x3", 6, (2616, 0)),       # k_bt_steps<true,26,16> with the arctic mirror on an odd idm: the seam row's pivot is its own image
    # 430 wide: 306 and 323 tiles of 26 x 16 / 26 x 15 exceed the CUs.  350 000 points in three layers: milliseconds on the device,
    # about a second a step in the C restatement, hence three steps
    ("chan_s@430x273x3", 3, (4015, 0)),    # k_bt_steps<true,40,15> without the arctic patch (40 x 16 leaves a 1-high row)
    ("tri_s@430x277x3", 3, (4015, 0)),     # the same with the arctic patch
    ("tri_s@430x280x3", 3, (4016, 0)),     # k_bt_steps<true,40,16> with the arctic patch
]


@pytest.mark.parametrize("cfg,nsteps,expected", SHAPE_SIZES, ids=[c for c, _, _ in SHAPE_SIZES])
def test_barotp_shape_free_run(cfg, nsteps, expected):
    """The default options' run: the shape and form asserted first; then == the C restatement's free run on the interior, and the
    bytes of every array of the runs with one kernel per equation, with one launch per substep pair and, where there is no arctic
    patch, without the blocked form and with the blocked form launched per four substeps."""
    case = make_case(cfg)
    assert case.name == cfg
    shapes, new = _device_run(case, [({}, nsteps)])
    assert shapes[0] == expected, f"{cfg}: barotp would run (shape, form) = {shapes[0]}, this test is about {expected}"
    _assert_equals_the_c_restatement(case, nsteps, new)
    variants = [dict(barotp_fused=0, barotp_persist=0), dict(barotp_persist=0)]
    if case.nreg != 2:
        variants += [dict(barotp_block=0), dict(barotp_block=2)]
    for opts in variants:
        sh, other = _device_run(case, [(opts, nsteps)])
        if opts.get("barotp_block") == 0:
            assert sh[0][1] == 0, (cfg, opts, sh)
        if opts.get("barotp_block") == 2 and expected[1] == 1:
            assert sh[0] == (expected[0], 2), (cfg, opts, sh)
        _assert_same_bytes(case, new, other, opts)


# ---- d. one context, forms switched -----------------------------------------------------------------------------------------------
def test_one_context_switches_barotp_forms():
    """jj = 261: the persistent pair form has 17 tile rows of 16, the blocked form 18 of 15, and both keep their completion counts
    in one buffer of the context.  One context runs two steps without the blocked form, two with it, two without: the selection must
    go 2616 -> 2615 -> 2616 and the six steps must equal the C restatement's and leave the bytes of a fresh context's six default steps
    (all forms are bit-identical).  This pins the results and the selection.  It does not observe a buffer too small for the second
    form -- the allocation grows with the tile count (bt_flags_restart), which is established by reading: a device allocation's
    granularity hides four stray bytes."""
    case = make_case("chan_s@20x261x3_tke")
    shapes, new = _device_run(case, [(dict(barotp_block=0), 2), (dict(barotp_block=1), 2), (dict(barotp_block=0), 2)])
    assert shapes == [(2616, 0), (2615, 1), (2616, 0)], shapes
    _assert_equals_the_c_restatement(case, 6, new)
    sh, fresh = _device_run(case, [({}, 6)])
    assert sh == [(2615, 1)], sh
    _assert_same_bytes(case, new, fresh, "one form throughout")


# ---- c. forced shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,nsteps", [("chan_s", 12), ("box_s", 8), ("fuk95", 6), ("chan_m", 6), ("tri_s", 8), ("chan_s_tke", 12), ("tri_s_tke", 8)])
@pytest.mark.parametrize("tile", [2615, 4015])
def test_forced_15_row_tiles_bit_identical(cfg, nsteps, tile):
    """tests/test_gpu_variants.py::test_variants_bit_identical, on its cases, with the barotp_tile pairs (3216, 2615) and (3216, 4015):
    k_bt_steps<false,26,15> and <false,40,15>, which no selection rule gives the pair-per-launch form, and the persistent and blocked
    kernels wherever those shapes are usable"""
    variants.test_variants_bit_identical(cfg, nsteps, "barotp_tile", (3216, tile))


# ---- e. k_diasig<G, DSG_MAXK> -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["chan_s@20x24x57_tke", "chan_s@20x24x120_tke"])
def test_density_classes_accumulate_with_more_than_56_layers(cfg):
    """k_diasig<G, DSG_MAXK>, the instantiation for kdm > 56 (every family has 53 layers at the most): chan_s_tke's columns cut into 57
    layers, the smallest kdm that selects it, and into 120, the cap.  tests/test_gpu_diasig.py's check_step_accumulates, against that
    file's numpy restatement, with the tables its tables_for derives at that kdm."""
    diasig.check_step_accumulates(cfg)


def check_class_cap():
    from blom_amd.gpu import BlomGpuError
    case, _, g = dyncore_context("chan_s@20x24x121_tke")
    try:
        g.dia_set_sigdia(25.0 + 0.05 * np.arange(case.kdm))
        with pytest.raises(BlomGpuError, match="the density classes need 2 <= kdm <= 120 and a sigdia of kdm values"):
            g.dia_select("umfll")
    finally:
        g.close()


def test_more_density_classes_than_the_kernel_holds_are_refused():
    check_class_cap()
