"""The heat and salt flux diagnostics inside a multi-step call (blomgpu_step, flux_diag): utflx usflx vtflx vsflx as
pbcor and diffus accumulate into them, u|v t|s fltd (k_eddtra_ts) and u|v t|s flld (k_diffus_tile) have no reader inside a step, so a
call of N steps keeps them current in its last two steps only.  What a caller can see must not know: after the call every array of
parity.STATE_FIELDS (util1..4, scratch shared between stages, left out) has the bytes that N calls of one step leave, on both time
levels, halos included -- `tobytes()`, no tolerance: nothing the step computes changes.  The count of steps that skipped
(blomgpu_get_real "flux_diag_steps_skipped") is asserted beside every comparison: max(0, N - 2) where the skip is due, 0 where
something reads the arrays every step (a diaacc row with one of them as its source, csdiag, a captured graph, the caller's
keep_flux_diagnostics); without it these tests would pass on a library that never skips.

Cases: chan_s_tke (periodic channel), tri_s_tke (arctic seam, nreg = 2), box_s (walls and land), each as the default sequence and as
config 2's step with live diffusivities (full_physics + difest_live, the state bench.py times).  N = 1..5: 3 is the first call that
skips, 4 leaves the other parity of the time levels last, 5 skips under both parities.

tests/test_hostemu_lazy_flux_diag.py runs the same functions on the host emulation of the library."""
import threading

import numpy as np
import pytest

from parity import STATE_FIELDS

pytestmark = pytest.mark.gpu

SKIP = {"util1", "util2", "util3", "util4"}
CASES = ["chan_s_tke", "tri_s_tke", "box_s"]
THE_TWELVE = ["utflx", "usflx", "vtflx", "vsflx", "utfltd", "usfltd", "vtfltd", "vsfltd", "utflld", "usflld", "vtflld", "vsflld"]
NMAX = 5
FLUX_ROWS = ["utflx", "usfltd", "vtflld", "utflxlvl"]     # a layer row of each of the three families and a depth-level row
OTHER_ROWS = ["temp", "uvel"]

_RUNS = {}      # the single-step references, computed once and shared (tests/test_hostemu_lazy_flux_diag.py swaps in its own)


def context(cfg, full):
    """the default stage sequence from the case's initial state, or config 2's step with live diffusivities and a surface forcing"""
    import test_gpu_diaacc as dia
    if full:
        return dia.full_context(cfg)
    return dia.dyncore_context(cfg)


def state(gpu):
    gpu.sync()
    return {nm: gpu.get(nm).tobytes() for nm in STATE_FIELDS if nm not in SKIP and gpu.has_field(nm)}


def skipped(gpu):
    return int(gpu.get_real("flux_diag_steps_skipped"))


def single_steps(cfg, full, rows=()):
    """NMAX calls of one step: the state after each, the accumulators of `rows` after four, and the count (0: a call of one step has
    no step to skip).  Never modified by its users."""
    key = (cfg, full, tuple(rows))
    if key not in _RUNS:
        _, _, g = context(cfg, full)
        try:
            if rows:
                g.dia_select(list(rows))
            states, acc = [], None
            for ns in range(NMAX):
                assert g.step(ns, 1) == ns + 1
                states.append(state(g))
                if rows and ns == 3:
                    acc = {nm: g.dia_get(nm).tobytes() for nm in rows}
            _RUNS[key] = dict(states=states, acc=acc, skipped=skipped(g))
        finally:
            g.close()
    return _RUNS[key]


def differing(got, want):
    assert set(got) == set(want)
    return sorted(nm for nm in got if got[nm] != want[nm])


# ---- 1. one call of N steps against N calls of one step ------------------------------------------------------------------------------
def check_one_call(cfg, full, n):
    ref = single_steps(cfg, full)
    assert ref["skipped"] == 0, "a call of one step skipped"
    _, _, g = context(cfg, full)
    try:
        assert g.step(0, n) == n
        got = state(g)
        assert set(THE_TWELVE) <= set(got)
        bad = differing(got, ref["states"][n - 1])
        assert not bad, (cfg, full, n, bad)
        assert skipped(g) == max(0, n - 2), (cfg, full, n, skipped(g))
        u = np.frombuffer(got["utflx"])
        assert np.isfinite(u).all() and np.abs(u).max() > 0.0
    finally:
        g.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", CASES)
def test_one_call_of_n_steps_leaves_the_bytes_of_n_single_step_calls(cfg, full, n):
    check_one_call(cfg, full, n)


# ---- 2. a diaacc selection -----------------------------------------------------------------------------------------------------------
def check_selection(cfg, full, rows, expect_skipped):
    """four steps in one call with `rows` selected: count, accumulators and state against four single-step calls"""
    ref = single_steps(cfg, full, rows)
    assert ref["skipped"] == 0
    _, _, g = context(cfg, full)
    try:
        g.dia_select(list(rows))
        assert g.step(0, 4) == 4
        assert skipped(g) == expect_skipped, (cfg, full, rows, skipped(g))
        assert g.dia_nacc() == 4
        acc = {nm: g.dia_get(nm).tobytes() for nm in rows}
        bad = differing(acc, ref["acc"])
        assert not bad, (cfg, full, "accumulators", bad)
        for nm in rows:
            # (the default sequence starts from zero diffusivities difint: its eddy-induced fluxes, usfltd here, rest)
            if full or nm != "usfltd":
                assert np.abs(np.frombuffer(acc[nm])).max() > 0.0, nm
        bad = differing(state(g), ref["states"][3])
        assert not bad, (cfg, full, "state", bad)
    finally:
        g.close()


@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", CASES)
def test_a_selected_flux_diagnostic_is_kept_current_in_every_step(cfg, full):
    check_selection(cfg, full, FLUX_ROWS, 0)


@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", CASES)
def test_a_selection_of_unrelated_rows_does_not_keep_them_current(cfg, full):
    check_selection(cfg, full, OTHER_ROWS, 2)


# ---- 3. what else reads the arrays every step -----------------------------------------------------------------------------------------
def check_never_skips(cfg, full, how):
    """four steps in one call: no step skips, and the state is the default's"""
    ref = single_steps(cfg, full)
    _, _, g = context(cfg, full)
    try:
        if how == "keep":
            g.keep_flux_diagnostics(1)
        else:
            g.set(how, 1)
        assert g.step(0, 4) == 4
        assert skipped(g) == 0, (cfg, full, how, skipped(g))
        bad = differing(state(g), ref["states"][3])
        assert not bad, (cfg, full, how, bad)
        if how == "keep":                                   # ... and the switch goes back
            g.keep_flux_diagnostics(0)
            assert g.step(4, 3) == 7
            assert skipped(g) == 1
    finally:
        g.close()


@pytest.mark.parametrize("how", ["keep", "csdiag", "use_graph"])
@pytest.mark.parametrize("full", [False, True], ids=["default", "full_physics_live"])
@pytest.mark.parametrize("cfg", CASES)
def test_off_switch_checksums_and_graph_replay_keep_every_step_whole(cfg, full, how):
    check_never_skips(cfg, full, how)


# ---- 4. tiles -------------------------------------------------------------------------------------------------------------------------
def check_tiles(cfg="chan_s", npx=1, npy=2, nsteps=5):
    """a 1 x 2 layout of one process (tests/test_gpu_tiles.py), one call of five steps on every tile, against the single tile stepped
    in five calls: every tile skips three steps, and the interiors have the single tile's bytes, the twelve arrays included"""
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd.tiles import tile_extents, tile_window, scatter_state, gather_interior
    from test_gpu_tiles import _single, ALL, CHECK
    case, masks, fields, ref = _single(cfg, nsteps)
    ii, jj = tile_extents(case, npx, npy)
    grp = TileGroup(npx, npy)
    tiles = {}
    try:
        for py in range(npy):
            for px in range(npx):
                tm = {k: tile_window(masks[k], case, npx, npy, px, py) for k in masks}
                t = BlomGpu(ii, jj, case.kdm, case.ntr, case.nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=px * ii, j0=py * jj)
                for nm, v in case.params.items():
                    if not nm.endswith("0"):
                        t.set(nm, v)
                t.set("delt1", case.params["baclin"])
                grp.attach(t, px, py)
                tiles[(px, py)] = t
        scatter_state(ref, tiles, case, npx, npy, [f for f in ALL if f in fields])
        for ns in range(nsteps):
            assert ref.step(ns, 1) == ns + 1
        assert skipped(ref) == 0
        errs = []

        def run(t):
            try:
                assert t.step(0, nsteps) == nsteps
                t.sync()
            except Exception as e:          # a failing tile would leave the others at a barrier
                errs.append(e)
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x.start() for x in th]
        [x.join(timeout=300) for x in th]
        assert not errs, errs
        for t in tiles.values():
            assert skipped(t) == nsteps - 2
        bad = []
        for nm in CHECK + THE_TWELVE:
            a = ref.get(nm)[:, 4:4 + case.jdm, 4:4 + case.idm]
            b = gather_interior(tiles, case, npx, npy, nm)
            if a.tobytes() != np.ascontiguousarray(b).tobytes():
                bad.append(nm)
        assert not bad, bad
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


def test_tiles_of_one_process_skip_and_match_the_single_tile():
    check_tiles()
