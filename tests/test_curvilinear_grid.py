"""The curvilinear test grids of blom_amd.cases.warped_grid (make_case(..., grid="warped" | "warped_eq")) are what the parity suites
need them to be: no two metric arrays agree anywhere, none equals its own neighbours, the Coriolis parameter differs between the
corners and the centre of every cell, halos and derived arrays follow phy/mod_inigeo.F90:100-156 bit for bit -- and every metric array
is read by some stage (scaling it alone changes a compared field), so that the suites that run on these grids are not vacuous for it."""
import itertools

import numpy as np
import pytest

from blom_amd.cases import default_grid, make_case, warped_grid, GRID_ITYPE, _DIMS
from blom_amd import hostinit
from blom_amd.stepper import dyncore_step, DYNCORE_STAGES
from parity import copy_state, diff_report, GRID_FIELDS, STATE_FIELDS, INT_FIELDS

BASE = ["scqx", "scqy", "scpx", "scpy", "scux", "scuy", "scvx", "scvy"]
CASES = ["chan_s", "chan_b", "box_s", "tri_s", "tri_m", "per_s", "fuk95"]
KINDS = ["warped", "warped_eq"]


def _inner(case, a):
    return a[4:4 + case.jdm, 4:4 + case.idm]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", CASES)
def test_no_two_metric_arrays_agree_and_none_equals_its_neighbours(cfg, kind):
    case = make_case(cfg, grid=kind)
    g = case.grid
    for a, b in itertools.combinations(BASE, 2):
        assert (_inner(case, g[a]) != _inner(case, g[b])).all(), (a, b)
    # (on tri_*, xctilr's arctic rule makes row jj the mirror image of row jj-1 (p, u) or of itself (q, v): at the fixed points of the
    # mirror it repeats a neighbour by construction, in the reference too, so the seam row is left out of the neighbour comparison)
    for nm in BASE + ["corioq", "coriop", "betafp"]:
        a = _inner(case, g[nm])
        if case.nreg == 2:
            a = a[:-1]
        assert (a[:, 1:] != a[:, :-1]).all(), (nm, "i+-1")
        assert (a[1:, :] != a[:-1, :]).all(), (nm, "j+-1")
        assert np.isfinite(g[nm]).all()
    for nm in BASE:
        assert (_inner(case, g[nm]) > 1.0).all()
    q, p = _inner(case, g["corioq"]), _inner(case, g["coriop"])
    assert (q != p).all()
    assert (q[:, 1:] != p[:, :-1]).all() and (q[1:, :] != p[:-1, :]).all() and (q[1:, 1:] != p[:-1, :-1]).all()      # the other corners
    assert (q != 0.0).all() and (p != 0.0).all()
    wet = _inner(case, case.depth) > 0.0
    if kind == "warped":
        assert (q > 0.0).all() and (p > 0.0).all()
    else:
        assert (p[wet] > 0.0).any() and (p[wet] < 0.0).any(), "f does not change sign on the wet points"
    assert (_inner(case, g["betafp"]) > 0.0).all()
    sx, sy = _inner(case, g["scpx"]), _inner(case, g["scpy"])
    assert 0.65 < sy.mean() / sx.mean() < 0.75
    assert sx.max() / sx.mean() > 1.2 and sx.min() / sx.mean() < 0.8


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cfg", CASES)
def test_halos_and_derived_arrays_follow_inigeo(cfg, kind):
    case = make_case(cfg, grid=kind)
    g = case.grid
    ii, jj, nreg = case.idm, case.jdm, case.nreg
    assert set(g) == set(GRID_ITYPE) and set(GRID_FIELDS) <= set(g)
    # halos: what xctilr gives from the interior, for the array's own point type
    for nm, it in GRID_ITYPE.items():
        a = np.zeros_like(g[nm])
        a[4:4 + jj, 4:4 + ii] = _inner(case, g[nm])
        hostinit.xctilr_np(a[None], 1, 1, 4, 4, nreg, ii, jj, itype=it)
        assert np.array_equal(a, g[nm]), nm
    # derived arrays: the formulas of the interior loop, then the same halo rule (mod_inigeo.F90:105-116, :144-153)
    with np.errstate(divide="ignore"):
        for pt in "pquv":
            assert np.array_equal(_inner(case, g[f"sc{pt}2"]), _inner(case, g[f"sc{pt}x"] * g[f"sc{pt}y"]))
        for nm, src in (("scq2i", "scq2"), ("scp2i", "scp2"), ("scuxi", "scux"), ("scvyi", "scvy"), ("scuyi", "scuy"), ("scvxi", "scvx")):
            assert np.array_equal(_inner(case, g[nm]), _inner(case, 1.0 / np.maximum(1.0, g[src]))), nm


def test_the_grid_is_a_named_argument_and_uniform_by_default():
    a, b = make_case("chan_s"), make_case("chan_s", grid="uniform")
    assert "grid" not in a.params and "grid" not in make_case("chan_s", grid="warped").params
    for nm in a.grid:
        assert np.array_equal(a.grid[nm], b.grid[nm])
        assert np.ptp(a.grid[nm]) == 0.0
    w = make_case("chan_s_tke", grid="warped", ntr=5, mommth="enedis")
    assert w.ntr == 5 and w.params["mommth"] == "enedis" and np.ptp(w.grid["scux"]) > 0.0
    assert np.array_equal(w.grid["scux"], warped_grid(*_DIMS["chan_s"][:2], 1, _DIMS["chan_s"][4], "warped")["scux"])
    with pytest.raises(AssertionError):
        make_case("fuk95_ref", grid="warped")
    with pytest.raises(AssertionError):
        make_case("chan_s", grid="nonsense")
    # default_grid: the grid of the calls that name none, inside the block alone
    with default_grid("warped"):
        d = make_case("chan_s_tke", ntr=5, mommth="enedis")
        assert np.ptp(make_case("chan_s", grid="uniform").grid["scux"]) == 0.0
    assert all(np.array_equal(d.grid[nm], w.grid[nm]) for nm in w.grid) and "grid" not in d.params
    assert np.ptp(make_case("chan_s").grid["scux"]) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# Every metric array is read: scaling one of them (interior and halo) by 1 + 2**-8 changes some compared field of a 3-step run, in the
# C restatement and -- where it is built -- in the compiled reference.  An array that changes nothing under any of the option sets goes
# into DEAD with the option that would make it live; the test fails when that list and the observation disagree in either direction.
# ---------------------------------------------------------------------------------------------------------------------------------
OPTION_SETS = [dict(), dict(mommth="enecon"), dict(mommth="enedis"), dict(pgfmth="dynamic enthalpy"), dict(bmcmth="dluc"),
               dict(mommth="enedis", pgfmth="dynamic enthalpy", bmcmth="dluc"), dict(mdv4hi=0.0, mdv4lo=0.0), dict(mdv4hi=0.02, mdv4lo=0.004)]
DEAD = {
    # no option: the reference reads scq2 in mod_inigeo alone, to form scq2i (phy/mod_inigeo.F90:108) and for its checksum; no stage of
    # the step and no kernel of the device library reads it (the momentum equation's vorticity uses scq2i)
    "scq2": None,
}
COMPARED = [f for f in STATE_FIELDS + INT_FIELDS if f not in ("util1", "util2")]


def _snapshot(be):
    out = {}
    for nm in COMPARED:
        try:
            out[nm] = np.array(be.get(nm))
        except KeyError:
            pass
    return out


def _run3(make_backend, case, scaled):
    be = make_backend(case)
    hostinit.init_state(be, case)
    if scaled is not None:
        be.put(scaled, (case.grid[scaled] * (1.0 + 2.0 ** -8))[None])
    ns = 0
    for _ in range(3):
        ns = dyncore_step(be, ns, case.params["baclin"], stages=DYNCORE_STAGES)
    return _snapshot(be)


def _coracle(case):
    from oracle.coracle import COracle
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    return COracle(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))


def _refbackend(case):
    from oracle.refblom import get_ref_backend
    return get_ref_backend(case.name, case.depth)


def _live_fields(make_backend, cfg):
    live = set()
    for opts in OPTION_SETS:
        case = make_case(cfg, grid="warped", **opts)
        base = _run3(make_backend, case, None)
        assert all(np.isfinite(a[np.abs(a) < 1.0e30]).all() for a in base.values() if a.dtype.kind == "f")
        for nm in GRID_FIELDS:
            if nm in live:
                continue
            got = _run3(make_backend, case, nm)
            if any(not np.array_equal(base[f], got[f], equal_nan=True) for f in base):
                live.add(nm)
    return live


@pytest.mark.parametrize("cfg", ["chan_s", "tri_s"])
def test_every_metric_array_is_read_by_the_c_restatement(cfg):
    from oracle.coracle import have_coracle
    if not have_coracle():
        pytest.skip("C oracle not built")
    live = _live_fields(_coracle, cfg)
    assert set(GRID_FIELDS) - live == set(DEAD), (sorted(set(GRID_FIELDS) - live), sorted(DEAD))


def test_every_metric_array_is_read_by_the_compiled_reference():
    from oracle.refblom import have_ref
    if not have_ref("chan_s"):
        pytest.skip("oracle/_ref/chan_s/libblomref.so not built")
    try:
        live = _live_fields(_refbackend, "chan_s")
    finally:                        # the reference instance is shared between tests: back to the defaults
        case = make_case("chan_s")
        hostinit.init_state(_refbackend(case), case)
    assert set(GRID_FIELDS) - live == set(DEAD), (sorted(set(GRID_FIELDS) - live), sorted(DEAD))


# ---------------------------------------------------------------------------------------------------------------------------------
# The C restatement against the reference's own compiled Fortran on these grids (tests/test_oracle_vs_reference.py's free run, with its
# step counts): every metric-dependent term of the restatement with its neighbour offsets.  Agreement in NaN would pass that comparison,
# so the reference's state after the run must be finite as well.
# ---------------------------------------------------------------------------------------------------------------------------------
def _freerun_on(grid, cfg, nsteps, eddy):
    from oracle import refblom
    from test_oracle_vs_reference import _freerun
    with default_grid(grid):
        _freerun(cfg, nsteps, eddy)
    ref = refblom._BACKENDS[cfg]                   # the instance _freerun stepped (get_ref_backend would reset it)
    for nm in COMPARED:
        try:
            a = np.asarray(ref.get(nm))
        except KeyError:
            continue
        assert a.dtype.kind != "f" or np.isfinite(a).all(), f"{nm} is not finite after {nsteps} steps on the {grid} grid"


@pytest.mark.parametrize("cfg,nsteps,grid", [("chan_s", 12, "warped"), ("box_s", 12, "warped"), ("tri_s", 8, "warped"), ("chan_s_tke", 12, "warped"),
                                             ("tri_s_tke", 8, "warped"), ("chan_s", 12, "warped_eq"), ("tri_s", 8, "warped_eq")])
def test_c_restatement_equals_the_compiled_reference(cfg, nsteps, grid):
    _freerun_on(grid, cfg, nsteps, False)


@pytest.mark.parametrize("cfg,nsteps,grid", [("chan_s_tke", 12, "warped"), ("tri_s", 8, "warped_eq")])
def test_c_restatement_equals_the_compiled_reference_with_eddy_fluxes(cfg, nsteps, grid):
    _freerun_on(grid, cfg, nsteps, True)
