"""diaacc's vertical mass fluxes on the device (k_diavfl_lyr, k_diavfl_lvl, blom_amd/csrc/stage_diaacc.hip): wflx wflx2 wflxlvl wflx2lvl.

The expected values are the reference's loops restated in numpy below (RestatedVfl): phy/mod_dia.F90:4647-4676 (wflx carried from
k = kk up to 1 out of the step's uflx, vflx at k + nn and dp - dpold at k + mm), :4693-4730 (ucum, vcum carried from d = ddm up to 1
out of uflxlvl - uflxold, vflxlvl - vflxold where the face's iu | iv is set, out to ii+1 | jj+1) and the copy of :1921-1942 in front
of them.  Every point sees the reference's operations in the reference's order in float64 (numpy does not contract; x**2 is x*x, as
amdflang lowers it).  The restatement is applied over the whole padded arrays to what a second, single-stepping context downloads
after each of its steps: uflx vflx dp dpold, and its own uflxlvl vflxlvl before and after the step.  Single steps do not fold tmsmt1
into tmsmt2, so that context's dpold is the reference's; the context under test takes its steps in ONE call.  The downloaded level
fluxes carry the halo that the stage's xctilr (:4681-4684) gave them: blom_amd.hostinit.xctilr_np on them must change nothing.
Everything is compared with ==, byte for byte over the whole padded array.

tests/test_hostemu_diavfl.py runs the same checks on the host emulation of the library."""
import numpy as np
import pytest

from blom_amd import hostinit
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import full_context, dyncore_context, same_bytes, differing

pytestmark = pytest.mark.gpu

FILL = 9.9692099683868690e+36         # nf90_fill_double
NAMES = "wflx wflx2 wflxlvl wflx2lvl".split()
FORMED_FROM = "uflx vflx uflxlvl vflxlvl".split()
OLD = "uflxold vflxold".split()               # ACC_UFLXOLD / ACC_VFLXOLD: in the group, handed out by dia_get, not selectable
SLOTS = NAMES + FORMED_FROM                   # the eight slots of the issue
GRID = dict(wflx="p", wflx2="p", wflxlvl="p", wflx2lvl="p", uflx="u", vflx="v", uflxlvl="u", vflxlvl="v", uflxold="u", vflxold="v")
LEVEL_NAMES = "templvl dzlvl utflxlvl vsflxlvl uflxlvl vflxlvl".split()     # level names every case admits, the group's own two among them
OLD_STATE = "dpold told sold trcold dpuold dpvold".split()  # what tmsmt1 writes: folded or not, the end of the call must agree

_LAYER_ADMITTED = lyr.admitted


class RestatedVfl:
    """phylyr(wflx, wflx2) and phylvl(wflxlvl, wflx2lvl) of one tile"""

    def __init__(self, case, masks, ddm):
        self.case, self.kk, self.ddm = case, case.kdm, ddm
        ii, jj = case.idm, case.jdm
        nj, ni = jj + 8, ii + 8
        self.shape = (nj, ni)
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + jj, 4:4 + ii] = True
        self.sel = own & (self.mask["p"] > 0)                     # do j = 1,jj; do l = 1,isp(j); do i = max(1,ifp),min(ii,ilp)
        ru = np.zeros((nj, ni), bool)
        ru[4:4 + jj, 4:5 + ii] = True                              # j = 1,jj;   i = max(1,ifu),min(ii+1,ilu)   :4695-4697
        rv = np.zeros((nj, ni), bool)
        rv[4:5 + jj, 4:4 + ii] = True                              # j = 1,jj+1; i = max(1,ifv),min(ii,ilv)     :4706-4708
        self.face = {"u": ru & (self.mask["u"] > 0), "v": rv & (self.mask["v"] > 0)}
        self.seen = dict(dp_moved=[], vcum_north=0.0)
        self.reset()

    def reset(self):
        zero = 0.0 * self.mask["p"].astype(np.float64)            # inilyr / inilvl: 0*mask over the whole padded plane
        self.acc = {nm: np.repeat(zero[None], self.ddm if nm.endswith("lvl") else self.kk, axis=0).copy() for nm in NAMES}
        self.nacc = 0

    def accumulate(self, s):
        """s: uflx, vflx (kk planes at k + nn), dp, dpold (kk planes at k + mm), scp2 (plane), ulvl0, vlvl0 (the level fluxes in front
        of the step: what :1921-1942 copies), ulvl1, vlvl1 (behind the step's acclvl and the exchange of :4681-4684)"""
        nj, ni = self.shape
        sel = self.sel[:-1, :-1]                                   # (nobody owns the last padded row or column)
        self.nacc += 1
        with np.errstate(all="ignore"):
            wflx = np.zeros((nj - 1, ni - 1))
            a, a2 = self.acc["wflx"], self.acc["wflx2"]
            moved = False
            for k in range(self.kk - 1, -1, -1):
                u, v = s["uflx"][k], s["vflx"][k]
                ddp = s["dp"][k] - s["dpold"][k]
                new = (wflx - (((u[:-1, 1:] - u[:-1, :-1]) + v[1:, :-1]) - v[:-1, :-1])) - (ddp * s["scp2"])[:-1, :-1]
                wflx[sel] = new[sel]
                a[k][:-1, :-1][sel] = (a[k][:-1, :-1] + wflx)[sel]
                a2[k][:-1, :-1][sel] = (a2[k][:-1, :-1] + wflx * wflx)[sel]
                moved = moved or bool((ddp[:-1, :-1][sel] != 0.0).any())
            self.seen["dp_moved"].append(moved)
            ucum, vcum = np.zeros((nj, ni)), np.zeros((nj, ni))
            a, a2 = self.acc["wflxlvl"], self.acc["wflx2lvl"]
            for d in range(self.ddm - 1, -1, -1):
                new = (ucum + s["ulvl1"][d]) - s["ulvl0"][d]
                ucum[self.face["u"]] = new[self.face["u"]]
                new = (vcum + s["vlvl1"][d]) - s["vlvl0"][d]
                vcum[self.face["v"]] = new[self.face["v"]]
                q = -(((ucum[:-1, 1:] - ucum[:-1, :-1]) + vcum[1:, :-1]) - vcum[:-1, :-1])
                a[d][:-1, :-1][sel] = (a[d][:-1, :-1] + q)[sel]
                a2[d][:-1, :-1][sel] = (a2[d][:-1, :-1] + q * q)[sel]
                jn = 4 + self.case.jdm                             # vcum(:, jj+1): on the arctic patch the row beyond the seam
                self.seen["vcum_north"] = max(self.seen["vcum_north"], float(np.abs(vcum[jn, 4:4 + self.case.idm]).max()))


def snapshot(gpu, nstep, kk, before):
    m, n, mm, nn, k1m, k1n = hostinit.step_indices(nstep, kk)
    return dict(uflx=gpu.get("uflx")[nn:nn + kk].copy(), vflx=gpu.get("vflx")[nn:nn + kk].copy(), dp=gpu.get("dp")[mm:mm + kk].copy(),
                dpold=gpu.get("dpold")[mm:mm + kk].copy(), scp2=gpu.get("scp2")[0].copy(), ulvl0=before["uflxlvl"], vlvl0=before["vflxlvl"],
                ulvl1=gpu.dia_get("uflxlvl"), vlvl1=gpu.dia_get("vflxlvl"))


def check_exchange_and_copy(case, before, gpu, snap):
    """behind the stage: uflxold | vflxold hold what uflxlvl | vflxlvl held in front of it, halo included (:1921-1942), and the level
    fluxes have the one-point halo of xctilr(1,ddm, 1,1, halo_uv | halo_vv): the update restated on the host changes nothing"""
    assert same_bytes(gpu.dia_get("uflxold"), before["uflxlvl"]) and same_bytes(gpu.dia_get("vflxold"), before["vflxlvl"])
    for key, itype in (("ulvl1", 13), ("vlvl1", 14)):
        again = snap[key].copy()
        hostinit.xctilr_np(again, 1, again.shape[0], 1, 1, case.nreg, case.idm, case.jdm, itype=itype)
        assert same_bytes(again, snap[key]), key
    ii, jj = case.idm, case.jdm
    if case.nreg == 1:                   # periodic in i: the halo column is the opposite owned column
        assert same_bytes(snap["ulvl1"][:, 4:4 + jj, 4 + ii], snap["ulvl1"][:, 4:4 + jj, 4])
        assert same_bytes(snap["ulvl1"][:, 4:4 + jj, 3], snap["ulvl1"][:, 4:4 + jj, 3 + ii])


def single_step(b, case, ns, ref):
    before = {nm: b.dia_get(nm) for nm in ("uflxlvl", "vflxlvl")}
    assert b.step(ns, 1) == ns + 1
    snap = snapshot(b, ns, case.kdm, before)
    check_exchange_and_copy(case, before, b, snap)
    if ref is not None:
        ref.accumulate(snap)
    return snap


# ---- one run per case, shared ------------------------------------------------------------------------------------------------------
_RUNS = {}
CASES = ["chan_s_tke", "box_s", "tri_s_tke"]
EXTENDED = {"chan_s_tke"}


def vfl_run(cfg):
    """Context B: the four names selected, single steps; after each the restatement is fed.  Four steps give E4 (extended: six give E6;
    then the names are selected afresh and two more single steps give B8).
    Context A: the four names plus the layer table and LEVEL_NAMES, step(0, 4) in ONE call; finalize; (extended) two steps, reset, two steps.
    (extended) Context C: A's selection without the four names, step(0, 4)."""
    if cfg in _RUNS:
        return _RUNS[cfg]
    extended = cfg in EXTENDED
    r = {}
    case, masks, b = full_context(cfg)
    a = None
    try:
        lnames = lyr.admitted(case) + LEVEL_NAMES
        r.update(case=case, masks=masks, lnames=lnames)
        b.dia_select(NAMES)
        ddm = len(b.dia_levels())
        r["levels"], r["depths"] = b.dia_levels(), b.get("depths")[0]
        ref = RestatedVfl(case, masks, ddm)
        r["init"] = {nm: v.copy() for nm, v in ref.acc.items()}
        for ns in range(4):
            single_step(b, case, ns, ref)
        r["E4"] = {nm: v.copy() for nm, v in ref.acc.items()}
        r["B4_own"] = {nm: b.dia_get(nm) for nm in SLOTS + OLD}
        r["B4_nacc"] = b.dia_nacc()
        r["B4_old"] = {nm: b.get(nm) for nm in OLD_STATE}
        r["seen"] = dict(ref.seen)
        _, _, a = full_context(cfg)
        a.dia_select(NAMES + lnames)
        assert a.step(0, 4) == 4
        r["A4"] = {nm: a.dia_get(nm) for nm in SLOTS + OLD}
        r["A4_nacc"] = a.dia_nacc()
        r["A4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
        r["A4_state"] = {nm: a.get(nm) for nm in list(STATE_FIELDS) + OLD_STATE if a.has_field(nm)}
        a.dia_finalize()
        r["A4_fin"] = {nm: a.dia_get(nm) for nm in NAMES}
        if extended:
            for ns in range(4, 6):
                single_step(b, case, ns, ref)
            r["E6"] = {nm: v.copy() for nm, v in ref.acc.items()}
            r["B6_own"] = {nm: b.dia_get(nm) for nm in SLOTS + OLD}
            assert a.step(4, 2) == 6
            a.dia_reset()
            r["A_reset"] = {nm: a.dia_get(nm) for nm in SLOTS + OLD}
            r["A_reset_nacc"] = a.dia_nacc()
            assert a.step(6, 2) == 8
            r["A8"] = {nm: a.dia_get(nm) for nm in SLOTS + OLD}
            r["A8_nacc"] = a.dia_nacc()
            b.dia_select(NAMES)                                     # afresh
            fresh = RestatedVfl(case, masks, ddm)
            for ns in range(6, 8):
                single_step(b, case, ns, fresh)
            r["B8"] = {nm: b.dia_get(nm) for nm in SLOTS + OLD}
            r["B8_nacc"] = b.dia_nacc()
            r["E8"] = fresh.acc
            a.close()
            _, _, a = full_context(cfg)                             # C
            a.dia_select(lnames)
            assert a.step(0, 4) == 4
            r["C4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
            r["C4_state"] = {nm: a.get(nm) for nm in list(STATE_FIELDS) + OLD_STATE if a.has_field(nm)}
    finally:
        if a is not None:
            a.close()
        b.close()
    _RUNS[cfg] = r
    return r


def owned_wet(r):
    nj, ni = r["case"].jdm + 8, r["case"].idm + 8
    sel = np.zeros((nj, ni), bool)
    sel[4:-4, 4:-4] = True
    return sel & (r["masks"]["ip"].reshape(nj, ni) > 0)


# ---- 1. the step accumulates what the loops would ----------------------------------------------------------------------------------
def check_step_accumulates(cfg):
    r = vfl_run(cfg)
    assert r["A4_nacc"] == 4 and r["B4_nacc"] == 4
    bad = differing(r["A4"], r["E4"])
    assert not bad, f"{cfg}: four steps in one call differ from the restated loops: {bad}"
    bad = differing(r["B4_own"], r["E4"])
    assert not bad, f"{cfg}: the single-stepping context's own accumulators differ from the restated loops: {bad}"
    # the slots the four are formed from, and the two that keep last step's level fluxes: one call == four calls
    bad = [nm for nm in FORMED_FROM + OLD if not same_bytes(r["A4"][nm], r["B4_own"][nm])]
    assert not bad, bad
    sel = owned_wet(r)
    for nm in NAMES:
        assert same_bytes(r["A4"][nm][:, ~sel], r["init"][nm][:, ~sel]), nm       # 0*mask everywhere else
    # tmsmt1 ran as its own launch in every step of the call: the *old arrays end as the single steps leave them
    bad = [nm for nm in OLD_STATE if not same_bytes(r["A4_state"][nm], r["B4_old"][nm])]
    assert not bad, bad


@pytest.mark.parametrize("cfg", CASES)
def test_step_accumulates_what_the_reference_loops_would(cfg):
    check_step_accumulates(cfg)


# ---- 2. the tests are not vacuous ------------------------------------------------------------------------------------------------------
def check_not_vacuous(cfg):
    r = vfl_run(cfg)
    case = r["case"]
    nj, ni = case.jdm + 8, case.idm + 8
    for nm in ("wflx", "wflxlvl", "wflx2", "wflx2lvl"):
        assert (np.abs(r["E4"][nm]) > 0.0).any(), nm
    # dp - dpold at an owned wet point in a step that the fold would have spoiled (every step of the call but its last)
    assert any(r["seen"]["dp_moved"][:3]), r["seen"]["dp_moved"]
    sel = owned_wet(r)
    iu, iv = (r["masks"][k].reshape(nj, ni) > 0 for k in ("iu", "iv"))
    closed = np.zeros((nj, ni), bool)
    closed[:-1, :-1] = ~iu[:-1, :-1] | ~iu[:-1, 1:] | ~iv[:-1, :-1] | ~iv[1:, :-1]
    assert (sel & closed).any(), "no wet p-point with a closed face"
    below = ~(r["depths"][None] > r["levels"][:, 0][:, None, None])            # msklvl: level d is kept exactly when bath > bnds(1,d)
    assert below[:, sel].any(), "no column with levels below its bathymetry"
    if cfg == "tri_s_tke":
        assert r["seen"]["vcum_north"] > 0.0, "vcum(jj+1) is zero all along the seam"
    print(cfg, "dp moved per step:", r["seen"]["dp_moved"], "closed faces at", int((sel & closed).sum()), "wet points;",
          "levels below the bottom:", int(below[:, sel].sum()), "max |vcum(jj+1)|:", r["seen"]["vcum_north"])


@pytest.mark.parametrize("cfg", CASES)
def test_the_cases_exercise_the_loops(cfg):
    check_not_vacuous(cfg)


# ---- 3. interface -------------------------------------------------------------------------------------------------------------------
def check_interface():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)
    try:
        kk = case.kdm
        named, full, whole = g.dia_names(), g.dia_names_all(), g.dia_names_full()
        assert len(named) == 111 and len(full) == 117 and full[:111] == named
        assert whole[:117] == full
        assert whole[117:] == [("wflx", 1, "p"), ("wflx2", 1, "p"), ("wflxlvl", 2, "p"), ("wflx2lvl", 2, "p"), ("uflxold", 4, "u"), ("vflxold", 4, "v")]
        for one in NAMES:                                            # any one of the four selects the group
            g.dia_select(one)
            ddm = len(g.dia_levels())
            for nm in SLOTS + OLD:
                want = (ddm if nm.endswith("lvl") or nm in OLD else kk, case.jdm + 8, case.idm + 8)
                got = g.dia_get(nm)
                assert got.shape == want and same_bytes(got, 0.0 * np.broadcast_to(masks["i" + GRID[nm]].reshape(want[1:]).astype(np.float64), want)), (one, nm)
            with pytest.raises(BlomGpuError, match="temp"):
                g.dia_get("temp")
            with pytest.raises(BlomGpuError, match="selected"):      # the level table is frozen like under any *lvl name
                g.dia_set_levels(levitus2x=True)
            assert len(g.dia_levels()) == ddm
        for internal in OLD:
            with pytest.raises(BlomGpuError, match=internal):
                g.dia_select("wflx " + internal)
        g.dia_select("wflx2lvl temp")
        assert g.step(0, 2) == 2 and g.dia_nacc() == 2
        w2, t2 = g.dia_get("wflx2lvl"), g.dia_get("temp")
        assert (w2 > 0.0).any()
        with pytest.raises(BlomGpuError, match="nonsense"):
            g.dia_select("wflx nonsense")
        assert same_bytes(g.dia_get("wflx2lvl"), w2) and same_bytes(g.dia_get("temp"), t2) and g.dia_nacc() == 2
        g.dia_select("temp")                                         # without the group the table may change again
        g.dia_set_levels(levitus2x=True)
        g.dia_select("wflx")
        assert g.dia_get("wflxlvl").shape[0] == 70 and g.dia_get("uflxold").shape[0] == 70
        g.dia_select("")
        with pytest.raises(BlomGpuError, match="wflx"):
            g.dia_get("wflx")
        # admitted under the other coordinates, as uflxlvl / vflxlvl are
        for vc in ("cntiso_hybrid", "plevel"):
            g.set("vcoord_type", vc)
            g.dia_select("wflxlvl")
            assert g.dia_get("wflx").shape[0] == kk
        g.dia_select("")
        g.set("vcoord_type", "isopyc_bulkml")
    finally:
        g.close()


def test_interface():
    check_interface()


# ---- 4. independence, finalize, reset ------------------------------------------------------------------------------------------------
def check_independence_finalize_reset():
    r = vfl_run("chan_s_tke")
    # the group changes no byte of the other accumulators (of uflxlvl / vflxlvl, which it exchanges: none at the owned points) ...
    exch = ("uflxlvl", "vflxlvl")
    bad = [nm for nm in r["lnames"] if nm not in exch and not same_bytes(r["A4_lyr"][nm], r["C4_lyr"][nm])]
    bad += [nm for nm in exch if not same_bytes(r["A4_lyr"][nm][:, 4:-4, 4:-4], r["C4_lyr"][nm][:, 4:-4, 4:-4])]
    assert not bad, bad
    # ... and none of the model state, the *old arrays among them although no tmsmt1 was folded
    bad = [nm for nm in r["C4_state"] if not same_bytes(r["A4_state"][nm], r["C4_state"][nm])]
    assert not bad, bad
    assert all(nm in r["C4_state"] for nm in OLD_STATE + ["uflx", "dp"])
    assert all((np.abs(r["A4_lyr"][nm]) > 0.0).any() for nm in ["temp", "sealv"] + LEVEL_NAMES)
    # finalize: msklvl on the two level names (:2676-2677), nothing on the two layer names
    sel = owned_wet(r)
    own = np.zeros_like(sel)
    own[4:-4, 4:-4] = True
    below = ~(r["depths"][None] > r["levels"][:, 0][:, None, None]) & own[None]
    for nm in ("wflxlvl", "wflx2lvl"):
        want = r["E4"][nm].copy()
        want[below] = FILL
        assert same_bytes(r["A4_fin"][nm], want), nm
    assert below.any() and not below.all()
    assert same_bytes(r["A4_fin"]["wflx"], r["E4"]["wflx"]) and same_bytes(r["A4_fin"]["wflx2"], r["E4"]["wflx2"])
    # reset: 0*mask in all eight slots and the two old ones, count 0; the next block equals a fresh selection's
    nj, ni = sel.shape
    for nm in SLOTS + OLD:
        z = 0.0 * r["masks"]["i" + GRID[nm]].reshape(1, nj, ni).astype(np.float64)
        assert same_bytes(r["A_reset"][nm], np.repeat(z, r["A_reset"][nm].shape[0], axis=0)), nm
    assert r["A_reset_nacc"] == 0
    assert not differing(r["A8"], r["B8"]), differing(r["A8"], r["B8"])
    assert not differing(r["A8"], r["E8"]), differing(r["A8"], r["E8"])
    assert r["A8_nacc"] == 2 and r["B8_nacc"] == 2
    assert (np.abs(r["A8"]["wflxlvl"]) > 0.0).any()


def test_independence_finalize_reset():
    check_independence_finalize_reset()


# ---- 5. tiles ---------------------------------------------------------------------------------------------------------------------------
def check_tiles(monkeypatch, npx=2, npy=1):
    """test_gpu_diaacc.check_tiles on a 2x1 and on a 1x2 group with the four names (and uflxlvl vflxlvl) added to its selection: every
    tile's slots are its window of the single tile's.  The u-faces at ii+1 of the first tile of 2x1 are the second tile's column 1:
    uflx(ii+1) of the step, and the halo of uflxlvl that the stage's exchange brings; likewise the v-faces at jj+1 on 1x2."""
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu, BlomGpuError
    monkeypatch.setattr(lyr, "admitted", lambda case: _LAYER_ADMITTED(case) + NAMES + ["uflxlvl", "vflxlvl"])
    import test_gpu_tiles
    monkeypatch.setattr(test_gpu_tiles, "FORCING", test_gpu_tiles.FORCING + ["depths"])      # the tiles need their window of the bathymetry
    seen, close = [], BlomGpu.close

    def closing(self):
        if self.ctx:
            try:
                seen.append(((self.idm, self.jdm), {nm: self.dia_get(nm) for nm in ("uflxlvl", "vflxlvl") + tuple(OLD)}))
            except BlomGpuError:
                pass                                                 # (a context without the selection)
        close(self)
    monkeypatch.setattr(BlomGpu, "close", closing)
    lyr.check_tiles("chan_s_tke", npx, npy)
    case = make_case("chan_s_tke")
    ii, jj = case.idm // npx, case.jdm // npy
    (t0, t1), (whole,) = [a for n, a in seen if n == (ii, jj)], [a for n, a in seen if n == (case.idm, case.jdm)]
    rows, cols = slice(4, 4 + jj), slice(4, 4 + ii)
    if npx == 2:
        u0, u1 = t0["uflxlvl"], t1["uflxlvl"]
        # the one-point halo is the neighbour tile's owned column: inside the domain, and across the periodic seam
        assert same_bytes(u1[:, rows, 3], u0[:, rows, 3 + ii]) and same_bytes(u0[:, rows, 4 + ii], u1[:, rows, 4])
        assert same_bytes(u0[:, rows, 3], u1[:, rows, 3 + ii]) and same_bytes(u1[:, rows, 4 + ii], u0[:, rows, 4])
        assert np.abs(u0[:, rows, 4 + ii]).max() > 0.0
    else:
        v0, v1 = t0["vflxlvl"], t1["vflxlvl"]
        assert same_bytes(v0[:, 4 + jj, cols], v1[:, 4, cols]) and same_bytes(v1[:, 3, cols], v0[:, 3 + jj, cols])
        assert np.abs(v0[:, 4 + jj, cols]).max() > 0.0
    # the old slots are windows of the single tile's too, the halo column | row at ii+1 | jj+1 included (it is what diavfl reads)
    for q, t in enumerate((t0, t1)):
        px, py = (q, 0) if npx == 2 else (0, q)
        assert same_bytes(t["uflxold"][:, rows, 4:5 + ii], whole["uflxold"][:, 4 + py * jj:4 + (py + 1) * jj, 4 + px * ii:5 + (px + 1) * ii]), q
        assert same_bytes(t["vflxold"][:, 4:5 + jj, cols], whole["vflxold"][:, 4 + py * jj:5 + (py + 1) * jj, 4 + px * ii:4 + (px + 1) * ii]), q


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_accumulate_their_window_of_the_single_tile(monkeypatch, npx, npy):
    check_tiles(monkeypatch, npx, npy)


# ---- 6. the graph option --------------------------------------------------------------------------------------------------------------------
def check_graph_replay(expect_replays):
    r = vfl_run("chan_s_tke")
    case, masks, g = full_context("chan_s_tke")
    try:
        g.set("use_graph", 1)
        g.dia_select(NAMES)
        assert g.step(0, 6) == 6
        got = {nm: g.dia_get(nm) for nm in SLOTS + OLD}
        assert not differing(got, r["E6"]), differing(got, r["E6"])
        assert not differing(got, r["B6_own"]), differing(got, r["B6_own"])
        assert g.dia_nacc() == 6
        if expect_replays:
            assert g.get_real("graph_steps") >= 1, "no step was replayed as a graph"
    finally:
        g.close()


def test_graph_replay_accumulates_the_same_bytes():
    import os
    check_graph_replay(expect_replays=os.environ.get("BLOM_HOSTEMU") != "1")


# ---- 7. the hybrid coordinate -----------------------------------------------------------------------------------------------------------------
def check_hybrid():
    """cntiso_hybrid: the stage on its own, twice, on fluxes and thicknesses the test puts"""
    case, masks, g = dyncore_context("chan_s", vcoord_type="cntiso_hybrid")
    try:
        kk, ii, jj = case.kdm, case.idm, case.jdm
        nj, ni = jj + 8, ii + 8
        y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / ii          # (periodic in i with period ii)
        idx = hostinit.step_indices(0, kk)
        mm, nn = idx[2], idx[3]
        g.dia_select("wflx")
        ref = RestatedVfl(case, masks, len(g.dia_levels()))
        for it in range(2):
            for f, mk, amp in (("uflx", "iu", 3.0e6), ("vflx", "iv", 2.0e6)):
                a = g.get(f)
                w = (masks[mk].reshape(nj, ni) > 0).astype(np.float64)
                for k in range(kk):
                    a[nn + k] = amp * (1 + it) * np.cos(x * (1 + k % 3) + k + it) * (1.0 + y) * w / (1.0 + k)
                g.put(f, a)
            a = g.get("dpold")
            a[mm:mm + kk] = g.get("dp")[mm:mm + kk] * (1.0 + 1.0e-3 * (1 + it) * np.sin(x + 3.0 * y))[None]
            g.put("dpold", a)
            before = {nm: g.dia_get(nm) for nm in ("uflxlvl", "vflxlvl")}
            g.diaacc(*idx)
            snap = snapshot(g, 0, kk, before)
            check_exchange_and_copy(case, before, g, snap)
            ref.accumulate(snap)
        assert g.dia_nacc() == 2
        got = {nm: g.dia_get(nm) for nm in NAMES}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        for nm in NAMES:
            assert (np.abs(got[nm]) > 0.0).any(), nm
        assert all(ref.seen["dp_moved"])
    finally:
        g.close()


def test_hybrid_coordinate():
    check_hybrid()
