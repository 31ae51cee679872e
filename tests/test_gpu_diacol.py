"""diaacc's column-derived diagnostics on the device (k_diacol, k_diapv, blom_amd/csrc/stage_diaacc.hip; k_cmn_mldl82<DIAG>,
stage_cmnfld.hip): sbot tbot t20d t17d mldl82 mldl82mn mldl82mx mldl82sq (2-D) and avdsg dpvor (kdm layers).

The expected values are the reference's loops restated in numpy below (RestatedCol): phy/mod_dia.F90:1251-1294 (the bottom values),
:1296-1366 (the isotherm depths), phy/mod_cmnfld_routines.F90:943-984 (mldl82, with the rho of tests/test_cmnfld.py), :1203-1234
(the potential vorticity pair), then acch2d / minh2d / maxh2d / sqh2d / acclyr.  Every point sees the reference's operations in the
reference's order in float64 (numpy does not contract; max / min are `a > b ? a : b` / `a < b ? a : b`, as amdflang lowers them).  The
restatement is applied over the whole padded arrays to what a second, single-stepping context downloads after each of its steps --
p temp saln dp z dz sigma absvor dpvor and the masks; the context under test takes its steps in ONE call.  Everything is compared
with ==, byte for byte over the whole padded array: inival*mask everywhere outside the owned masked points.

The reference leaves kup undefined where an isotherm walk ends below the first layer with nothing but massless layers above it; the
device starts kup at 1 there, the restatement does the same, and the tests assert that no owned column of theirs is of that kind.

absvor and dpvor are no pinned state (tests/parity.py: STATE_FIELDS does not hold them): check_pin compares the device's with the
compiled reference's at every q-point a wet owned p-point touches, both sides starting from the reference's arrays (the land
q-points momtum never writes keep the reference's initial spval).

tests/test_hostemu_diacol.py runs the same checks on the host emulation of the library."""
import contextlib

import numpy as np
import pytest

from blom_amd import hostinit
from blom_amd.cases import default_grid, make_case
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import full_context, dyncore_context, same_bytes, differing
from test_cmnfld import rho

pytestmark = pytest.mark.gpu

ONEM, ONECM, ONEMM, EPSILP, SPVAL, GRAV = 9806.0, 98.06, 9.806, 1.0e-12, 1.0e33, 9.806
DBCL82 = 0.0003                       # phy/mod_cmnfld_routines.F90: dbcl82
EPSIL = 1.0e-11                       # finlyr, :6126
FILL = 9.9692099683868690e+36         # nf90_fill_double
COL2D = "sbot tbot t20d t17d".split()
ML = "mldl82 mldl82mn mldl82mx mldl82sq".split()
PV = "avdsg dpvor".split()
NAMES2D = COL2D + ML
NAMES = NAMES2D + PV
INIVAL = dict(mldl82mn=SPVAL, mldl82mx=-SPVAL)                    # :5900-5901; 0. otherwise

_LAYER_ADMITTED = lyr.admitted


def fmax(a, b):
    return np.where(a > b, a, b)


def fmin(a, b):
    return np.where(a < b, a, b)


class RestatedCol:
    """the ten accumulators of one tile"""

    def __init__(self, case, masks):
        self.case, self.kk = case, case.kdm
        ii, jj = case.idm, case.jdm
        nj, ni = jj + 8, ii + 8
        self.shape = (nj, ni)
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + jj, 4:4 + ii] = True
        self.sel = own & (self.mask["p"] > 0)                     # do j = 1,jj; do l = 1,isp(j); do i = max(1,ifp),min(ii,ilp)
        iu, iv = (self.mask["u"] > 0).astype(np.int64), (self.mask["v"] > 0).astype(np.int64)
        z = np.zeros((nj, ni))
        self.corner = {}
        for nm, a in (("sw", np.minimum(1, iu[:-1, :-1] + iv[:-1, :-1])), ("se", np.minimum(1, iu[:-1, 1:] + iv[:-1, :-1])),
                      ("nw", np.minimum(1, iu[:-1, :-1] + iv[1:, :-1])), ("ne", np.minimum(1, iu[:-1, 1:] + iv[1:, :-1]))):   # :1208-1211
            self.corner[nm] = z.copy()
            self.corner[nm][:-1, :-1] = a
        self.seen = dict(bot_many=0, bot_last=0, thin=0, iso={20.0: dict(first=0, none=0, interp=0, skipped=0, kup_undefined=0),
                                                              17.0: dict(first=0, none=0, interp=0, skipped=0, kup_undefined=0)},
                         ml_found=0, ml_none=0, dsig=[0, 0, 0])
        self.reset()

    def reset(self):
        self.acc = {}
        for nm in NAMES:
            plane = np.float64(INIVAL.get(nm, 0.0)) * self.mask["p"].astype(np.float64)      # inih2d / inilyr over the whole padded plane
            self.acc[nm] = np.repeat(plane[None], self.kk if nm in PV else 1, axis=0).copy()
        self.nacc = 0

    # ---- the derived fields of one step ----
    def bottom(self, s):
        """:1256-1292"""
        kk, sel = self.kk, self.sel
        p, temp, saln = s["p"], s["temp"], s["saln"]
        sb, tb, dps = (np.zeros(self.shape) for _ in range(3))
        nq = np.zeros(self.shape, np.int64)
        lim = p[kk] - ONEM                                          # p(kk+1) - dpbot
        for k in range(kk):
            q = fmax(0.0, p[k + 1] - fmax(lim, p[k]))
            sb = sb + saln[k] * q
            tb = tb + temp[k] * q
            dps = dps + q
            nq += q > 0.0
            last = q
        thick = dps > ONEMM
        q = 1.0 / dps
        sb, tb = np.where(thick, sb * q, saln[0]), np.where(thick, tb * q, temp[0])
        self.seen["bot_many"] += int((sel & (nq > 1)).sum())
        self.seen["bot_last"] += int((sel & (nq == 1) & (last > 0.0)).sum())
        self.seen["thin"] += int((sel & ~thick).sum())
        return sb, tb

    def isotherm(self, s, tx):
        """:1301-1325 | :1337-1361"""
        kk, sel = self.kk, self.sel
        temp, dp, z, dz = s["temp"], s["dp"], s["z"], s["dz"]
        going = np.ones(self.shape, bool)
        kup, ke = np.ones(self.shape, np.int64), np.zeros(self.shape, np.int64)
        moved, skipped = np.zeros(self.shape, bool), np.zeros(self.shape, bool)
        for k in range(kk):
            thick, warm = dp[k] > ONECM, temp[k] > tx
            skipped |= going & ~thick & moved                      # a massless layer below a warm one, the walk still going
            up = going & thick & warm
            kup[up] = k + 1
            moved |= up
            end = going & thick & ~warm
            ke[end] = k + 1
            going &= ~end
        first, none = ke == 1, ke == 0
        interp = ~first & ~none
        iu, ie = (kup - 1)[None], np.maximum(ke - 1, 0)[None]
        pick = lambda a, i: np.take_along_axis(a, i, axis=0)[0]
        zup = pick(z, iu) + 0.5 * pick(dz, iu)
        zlo = pick(z, ie) + 0.5 * pick(dz, ie)
        tup = pick(temp, iu)
        tlo = fmin(pick(temp, ie), tup - EPSILP)
        d = np.where(first, 0.0, np.where(none, z[kk], (zup * (tlo - tx) + zlo * (tx - tup)) / (tlo - tup)))
        b = self.seen["iso"][tx]
        b["first"] += int((sel & first).sum())
        b["none"] += int((sel & none).sum())
        b["interp"] += int((sel & interp).sum())
        b["skipped"] += int((sel & interp & skipped).sum())
        b["kup_undefined"] += int((sel & interp & ~moved).sum())
        return d

    def mldl82(self, s):
        """phy/mod_cmnfld_routines.F90:943-984"""
        kk, sel = self.kk, self.sel
        p, temp, saln, dp, z, dz = s["p"], s["temp"], s["saln"], s["dp"], s["z"], s["dz"]
        zup = z[0] + 0.5 * dz[0]
        dbup = np.zeros(self.shape)
        going = np.ones(self.shape, bool)
        out = np.zeros(self.shape)
        for k in range(1, kk):
            thick = dp[k] > ONECM
            plo = p[k] + 0.5 * dp[k]
            zlo = z[k] + 0.5 * dz[k]
            dblo = GRAV * (1.0 - rho(plo, temp[0], saln[0]) / rho(plo, temp[k], saln[k]))
            below = going & thick & ~(dblo <= DBCL82)
            db = fmin(dbup, DBCL82 - EPSILP)
            val = (zup * (dblo - DBCL82) + zlo * (DBCL82 - db)) / (dblo - db) - z[0]
            out[below] = val[below]
            inside = going & thick & (dblo <= DBCL82)
            zup, dbup = np.where(inside, zlo, zup), np.where(inside, dblo, dbup)
            going &= ~below
        out[going] = (z[kk] - z[0])[going]
        self.seen["ml_found"] += int((sel & ~going).sum())
        self.seen["ml_none"] += int((sel & going).sum())
        return out

    def pv(self, s):
        """:1218-1234"""
        kk, sel = self.kk, self.sel
        sg, av, dv = s["sigma"], s["absvor"], s["dpvor"]
        c = self.corner
        t1, t2 = np.zeros((kk,) + self.shape), np.zeros((kk,) + self.shape)

        def corners(a):
            return ((a[:-1, :-1] * c["sw"][:-1, :-1] + a[:-1, 1:] * c["se"][:-1, :-1]) + a[1:, :-1] * c["nw"][:-1, :-1]) + a[1:, 1:] * c["ne"][:-1, :-1]
        for k in range(kk):
            if k + 1 <= 2:
                dsig, case = fmax(0.0, sg[1] - sg[0]), 0
            elif k + 1 == kk:
                dsig, case = fmax(0.0, sg[k] - fmax(sg[k - 1], sg[1])), 1
            else:
                dsig, case = 0.5 * fmax(0.0, sg[k + 1] - fmax(sg[k - 1], sg[1])), 2
            t1[k][:-1, :-1] = corners(av[k]) * dsig[:-1, :-1]
            t2[k][:-1, :-1] = corners(dv[k])
            self.seen["dsig"][case] += int((sel & (t1[k] != 0.0)).sum())
        return t1, t2

    def accumulate(self, s):
        """s: p (kk+1 planes), temp saln dp sigma (kk planes at k + mm), z (kk+1), dz (kk), absvor dpvor (planes 1..kk).  Returns the
        restated mldl82."""
        sel, a = self.sel, self.acc
        self.nacc += 1
        with np.errstate(all="ignore"):
            sb, tb = self.bottom(s)
            ml = self.mldl82(s)
            t1, t2 = self.pv(s)
            fld = dict(sbot=sb, tbot=tb, t20d=self.isotherm(s, 20.0), t17d=self.isotherm(s, 17.0), mldl82=ml)
            for nm, f in fld.items():
                a[nm][0][sel] = (a[nm][0] + f)[sel]                                 # acch2d, :5256
            a["mldl82mn"][0][sel] = fmin(a["mldl82mn"][0], ml)[sel]               # minh2d, :5392
            a["mldl82mx"][0][sel] = fmax(a["mldl82mx"][0], ml)[sel]               # maxh2d, :5330
            a["mldl82sq"][0][sel] = (a["mldl82sq"][0] + ml * ml)[sel]             # sqh2d, :5454
            a["avdsg"][:, sel] = (a["avdsg"] + t1)[:, sel]                         # acclyr, :5500
            a["dpvor"][:, sel] = (a["dpvor"] + t2)[:, sel]
        return ml

    def finalized(self):
        """finlyr(ACC_AVDSG, ACC_DPVOR, 'p'), :2608, :6137-6141"""
        with np.errstate(all="ignore"):
            out = self.acc["avdsg"].copy()
            out[:, self.sel] = np.where(self.acc["dpvor"] > EPSIL, self.acc["avdsg"] / self.acc["dpvor"], FILL)[:, self.sel]
        return out


def snapshot(gpu, idx, kk):
    m, n, mm, nn, k1m, k1n = idx
    s = dict(p=gpu.get("p"), z=gpu.get("z"), dz=gpu.get("dz"), absvor=gpu.get("absvor")[:kk].copy(), dpvor=gpu.get("dpvor")[:kk].copy())
    for nm in ("temp", "saln", "dp", "sigma"):
        s[nm] = gpu.get(nm)[mm:mm + kk].copy()
    s["mldl82_dev"] = gpu.get("mldl82")[0]
    return s


def single_step(b, case, ns, ref):
    assert b.step(ns, 1) == ns + 1
    snap = snapshot(b, hostinit.step_indices(ns, case.kdm), case.kdm)
    ml = ref.accumulate(snap)
    # the device field under isopyc_bulkml, formed for the diagnostics alone (phy/mod_cmnfld_routines.F90:1109-1113)
    assert same_bytes(snap["mldl82_dev"][ref.sel], ml[ref.sel]), f"the device field mldl82 differs from :943-984 after step {ns + 1}"
    return snap


def copy_seen(seen):
    return dict(seen, iso={k: dict(v) for k, v in seen["iso"].items()}, dsig=list(seen["dsig"]))


# ---- one run per (case, grid), shared ---------------------------------------------------------------------------------------------
_RUNS = {}
CASES = ["chan_s_tke", "box_s", "tri_s_tke"]
EXTENDED = {"chan_s_tke"}


def col_run(cfg, grid=None):
    """Context B: the ten names selected, single steps; after each the restatement is fed.  Four steps give E4.
    Context A: the ten names plus the layer table, step(0, 4) in ONE call; finalize; (extended) two steps, reset, two steps.
    (extended) B selects afresh and takes two more single steps (E8 on a fresh restatement); context C: A's selection without the
    ten names, step(0, 4)."""
    key = (cfg, grid)
    if key in _RUNS:
        return _RUNS[key]
    extended = cfg in EXTENDED and grid is None
    r = {}
    with default_grid(grid) if grid else contextlib.nullcontext():
        case, masks, b = full_context(cfg)
    a = None
    try:
        with default_grid(grid) if grid else contextlib.nullcontext():
            lnames = lyr.admitted(case)
            r.update(case=case, masks=masks, lnames=lnames)
            b.dia_select(NAMES)
            ref = RestatedCol(case, masks)
            r["init"] = {nm: v.copy() for nm, v in ref.acc.items()}
            r["B0"] = {nm: b.dia_get(nm) for nm in NAMES}
            r["temp_max"] = -1.0e30
            for ns in range(4):
                snap = single_step(b, case, ns, ref)
                r["temp_max"] = max(r["temp_max"], float(snap["temp"][:, ref.sel].max()))
            r["E4"] = {nm: v.copy() for nm, v in ref.acc.items()}
            r["E4_fin"] = ref.finalized()
            r["B4_own"] = {nm: b.dia_get(nm) for nm in NAMES}
            r["B4_nacc"] = b.dia_nacc()
            r["seen"] = copy_seen(ref.seen)
            r["corner"] = ref.corner
            _, _, a = full_context(cfg)
            a.dia_select(NAMES + lnames)
            assert a.step(0, 4) == 4
            r["A4"] = {nm: a.dia_get(nm) for nm in NAMES}
            r["A4_nacc"] = a.dia_nacc()
            r["A4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
            r["A4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
            a.dia_finalize()
            r["A4_fin"] = {nm: a.dia_get(nm) for nm in NAMES}
            if extended:
                for ns in range(4, 6):
                    single_step(b, case, ns, ref)
                r["E6"] = {nm: v.copy() for nm, v in ref.acc.items()}
                assert a.step(4, 2) == 6
                a.dia_reset()
                r["A_reset"] = {nm: a.dia_get(nm) for nm in NAMES}
                r["A_reset_nacc"] = a.dia_nacc()
                assert a.step(6, 2) == 8
                r["A8"] = {nm: a.dia_get(nm) for nm in NAMES}
                r["A8_nacc"] = a.dia_nacc()
                b.dia_select(NAMES)                                     # afresh
                fresh = RestatedCol(case, masks)
                for ns in range(6, 8):
                    single_step(b, case, ns, fresh)
                r["B8"] = {nm: b.dia_get(nm) for nm in NAMES}
                r["E8"] = fresh.acc
                a.close()
                _, _, a = full_context(cfg)                             # C
                a.dia_select(lnames)
                assert a.step(0, 4) == 4
                r["C4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
                r["C4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
    finally:
        if a is not None:
            a.close()
        b.close()
    _RUNS[key] = r
    return r


def owned_wet(r):
    nj, ni = r["case"].jdm + 8, r["case"].idm + 8
    sel = np.zeros((nj, ni), bool)
    sel[4:-4, 4:-4] = True
    return sel & (r["masks"]["ip"].reshape(nj, ni) > 0)


# ---- 1. the step accumulates what the loops would ----------------------------------------------------------------------------------
def check_step_accumulates(cfg, grid=None):
    r = col_run(cfg, grid)
    assert r["A4_nacc"] == 4 and r["B4_nacc"] == 4
    assert not differing(r["B0"], r["init"]), differing(r["B0"], r["init"])        # fresh slots: inival*mask
    bad = differing(r["A4"], r["E4"])
    assert not bad, f"{cfg}: four steps in one call differ from the restated loops: {bad}"
    bad = differing(r["B4_own"], r["E4"])
    assert not bad, f"{cfg}: the single-stepping context's own accumulators differ from the restated loops: {bad}"
    sel = owned_wet(r)
    for nm in NAMES:
        assert same_bytes(r["A4"][nm][:, ~sel], r["init"][nm][:, ~sel]), nm       # inival*mask everywhere else
    assert r["seen"]["iso"][20.0]["kup_undefined"] == 0 and r["seen"]["iso"][17.0]["kup_undefined"] == 0


@pytest.mark.parametrize("cfg", CASES)
def test_step_accumulates_what_the_reference_loops_would(cfg):
    check_step_accumulates(cfg)


def test_step_accumulates_on_the_warped_grid():
    check_step_accumulates("chan_s_tke", "warped_eq")


# ---- 2. the tests are not vacuous ------------------------------------------------------------------------------------------------------
def check_not_vacuous(cfg):
    r = col_run(cfg)
    seen, e = r["seen"], r["E4"]
    print(cfg, "seen:", seen, "max temp:", r["temp_max"])
    # sbot / tbot: a bottom onem that spans more than one layer, and one that lies in the last layer alone
    assert seen["bot_many"] > 0 and seen["bot_last"] > 0, seen
    assert (np.abs(e["sbot"]) > 0.0).any() and (np.abs(e["tbot"]) > 0.0).any()
    # mldl82: the search found the depth somewhere (the other exit: check_prepared_columns), and the depth moves
    assert seen["ml_found"] > 0, seen
    assert (e["mldl82mn"] < e["mldl82mx"]).any(), "mldl82mn < mldl82mx nowhere after four steps"
    assert (e["mldl82"] > 0.0).any() and (e["mldl82sq"] > 0.0).any()
    # avdsg: non-zero in each of the three cases of dsig
    assert all(n > 0 for n in seen["dsig"]), seen["dsig"]
    assert (e["avdsg"] != 0.0).any() and (e["dpvor"] > 0.0).any()
    if cfg == "box_s":
        c, sel = r["corner"], owned_wet(r)
        lo = np.minimum.reduce([c[k] for k in c])
        hi = np.maximum.reduce([c[k] for k in c])
        assert (sel & (lo == 0.0) & (hi == 1.0)).any(), "no wet point with one corner masked and another not"


@pytest.mark.parametrize("cfg", CASES)
def test_the_cases_exercise_the_loops(cfg):
    check_not_vacuous(cfg)


# ---- 3. prepared columns: the cases' own temperatures never reach 20 degC ------------------------------------------------------------
def prepared_columns(r):
    """three owned wet columns in a row of the case's interior, a layer apart from each other"""
    sel = owned_wet(r)
    jj = 4 + r["case"].jdm // 2
    cols = [i for i in range(4, 4 + r["case"].idm) if sel[jj, i]]
    assert len(cols) >= 5
    return jj, cols[0], cols[2], cols[4]


def check_prepared_columns(cfg="chan_s_tke"):
    r = col_run(cfg)
    assert r["temp_max"] < 20.0, "the case reaches 20 degC by itself"
    case, masks, g = full_context(cfg)
    try:
        kk = case.kdm
        assert kk >= 5
        g.dia_select(NAMES2D)
        assert g.step(0, 2) == 2
        idx = hostinit.step_indices(1, kk)
        mm = idx[2]
        jj, i1, i2, i3 = prepared_columns(r)
        temp, saln, dp = g.get("temp"), g.get("saln"), g.get("dp")
        # an offset that carries the upper layers above 20 degC and leaves the deep ones below 17
        sel = owned_wet(r)
        # (the case's temperature varies more along the channel than down the column: the offset goes linearly from the one that
        # lifts the coldest surface point to 21 degC to the one that leaves the warmest bottom point at 16)
        top, deep = 21.0 - float(temp[mm][sel].min()), 16.0 - float(temp[mm + kk - 1][sel].max())
        for k in range(kk):
            temp[mm + k] += top + (deep - top) * k / (kk - 1)
        assert (temp[mm][sel] > 20.0).all() and (temp[mm + kk - 1][sel] < 17.0).all()
        temp[mm, jj, i1] = 16.5                                          # 1: a surface layer <= 17
        temp[mm:mm + kk, jj, i2] = 25.0                                  # 2: every layer above 20 -- and homogeneous: mldl82's k > kk exit
        saln[mm:mm + kk, jj, i2] = 35.0
        temp[mm:mm + kk, jj, i3] = [25.0, 24.0, 23.0] + [5.0 - 0.5 * k for k in range(kk - 3)]      # 3: a massless layer between warm and cold
        dp[mm:mm + kk, jj, i3] = dp[mm:mm + kk, jj, i3].sum() / (kk - 1)
        dp[mm + 2, jj, i3] = 0.0
        g.put("temp", temp)
        g.put("saln", saln)
        g.put("dp", dp)
        g.dia_reset()
        g.stage("cmnfld1", *idx)
        g.diaacc(*idx)
        assert g.dia_nacc() == 1
        ref = RestatedCol(case, masks)
        snap = snapshot(g, idx, kk)
        ml = ref.accumulate(snap)
        assert same_bytes(snap["mldl82_dev"][ref.sel], ml[ref.sel])
        got = {nm: g.dia_get(nm) for nm in NAMES2D}
        want = {nm: ref.acc[nm] for nm in NAMES2D}
        assert not differing(got, want), differing(got, want)
        print("prepared columns:", ref.seen)
        for tx in (20.0, 17.0):
            b = ref.seen["iso"][tx]
            assert b["first"] > 0 and b["none"] > 0 and b["interp"] > 0 and b["skipped"] > 0 and b["kup_undefined"] == 0, (tx, b)
        assert ref.seen["ml_none"] > 0 and ref.seen["ml_found"] > 0, ref.seen
        # the three columns ended where they were meant to
        for nm in ("t20d", "t17d"):
            assert got[nm][0, jj, i1] == 0.0 and got[nm][0, jj, i2] == snap["z"][kk, jj, i2] and 0.0 < got[nm][0, jj, i3] < snap["z"][kk, jj, i3], nm
        assert got["mldl82"][0, jj, i2] == snap["z"][kk, jj, i2] - snap["z"][0, jj, i2]
    finally:
        g.close()


def test_prepared_columns_take_every_outcome_of_the_isotherm_walk():
    check_prepared_columns()


# ---- 4. interface -------------------------------------------------------------------------------------------------------------------
def check_interface():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)
    try:
        kk = case.kdm
        nj, ni = case.jdm + 8, case.idm + 8
        full, ext = g.dia_names_full(), g.dia_names_ext()
        assert len(g.dia_names()) == 111 and len(g.dia_names_all()) == 117 and len(full) == 123 and len(ext) == 133
        assert ext[:123] == full
        assert ext[123:] == [(nm, 0, "p") for nm in NAMES2D] + [(nm, 1, "p") for nm in PV]
        ipm = masks["ip"].reshape(nj, ni).astype(np.float64)
        for one in PV:                                                # either of the pair selects both
            g.dia_select(one)
            for nm in PV:
                got = g.dia_get(nm)
                assert got.shape == (kk, nj, ni) and same_bytes(got, np.repeat((0.0 * ipm)[None], kk, axis=0)), (one, nm)
            with pytest.raises(BlomGpuError, match="sbot"):
                g.dia_get("sbot")
        g.dia_select(NAMES2D)
        for nm in NAMES2D:                                            # fresh slots: 0*mask, +spval*mask, -spval*mask
            got = g.dia_get(nm)
            assert got.shape == (1, nj, ni) and same_bytes(got[0], np.float64(INIVAL.get(nm, 0.0)) * ipm), nm
        land = ipm == 0.0
        assert land.any() and not np.signbit(g.dia_get("mldl82mn")[0][land]).any() and np.signbit(g.dia_get("mldl82mx")[0][land]).all()
        with pytest.raises(BlomGpuError, match="avdsg"):
            g.dia_get("avdsg")
        # an unknown name leaves selection and accumulators untouched
        g.dia_select("sbot mldl82mn dpvor temp")
        assert g.step(0, 2) == 2 and g.dia_nacc() == 2
        keep = {nm: g.dia_get(nm) for nm in ("sbot", "mldl82mn", "avdsg", "dpvor", "temp")}
        assert (keep["sbot"] > 0.0).any() and (keep["dpvor"] > 0.0).any() and (keep["mldl82mn"] > 0.0).any()
        with pytest.raises(BlomGpuError, match="nonsense"):
            g.dia_select("t20d nonsense")
        assert all(same_bytes(g.dia_get(nm), v) for nm, v in keep.items()) and g.dia_nacc() == 2
        with pytest.raises(BlomGpuError, match="t20d"):
            g.dia_get("t20d")
        g.dia_select("")
        # the names that need z / dz are refused where the step sequence does not run cmnfld1: at the selection ...
        g.set("cmnfld1", 0)
        for nm in ["t20d", "t17d"] + ML:
            with pytest.raises(BlomGpuError, match=nm):
                g.dia_select("sbot " + nm)
        g.dia_select("sbot tbot avdsg")                                # (these read neither)
        assert g.step(2, 1) == 3
        # ... and again at the step
        g.set("cmnfld1", 1)
        g.dia_select("t17d mldl82sq")
        g.set("cmnfld1", 0)
        with pytest.raises(BlomGpuError, match="t17d mldl82sq"):
            g.step(3, 1)
        g.set("cmnfld1", 1)
        assert g.step(3, 1) == 4
        g.dia_select("")
        # no refusal under the other coordinates: there mldl82 is the field cmnfld1 forms anyway
        g.set("cmnfld1", 0)
        for vc in ("cntiso_hybrid", "plevel"):
            g.set("vcoord_type", vc)
            g.dia_select(NAMES)
            assert g.dia_get("avdsg").shape[0] == kk
        g.dia_select("")
        g.set("vcoord_type", "isopyc_bulkml")
    finally:
        g.close()


def test_interface():
    check_interface()


# ---- 5. independence, finalize, reset ------------------------------------------------------------------------------------------------
def check_independence_finalize_reset():
    r = col_run("chan_s_tke")
    # the ten names change no byte of the other accumulators ...
    bad = [nm for nm in r["lnames"] if not same_bytes(r["A4_lyr"][nm], r["C4_lyr"][nm])]
    assert not bad, bad
    # ... and none of the model state
    bad = [nm for nm in r["C4_state"] if not same_bytes(r["A4_state"][nm], r["C4_state"][nm])]
    assert not bad, bad
    assert all(nm in r["C4_state"] for nm in ["temp", "saln", "dp", "p", "sigma", "u"])
    assert all((np.abs(r["A4_lyr"][nm]) > 0.0).any() for nm in ["temp", "sealv", "maxbld"])
    # finalize: avdsg / dpvor where dpvor > epsil, the fill value elsewhere among the owned wet points; the nine others stay
    assert same_bytes(r["A4_fin"]["avdsg"], r["E4_fin"])
    sel = owned_wet(r)
    assert (r["E4"]["dpvor"][:, sel] > EPSIL).any() and not same_bytes(r["E4_fin"], r["E4"]["avdsg"])
    bad = [nm for nm in NAMES if nm != "avdsg" and not same_bytes(r["A4_fin"][nm], r["E4"][nm])]
    assert not bad, bad
    # reset: every slot back to its own initial value, count 0; the next block equals a fresh selection's
    assert not differing(r["A_reset"], r["init"]), differing(r["A_reset"], r["init"])
    assert r["A_reset_nacc"] == 0
    assert not differing(r["A8"], r["B8"]), differing(r["A8"], r["B8"])
    assert not differing(r["A8"], r["E8"]), differing(r["A8"], r["E8"])
    assert r["A8_nacc"] == 2
    assert (r["A8"]["mldl82mn"][0][sel] < SPVAL).all() and (r["A8"]["mldl82mx"][0][sel] > -SPVAL).all()


def test_independence_finalize_reset():
    check_independence_finalize_reset()


# ---- 6. tiles ---------------------------------------------------------------------------------------------------------------------------
def check_tiles(monkeypatch, npx=2, npy=1):
    """test_gpu_diaacc.check_tiles on a 2x1 and on a 1x2 group with the ten names added to its selection: every tile's slots are its
    window of the single tile's.  The q-points at ii+1 of the first tile of 2x1 are the second tile's column 1, those at jj+1 on 1x2
    the second tile's row 1: this is what decides the corners of absvor and dpvor that momtum leaves in a tile's halo."""
    monkeypatch.setattr(lyr, "admitted", lambda case: _LAYER_ADMITTED(case) + NAMES)
    lyr.check_tiles("chan_s_tke", npx, npy)


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_tiles_accumulate_their_window_of_the_single_tile(monkeypatch, npx, npy):
    check_tiles(monkeypatch, npx, npy)


# ---- 7. the graph option --------------------------------------------------------------------------------------------------------------------
def check_graph_replay(expect_replays):
    r = col_run("chan_s_tke")
    case, masks, g = full_context("chan_s_tke")
    try:
        g.set("use_graph", 1)
        g.dia_select(NAMES)
        assert g.step(0, 6) == 6
        got = {nm: g.dia_get(nm) for nm in NAMES}
        assert not differing(got, r["E6"]), differing(got, r["E6"])
        assert g.dia_nacc() == 6
        if expect_replays:
            assert g.get_real("graph_steps") >= 1, "no step was replayed as a graph"
    finally:
        g.close()


def test_graph_replay_accumulates_the_same_bytes():
    import os
    check_graph_replay(expect_replays=os.environ.get("BLOM_HOSTEMU") != "1")


# ---- 8. the hybrid coordinate -----------------------------------------------------------------------------------------------------------------
def check_hybrid():
    """cntiso_hybrid: cmnfld1 and diaacc as stages of their own (the Fortran host's path), twice, on a state the test puts; mldl82 is
    the field cmnfld1 forms for the mixed layer depth there"""
    case, masks, g = dyncore_context("chan_s", vcoord_type="cntiso_hybrid")
    try:
        kk, ii, jj = case.kdm, case.idm, case.jdm
        nj, ni = jj + 8, ii + 8
        y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / ii
        idx = hostinit.step_indices(0, kk)
        mm = idx[2]
        g.dia_select(NAMES)
        ref = RestatedCol(case, masks)
        for it in range(2):
            for f, amp in (("absvor", 1.0e-4), ("dpvor", 3.0e5)):
                a = g.get(f)
                for k in range(kk):
                    a[k] = amp * (1.0 + 0.3 * np.cos(x * (1 + k % 3) + k + it) * (1.0 + y)) / (1.0 + 0.1 * k)
                g.put(f, a)
            t = g.get("temp")
            t[mm:mm + kk] = t[mm:mm + kk] * (1.0 + 0.02 * (1 + it) * np.sin(x + 3.0 * y))[None]
            g.put("temp", t)
            g.stage("cmnfld1", *idx)
            g.diaacc(*idx)
            snap = snapshot(g, idx, kk)
            ml = ref.accumulate(snap)
            assert same_bytes(snap["mldl82_dev"][ref.sel], ml[ref.sel])
            assert same_bytes(g.get("mld")[0][ref.sel], ml[ref.sel])
        assert g.dia_nacc() == 2
        got = {nm: g.dia_get(nm) for nm in NAMES}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        for nm in ("sbot", "tbot", "mldl82", "mldl82sq", "avdsg", "dpvor"):
            assert (np.abs(got[nm]) > 0.0).any(), nm
    finally:
        g.close()


def test_hybrid_coordinate():
    check_hybrid()


# ---- 9. absvor and dpvor against the compiled reference ---------------------------------------------------------------------------------------
PIN = [("chan_s", None), ("box_s", None), ("tri_s", None), ("chan_s", "warped_eq")]


def check_pin(cfg, grid, nsteps=3):
    """after every step of the dynamical core: planes 1..kk of absvor and dpvor, the device's against the reference's own momtum
    (phy/mod_momtum.F90:477-496), at every q-point a wet owned p-point touches -- (i,j), (i+1,j), (i,j+1), (i+1,j+1): the rim at
    ii+1 and jj+1 is in a halo that nothing exchanges"""
    from oracle.refblom import get_ref_backend, have_ref
    from blom_amd.gpu import BlomGpu
    from blom_amd.stepper import dyncore_step
    from parity import copy_state
    if not have_ref(cfg):
        pytest.skip(f"oracle/_ref/{cfg}/libblomref.so not built")
    with default_grid(grid) if grid else contextlib.nullcontext():
        case = make_case(cfg)
        ref = get_ref_backend(cfg, case.depth)
        hostinit.init_state(ref, case)
        gpu = BlomGpu(case.idm, case.jdm, case.kdm, ref.ntr, ref.nreg, ref.masks)
        try:
            for nm, v in case.params.items():
                if not nm.endswith("0"):
                    gpu.set(nm, v)
            copy_state(ref, gpu)
            for f in ("absvor", "dpvor"):                                # (no state fields: the land q-points momtum never writes keep
                gpu.put(f, ref.get(f))                                   # the reference's initial spval on both sides)
            gpu.set("delt1", case.params["baclin"])
            kk, nj, ni = case.kdm, case.jdm + 8, case.idm + 8
            wet = np.zeros((nj, ni), bool)
            wet[4:4 + case.jdm, 4:4 + case.idm] = True
            wet &= np.asarray(ref.masks["ip"]).reshape(nj, ni) > 0
            touched = np.zeros((nj, ni), bool)
            for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1)):
                touched[dj:nj - 1 + dj, di:ni - 1 + di] |= wet[:-1, :-1]
            rim = touched.copy()
            rim[:4 + case.jdm, :4 + case.idm] = False
            assert rim.any() or cfg == "box_s"                          # (the box is closed: land all along ii and jj)
            ns = 0
            for _ in range(nsteps):
                ns = dyncore_step(ref, ns, case.params["baclin"])
                assert gpu.step(ns - 1, 1) == ns
                for f in ("absvor", "dpvor"):
                    a, b = ref.get(f)[:kk], gpu.get(f)[:kk]
                    inner = same_bytes(a[:, touched & ~rim], b[:, touched & ~rim])
                    outer = same_bytes(a[:, rim], b[:, rim])
                    assert inner and outer, f"{cfg} {grid} step {ns}: {f} differs from the reference's: interior {'equal' if inner else 'DIFFERS'}, rim ii+1 / jj+1 {'equal' if outer else 'DIFFERS'}"
                    assert (np.abs(b[:, rim]) > 0.0).any() or cfg == "box_s", f
        finally:
            gpu.close()


@pytest.mark.parametrize("cfg,grid", PIN)
def test_absvor_and_dpvor_equal_the_compiled_reference(cfg, grid):
    check_pin(cfg, grid)
