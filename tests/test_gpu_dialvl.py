"""diaacc's z-level (Levitus) accumulators on the device (k_dialvl, blom_amd/csrc/stage_diaacc.hip).

The expected values are the reference's loops restated in numpy below: diazlv (phy/mod_dia.F90:4737-4993) with its carried ind1, its
`cycle` and `exit`, k outer and the columns vectorised; acclvl (:5709-5781) over ind1..ind2 with the weights diazlv stored; msklvl
(:6659-6738); inilvl (:5117-5178); the calls of diaacc (:2000-2053, :2119-2168, :2222-2271).  The same operations in the same order in
float64, applied to the arrays a second context downloads after each of its steps.  The restatement does NOT use the kernel's
reformulation (a layer reaches a level iff two comparisons hold); it walks the levels as the reference does.  Everything is compared
with ==, byte for byte over the whole padded array.

tests/test_hostemu_dialvl.py runs the small cases on the host emulation of the library."""
import numpy as np
import pytest

from blom_amd import hostinit
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import full_context, dyncore_context, same_bytes, differing

pytestmark = pytest.mark.gpu

EPSILP = 1.0e-12                      # phy/mod_constants.F90:43
DZEPS, DPEPS, FLXEPS = 1e1 * EPSILP, 1e5 * EPSILP, 1e5 * EPSILP      # :4760-4762
FILL = 9.9692099683868690e+36         # nf90_fill_double
MAXLEV = 128                          # the library's stated cap on ddm (include/blomgpu.h)

# depthslev_bnds (:119-128; LEVITUS2X :142-159) as the edges e[0..ddm]: bnds(1,d) = e[d-1], bnds(2,d) = e[d]
EDGES35 = [0.0, 5.0, 15.0, 25.0, 40.0, 62.5, 87.5, 112.5, 137.5, 175.0, 225.0, 275.0, 350.0, 450.0, 550.0, 650.0, 750.0, 850.0, 950.0,
           1050.0, 1150.0, 1250.0, 1350.0, 1450.0, 1625.0, 1875.0, 2250.0, 2750.0, 3250.0, 3750.0, 4250.0, 4750.0, 5250.0, 5750.0,
           6250.0, 8000.0]
EDGES70 = [0.0, 2.5, 7.5, 12.5, 17.5, 22.5, 27.5, 35.0, 45.0, 56.2, 68.8, 81.2, 93.8, 106.2, 118.8, 131.2, 143.8, 162.5, 187.5, 212.5,
           237.5, 262.5, 287.5, 325.0, 375.0, 425.0, 475.0, 525.0, 575.0, 625.0, 675.0, 725.0, 775.0, 825.0, 875.0, 925.0, 975.0,
           1025.0, 1075.0, 1125.0, 1175.0, 1225.0, 1275.0, 1325.0, 1375.0, 1425.0, 1475.0, 1562.5, 1687.5, 1812.5, 1937.5, 2125.0,
           2375.0, 2625.0, 2875.0, 3125.0, 3375.0, 3625.0, 3875.0, 4125.0, 4375.0, 4625.0, 4875.0, 5125.0, 5375.0, 5625.0, 5875.0,
           6125.0, 6375.0, 6625.0, 8000.0]
COARSE = [0.0, 50.0, 300.0, 700.0, 8000.0]


def bnds_of(edges):
    e = np.asarray(edges, dtype=np.float64)
    return np.stack([e[:-1], e[1:]], axis=1)


# ---- the table, restated from diaacc's calls: name -> (grid, layer-table source, flux weights?) -----------------------------------
_UF = "uflx utflx usflx umfltd umflsm utfltd utflsm utflld usfltd usflsm usflld".split()
LVL = {"uvellvl": ("u", "uvel", False)}
LVL.update({nm + "lvl": ("u", nm, True) for nm in _UF})
LVL["vvellvl"] = ("v", "vvel", False)
LVL.update({"v" + nm[1:] + "lvl": ("v", "v" + nm[1:], True) for nm in _UF})
LVL.update({nm + "lvl": ("p", nm, False) for nm in "saln temp bfsq difint difiso difdia tke gls_psi dz".split()})
HYBRID_REFUSED = "uvellvl vvellvl salnlvl templvl".split()
CHANNEL_SET = "templvl salnlvl uvellvl vvellvl uflxlvl vflxlvl utflxlvl vtflxlvl usflxlvl vsflxlvl difdialvl difisolvl dzlvl".split()


_LAYER_ADMITTED = lyr.admitted


def admitted_lvl(case):
    ok = set(_LAYER_ADMITTED(case))
    return [nm for nm, r in LVL.items() if r[1] in ok]


def fmax(a, b):
    return np.where(a > b, a, b)         # MAX as amdflang lowers it


def fmin(a, b):
    return np.where(a < b, a, b)


class RestatedLvl:
    """phylvl of the selected names on one tile; `strict` overrides the comparisons of a grid (test 3 only)"""

    def __init__(self, case, masks, names, depths, bnds):
        self.case, self.names, self.kk = case, list(names), case.kdm
        self.bnds = np.asarray(bnds, dtype=np.float64)
        self.ddm = len(self.bnds)
        nj, ni = case.jdm + 8, case.idm + 8
        self.shape = (nj, ni)
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + case.jdm, 4:4 + case.idm] = True
        self.own = own
        self.cols = {g: np.flatnonzero((own & (self.mask[g] > 0)).ravel()) for g in "puv"}
        d = np.asarray(depths, dtype=np.float64).reshape(nj, ni)
        # pbath, ubath, vbath: :1074-1091
        self.bath = {"p": d, "u": fmin(d, np.roll(d, 1, axis=1)), "v": fmin(d, np.roll(d, 1, axis=0))}
        self.nacc = 0
        self.cover = {g: dict(a=0, b=0, c=0, d=0) for g in "puv"}
        self.visits = {}                                            # grid -> set of (k, d) at the watched column
        self.watch = {}
        self.reset()

    def reset(self):
        self.acc = {nm: np.repeat((0.0 * self.mask[LVL[nm][0]].astype(np.float64))[None], self.ddm, axis=0).copy() for nm in self.names}
        self.nacc = 0

    def diazlv_columns(self, g, thick, cond_src, strict=None):
        """diazlv for all k of one grid on the compressed columns: yields (k, ind1, ind2, weights, weightsflx) per layer with 0-based,
        inclusive ind1..ind2 (ind2 < ind1: nothing).  thick[k], cond_src[k] are the columns' dp|dpu|dpv(k+mm), dp(km)|flx(kn)."""
        kk, ddm, lo, hi = self.kk, self.ddm, self.bnds[:, 0], self.bnds[:, 1]
        strict = (g != "p") if strict is None else strict
        bath = self.bath[g].ravel()[self.cols[g]]
        nc = len(bath)
        dlev = np.stack([fmax(np.float64(DZEPS), fmin(bath, hi[d]) - lo[d]) for d in range(ddm)])          # :4776-4789
        zbot = np.empty((kk, nc))
        zbot[0] = thick[0] if g == "p" else fmax(thick[0], np.float64(DPEPS))
        for kl in range(1, kk):
            zbot[kl] = zbot[kl - 1] + (thick[kl] if g == "p" else fmax(thick[kl], np.float64(DPEPS)))
        ztop = np.zeros((kk, nc))
        with np.errstate(all="ignore"):
            zbot[0] = zbot[0] * bath / zbot[kk - 1]
            for kl in range(1, kk):                                 # zbot(kk) is still the total until its own turn
                zbot[kl] = zbot[kl] * bath / zbot[kk - 1]
                ztop[kl] = zbot[kl - 1]
        self.zbot = zbot
        ind1 = np.zeros(nc, np.int64)
        failed = np.zeros(nc, bool)
        fed = np.zeros((ddm, nc), np.int32)
        cv = self.cover[g]
        wcol = self.watch.get(g)
        for k in range(kk):
            cond = (cond_src[k] > DPEPS) if g == "p" else (np.abs(cond_src[k]) > FLXEPS)
            cv["c"] += int((failed & cond).any())
            failed |= ~cond
            ind2 = np.full(nc, -1, np.int64)
            w = np.zeros((ddm, nc))
            wf = np.zeros((ddm, nc))
            inloop = np.flatnonzero(cond)
            d0 = int(ind1[inloop].min()) if len(inloop) else ddm
            with np.errstate(all="ignore"):
                for d in range(d0, ddm):
                    if not len(inloop):
                        break
                    c = inloop[ind1[inloop] <= d]                   # do d = ind1(i,j), ddm
                    zt, zb = ztop[k, c], zbot[k, c]
                    skip = (hi[d] < zt) if strict else (hi[d] <= zt)
                    ind1[c[skip]] = d + 1                           # cycle
                    cv["d"] += int(skip.any())
                    c, zt, zb = c[~skip], zt[~skip], zb[~skip]
                    out = (lo[d] > zb) if strict else (lo[d] >= zb)
                    inloop = np.setdiff1d(inloop, c[out], assume_unique=True)       # exit
                    c, zt, zb = c[~out], zt[~out], zb[~out]
                    ind2[c] = d
                    r = fmin(zb, hi[d]) - fmax(zt, lo[d])
                    w[d, c] = r / dlev[d, c]
                    wf[d, c] = r / (zb - zt)
                    fed[d, c] += 1
                    if wcol is not None and wcol in c:
                        self.visits.setdefault(g, set()).add((k, d))
            cv["a"] += int(((ind2 - ind1 + 1 >= 3) & (ind2 >= 0)).any())
            yield k, ind1.copy(), ind2, w, wf
        cv["b"] += int((fed >= 2).any())

    def accumulate(self, gpu, nstep, strict=None):
        kk = self.kk
        m, n, mm, nn, k1m, k1n = hostinit.step_indices(nstep, kk)
        get = {}

        def fld(name):
            if name not in get:
                get[name] = gpu.get(name).reshape(-1, self.shape[0] * self.shape[1])
            return get[name]

        def source(g, f):
            c = self.cols[g]
            if f == "uvel":
                return fld("u")[mm:mm + kk][:, c] + fld("ub")[m - 1][None, c]          # :1180
            if f == "vvel":
                return fld("v")[mm:mm + kk][:, c] + fld("vb")[m - 1][None, c]          # :1195
            if f in ("tke", "gls_psi"):
                it = self.case.params["itrtke" if f == "tke" else "itrgls"]
                o = (it - 1) * 2 * kk + mm
                return fld("trc")[o:o + kk][:, c]
            if f in ("saln", "temp"):
                return fld(f)[mm:mm + kk][:, c]
            if f in ("bfsq", "difint", "difiso", "difdia", "dz"):
                return fld("bfsql" if f == "bfsq" else f)[0:kk][:, c]
            return fld(f)[nn:nn + kk][:, c]                                             # the fluxes, k1n
        self.nacc += 1
        for g, tname, cname, clev in (("u", "dpu", "uflx", nn), ("v", "dpv", "vflx", nn), ("p", "dp", "dp", mm)):
            names = [nm for nm in self.names if LVL[nm][0] == g]
            if not names:
                continue
            c = self.cols[g]
            src = {nm: source(g, LVL[nm][1]) for nm in names}
            a = {nm: self.acc[nm].reshape(self.ddm, -1)[:, c] for nm in names}
            st = None if strict is None else strict.get(g)
            for k, ind1, ind2, w, wf in self.diazlv_columns(g, fld(tname)[mm:mm + kk][:, c], fld(cname)[clev:clev + kk][:, c], st):
                if (ind2 < 0).all():
                    continue
                for nm in names:                                    # acclvl: do d = ind1, ind2
                    ww = wf if LVL[nm][2] else w
                    for d in range(int(ind1.min()), int(ind2.max()) + 1):
                        t = np.flatnonzero((ind1 <= d) & (d <= ind2))
                        with np.errstate(all="ignore"):
                            a[nm][d, t] = a[nm][d, t] + src[nm][k, t] * ww[d, t]
            for nm in names:
                self.acc[nm].reshape(self.ddm, -1)[:, c] = a[nm]

    def msklvl(self):
        """returns the masked copies: levels kmax+1..ddm of every owned point (wet or not) are nf90_fill_double"""
        out = {}
        for nm in self.names:
            bath = self.bath[LVL[nm][0]]
            kmax = np.zeros(self.shape, np.int64)
            for k in range(self.ddm):
                kmax[bath > self.bnds[k, 0]] = k + 1
            a = self.acc[nm].copy()
            for k in range(self.ddm):
                a[k][self.own & (k + 1 > kmax)] = FILL
            out[nm] = a
        return out


# ---- one run per case, shared ------------------------------------------------------------------------------------------------------
_RUNS = {}
CASES = ["chan_s_tke", "box_s", "tri_s_tke"]
EXTENDED = {"chan_s_tke"}


def lvl_run(cfg, edges=None):
    """Context A: the layer table and every admitted level name, step(0, 4) at once; finalize; (extended) reset and step(4, 4).
    Context B: no selection, four single steps, numpy (levels: RestatedLvl, layers: test_gpu_diaacc.Restated) after each; (extended)
    two more for the graph test, the level names selected afresh at step 4 and stepped to 8."""
    key = (cfg, tuple(edges) if edges else None)
    if key in _RUNS:
        return _RUNS[key]
    extended = cfg in EXTENDED and edges is None
    r = {}
    case, masks, a = full_context(cfg)
    _, _, b = full_context(cfg)
    try:
        lnames, names = lyr.admitted(case), admitted_lvl(case)
        r.update(case=case, masks=masks, names=names, lnames=lnames)
        if edges:
            a.dia_set_levels(bnds_of(edges))
        bnds = a.dia_levels()
        r["bnds"] = bnds
        a.dia_select(lnames + names)
        assert a.step(0, 4) == 4
        r["A4"] = {nm: a.dia_get(nm) for nm in lnames + names}
        r["A4_nacc"] = a.dia_nacc()
        r["A4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
        ref = RestatedLvl(case, masks, names, b.get("depths")[0], bnds)
        lref = lyr.Restated(case, masks, lnames)
        r["init"] = {nm: v.copy() for nm, v in ref.acc.items()}
        for ns in range(4):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
            lref.accumulate(b, ns)
        r["E4"] = {nm: v.copy() for nm, v in ref.acc.items()}
        r["E4_lyr"] = {nm: v.copy() for nm, v in lref.acc.items()}
        r["cover"] = {g: dict(v) for g, v in ref.cover.items()}
        r["B4_state"] = {nm: b.get(nm) for nm in STATE_FIELDS if b.has_field(nm)}
        r["E4_fin"] = ref.msklvl()
        a.dia_finalize()
        r["A4_fin"] = {nm: a.dia_get(nm) for nm in names}
        if extended:
            a.dia_reset()
            r["A_reset"] = {nm: a.dia_get(nm) for nm in names}
            r["A_reset_nacc"] = a.dia_nacc()
            assert a.step(4, 4) == 8
            r["A8"] = {nm: a.dia_get(nm) for nm in names}
            r["A8_nacc"] = a.dia_nacc()
            b.dia_select(names)
            for ns in range(4, 8):
                assert b.step(ns, 1) == ns + 1
                if ns < 6:
                    ref.accumulate(b, ns)
                if ns == 5:
                    r["E6"] = {nm: v.copy() for nm, v in ref.acc.items()}
            r["B8"] = {nm: b.dia_get(nm) for nm in names}
            r["B8_nacc"] = b.dia_nacc()
        if not edges:
            # A layer that fails its condition above layers that pass -- the cases do not produce one on every grid by themselves --
            # is put there: layer 3 of every third column loses its mass (p) / its mass flux (u, v), and the stage runs once on that.
            ns = 7 if extended else 3
            idx = hostinit.step_indices(ns, case.kdm)
            nj, ni = case.jdm + 8, case.idm + 8
            third = ((np.arange(nj)[:, None] + np.arange(ni)[None, :]) % 3 == 0)
            for nm, lev in (("dp", idx[2] + 2), ("uflx", idx[3] + 2), ("vflx", idx[3] + 2)):
                f = b.get(nm)
                f[lev][third] = 0.0
                b.put(nm, f)
            b.dia_select(names)
            b.diaacc(*idx)
            pin = RestatedLvl(case, masks, names, b.get("depths")[0], bnds)
            pin.accumulate(b, ns)
            r["pinch_got"] = {nm: b.dia_get(nm) for nm in names}
            r["pinch_want"] = pin.acc
            r["pinch_cover"] = {g: dict(v) for g, v in pin.cover.items()}
    finally:
        a.close()
        b.close()
    _RUNS[key] = r
    return r


# ---- 1. the step accumulates what the reference's loops would --------------------------------------------------------------------
def check_step_accumulates(cfg, edges=None):
    r = lvl_run(cfg, edges)
    assert len(r["names"]) >= 31 and r["A4_nacc"] == 4
    bad = differing({nm: r["A4"][nm] for nm in r["names"]}, r["E4"])
    assert not bad, f"{cfg}: level accumulators that differ from the restated loops: {bad}"
    nj, ni = r["case"].jdm + 8, r["case"].idm + 8
    for nm in r["names"]:
        g = LVL[nm][0]
        sel = np.zeros((nj, ni), bool)
        sel[4:-4, 4:-4] = True
        sel &= r["masks"]["i" + g].reshape(nj, ni) > 0
        assert same_bytes(r["A4"][nm][:, ~sel], r["init"][nm][:, ~sel]), nm      # 0*mask everywhere else
    for nm in ("templvl", "salnlvl", "uvellvl", "vvellvl", "uflxlvl", "vflxlvl", "dzlvl"):
        assert (np.abs(r["A4"][nm]) > 0.0).any(), nm
    if "pinch_got" in r:
        bad = differing(r["pinch_got"], r["pinch_want"])
        assert not bad, f"{cfg}: with a layer failing its condition in mid-column: {bad}"


@pytest.mark.parametrize("cfg", CASES)
def test_step_accumulates_what_the_reference_loops_would(cfg):
    check_step_accumulates(cfg)


# ---- 2. coverage: test 1 cannot pass vacuously --------------------------------------------------------------------------------------
def check_coverage(cfg):
    """per case and grid, on the restatement of runs that check_step_accumulates compares: (a) a layer feeds >= 3 levels, (b) a level
    is fed by >= 2 layers, (d) ind1 advances past a level -- in the four steps with the default table (the coarse table is run and
    compared too: there every level is fed by several layers); (c) a layer fails its condition while a later one of the column
    passes -- in the run of the stage on the state with the emptied third layer (lvl_run)"""
    r = lvl_run(cfg)
    print(cfg, "default table:", r["cover"], "emptied layer:", r["pinch_cover"])
    for g in "puv":
        cv = r["cover"][g]
        assert cv["a"] > 0 and cv["b"] > 0 and cv["d"] > 0, (cfg, g, cv)
        assert r["pinch_cover"][g]["c"] > 0, (cfg, g, r["pinch_cover"][g])
    check_step_accumulates(cfg, COARSE)
    rc = lvl_run(cfg, COARSE)
    print(cfg, "coarse table:", rc["cover"])
    for g in "puv":
        assert rc["cover"][g]["b"] > 0, (cfg, g)


@pytest.mark.parametrize("cfg", CASES)
def test_the_cases_cover_the_walk(cfg):
    check_coverage(cfg)


# ---- 3. a bound that equals an interface exactly ---------------------------------------------------------------------------------------
def check_equality_case():
    case, masks, g = full_context("chan_s_tke")
    try:
        kk = case.kdm
        assert g.step(0, 2) == 2
        idx = hostinit.step_indices(1, kk)
        m, n, mm, nn, k1m, k1n = idx
        probe = RestatedLvl(case, masks, [], g.get("depths")[0], bnds_of(EDGES35))
        flat = lambda nm: g.get(nm).reshape(-1, probe.shape[0] * probe.shape[1])
        edges, chosen = {0.0, 8000.0}, {}
        for gr, tn, cn, cl in (("p", "dp", "dp", mm), ("u", "dpu", "uflx", nn), ("v", "dpv", "vflx", nn)):
            c = probe.cols[gr]
            th, cs = flat(tn)[mm:mm + kk][:, c], flat(cn)[cl:cl + kk][:, c]
            list(probe.diazlv_columns(gr, th, cs))                   # fills probe.zbot
            zb = probe.zbot
            ok = (cs > DPEPS) if gr == "p" else (np.abs(cs) > FLXEPS)
            # a column with two adjacent layers that both pass and a distinct interface between them
            pair = ok[:-1] & ok[1:] & (np.diff(zb, axis=0) > 1.0) & (zb[:-1] > 1.0)
            col = int(np.flatnonzero(pair.any(axis=0))[0])
            chosen[gr] = col
            ks = np.flatnonzero(pair[:, col])
            edges |= {float(zb[k, col]) for k in ks}
        table = bnds_of(sorted(edges))
        assert 3 <= len(table) <= MAXLEV
        g.dia_set_levels(table)
        assert same_bytes(g.dia_levels(), table)
        names = admitted_lvl(case)
        g.dia_select(names)
        g.diaacc(*idx)
        g.diaacc(*idx)
        assert g.dia_nacc() == 2
        got = {nm: g.dia_get(nm) for nm in names}
        # the case bites: at the chosen columns the grid's own comparisons and the other grid family's visit different (k, d)
        for gr in "puv":
            seen = {}
            for st in (False, True):
                ref = RestatedLvl(case, masks, [nm for nm in names if LVL[nm][0] == gr], g.get("depths")[0], table)
                ref.watch = {gr: chosen[gr]}
                ref.accumulate(g, 1, strict={gr: st})
                seen[st] = ref.visits.get(gr, set())
            assert seen[False] != seen[True] and seen[False] <= seen[True], (gr, seen)
        ref = RestatedLvl(case, masks, names, g.get("depths")[0], table)
        ref.accumulate(g, 1)
        ref.accumulate(g, 1)
        assert not differing(got, ref.acc), differing(got, ref.acc)
        assert (np.abs(got["uflxlvl"]) > 0.0).any() and (np.abs(got["templvl"]) > 0.0).any()
    finally:
        g.close()


def test_a_bound_equal_to_an_interface():
    check_equality_case()


# ---- 4. dia_set_levels ------------------------------------------------------------------------------------------------------------------
def check_set_levels():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = full_context("box_s")
    _, _, b = full_context("box_s")
    try:
        assert same_bytes(g.dia_levels(), bnds_of(EDGES35))
        with pytest.raises(BlomGpuError, match="at most %d levels" % MAXLEV):
            g.dia_set_levels(bnds_of(np.arange(MAXLEV + 2) * 10.0))
        bad = bnds_of(EDGES35).copy()
        bad[7, 1] = bad[7, 0]
        with pytest.raises(BlomGpuError, match="not increasing"):
            g.dia_set_levels(bad)
        bad = bnds_of(EDGES35).copy()
        bad[7, 1] -= 1.0
        with pytest.raises(BlomGpuError, match="not contiguous"):
            g.dia_set_levels(bad)
        assert same_bytes(g.dia_levels(), bnds_of(EDGES35))          # a refused table changes nothing
        g.dia_set_levels(bnds_of(COARSE))
        assert same_bytes(g.dia_levels(), bnds_of(COARSE))
        g.dia_set_levels(None)
        assert same_bytes(g.dia_levels(), bnds_of(EDGES35))
        g.dia_set_levels(levitus2x=True)
        assert len(EDGES70) == 71 and same_bytes(g.dia_levels(), bnds_of(EDGES70))
        names = admitted_lvl(case)
        g.dia_select(names)
        with pytest.raises(BlomGpuError, match="selected"):
            g.dia_set_levels(None)
        assert g.step(0, 1) == 1 and b.step(0, 1) == 1
        ref = RestatedLvl(case, masks, names, b.get("depths")[0], bnds_of(EDGES70))
        ref.accumulate(b, 0)
        got = {nm: g.dia_get(nm) for nm in names}
        assert got["templvl"].shape[0] == 70
        assert not differing(got, ref.acc), differing(got, ref.acc)
        g.dia_select("temp")                                         # no level name selected any more
        g.dia_set_levels(None)
    finally:
        g.close()
        b.close()


def test_set_levels_validates_and_the_70_level_table_runs():
    check_set_levels()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)           # no TKE tracers
    try:
        rows = {nm: (k, gr) for nm, k, gr in g.dia_names()}
        assert len(rows) == 78 + 33 and list(rows)[:78] == lyr.TABLE and list(rows)[78:] == list(LVL)
        assert all(rows[nm] == (2, LVL[nm][0]) for nm in LVL)
        g.dia_select("templvl uflxlvl")
        with pytest.raises(BlomGpuError, match="temp"):
            g.dia_get("temp")                                        # level names add no dependencies
        assert g.step(0, 2) == 2
        t2, u2 = g.dia_get("templvl"), g.dia_get("uflxlvl")
        assert np.abs(t2).max() > 0.0 and g.dia_nacc() == 2
        for lst, word in (("templvl tkelvl", "tkelvl"), ("gls_psilvl", "gls_psilvl"), ("templvl nonsenselvl", "nonsenselvl")):
            with pytest.raises(BlomGpuError, match=word):
                g.dia_select(lst)
        assert same_bytes(g.dia_get("templvl"), t2) and same_bytes(g.dia_get("uflxlvl"), u2) and g.dia_nacc() == 2
        # the hybrid coordinate forms these four inside ale_regrid_remap (:1944, :2059, :2174 leave them out)
        for vc in ("cntiso_hybrid", "plevel"):
            g.set("vcoord_type", vc)
            for nm in HYBRID_REFUSED:
                with pytest.raises(BlomGpuError, match=nm + ".*ale_regrid_remap"):
                    g.dia_select("dzlvl " + nm)
            assert same_bytes(g.dia_get("templvl"), t2) and g.dia_nacc() == 2
        g.dia_select("dzlvl uflxlvl bfsqlvl")                        # the rest of the family is admitted there (:1944, :2059, :2174)
        g.set("vcoord_type", "isopyc_bulkml")
        # dzlvl follows dz's rule: a sequence without cmnfld1 refuses it at the step
        g.set("cmnfld1", 0)
        g.dia_select("dzlvl")
        with pytest.raises(BlomGpuError, match="dzlvl"):
            g.step(2, 1)
    finally:
        g.close()


def test_refusals_keep_the_selection():
    check_refusals()


# ---- 6. finalise, reset, independence ---------------------------------------------------------------------------------------------------
def check_finalize(cfg):
    r = lvl_run(cfg)
    bad = differing(r["A4_fin"], r["E4_fin"])
    assert not bad, f"{cfg}: finalised level accumulators that differ from the restated msklvl: {bad}"
    t = r["A4_fin"]["templvl"][:, 4:-4, 4:-4]
    assert (t == FILL).any() and (t != FILL).any()


@pytest.mark.parametrize("cfg", CASES)
def test_finalize_is_the_restated_msklvl(cfg):
    check_finalize(cfg)


def check_reset_and_independence():
    r = lvl_run("chan_s_tke")
    assert not differing(r["A_reset"], r["init"]) and r["A_reset_nacc"] == 0
    assert not differing(r["A8"], r["B8"]), differing(r["A8"], r["B8"])
    assert r["A8_nacc"] == 4 and r["B8_nacc"] == 4
    assert (np.abs(r["A8"]["templvl"]) > 0.0).any()
    # the level names change no byte of the layer / 2-D accumulators and none of the model state
    bad = differing({nm: r["A4"][nm] for nm in r["lnames"]}, r["E4_lyr"])
    assert not bad, bad
    bad = [nm for nm in r["B4_state"] if not same_bytes(r["A4_state"][nm], r["B4_state"][nm])]
    assert not bad, bad


def test_reset_nacc_and_independence():
    check_reset_and_independence()


# ---- 7. graph replay, tiles -----------------------------------------------------------------------------------------------------------------
def check_graph_replay(expect_replays):
    r = lvl_run("chan_s_tke")
    case, masks, g = full_context("chan_s_tke")
    try:
        g.set("use_graph", 1)
        g.dia_select(r["names"])
        assert g.step(0, 6) == 6
        got = {nm: g.dia_get(nm) for nm in r["names"]}
        assert not differing(got, r["E6"]), differing(got, r["E6"])
        assert g.dia_nacc() == 6
        if expect_replays:
            assert g.get_real("graph_steps") >= 1, "no step was replayed as a graph"
    finally:
        g.close()


def test_graph_replay_accumulates_the_same_bytes():
    import os
    check_graph_replay(expect_replays=os.environ.get("BLOM_HOSTEMU") != "1")


def check_tiles(monkeypatch):
    """test_gpu_diaacc.check_tiles with the level names added to its selection: each tile of a 2x1 group holds its window"""
    monkeypatch.setattr(lyr, "admitted", lambda case: _LAYER_ADMITTED(case) + admitted_lvl(case))
    import test_gpu_tiles
    monkeypatch.setattr(test_gpu_tiles, "FORCING", test_gpu_tiles.FORCING + ["depths"])      # the tiles need their window of the bathymetry
    lyr.check_tiles()


def test_tiles_accumulate_their_window_of_the_single_tile(monkeypatch):
    check_tiles(monkeypatch)


# ---- 8. full size -------------------------------------------------------------------------------------------------------------------------
def test_channel_size_level_set():
    """208x512x53: 13 names x 35 levels of 216x520 doubles (slot offsets are size_t in the kernel); two steps against the restatement"""
    case, masks, a = full_context("channel_tke")
    _, _, b = full_context("channel_tke")
    try:
        a.dia_select(CHANNEL_SET)
        assert a.step(0, 2) == 2
        ref = RestatedLvl(case, masks, CHANNEL_SET, b.get("depths")[0], a.dia_levels())
        for ns in range(2):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
        got = {nm: a.dia_get(nm) for nm in CHANNEL_SET}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        assert a.dia_nacc() == 2
        for nm in CHANNEL_SET:
            assert np.abs(got[nm]).max() > 0.0, nm
    finally:
        a.close()
        b.close()
