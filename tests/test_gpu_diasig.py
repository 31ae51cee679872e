"""diaacc's density-class mass fluxes on the device (k_diasig, blom_amd/csrc/stage_diaacc.hip): umfll umfltdl umflsml vmfll vmfltdl vmflsml.

The expected values are the reference's loops restated in numpy below (bin_columns): phy/mod_dia.F90:1398-1453 | :1471-1526 with
the per-column kup carried down the layers, both branches of the search with their exits, the klo search against sigdia(klo) +
sigeps, the three pieces or the whole flux, bins that start from zero and are added to the accumulator afterwards (acclyr, :5500).
k is the outer loop and the columns are vectorised; every column sees the operations of the reference in the reference's order, in
float64 (numpy does not contract).  The restatement is applied to arrays a second context downloads after each of its single
steps; sigint is taken from the device INCLUDING its halo, after the stage, and is itself pinned separately (check_sigint): the
formula of :1372-1390 at the owned p-points, xctilr's one-point halo (:1392, blom_amd.hostinit.xctilr_np), nothing else touched.
Everything is compared with ==, byte for byte over the whole padded array.

tests/test_hostemu_diasig.py runs the small cases on the host emulation of the library."""
import numpy as np
import pytest

from blom_amd import hostinit
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import full_context, dyncore_context, same_bytes, differing

pytestmark = pytest.mark.gpu

SIGEPS = 1.0e-9                       # phy/mod_dia.F90:1120
# name -> (grid, source at k + nn); the acclyr calls :1457, :1461, :1465, :1530, :1534, :1538
CLS = dict(umfll=("u", "uflx"), umfltdl=("u", "umfltd"), umflsml=("u", "umflsm"),
           vmfll=("v", "vflx"), vmfltdl=("v", "vmfltd"), vmflsml=("v", "vmflsm"))
NAMES = list(CLS)
COUNTERS = ("A", "B", "C", "D", "E")

_LAYER_ADMITTED = lyr.admitted
_LAYER_OPTIONS = lyr.options


def fmax(a, b):
    return np.where(a > b, a, b)         # MAX as amdflang lowers it


def fmin(a, b):
    return np.where(a < b, a, b)


def new_cover():
    return dict(A=0, B=0, C=0, D=0, E=0, E_kup=0, E_klo=0)


def bin_columns(sc, sn, flxs, sd, cover=None):
    """one step's tmp3d of :1398-1453 on compressed columns.  sc, sn: sigint(kk, ncol) at the point and at its western | southern
    neighbour; flxs: list of (kk, ncol) fluxes at k + nn; sd: sigdia(kk).  Returns the list of (kk, ncol) bins.  kup, klo are the
    reference's 1-based indices: sigdia(x) = sd[x - 1], tmp(:,:,x) = tmp[x - 1].  cover counts (A) kup advanced, (B) kup retreated,
    (C) the loop kt = kup..klo-2 ran, (D) the branch kup == klo, (E) an exit at kk (of either search)."""
    kk, nc = sc.shape
    sd = np.asarray(sd, dtype=np.float64)
    cover = new_cover() if cover is None else cover
    tmp = [np.zeros((kk, nc)) for _ in flxs]                      # tmp3d(:,:,:) = 0.
    kup = np.full(nc, 2, np.int64)                                # kup_arr(:) = 2
    with np.errstate(all="ignore"):
        for k in range(kk):
            kl = min(kk - 1, k + 1)
            sigup = .5 * (sn[k] + sc[k])
            siglo = .5 * (sn[kl] + sc[kl])
            sigmin, sigmax = fmin(sigup, siglo), fmax(sigup, siglo)
            first = sigmin > sd[kup - 2]                          # if (sigmin > sigdia(kup-1)) then
            act = first.copy()
            while True:                                           # do while (sigmin > sigdia(kup))
                act &= sigmin > sd[kup - 1]
                ex = act & (kup == kk)                            # if (kup == kk) exit
                cover["E_kup"] += int(ex.sum())
                act &= ~ex
                if not act.any():
                    break
                kup[act] += 1
                cover["A"] += int(act.sum())
            act = ~first
            while True:                                           # else: do
                act &= kup != 2                                   # if (kup == 2) exit
                act &= ~(sigmin > sd[kup - 2])                    # if (sigmin > sigdia(kup-1)) exit
                if not act.any():
                    break
                kup[act] -= 1
                cover["B"] += int(act.sum())
            klo = kup.copy()
            act = np.ones(nc, bool)
            while True:                                           # do while (sigmax > sigdia(klo) + sigeps)
                act &= sigmax > sd[klo - 1] + SIGEPS
                ex = act & (klo == kk)
                cover["E_klo"] += int(ex.sum())
                act &= ~ex
                if not act.any():
                    break
                klo[act] += 1
            split = kup < klo
            cover["D"] += int((~split).sum())
            s = np.flatnonzero(split)
            w_ = np.flatnonzero(~split)
            q = 1. / (sigmax - sigmin)
            w1 = (sd[kup[s] - 1] - sigmin[s]) * q[s]               # (sigdia(kup) - sigmin)*q
            mids, d = [], 0
            while True:                                           # do kt = kup, klo-2
                kt = kup + d
                m = np.flatnonzero(split & (kt <= klo - 2))
                if not len(m):
                    break
                mids.append((m, kt[m], (sd[kt[m]] - sd[kt[m] - 1]) * q[m]))      # (sigdia(kt+1) - sigdia(kt))*q
                cover["C"] += len(m)
                d += 1
            w3 = (sigmax[s] - sd[klo[s] - 2]) * q[s]               # (sigmax - sigdia(klo-1))*q
            for t, flx in zip(tmp, flxs):
                f = flx[k]
                t[kup[s] - 2, s] = t[kup[s] - 2, s] + w1 * f[s]
                for m, ktm, wm in mids:
                    t[ktm - 1, m] = t[ktm - 1, m] + wm * f[m]
                t[klo[s] - 2, s] = t[klo[s] - 2, s] + w3 * f[s]
                t[kup[w_] - 2, w_] = t[kup[w_] - 2, w_] + f[w_]
    cover["E"] = cover["E_kup"] + cover["E_klo"]
    return tmp


class RestatedSig:
    """phylyr of the selected class names on one tile"""

    def __init__(self, case, masks, names, sigdia):
        self.case, self.names, self.kk = case, list(names), case.kdm
        self.sd = np.asarray(sigdia, dtype=np.float64).copy()
        nj, ni = case.jdm + 8, case.idm + 8
        self.shape = (nj, ni)
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + case.jdm, 4:4 + case.idm] = True
        self.own = own
        self.cols = {g: np.flatnonzero((own & (self.mask[g] > 0)).ravel()) for g in "uv"}
        self.nbr = {"u": self.cols["u"] - 1, "v": self.cols["v"] - ni}
        self.cover = {g: new_cover() for g in "uv"}
        self.reset()

    def reset(self):
        self.acc = {nm: np.repeat((0.0 * self.mask[CLS[nm][0]].astype(np.float64))[None], self.kk, axis=0).copy() for nm in self.names}
        self.nacc = 0

    def accumulate_arrays(self, sigint, flx):
        """sigint: (kk, nj, ni) with its halo; flx: source name -> (kk, nj, ni), the planes k + nn"""
        kk = self.kk
        si = sigint.reshape(kk, -1)
        self.nacc += 1
        for g in "uv":
            names = [nm for nm in self.names if CLS[nm][0] == g]
            if not names:
                continue
            c = self.cols[g]
            tmp = bin_columns(si[:, c], si[:, self.nbr[g]], [flx[CLS[nm][1]].reshape(kk, -1)[:, c] for nm in names], self.sd, self.cover[g])
            for nm, t in zip(names, tmp):
                a = self.acc[nm].reshape(kk, -1)
                a[:, c] = a[:, c] + t                              # acclyr, op 0: every class, touched or not

    def accumulate(self, gpu, nstep):
        self.accumulate_arrays(*snapshot(gpu, nstep, self.kk))


def snapshot(gpu, nstep, kk):
    """what the restatement reads after the step that started from step count nstep: sigint, and the sources at k + nn"""
    nn = hostinit.step_indices(nstep, kk)[3]
    return gpu.get("sigint"), {f: gpu.get(f)[nn:nn + kk].copy() for f in sorted({v[1] for v in CLS.values()})}


def check_sigint(case, masks, before, after, sigma_mm):
    """sigint after the stage under isopyc_bulkml: the owned wet p-points hold :1377 | :1384 of the downloaded sigma, then xctilr
    (1, 1, halo_ps) gave the one-point halo (on the arctic patch it also folds row jj, as the reference's does); every other point
    keeps what it held"""
    kk, ii, jj = case.kdm, case.idm, case.jdm
    nj, ni = jj + 8, ii + 8
    wet = np.zeros((nj, ni), bool)
    wet[4:4 + jj, 4:4 + ii] = True
    wet &= masks["ip"].reshape(nj, ni) > 0
    want = before.copy()
    want[0][wet] = sigma_mm[0][wet]
    for k in range(1, kk):
        want[k][wet] = (.5 * (sigma_mm[k - 1] + sigma_mm[k]))[wet]
    owned_formula = want.copy()
    hostinit.xctilr_np(want, 1, kk, 1, 1, case.nreg, ii, jj, itype=1)
    assert same_bytes(after, want), "sigint differs from the formula at the owned points + xctilr's halo + untouched elsewhere"
    if case.nreg == 1:                   # periodic in i: the halo column is the opposite owned column
        assert same_bytes(after[:, 4:4 + jj, 3], owned_formula[:, 4:4 + jj, 3 + ii])
        assert same_bytes(after[:, 4:4 + jj, 4 + ii], owned_formula[:, 4:4 + jj, 4])
    untouched = np.ones((nj, ni), bool)
    untouched[3:5 + jj, 3:5 + ii] = False
    assert same_bytes(after[:, untouched], before[:, untouched])


# ---- the sigdia tables of a case ------------------------------------------------------------------------------------------------
_TABLES = {}


def tables_for(cfg):
    """three tables of kdm values: the case's reference densities (the column of sigmar at a wet point of the initial state); the
    same shifted by half a class; kdm values spaced evenly over the range sigint takes in the first two layers of the initial state"""
    if cfg in _TABLES:
        return _TABLES[cfg]
    case, masks, g = full_context(cfg)
    try:
        sigmar, sigma = g.get("sigmar"), g.get("sigma")
    finally:
        g.close()
    nj, ni = case.jdm + 8, case.idm + 8
    wet = np.zeros((nj, ni), bool)
    wet[4:-4, 4:-4] = True
    wet &= masks["ip"].reshape(nj, ni) > 0
    j, i = np.argwhere(wet)[0]
    ref = sigmar[:case.kdm, j, i].astype(np.float64).copy()
    assert (np.diff(ref) >= 0).all() and ref[-1] > ref[0], ref          # (the two mixed-layer classes of isopyc_bulkml coincide)
    half = ref - .5 * np.diff(ref, prepend=2 * ref[0] - ref[1])
    s1, s2 = sigma[0][wet], (.5 * (sigma[0] + sigma[1]))[wet]
    lo, hi = min(s1.min(), s2.min()), max(s1.max(), s2.max())
    assert hi > lo, (lo, hi)
    _TABLES[cfg] = dict(ref=ref, half=half, fine=np.linspace(lo, hi, case.kdm))
    return _TABLES[cfg]


# ---- one run per case, shared ------------------------------------------------------------------------------------------------------
_RUNS = {}
CASES = ["chan_s_tke", "box_s", "tri_s_tke"]
EXTENDED = {"chan_s_tke"}
TABLES = ("ref", "half", "fine")
LEVEL_NAMES = "templvl uflxlvl vflxlvl dzlvl".split()      # z-level names every case admits: k_dialvl runs behind the new stage


def sig_run(cfg):
    """Context B: the six names selected (so that the stage writes sigint), four single steps; after each the arrays the restatement
    reads are kept and sigint itself is checked.  The restatement is applied to the kept arrays once per table.
    Contexts A (one per table): the six names plus the layer table and LEVEL_NAMES, step(0, 4) at once.
    (extended) A of the first table: finalize, reset, step(4, 4).  B: the names selected afresh at step 4, four more single steps; the
    first table's restatement goes on to its 6-step total.  A context C without the six names for the independence check.
    Last, on B: a sigma whose third layer is lighter than its first in every third column is put, and the stage runs once on that
    state with each table."""
    if cfg in _RUNS:
        return _RUNS[cfg]
    extended = cfg in EXTENDED
    tabs = tables_for(cfg)
    r = dict(tabs=tabs)
    case, masks, b = full_context(cfg)
    kk = case.kdm
    a = None
    try:
        lnames = lyr.admitted(case) + LEVEL_NAMES                  # "the other accumulators": 2-D, layers and a few depth levels
        r.update(case=case, masks=masks, lnames=lnames)
        b.dia_set_sigdia(tabs["ref"])
        b.dia_select(NAMES)
        snaps = []
        for ns in range(4):
            before = b.get("sigint")
            assert b.step(ns, 1) == ns + 1
            snaps.append(snapshot(b, ns, kk))
            mm = hostinit.step_indices(ns, kk)[2]
            check_sigint(case, masks, before, snaps[-1][0], b.get("sigma")[mm:mm + kk])
        r["B4_own"] = {nm: b.dia_get(nm) for nm in NAMES}
        refs = {}
        for tn in TABLES:
            refs[tn] = RestatedSig(case, masks, NAMES, tabs[tn])
            for sn in snaps:
                refs[tn].accumulate_arrays(*sn)
        r["init"] = {nm: np.repeat((0.0 * masks["i" + CLS[nm][0]].reshape(1, case.jdm + 8, case.idm + 8).astype(np.float64)), kk, axis=0) for nm in NAMES}
        r["E4"] = {tn: {nm: v.copy() for nm, v in refs[tn].acc.items()} for tn in TABLES}
        r["cover"] = {tn: {g: dict(v) for g, v in refs[tn].cover.items()} for tn in TABLES}
        lref = None
        for tn in TABLES:
            _, _, a = full_context(cfg)
            a.dia_set_sigdia(tabs[tn])
            a.dia_select(NAMES + lnames)
            assert a.step(0, 4) == 4
            r.setdefault("A4", {})[tn] = {nm: a.dia_get(nm) for nm in NAMES}
            r.setdefault("A4_nacc", {})[tn] = a.dia_nacc()
            if tn == "ref":
                r["A4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
                r["A4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
                r["A_sigdia"] = a.dia_sigdia()
                a.dia_finalize()
                r["A4_fin"] = {nm: a.dia_get(nm) for nm in NAMES}
                if extended:
                    a.dia_reset()
                    r["A_reset"] = {nm: a.dia_get(nm) for nm in NAMES}
                    r["A_reset_nacc"] = a.dia_nacc()
                    assert a.step(4, 4) == 8
                    r["A8"] = {nm: a.dia_get(nm) for nm in NAMES}
                    r["A8_nacc"] = a.dia_nacc()
            a.close()
            a = None
        if extended:
            _, _, a = full_context(cfg)                             # C: the layer table alone
            a.dia_select(lnames)
            assert a.step(0, 4) == 4
            r["C4_lyr"] = {nm: a.dia_get(nm) for nm in lnames}
            r["C4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
            a.close()
            a = None
            b.dia_select(NAMES)                                     # afresh
            for ns in range(4, 8):
                assert b.step(ns, 1) == ns + 1
                if ns < 6:
                    refs["ref"].accumulate(b, ns)
                if ns == 5:
                    r["E6"] = {nm: v.copy() for nm, v in refs["ref"].acc.items()}
            r["B8"] = {nm: b.dia_get(nm) for nm in NAMES}
            r["B8_nacc"] = b.dia_nacc()
        # the engineered state: layer 3 lighter than everything above it in every third column
        ns = 7 if extended else 3
        idx = hostinit.step_indices(ns, kk)
        mm = idx[2]
        nj, ni = case.jdm + 8, case.idm + 8
        third = ((np.arange(nj)[:, None] + np.arange(ni)[None, :]) % 3 == 0)
        f = b.get("sigma")
        f[mm + 2][third] = f[mm][third] - 1.0
        b.put("sigma", f)
        r["inv_got"], r["inv_want"], r["inv_cover"] = {}, {}, {}
        for tn in TABLES:
            b.dia_select("")
            b.dia_set_sigdia(tabs[tn])
            b.dia_select(NAMES)
            before = b.get("sigint")
            b.diaacc(*idx)
            inv = RestatedSig(case, masks, NAMES, tabs[tn])
            inv.accumulate(b, ns)
            check_sigint(case, masks, before, b.get("sigint"), b.get("sigma")[mm:mm + kk])
            r["inv_got"][tn] = {nm: b.dia_get(nm) for nm in NAMES}
            r["inv_want"][tn] = inv.acc
            r["inv_cover"][tn] = {g: dict(v) for g, v in inv.cover.items()}
    finally:
        if a is not None:
            a.close()
        b.close()
    _RUNS[cfg] = r
    return r


# ---- 1. the step accumulates what the reference's loops would --------------------------------------------------------------------
def check_step_accumulates(cfg):
    r = sig_run(cfg)
    nj, ni = r["case"].jdm + 8, r["case"].idm + 8
    for tn in TABLES:
        assert r["A4_nacc"][tn] == 4
        bad = differing(r["A4"][tn], r["E4"][tn])
        assert not bad, f"{cfg}, table {tn}: class accumulators that differ from the restated loops: {bad}"
        for nm in NAMES:
            sel = np.zeros((nj, ni), bool)
            sel[4:-4, 4:-4] = True
            sel &= r["masks"]["i" + CLS[nm][0]].reshape(nj, ni) > 0
            assert same_bytes(r["A4"][tn][nm][:, ~sel], r["init"][nm][:, ~sel]), nm      # 0*mask everywhere else
        for nm in ("umfll", "vmfll"):
            assert (np.abs(r["A4"][tn][nm]) > 0.0).any(), (tn, nm)
        bad = differing(r["inv_got"][tn], r["inv_want"][tn])
        assert not bad, f"{cfg}, table {tn}: on the state with the inverted third layer: {bad}"
    assert not differing(r["B4_own"], r["E4"]["ref"])              # the single-stepping context's own accumulators


@pytest.mark.parametrize("cfg", CASES)
def test_step_accumulates_what_the_reference_loops_would(cfg):
    check_step_accumulates(cfg)


# ---- 2. coverage: test 1 cannot pass vacuously --------------------------------------------------------------------------------------
def check_coverage(cfg):
    """per case and grid, over the three tables, in runs that check_step_accumulates compares: (A) kup advanced, (B) kup retreated,
    (C) the middle loop ran, (D) the branch kup == klo, (E) an exit at kk.  The free runs and the run of the stage on the state with
    the inverted third layer (sig_run) are counted together and printed apart."""
    r = sig_run(cfg)
    for g in "uv":
        tot = {x: 0 for x in COUNTERS}
        for tn in TABLES:
            print(cfg, g, tn, "free:", r["cover"][tn][g], "inverted layer:", r["inv_cover"][tn][g])
            for x in COUNTERS:
                tot[x] += r["cover"][tn][g][x] + r["inv_cover"][tn][g][x]
        assert all(tot[x] > 0 for x in COUNTERS), (cfg, g, tot)


@pytest.mark.parametrize("cfg", CASES)
def test_the_cases_cover_the_search(cfg):
    check_coverage(cfg)


# ---- 3. the restatement itself (numpy only) ------------------------------------------------------------------------------------------
def check_restatement_conserves():
    rng = np.random.default_rng(7)
    kk, nc = 9, 400
    eps = np.finfo(np.float64).eps
    sd = 24.0 + np.cumsum(rng.uniform(0.1, 0.6, kk))
    for trial in range(3):
        # interface densities increasing in k, with an inversion in every third column; some columns lighter than sigdia(1), some
        # denser than sigdia(kk)
        base = rng.uniform(sd[0] - 1.0, sd[0] + 1.5, nc)
        sc = base[None] + np.cumsum(rng.uniform(0.0, 0.9, (kk, nc)), axis=0)
        sc[2, ::3] = sc[0, ::3] - 0.7
        sn = sc + rng.uniform(-0.05, 0.05, (kk, nc))
        flx = rng.normal(0.0, 1.0e6, (kk, nc))
        one = np.zeros((kk, nc))
        kone = trial * 3 + 1
        one[kone] = 1.0
        cover = new_cover()
        tmp, wsum = bin_columns(sc, sn, [flx, one], sd, cover)
        assert all(cover[x] > 0 for x in COUNTERS), cover
        # per column the classes hold what the layers carried
        err = np.abs(tmp.sum(axis=0) - flx.sum(axis=0))
        assert (err <= 4 * kk * eps * np.abs(flx).sum(axis=0)).all(), err.max()
        # the weights of a layer sum to 1 up to rounding (at most 4 kdm additions)
        assert (np.abs(wsum.sum(axis=0) - 1.0) <= 4 * kk * eps).all()
        # bins start from zero and the last class is never written (bins kup-1 .. klo-1 <= kk-1)
        assert (tmp[kk - 1] == 0.0).all()


def test_restatement_conserves_the_flux_and_its_weights_sum_to_one():
    check_restatement_conserves()



# ---- 4. interface ---------------------------------------------------------------------------------------------------------------------
def check_interface():
    from blom_amd.gpu import BlomGpuError
    import test_gpu_dialvl as lvl
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)
    try:
        kk = case.kdm
        named, full = g.dia_names(), g.dia_names_all()
        assert len(named) == 78 + 33 and [x[0] for x in named] == lyr.TABLE + list(lvl.LVL)
        assert full[:111] == named
        assert full[111:] == [(nm, 3, CLS[nm][0]) for nm in NAMES]
        assert g.dia_sigdia().shape == (0,)
        with pytest.raises(BlomGpuError, match="sigdia"):
            g.dia_select("umfll")
        tab = 25.0 + 0.5 * np.arange(kk) + 1e-3 * np.sin(np.arange(kk))
        g.dia_set_sigdia(tab)
        assert same_bytes(g.dia_sigdia(), tab)
        g.dia_select("umfll vmfltdl temp")
        assert g.dia_get("umfll").shape[0] == kk
        with pytest.raises(BlomGpuError, match="uflx"):
            g.dia_get("uflx")                                        # class names add no dependencies
        assert g.step(0, 2) == 2
        u2, v2, t2 = g.dia_get("umfll"), g.dia_get("vmfltdl"), g.dia_get("temp")
        assert g.dia_nacc() == 2
        bad = tab.copy()
        bad[2] = np.nan
        for arg, word in ((tab[:-1], "kdm"), (np.append(tab, 40.0), "kdm"), (bad, "not finite"), (tab + 1.0, "selected"), (None, "selected")):
            with pytest.raises(BlomGpuError, match=word):
                g.dia_set_sigdia(arg)
            assert same_bytes(g.dia_sigdia(), tab)
            assert same_bytes(g.dia_get("umfll"), u2) and same_bytes(g.dia_get("vmfltdl"), v2) and same_bytes(g.dia_get("temp"), t2)
            assert g.dia_nacc() == 2
        with pytest.raises(BlomGpuError, match="nonsensel"):
            g.dia_select("umfll nonsensel")
        assert same_bytes(g.dia_get("umfll"), u2) and g.dia_nacc() == 2
        # without a class name selected the table may change; a wrong length or a NaN still may not
        g.dia_select("temp")
        for arg, word in ((tab[:-1], "kdm"), (bad, "not finite")):
            with pytest.raises(BlomGpuError, match=word):
                g.dia_set_sigdia(arg)
            assert same_bytes(g.dia_sigdia(), tab)
        g.dia_set_sigdia(tab + 1.0)
        assert same_bytes(g.dia_sigdia(), tab + 1.0)
        g.dia_set_sigdia(None)
        assert g.dia_sigdia().shape == (0,)
        with pytest.raises(BlomGpuError, match="sigdia"):
            g.dia_select("temp vmfll")
        assert np.abs(g.dia_get("temp")).max() == 0.0                # the refused list left the selection of "temp" alone
        with pytest.raises(BlomGpuError, match="vmfll"):
            g.dia_get("vmfll")
        # plevel never writes sigint; the hybrid coordinate is admitted
        g.dia_set_sigdia(tab)
        g.set("vcoord_type", "plevel")
        with pytest.raises(BlomGpuError, match="sigint"):
            g.dia_select("temp umfll")
        with pytest.raises(BlomGpuError, match="vmfll"):
            g.dia_get("vmfll")
        g.set("vcoord_type", "cntiso_hybrid")
        g.dia_select("temp umfll")
        assert g.dia_get("umfll").shape[0] == kk
        g.set("vcoord_type", "plevel")                               # ... and a selection made before the coordinate changed is refused at the step
        with pytest.raises(BlomGpuError, match="sigint"):
            g.step(2, 1)
        g.set("vcoord_type", "isopyc_bulkml")
    finally:
        g.close()


def test_interface_and_refusals():
    check_interface()


# ---- 5. independence, finalize, reset -----------------------------------------------------------------------------------------------------
def check_independence_finalize_reset():
    r = sig_run("chan_s_tke")
    assert same_bytes(r["A_sigdia"], r["tabs"]["ref"])
    # the six names change no byte of the other accumulators and none of the model state (sigint is theirs to write)
    bad = differing(r["A4_lyr"], r["C4_lyr"])
    assert not bad, bad
    bad = [nm for nm in r["C4_state"] if nm != "sigint" and not same_bytes(r["A4_state"][nm], r["C4_state"][nm])]
    assert not bad, bad
    assert all((np.abs(r["A4_lyr"][nm]) > 0.0).any() for nm in ["temp", "sealv"] + LEVEL_NAMES)
    # finlyr's list (:2597-2611) does not hold them
    assert not differing(r["A4_fin"], r["A4"]["ref"])
    assert not differing(r["A_reset"], r["init"]) and r["A_reset_nacc"] == 0
    assert not differing(r["A8"], r["B8"]), differing(r["A8"], r["B8"])
    assert r["A8_nacc"] == 4 and r["B8_nacc"] == 4
    assert (np.abs(r["A8"]["umfll"]) > 0.0).any()


def test_independence_finalize_reset():
    check_independence_finalize_reset()


# ---- 6. tiles ---------------------------------------------------------------------------------------------------------------------------
def check_tiles(monkeypatch):
    """test_gpu_diaacc.check_tiles on a 2x1 group with the six names added to its selection and the table set on every tile: the u
    columns at i = 1 of the second tile read the first tile's sigint, those of the first tile the second's across the periodic seam"""
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu
    tab = tables_for("chan_s_tke")["half"]

    def options(g):
        _LAYER_OPTIONS(g)
        g.dia_set_sigdia(tab)
    monkeypatch.setattr(lyr, "options", options)
    monkeypatch.setattr(lyr, "admitted", lambda case: _LAYER_ADMITTED(case) + NAMES)
    # sigint itself on the tiles: every context hands over its sigint as it is closed (the two tiles in their order, then the single tile)
    seen, close = [], BlomGpu.close

    def closing(self):
        if self.ctx:
            seen.append((self.idm, self.get("sigint")))
        close(self)
    monkeypatch.setattr(BlomGpu, "close", closing)
    lyr.check_tiles()
    case = make_case("chan_s_tke")
    ii, jj = case.idm // 2, case.jdm
    (t0, t1), (whole,) = [a for n, a in seen if n == ii], [a for n, a in seen if n == case.idm]
    rows = slice(4, 4 + jj)
    # the one-point halo is the neighbour tile's owned column: inside the domain, and across the periodic seam
    assert same_bytes(t1[:, rows, 3], t0[:, rows, 3 + ii]) and same_bytes(t0[:, rows, 4 + ii], t1[:, rows, 4])
    assert same_bytes(t0[:, rows, 3], t1[:, rows, 3 + ii]) and same_bytes(t1[:, rows, 4 + ii], t0[:, rows, 4])
    # ... and the owned wet points are the single tile's window (the formula of :1372-1390, pinned on the single tile by check_sigint)
    ip = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)[2].reshape(jj + 8, case.idm + 8)
    for px, t in enumerate((t0, t1)):
        wet = ip[rows, 4 + px * ii:4 + (px + 1) * ii] > 0
        assert wet.any() and same_bytes(t[:, rows, 4:4 + ii][:, wet], whole[:, rows, 4 + px * ii:4 + (px + 1) * ii][:, wet]), px
    assert np.abs(t0[:, rows, 4 + ii]).max() > 0.0


def test_tiles_accumulate_their_window_of_the_single_tile(monkeypatch):
    check_tiles(monkeypatch)


# ---- 7. the graph option --------------------------------------------------------------------------------------------------------------------
def check_graph_replay(expect_replays):
    r = sig_run("chan_s_tke")
    case, masks, g = full_context("chan_s_tke")
    try:
        g.set("use_graph", 1)
        g.dia_set_sigdia(r["tabs"]["ref"])
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
    """cntiso_hybrid: the stage takes the sigint it finds (ale_regrid_remap's) and only exchanges its halo"""
    case, masks, g = dyncore_context("chan_s", vcoord_type="cntiso_hybrid")
    try:
        kk, ii, jj = case.kdm, case.idm, case.jdm
        nj, ni = jj + 8, ii + 8
        y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / ii
        si = np.stack([24.0 + 0.9 * k + 0.4 * np.sin(x + 0.3 * k) * (0.5 + y) + 0.3 * y for k in range(kk)])
        si[4][:, ::3] = si[0][:, ::3] - 0.6                          # an inversion in every third column, under layers that advanced kup
        si[:, :4, :] = -7.0                                           # what the halo holds beforehand must not matter ...
        si[:, :, :4] = -7.0
        si[:, :, 4 + ii:] = -7.0
        g.put("sigint", si)
        idx = hostinit.step_indices(0, kk)
        nn = idx[3]
        for f, amp in (("uflx", 3.0e6), ("umfltd", 2.0e5), ("umflsm", -1.0e5), ("vflx", 2.0e6), ("vmfltd", 1.0e5), ("vmflsm", 4.0e4)):
            a = g.get(f)
            for k in range(kk):
                a[nn + k] = amp * np.cos(x * (1 + k % 3) + k) * (1.0 + y) / (1.0 + k)
            g.put(f, a)
        tab = np.linspace(24.2, 24.0 + 0.9 * (kk - 2), kk)             # (the deepest interfaces lie beyond the last class)
        g.dia_set_sigdia(tab)
        g.dia_select(NAMES)
        ref = RestatedSig(case, masks, NAMES, tab)
        for it in range(2):
            g.diaacc(*idx)
            after = g.get("sigint")
            assert same_bytes(after[:, 4:4 + jj, 4:4 + ii], si[:, 4:4 + jj, 4:4 + ii])      # the owned points are the caller's
            assert same_bytes(after[:, 4:4 + jj, 3], si[:, 4:4 + jj, 3 + ii])               # ... the periodic halo is exchanged
            ref.accumulate(g, 0)
        assert g.dia_nacc() == 2
        got = {nm: g.dia_get(nm) for nm in NAMES}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        for nm in NAMES:
            assert (np.abs(got[nm]) > 0.0).any(), nm
        for gr in "uv":
            assert all(ref.cover[gr][x] > 0 for x in COUNTERS), (gr, ref.cover[gr])
    finally:
        g.close()


def test_hybrid_coordinate_uses_the_sigint_it_finds():
    check_hybrid()


# ---- 9. full size ---------------------------------------------------------------------------------------------------------------------------
def put_submesoscale(g, case, masks):
    """isopyc_bulkml leaves umflsm / vmflsm as they were initialised -- zero (test_gpu_diaacc.MAY_REST) -- so two of the six names would
    bin zeros only.  A small smooth flux through the wet faces (1e-4 of the resolved flux or less) is put there before the first step;
    the model carries it along unchanged."""
    nj, ni = case.jdm + 8, case.idm + 8
    y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / case.idm
    for f, mk, amp in (("umflsm", "iu", 1.0e8), ("vmflsm", "iv", -0.6e8)):
        a = g.get(f)
        w = (masks[mk].reshape(nj, ni) > 0).astype(np.float64)
        for l in range(a.shape[0]):
            a[l] = amp * np.cos(3 * x + 0.7 * l) * (1.0 + y) * w / (1.0 + l % case.kdm)
        g.put(f, a)


def test_channel_size_class_set():
    """208x512x53: the six names (one wave per block, 53 bins per lane in LDS), two steps against the restatement"""
    tab = tables_for("channel_tke")["ref"]
    case, masks, a = full_context("channel_tke")
    _, _, b = full_context("channel_tke")
    try:
        for g in (a, b):
            put_submesoscale(g, case, masks)
            g.dia_set_sigdia(tab)
            g.dia_select(NAMES)
        assert a.step(0, 2) == 2
        ref = RestatedSig(case, masks, NAMES, tab)
        for ns in range(2):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
        got = {nm: a.dia_get(nm) for nm in NAMES}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        assert a.dia_nacc() == 2
        print("channel_tke coverage:", ref.cover)
        for nm in NAMES:
            assert np.abs(got[nm]).max() > 0.0, nm
    finally:
        a.close()
        b.close()
