"""templvl salnlvl uvellvl vvellvl under vcoord_type = 'cntiso_hybrid' / 'plevel' (blom_amd/csrc/stage_ale.hip: k_ale_zl_edges, the engine's
maps with n_dst = ddm, k_ale_zl_add; blomgpu_dia_alarm, blomgpu_ale_remap_diazlv).

A CROSS-CHECK WITH RESTATED GLUE, not a run of the reference's routine: remap_trc_diazlv_jslice and the velocity blocks of
phy/mod_ale_regrid_remap.F90 cannot be run, because the real module is compiled against a mod_dia stand-in whose accumulation flags are
zero.  The check is pinned one level down.  The heavy part -- prepare_reconstruction, reconstruct, prepare_remapping, remap with n_dst = ddm
-- goes through the compiled reference's own mod_hor3map (h3m_cases.run_ref, oracle/_ref/hor3map/libhor3mapref.so); where that library is
absent, through the device engine of blom_amd.hor3map, which tests/test_gpu_hor3map.py pins on the reference.  Only the glue is restated
in numpy below, each line with the line of phy/mod_ale_regrid_remap.F90 it restates: the column copy, the q rescaling, the target edges,
the additions, the masks.  The states the samples are formed from are downloaded from a second context that has no selection.
Everything is compared with ==, byte for byte over the whole padded array.

tests/test_hostemu_dia_hybrid.py runs the same functions on the host emulation of the library."""
import threading

import numpy as np
import pytest

from blom_amd.cases import make_case
from blom_amd import hostinit
from parity import STATE_FIELDS
import h3m_cases

pytestmark = pytest.mark.gpu

NAMES = ["templvl", "salnlvl", "uvellvl", "vvellvl"]
GRID = dict(templvl="p", salnlvl="p", uvellvl="u", vvellvl="v")
OTHERS = ["dzlvl", "uflxlvl", "bfsqlvl", "temp"]        # what else test 3 selects: level rows of k_dialvl and a weighted layer row
FILL = 9.9692099683868690e+36                            # nf90_fill_double
EDGES35 = [0.0, 5.0, 15.0, 25.0, 40.0, 62.5, 87.5, 112.5, 137.5, 175.0, 225.0, 275.0, 350.0, 450.0, 550.0, 650.0, 750.0, 850.0, 950.0,
           1050.0, 1150.0, 1250.0, 1350.0, 1450.0, 1625.0, 1875.0, 2250.0, 2750.0, 3250.0, 3750.0, 4250.0, 4750.0, 5250.0, 5750.0,
           6250.0, 8000.0]                               # depthslev_bnds, phy/mod_dia.F90:119-128
METHOD = dict(plm=h3m_cases.PLM, ppm=h3m_cases.PPM, pqm=h3m_cases.PQM)
LIMITING = dict(monotonic=h3m_cases.MONOTONIC, non_oscillatory=h3m_cases.NON_OSCILLATORY)
STATE = ["p", "dp", "temp", "saln", "u", "v", "dpu", "dpv", "pu", "pv", "ub", "vb"]      # what the samples are formed from


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def differing(got, want):
    return [nm for nm in want if not same_bytes(got[nm], want[nm])]


def bnds_of(edges):
    e = np.asarray(edges, dtype=np.float64)
    return np.stack([e[:-1], e[1:]], axis=1)


def fmin(a, b):
    return np.where(a < b, a, b)          # MIN as amdflang lowers it


def ale_options(cfg, method):
    from test_xcheck_ale import OPTIONS
    base = cfg.split("_tk")[0]
    return dict(OPTIONS[base], regrid_method=method)


# ---- contexts --------------------------------------------------------------------------------------------------------------------------
def hybrid_context(cfg, vcoord, method, neutral=False, ntr=None):
    """the step of the hybrid coordinates as tests/test_gpu_tiles.py::test_hybrid_step_on_tiles sets it up, with the ALE option set of
    tests/test_xcheck_ale.py for the grid"""
    from blom_amd.gpu import BlomGpu
    from test_gpu_tiles import hybrid_inputs
    from test_xcheck_ale import set_device_ale_options
    case = make_case(cfg) if ntr is None else make_case(cfg, ntr=ntr)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    g = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(g, case)
    for nm, a in hybrid_inputs(case).items():
        g.put(nm, a)
    kk = case.kdm
    pbot = float(np.max(g.get("p")[kk][ip > 0]))
    g.set("vcoord_type", vcoord)
    set_device_ale_options(g, ale_options(cfg, method))
    g.set("mlrmth", "fox08")
    g.set("swamxd", 200.0)
    g.set("brine_mlbase_frac", 0.4)
    g.set_vector("plevel", 0.3 * pbot * (np.arange(kk) / kk) ** 1.3)
    g.set("ltedtp_opt", 2 if neutral else 1)
    g.set("ndiff_surface_align", 1)
    g.stage("cmnfld1", *hostinit.step_indices(0, kk))
    return case, masks, g


def window(g, nsteps, kk):
    """the reference's window of nsteps steps: the step after an output takes no sample at its start, the others do, the last one takes
    the end-of-step sample (phy/mod_ale_regrid_remap.F90:1524-1531, :2014-2017)"""
    g.dia_alarm(1)
    assert g.step(0, 1) == 1
    g.dia_alarm(0)
    assert g.step(1, nsteps - 1) == nsteps
    g.dia_alarm(1)
    g.ale_remap_diazlv(*hostinit.step_indices(nsteps - 1, kk))


# ---- the glue, restated -----------------------------------------------------------------------------------------------------------------
class Restated:
    """the four accumulators of one tile, summed from samples of downloaded states"""

    def __init__(self, case, masks, depths, bnds, opts, names=NAMES):
        self.case, self.kk, self.names = case, case.kdm, list(names)
        self.bnds = np.asarray(bnds, dtype=np.float64)
        self.ddm = len(self.bnds)
        nj, ni = case.jdm + 8, case.idm + 8
        self.shape, self.ni = (nj, ni), ni
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + case.jdm, 4:4 + case.idm] = True                    # i = 1..ii, j = 1..jj
        self.own = own
        self.cols = {g: np.flatnonzero((own & (self.mask[g] > 0)).ravel()) for g in "puv"}
        d = np.asarray(depths, dtype=np.float64).reshape(nj, ni)
        # pbath, ubath, vbath: phy/mod_dia.F90:1074-1091
        self.bath = {"p": d, "u": fmin(d, np.roll(d, 1, axis=1)), "v": fmin(d, np.roll(d, 1, axis=0))}
        self.method = METHOD[opts["reconstruction_method"]]
        self.ord = (int(opts["upper_bndr_ord"]), int(opts["lower_bndr_ord"]))
        lt = LIMITING[opts["tracer_limiting"]]
        # tracer_limiting = non_oscillatory: T keeps it, S gets non_oscillatory_posdef (:1419-1431)
        ls = h3m_cases.NON_OSCILLATORY_POSDEF if lt == h3m_cases.NON_OSCILLATORY else lt
        tpc = (opts["tracer_pc_upper_bndr"], opts["tracer_pc_lower_bndr"])
        vpc = (opts["velocity_pc_upper_bndr"], opts["velocity_pc_lower_bndr"])
        self.src = dict(templvl=(lt,) + tpc, salnlvl=(ls,) + tpc, uvellvl=(LIMITING[opts["velocity_limiting"]],) + vpc,
                        vvellvl=(LIMITING[opts["velocity_limiting"]],) + vpc)
        self.cover = dict(below=0, level_spans_layers=0, layer_spans_levels=0, massless=0, q_u=0, q_v=0, coincide=0)
        self.reset()

    def reset(self):
        self.acc = {nm: np.repeat((0.0 * self.mask[GRID[nm]].astype(np.float64))[None], self.ddm, axis=0).copy() for nm in self.names}

    def engine(self, nm, x_src, u_src, x_dst):
        """prepare_reconstruction -> reconstruct -> prepare_remapping -> remap of the reference's own mod_hor3map, n_dst = ddm"""
        lim, pcl, pcr = self.src[nm]
        run = h3m_cases.run_ref if h3m_cases.have_ref() else h3m_cases.run_gpu
        x_src, u_src, x_dst = (np.ascontiguousarray(a, dtype=np.float64) for a in (x_src, u_src, x_dst))
        lo, hi = u_src.min(1, keepdims=True), u_src.max(1, keepdims=True)
        r = run(self.method, self.ord[0], self.ord[1], lim, pcl, pcr, x_src, u_src, x_dst, np.ascontiguousarray(.5 * (lo + hi)), h3m_cases.METHOD_1)
        bad = r["errs"][:, [0, 1, 4, 5]]
        assert not bad.any(), (nm, "errstat", bad[np.flatnonzero(bad.any(axis=1))[:3]])
        self.cover["massless"] += int((r["n_act"] < self.kk).any())
        return r["u_dst"]

    def edges(self, g, x_src):
        """:1082-1088 | :1820-1826 | :1916-1922; x_src: (ncol, kk+1)"""
        c, ddm = self.cols[g], self.ddm
        q = 1.0 / self.bath[g].ravel()[c]                                                    # q = 1._r8/pbath(i,j)
        p1, pb = x_src[:, 0], x_src[:, self.kk]
        x = np.empty((len(c), ddm + 1))
        x[:, 0] = p1                                                                          # p_dst(1) = p_src(1,i)
        for kd in range(1, ddm):
            x[:, kd] = fmin(self.bnds[kd, 0] * q, np.float64(1.0)) * (pb - p1) + p1           # min(bnds(1,kd)*q, 1)*(p_src(kk+1) - p_src(1)) + p_src(1)
        x[:, ddm] = pb                                                                        # p_dst(ddm+1) = p_src(kk+1,i)
        # what the columns exercise (test 2)
        inner = x_src[:, 1:self.kk]
        cv = self.cover
        cv["below"] += int((x[:, ddm - 1] == pb).any())                                       # the last level (at least) is empty: wholly below the bottom
        for d in range(ddm):
            inside = (inner > x[:, d:d + 1]) & (inner < x[:, d + 1:d + 2])
            cv["level_spans_layers"] += int(inside.any())
        for k in range(self.kk):
            inside = (x[:, 1:ddm] > x_src[:, k:k + 1]) & (x[:, 1:ddm] < x_src[:, k + 1:k + 2])
            cv["layer_spans_levels"] += int(inside.any())
        live = (inner > p1[:, None]) & (inner < pb[:, None])
        cv["coincide"] += int(((x[:, 1:ddm, None] == inner[:, None, :]) & live[:, None, :]).any())
        return x

    def p_src(self, st, lev):
        """:207-210: p_src(1) = p(i,j,1), p_src(k+1) = p_src(k) + dp(i,j,k+lev)"""
        c, kk = self.cols["p"], self.kk
        x = np.empty((len(c), kk + 1))
        x[:, 0] = st["p"][0][c]
        for k in range(kk):
            x[:, k + 1] = x[:, k] + st["dp"][k + lev][c]
        return x

    def uv_src(self, st, g, lev, util):
        """:1767-1776 (old dpu, util1) | :2060-2069 (dpu(km), p as it stands): pu(k+1) = pu(k) + dpu(k+lev); q = min(util(i-1,j), util(i,j))/pu(kk+1);
        p_src(k) = pu(k)*q"""
        c, kk = self.cols[g], self.kk
        pz, dpz = (st["pu"], st["dpu"]) if g == "u" else (st["pv"], st["dpv"])
        x = np.empty((len(c), kk + 1))
        x[:, 0] = pz[0][c]
        for k in range(kk):
            x[:, k + 1] = x[:, k] + dpz[k + lev][c]
        q = fmin(util[c - (1 if g == "u" else self.ni)], util[c]) / x[:, kk]
        self.cover["q_" + g] += int((q != 1.0).any())
        return x * q[:, None]

    def sample(self, st, nstep, end):
        """the start-of-step sample of the step that starts from step count nstep (time level n, :1674-1677, :1817-1853, :1913-1949), or the
        end-of-step sample of that step (time level m, ale_remap_diazlv :1986-2201); st: the state downloaded before | after the step"""
        kk = self.kk
        m, n, mm, nn, k1m, k1n = hostinit.step_indices(nstep, kk)
        lev, bt = (mm, m - 1) if end else (nn, n - 1)
        with np.errstate(all="ignore"):
            if "templvl" in self.acc or "salnlvl" in self.acc:
                c = self.cols["p"]
                xs = self.p_src(st, lev)
                xd = self.edges("p", xs)
                for nm, f in (("templvl", "temp"), ("salnlvl", "saln")):
                    if nm in self.acc:
                        rm = self.engine(nm, xs, st[f][lev:lev + kk][:, c].T, xd)
                        a = self.acc[nm].reshape(self.ddm, -1)
                        a[:, c] = a[:, c] + rm.T                                              # phylvl = phylvl + trc_rm(kd), :1107-1110
            # util1 = p(kk+1) before p is rebuilt (:1720) | p(kk+1) as it stands at the end of the step (:2066): the downloaded array both times
            util = st["p"][kk]
            for nm, g, f, b in (("uvellvl", "u", "u", "ub"), ("vvellvl", "v", "v", "vb")):
                if nm not in self.acc:
                    continue
                c = self.cols[g]
                xs = self.uv_src(st, g, lev, util)
                xd = self.edges(g, xs)
                rm = self.engine(nm, xs, st[f][lev:lev + kk][:, c].T, xd)
                a = self.acc[nm].reshape(self.ddm, -1)
                a[:, c] = (a[:, c] + rm.T) + st[b][bt][None, c]                               # phylvl + v_rm_diazlv(kd) + ub(i,j,n | m), :1846-1848

    def msklvl(self):
        """phy/mod_dia.F90:6659-6738 on p / u / v (:2650-2651, :2674-2675): levels kmax+1..ddm of every owned point become nf90_fill_double"""
        out = {}
        for nm in self.names:
            bath = self.bath[GRID[nm]]
            kmax = np.zeros(self.shape, np.int64)
            for k in range(self.ddm):
                kmax[bath > self.bnds[k, 0]] = k + 1
            a = self.acc[nm].copy()
            for k in range(self.ddm):
                a[k][self.own & (k + 1 > kmax)] = FILL
            out[nm] = a
        return out


def download(g):
    nj_ni = g.nj * g.ni
    return {nm: g.get(nm).reshape(-1, nj_ni) for nm in STATE}


# ---- one pair of runs per case, shared -------------------------------------------------------------------------------------------------
_STATES, _RUNS = {}, {}
NSTEPS = 4
# (grid, vcoord_type, regrid_method): PLM, PPM and PQM, both piecewise-constant boundary flags (tests/test_xcheck_ale.py: OPTIONS)
CASES = [("chan_s", "cntiso_hybrid", "nudge"), ("box_s", "cntiso_hybrid", "direct"), ("tri_s", "plevel", "direct")]
FUK95 = ("fuk95", "cntiso_hybrid", "nudge")           # the option set of the reference's tests/fuk95/limits: ppm, 6/4, non-oscillatory, nudge


def massless_bottom(g, case):
    """two massless bottom layers in every fifth column (their mass goes to the layer above, so the column keeps its bottom pressure)"""
    kk = case.kdm
    nj, ni = case.jdm + 8, case.idm + 8
    fifth = ((np.arange(nj)[:, None] * 3 + np.arange(ni)[None, :]) % 5 == 0)
    dp = g.get("dp")
    for lev in (0, kk):
        dp[lev + kk - 3][fifth] += dp[lev + kk - 2][fifth] + dp[lev + kk - 1][fifth]
        dp[lev + kk - 2][fifth] = 0.0
        dp[lev + kk - 1][fifth] = 0.0
    g.put("dp", dp)


def states(key):
    """context B: no selection; the state before each of the window's steps that samples at its start, and after the last one"""
    if key in _STATES:
        return _STATES[key]
    cfg, vcoord, method = key[:3]
    kw = dict(key[3:])
    case, masks, b = hybrid_context(cfg, vcoord, method, **kw)
    try:
        r = dict(case=case, masks=masks, depths=b.get("depths")[0].copy(), st={})
        assert b.step(0, 1) == 1
        for ns in range(1, NSTEPS):
            r["st"][ns] = download(b)
            assert b.step(ns, 1) == ns + 1
        r["st"]["end"] = download(b)
        r["state"] = {nm: b.get(nm) for nm in STATE_FIELDS if b.has_field(nm)}
    finally:
        b.close()
    _STATES[key] = r
    return r


def expected(key, bnds):
    s = states(key)
    ref = Restated(s["case"], s["masks"], s["depths"], bnds, ale_options(key[0], key[2]))
    init = {nm: v.copy() for nm, v in ref.acc.items()}
    for ns in range(1, NSTEPS):
        ref.sample(s["st"][ns], ns, end=False)
    ref.sample(s["st"]["end"], NSTEPS - 1, end=True)
    return ref, init


def device(key, edges=None):
    """context A: the four names selected, the reference's window, dia_finalize"""
    rk = (key, tuple(edges) if edges is not None else None)
    if rk in _RUNS:
        return _RUNS[rk]
    cfg, vcoord, method = key[:3]
    case, masks, a = hybrid_context(cfg, vcoord, method, **dict(key[3:]))
    try:
        if edges is not None:
            a.dia_set_levels(bnds_of(edges))
        r = dict(bnds=a.dia_levels())
        a.dia_alarm(1)                                               # (a declared alarm admits the names)
        a.dia_select(NAMES)
        r["init"] = {nm: a.dia_get(nm) for nm in NAMES}
        window(a, NSTEPS, case.kdm)
        r["got"] = {nm: a.dia_get(nm) for nm in NAMES}
        r["nacc"] = a.dia_nacc()
        r["state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
        a.dia_finalize()
        r["fin"] = {nm: a.dia_get(nm) for nm in NAMES}
    finally:
        a.close()
    _RUNS[rk] = r
    return r


def coinciding_table(key):
    """a short table with one bound that the target-edge formula maps EXACTLY onto a source interface of some owned wet p-column of a
    start-of-step sample: the bound is searched among the neighbours of bath*(p_src(k) - p_src(1))/(p_src(kk+1) - p_src(1))"""
    s = states(key)
    probe = Restated(s["case"], s["masks"], s["depths"], bnds_of(EDGES35), ale_options(key[0], key[2]))
    xs = probe.p_src(s["st"][2], hostinit.step_indices(2, probe.kk)[3])
    bath = probe.bath["p"].ravel()[probe.cols["p"]]
    p1, pb = xs[:, 0], xs[:, probe.kk]
    for col in range(len(bath)):
        for k in range(2, probe.kk):
            t = xs[col, k]
            if not (p1[col] < t < pb[col]) or xs[col, k] == xs[col, k - 1]:
                continue
            b0 = bath[col] * (t - p1[col]) / (pb[col] - p1[col])
            if not (60.0 < b0 < 0.9 * bath[col]):
                continue
            cand = [b0]
            for _ in range(16):
                cand = [np.nextafter(cand[0], -np.inf)] + cand + [np.nextafter(cand[-1], np.inf)]
            for b in cand:
                if fmin(b * (1.0 / bath[col]), np.float64(1.0)) * (pb[col] - p1[col]) + p1[col] == t:
                    return [0.0, 30.0, float(b), float(b) + 400.0, 8000.0]
    raise AssertionError("no bound found that coincides with a source interface")


# ---- 1. the reference's window -------------------------------------------------------------------------------------------------------------
def check_window(key, edges=None):
    r = device(key, edges)
    ref, init = expected(key, r["bnds"])
    s = states(key)
    print(key, "ddm", ref.ddm, "engine:", "reference mod_hor3map" if h3m_cases.have_ref() else "device engine", "cover", ref.cover)
    assert r["nacc"] == NSTEPS                                       # nacc counts as before: diaacc, once per step
    assert not differing(r["init"], init), differing(r["init"], init)
    bad = differing(r["got"], ref.acc)
    assert not bad, f"{key}: accumulators that differ from the restated sums of the {NSTEPS - 1} + 1 samples: {bad}"
    nj, ni = s["case"].jdm + 8, s["case"].idm + 8
    for nm in NAMES:
        sel = ref.own & (ref.mask[GRID[nm]] > 0)
        assert same_bytes(r["got"][nm][:, ~sel], np.zeros((ref.ddm, int((~sel).sum())))), nm      # 0. everywhere else
        assert (np.abs(r["got"][nm]) > 0.0).any(), nm
    bad = differing(r["fin"], ref.msklvl())
    assert not bad, f"{key}: finalised accumulators that differ from the restated msklvl: {bad}"
    t = r["fin"]["templvl"][:, 4:-4, 4:-4]
    assert (t == FILL).any() and (t != FILL).any()
    # the selection changes no byte of the model state
    bad = [nm for nm in s["state"] if not same_bytes(r["state"][nm], s["state"][nm])]
    assert not bad, bad
    return ref


@pytest.mark.parametrize("key", CASES + [FUK95], ids=lambda k: "-".join(k))
def test_window_equals_the_restated_sums(key):
    check_window(key)


def check_short_table(key):
    edges = coinciding_table(key)
    ref = check_window(key, edges)
    assert ref.cover["coincide"] > 0, "no bound of the short table coincides with a source interface"


@pytest.mark.parametrize("key", CASES, ids=lambda k: "-".join(k))
def test_short_table_with_a_bound_on_a_source_interface(key):
    check_short_table(key)


# ---- 2. coverage: test 1 cannot pass vacuously -----------------------------------------------------------------------------------------------
def check_coverage():
    total = {}
    for key in CASES:
        r = device(key)
        ref, _ = expected(key, r["bnds"])
        print(key, ref.cover)
        for k, v in ref.cover.items():
            total[k] = total.get(k, 0) + v
        # every case by itself: an empty level below the bottom, a level over several layers, a layer over several levels
        assert ref.cover["below"] > 0 and ref.cover["level_spans_layers"] > 0 and ref.cover["layer_spans_levels"] > 0, (key, ref.cover)
    assert total["massless"] > 0, "no column with massless bottom layers (n_src_actual < kk)"
    assert total["q_u"] > 0 and total["q_v"] > 0, "no u- / v-point whose neighbouring bottoms differ"
    # ... and a state made for it: two massless bottom layers in every fifth column, one sample of each kind on it
    key = CASES[0]
    case, masks, g = hybrid_context(*key)
    try:
        g.dia_alarm(0)
        g.dia_select(NAMES)
        assert g.step(0, 1) == 1
        g.dia_reset()
        massless_bottom(g, case)
        ref = Restated(case, masks, g.get("depths")[0], g.dia_levels(), ale_options(key[0], key[2]))
        before = download(g)
        assert g.step(1, 1) == 2
        ref.sample(before, 1, end=False)
        assert ref.cover["massless"] > 0
        g.dia_alarm(1)
        ref.sample(download(g), 1, end=True)
        g.ale_remap_diazlv(*hostinit.step_indices(1, case.kdm))
        got = {nm: g.dia_get(nm) for nm in NAMES}
        assert not differing(got, ref.acc), differing(got, ref.acc)
    finally:
        g.close()


def test_the_cases_cover_the_remap():
    check_coverage()


# ---- 3. the alarm's gating -------------------------------------------------------------------------------------------------------------------
def check_gating():
    key = CASES[0]
    s = states(key)
    kk = s["case"].kdm
    runs = {}
    for tag, names, alarm in (("one", NAMES + OTHERS, 1), ("zero", NAMES + OTHERS, 0), ("without", OTHERS, None)):
        case, masks, g = hybrid_context(*key)
        try:
            if alarm is not None:
                g.dia_alarm(alarm)
            g.dia_select(names)
            r = dict(init={nm: g.dia_get(nm) for nm in names})
            assert g.step(0, 2) == 2
            r["stepped"] = {nm: g.dia_get(nm) for nm in names}
            r["before_end"] = download(g)
            g.ale_remap_diazlv(*hostinit.step_indices(1, kk))
            r["ended"] = {nm: g.dia_get(nm) for nm in names}
            r["state"] = {nm: g.get(nm) for nm in STATE_FIELDS if g.has_field(nm)}
            r["bnds"], r["depths"], r["case"], r["masks"] = g.dia_levels(), g.get("depths")[0], case, masks
            runs[tag] = r
        finally:
            g.close()
    one, zero, wo = runs["one"], runs["zero"], runs["without"]
    four = lambda d: {nm: d[nm] for nm in NAMES}
    # alarm 1: the steps add nothing, ale_remap_diazlv adds one end-of-step sample
    assert not differing(four(one["stepped"]), four(one["init"]))
    ref = Restated(one["case"], one["masks"], one["depths"], one["bnds"], ale_options(key[0], key[2]))
    ref.sample(one["before_end"], 1, end=True)
    assert not differing(four(one["ended"]), ref.acc), differing(four(one["ended"]), ref.acc)
    # alarm 0: the steps add (both of them: no output went before), ale_remap_diazlv adds nothing
    assert len(differing(four(zero["stepped"]), four(zero["init"]))) == 4
    assert not differing(four(zero["ended"]), four(zero["stepped"]))
    # the other accumulators and the model state do not see the four names
    for r in (one, zero):
        bad = differing({nm: r["ended"][nm] for nm in OTHERS}, {nm: wo["ended"][nm] for nm in OTHERS})
        assert not bad, bad
        bad = [nm for nm in wo["state"] if not same_bytes(r["state"][nm], wo["state"][nm])]
        assert not bad, bad
    for nm in OTHERS:
        assert (np.abs(wo["ended"][nm]) > 0.0).any(), nm


def test_the_alarm_gates_the_two_samples():
    check_gating()


# ---- 4. refusals and what must not change -----------------------------------------------------------------------------------------------------
def check_refusals():
    from blom_amd.gpu import BlomGpuError
    from test_gpu_diaacc import dyncore_context
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)
    _, _, b = dyncore_context("chan_s", cmnfld1=1)
    try:
        assert (len(g.dia_names()), len(g.dia_names_all()), len(g.dia_names_full()), len(g.dia_names_ext())) == (111, 117, 123, 133)
        six = hostinit.step_indices(0, case.kdm)
        with pytest.raises(BlomGpuError, match="isopyc_bulkml"):
            g.ale_remap_diazlv(*six)
        with pytest.raises(BlomGpuError, match="blomgpu_dia_alarm.*0 or 1"):
            g.dia_alarm(2)
        with pytest.raises(BlomGpuError, match="blomgpu_dia_alarm"):
            g.dia_alarm(-1)
        # isopyc_bulkml: the names are k_dialvl's and the alarm is ignored
        g.dia_select("templvl uvellvl")
        b.dia_select("templvl uvellvl")
        g.dia_alarm(0)
        assert g.step(0, 2) == 2 and b.step(0, 2) == 2
        t2 = g.dia_get("templvl")
        assert same_bytes(t2, b.dia_get("templvl")) and same_bytes(g.dia_get("uvellvl"), b.dia_get("uvellvl")) and np.abs(t2).max() > 0.0
    finally:
        g.close()
        b.close()
    # undeclared alarm under the hybrid coordinates: refused at the selection and at the step, with the old words; the selection stays
    case, masks, g = dyncore_context("chan_s", cmnfld1=1)
    try:
        g.dia_select("templvl uflxlvl")
        assert g.step(0, 1) == 1
        t1 = g.dia_get("templvl")
        for vc in ("cntiso_hybrid", "plevel"):
            g.set("vcoord_type", vc)
            for nm in NAMES:
                with pytest.raises(BlomGpuError, match=nm + ".*ale_regrid_remap.*has not been declared.*blomgpu_dia_alarm"):
                    g.dia_select("dzlvl " + nm)
            with pytest.raises(BlomGpuError, match="templvl.*ale_regrid_remap.*has not been declared.*blomgpu_dia_alarm"):
                g.step(1, 1)
            assert same_bytes(g.dia_get("templvl"), t1) and g.dia_nacc() == 1
            g.ale_remap_diazlv(*hostinit.step_indices(0, case.kdm))          # alarm undeclared: nothing
            assert same_bytes(g.dia_get("templvl"), t1)
        g.dia_alarm(0)
        g.dia_select("dzlvl templvl")                                        # declared: admitted
        g.dia_get("templvl")
    finally:
        g.close()


def test_refusals_and_non_changes():
    check_refusals()


# ---- 5. tiles --------------------------------------------------------------------------------------------------------------------------------
def check_tiles(cfg, npx, npy, vcoord, method, nsteps=3):
    """every tile's four accumulators are its window of the single tile's -- the u-points on a tile's west edge and the v-points on its
    south edge read p(kk+1) of the neighbour through the halo"""
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd.tiles import tile_extents, tile_window, scatter_state
    from test_gpu_tiles import _single, ALL, HYBRID_INPUTS, hybrid_inputs
    from test_xcheck_ale import set_device_ale_options
    case, masks, fields, ref = _single(cfg, nsteps)
    kk = case.kdm
    f = hybrid_inputs(case)
    for nm, a in f.items():
        ref.put(nm, a)
    if not np.abs(ref.get("depths")).max() > 0.0:
        ref.put("depths", hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)[1][None])
    pbot = float(np.max(ref.get("p")[kk][masks["ip"] > 0]))
    plevel = 0.3 * pbot * (np.arange(kk) / kk) ** 1.3
    ii, jj = tile_extents(case, npx, npy)
    grp = TileGroup(npx, npy)
    tiles = {}
    for py in range(npy):
        for px in range(npx):
            tm = {k: tile_window(masks[k], case, npx, npy, px, py) for k in masks}
            t = BlomGpu(ii, jj, kk, case.ntr, case.nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=px * ii, j0=py * jj)
            for nm, v in case.params.items():
                if not nm.endswith("0"):
                    t.set(nm, v)
            t.set("delt1", case.params["baclin"])
            grp.attach(t, px, py)
            tiles[(px, py)] = t
    scatter_state(ref, tiles, case, npx, npy, [nm for nm in ALL if nm in fields] + [nm for nm in HYBRID_INPUTS if nm in f] + ["depths"])

    def run_window(g):
        g.set("vcoord_type", vcoord)
        set_device_ale_options(g, ale_options(cfg, method))
        g.set("mlrmth", "fox08")
        g.set("swamxd", 200.0)
        g.set("brine_mlbase_frac", 0.4)
        g.set_vector("plevel", plevel)
        g.set("ltedtp_opt", 1)
        g.stage("cmnfld1", *hostinit.step_indices(0, kk))
        g.dia_alarm(1)
        g.dia_select(NAMES)
        window(g, nsteps, kk)
    errs = []

    def run(t):
        try:
            run_window(t)
            t.sync()
        except Exception as e:          # a failing tile would leave the others at a barrier
            errs.append(e)
    try:
        run_window(ref)
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x.start() for x in th]
        [x.join(timeout=300) for x in th]
        assert not errs, errs
        bad = []
        for nm in NAMES:
            whole = ref.dia_get(nm)
            assert (np.abs(whole) > 0.0).any(), nm
            for (px, py), t in tiles.items():
                mine = t.dia_get(nm)[:, 4:4 + jj, 4:4 + ii]
                if not same_bytes(mine, whole[:, 4 + py * jj:4 + (py + 1) * jj, 4 + px * ii:4 + (px + 1) * ii]):
                    bad.append((nm, px, py))
        assert not bad, bad
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


@pytest.mark.parametrize("cfg,npx,npy,vcoord,method", [("chan_s", 2, 1, "cntiso_hybrid", "nudge"), ("chan_s", 1, 2, "plevel", "direct"),
                                                       ("tri_s", 2, 2, "cntiso_hybrid", "nudge")])
def test_tiles_hold_their_window_of_the_single_tile(cfg, npx, npy, vcoord, method):
    check_tiles(cfg, npx, npy, vcoord, method)


# ---- 6. neutral diffusion (the stage's side streams are busy), more tracers than one engine batch ------------------------------------------------
NEUTRAL = ("chan_s", "cntiso_hybrid", "nudge", ("neutral", True))
MANY = ("tri_s", "cntiso_hybrid", "direct", ("ntr", 9))        # T, S + 9 tracers: two batches of the engine's *_many calls, T and S in the first


@pytest.mark.parametrize("key", [NEUTRAL, MANY], ids=["neutral", "eleven_fields"])
def test_window_with_neutral_diffusion_and_with_many_tracers(key):
    check_window(key)


# ---- 7. the graph option ----------------------------------------------------------------------------------------------------------------------------
def check_graph_option(expect_replays):
    key = CASES[0]
    out = {}
    for tag, graph in (("plain", 0), ("graph", 1)):
        case, masks, g = hybrid_context(*key)
        try:
            g.set("use_graph", graph)
            g.dia_alarm(0)
            g.dia_select(NAMES)
            # (a capture waits for two plain steps after the last change; the time step changes after the first step of a run)
            assert g.step(0, 5) == 5                                 # alarm 0: captured in step 3, replayed with the in-step launches
            mid = {nm: g.dia_get(nm) for nm in NAMES}
            g.dia_alarm(1)
            assert g.step(5, 3) == 8                                 # alarm 1: a replay of the other value's graph would go on adding
            after = {nm: g.dia_get(nm) for nm in NAMES}
            assert not differing(after, mid), differing(after, mid)
            g.ale_remap_diazlv(*hostinit.step_indices(7, case.kdm))
            g.dia_alarm(0)
            assert g.step(8, 3) == 11
            out[tag] = {nm: g.dia_get(nm) for nm in NAMES}
            assert g.dia_nacc() == 11
            if graph and expect_replays:
                assert g.get_real("graph_steps") >= 3, "no step was replayed as a graph under either value of the alarm"
        finally:
            g.close()
    assert not differing(out["graph"], out["plain"]), differing(out["graph"], out["plain"])
    for nm in NAMES:
        assert (np.abs(out["plain"][nm]) > 0.0).any(), nm


def test_graph_replay_follows_the_alarm():
    import os
    check_graph_option(expect_replays=os.environ.get("BLOM_HOSTEMU") != "1")


# ---- 8. reset, independence ---------------------------------------------------------------------------------------------------------------------------
def check_reset_and_independence():
    key = CASES[1]
    r = device(key)
    case, masks, a = hybrid_context(*key)
    _, _, b = hybrid_context(*key)
    try:
        a.dia_alarm(0)
        b.dia_alarm(1)
        a.dia_select(NAMES)
        b.dia_select(NAMES)
        assert a.step(0, 2) == 2 and b.step(0, 2) == 2
        ga, gb = {nm: a.dia_get(nm) for nm in NAMES}, {nm: b.dia_get(nm) for nm in NAMES}
        assert len(differing(ga, r["init"])) == 4                    # a has sampled twice ...
        assert not differing(gb, r["init"])                          # ... b, whose alarm is 1, not at all
        a.dia_reset()
        assert not differing({nm: a.dia_get(nm) for nm in NAMES}, r["init"]) and a.dia_nacc() == 0
        assert b.dia_nacc() == 2
        # after the reset a goes through the window, stepping on from its state: its own sums, b still untouched
        b.ale_remap_diazlv(*hostinit.step_indices(1, case.kdm))
        assert len(differing({nm: b.dia_get(nm) for nm in NAMES}, r["init"])) == 4
        assert not differing({nm: a.dia_get(nm) for nm in NAMES}, r["init"])
    finally:
        a.close()
        b.close()


def test_reset_and_two_contexts():
    check_reset_and_independence()
