"""diaacc on the device (blom_amd/csrc/stage_diaacc.hip): the time-mean diagnostics of phy/mod_dia.F90 accumulated by blomgpu_step.

No reference library is needed: the expected values are the reference's loops restated in numpy below -- acch2d (:5182-5281),
maxh2d (:5285-5343), sqh2d (:5409-5467), acclyr (:5471-5600), inih2d / inilyr (:5001-5113), finlyr (:6114-6185) with the sources
of diaacc's calls (:1148-1199, :1547-1913) -- the same operations in the same order in float64 (numpy does not contract), applied
to the arrays a second context downloads after each of its steps.  Everything is compared with ==, byte for byte over the whole
padded array: halo, land and the -0.0 that maxbld's -spval leaves on land included.

tests/test_hostemu_diaacc.py runs the small cases on the host emulation of the library."""
import threading

import numpy as np
import pytest

from blom_amd.cases import make_case
from blom_amd import hostinit
from parity import STATE_FIELDS

pytestmark = pytest.mark.gpu

ONEM = 9806.0                         # phy/mod_constants.F90
SPVAL = 1.0e33
EPSIL = 1.0e-11                       # :6126
FILL = 9.9692099683868690e+36         # nf90_fill_double

# ---- the table, restated from diaacc's calls: name -> (grid, field, level) with level "m" | "n" | "k1m" | "k1n" | "kk+1" | 0 ----
H2D = dict(
    ub=("u", "ub", "m"), ubflxs=("u", "ubflxs", "n"), taux=("u", "taux", 0), vb=("v", "vb", "m"), vbflxs=("v", "vbflxs", "n"),
    tauy=("v", "tauy", 0), psrf=("p", "p", 0), pbot=("p", "p", "kk+1"), sealv=("p", "z", 0), sigmx=("p", "sigma", "k1m"),
    swa=("p", "swa", 0), nsf=("p", "nsf", 0), hmltfz=("p", "hmltfz", 0), lip=("p", "lip", 0), sop=("p", "sop", 0), eva=("p", "eva", 0),
    fmltfz=("p", "fmltfz", 0), sfl=("p", "sfl", 0), rnfflx=("p", "rnf", 0), rfiflx=("p", "rfi", 0), ustar=("p", "ustar", 0),
    ustar3=("p", "ustar3", 0), idkedt=("p", "idkedt", 0), mtkeus=("p", "mtkeus", 0), mtkeni=("p", "mtkeni", 0),
    mtkebf=("p", "mtkebf", 0), mtkers=("p", "mtkers", 0), mtkepe=("p", "mtkepe", 0), mtkeke=("p", "mtkeke", 0),
    sss=("p", "saln", "k1m"), sst=("p", "temp", "k1m"), bld=("p", "dpml", 0), surflx=("p", "surflx", 0), salflx=("p", "salflx", 0),
    surrlx=("p", "surrlx", 0), salrlx=("p", "salrlx", 0), brnflx=("p", "brnflx", 0), brnpd=("p", "pbrnda", 0))
MAX2D = dict(maxbld=("p", "dpml", 0))
SQ2D = dict(slvsq=("p", "z", 0), ssssq=("p", "saln", "k1m"), sstsq=("p", "temp", "k1m"))
# layers: name -> (grid, field, first level, weight field at k1m or None)
_UF = "uflx utflx usflx umfltd umflsm utfltd utflsm utflld usfltd usflsm usflld".split()
LYR = dict(uvel=("u", "uvel", "k1m", "dpu"), dpu=("u", "dpu", "k1m", None))
LYR.update({nm: ("u", nm, "k1n", None) for nm in _UF})
LYR.update(vvel=("v", "vvel", "k1m", "dpv"), dpv=("v", "dpv", "k1m", None))
LYR.update({"v" + nm[1:]: ("v", "v" + nm[1:], "k1n", None) for nm in _UF})
LYR.update(saln=("p", "saln", "k1m", "dp"), temp=("p", "temp", "k1m", "dp"), dp=("p", "dp", "k1m", None), dz=("p", "dz", 0, None),
           bfsq=("p", "bfsql", 0, "dp"), difint=("p", "difint", 0, "dp"), difiso=("p", "difiso", 0, "dp"), difdia=("p", "difdia", 0, "dp"),
           tke=("p", "trc_tke", "k1m", "dp"), gls_psi=("p", "trc_gls", "k1m", "dp"))
TABLE = list(H2D) + list(MAX2D) + list(SQ2D) + list(LYR)
WEIGHTED = {nm: r[3] for nm, r in LYR.items() if r[3]}           # the pairs finlyr is called for, :2597-2611
Z_BASED = ("sealv", "slvsq", "dz")
MONTHLY = ("dp temp saln uvel vvel uflx vflx utflx vtflx usflx vsflx umfltd vmfltd difdia difiso dz sealv sst sss ub vb bld maxbld surflx "
           "salflx ustar slvsq").split()

# Accumulators that may stay zero (or stop changing) on the test cases, each with its reason; every other one must be non-zero
# somewhere after 4 steps and differ from its value after 3.  At most a quarter of the table, and none of MUST_MOVE.
MAY_REST = {
    "umflsm": "eddtra_gm_isopyc_bulkml leaves the submesoscale mass fluxes zero (no mixed layer restratification on this coordinate)",
    "vmflsm": "as umflsm", "utflsm": "as umflsm", "vtflsm": "as umflsm", "usflsm": "as umflsm", "vsflsm": "as umflsm",
    "psrf": "p(:,:,1) is zero: the model has no atmospheric pressure loading here",
    "hmltfz": "no sea ice model: melting / freezing heat flux stays as initialised (zero)",
    "fmltfz": "as hmltfz (fresh water)", "sfl": "as hmltfz (salt flux)",
    "brnflx": "no sea ice: no brine rejection", "brnpd": "as brnflx (pbrnda stays zero)",
    "mtkeke": "the kinetic energy term of the mixed layer's TKE balance is set only with rm5 /= 0 (namelist default 0)",
}
MUST_MOVE = "dp temp saln uvel vvel dpu dpv uflx vflx utflx vtflx usflx vsflx sealv sst sss ub vb ubflxs vbflxs bld maxbld".split()


def admitted(case):
    """the whole table as far as the case's tracer set admits it (tke / gls_psi: :1907)"""
    p = case.params
    return [nm for nm in TABLE if not (nm == "tke" and p.get("itrtke", -1) < 1) and not (nm == "gls_psi" and not (p.get("itrtke", -1) >= 1 and p.get("gls", 0)))]


# ---- contexts ------------------------------------------------------------------------------------------------------------------
def forcing(gpu, case):
    """surface fluxes of both signs, fresh water, runoff and a wind stress, so that no forcing accumulator rests (the channel's own
    forcing is zero: blom_amd.hostinit.init_forcing)"""
    nj, ni = case.jdm + 8, case.idm + 8
    y = np.linspace(-1.0, 1.0, nj)[:, None] + 0.0 * np.arange(ni)[None, :]
    x = np.linspace(0.0, 2 * np.pi, ni)[None, :] + 0.0 * y
    gpu.put("nsf", (300.0 * (y + 0.3 * np.sin(x)))[None])
    gpu.put("swa", (120.0 * (1.0 + np.cos(x)) * (y > -0.5))[None])
    gpu.put("eva", (-2e-5 * (1.0 + 0.5 * np.sin(2 * x)))[None])
    gpu.put("lip", (3e-5 * (y > 0.0))[None])
    gpu.put("sop", (1e-5 * (y < 0.2) * (1.0 + np.sin(x)))[None])
    gpu.put("rnf", (2e-6 * (1.0 + np.cos(3 * x)))[None])
    gpu.put("rfi", (1e-6 * (1.0 + np.sin(2 * x) * y))[None])
    gpu.put("tauy", 0.3 * gpu.get("taux") * np.cos(x)[None])         # the cases' wind is zonal


def options(gpu):
    gpu.set("niwgf", 0.4)
    gpu.set("trxday", 20.0)                                          # relaxation towards the climatologies on: surrlx, salrlx
    gpu.set("srxday", 40.0)


def full_context(cfg, device=0, live=True):
    """config 2's step as bench.device_for_bench sets it up, plus the forcing above"""
    import bench
    case = make_case(cfg)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    gpu = bench.device_for_bench(case, nreg, masks, live=live, device=device)
    forcing(gpu, case)
    options(gpu)
    return case, masks, gpu


def dyncore_context(cfg, **opts):
    """the dynamical core alone, as tests/test_hostemu_kernels.py::_run"""
    from blom_amd.gpu import BlomGpu
    case = make_case(cfg)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(gpu, case)
    for k, v in opts.items():
        gpu.set(k, v)
    return case, masks, gpu


# ---- the reference's loops in numpy ----------------------------------------------------------------------------------------------
class Restated:
    def __init__(self, case, masks, names, isopyc=True):
        self.case, self.names, self.isopyc = case, list(names), isopyc
        self.kk = case.kdm
        nj, ni = case.jdm + 8, case.idm + 8
        self.mask = {g: masks["i" + g].reshape(nj, ni) for g in "puv"}
        own = np.zeros((nj, ni), bool)
        own[4:4 + case.jdm, 4:4 + case.idm] = True                 # i = 1..ii, j = 1..jj: min(ii, il*) on the u-grid too
        self.sel = {g: own & (self.mask[g] > 0) for g in "puv"}
        self.nacc = 0
        self.acc = {}
        self.reset()

    def grid(self, nm):
        return (H2D.get(nm) or MAX2D.get(nm) or SQ2D.get(nm) or LYR.get(nm))[0]

    def reset(self):
        # inih2d / inilyr: inival*mask over the whole padded plane; inival = -spval for maxbld, 0 otherwise
        for nm in self.names:
            inival = np.float64(-SPVAL if nm in MAX2D else 0.0)
            plane = inival * self.mask[self.grid(nm)].astype(np.float64)
            self.acc[nm] = np.repeat(plane[None], self.kk if nm in LYR else 1, axis=0).copy()
        self.nacc = 0

    def accumulate(self, gpu, nstep):
        """diaacc(m,n,mm,nn,k1m,k1n) of the step that started from step count nstep, on the arrays gpu holds now"""
        kk = self.kk
        m, n, mm, nn, k1m, k1n = hostinit.step_indices(nstep, kk)
        lev = {"m": m - 1, "n": n - 1, "k1m": k1m - 1, "k1n": k1n - 1, "kk+1": kk, 0: 0}
        cache = {}

        def fld(name):
            if name not in cache:
                if name == "dpml":                                  # :1148-1171
                    cache[name] = (fld("dp")[mm] + fld("dp")[mm + 1])[None] if self.isopyc else (fld("OBLdepth")[0] * ONEM)[None]
                elif name == "uvel":                                # :1180
                    cache[name] = fld("u")[mm:mm + kk] + fld("ub")[m - 1][None]
                elif name == "vvel":                                # :1195
                    cache[name] = fld("v")[mm:mm + kk] + fld("vb")[m - 1][None]
                elif name in ("trc_tke", "trc_gls"):                # trc(:,:,k1m,itrtke), :1909-1913
                    it = self.case.params["itrtke" if name == "trc_tke" else "itrgls"]
                    cache[name] = fld("trc")[(it - 1) * 2 * kk + mm:(it - 1) * 2 * kk + mm + kk]
                else:
                    cache[name] = gpu.get(name)
            return cache[name]
        self.nacc += 1                                              # :1123-1125
        with np.errstate(all="ignore"):
            for nm in self.names:
                a = self.acc[nm]
                if nm in LYR:
                    g, f, l0, w = LYR[nm]
                    src = fld(f) if f in ("uvel", "vvel", "trc_tke", "trc_gls") else fld(f)[lev[l0]:lev[l0] + kk]
                    new = a + src * fld(w)[mm:mm + kk] if w else a + src           # :5513 / :5500
                else:
                    g, f, l0 = H2D.get(nm) or MAX2D.get(nm) or SQ2D.get(nm)
                    src = fld(f)[lev[l0]][None]
                    if nm in MAX2D:
                        new = np.where(a > src, a, src)             # max(acc, fld) as amdflang lowers it, :5330
                    elif nm in SQ2D:
                        new = a + src * src                         # :5454
                    else:
                        new = a + src                               # :5256
                s = self.sel[g]
                a[:, s] = new[:, s]

    def finlyr(self):
        """finlyr for the weighted pairs (:2597-2611, :6137-6141); returns the finalised copies"""
        out = {}
        with np.errstate(all="ignore"):
            for nm, w in WEIGHTED.items():
                if nm not in self.acc:
                    continue
                a, wg = self.acc[nm].copy(), self.acc[w]
                s = self.sel[self.grid(nm)]
                a[:, s] = np.where(wg > EPSIL, a / wg, FILL)[:, s]
                out[nm] = a
        return out


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def differing(got, want):
    return [nm for nm in want if not same_bytes(got[nm], want[nm])]


# ---- one run per case, shared by the tests below --------------------------------------------------------------------------------
_RUNS = {}


def case_run(cfg, extended=False):
    """Context A: the whole table selected, step(0, 4) in one call; then dia_finalize; (extended) dia_reset and step(4, 4).
    Context B: four single steps without a selection, numpy accumulating after each; (extended) then the table selected on it --
    a fresh set of accumulators -- and four more single steps, numpy going on to its 6-step total."""
    key = (cfg, extended)
    if key in _RUNS:
        return _RUNS[key]
    if (cfg, True) in _RUNS:
        return _RUNS[(cfg, True)]
    r = {}
    case, masks, a = full_context(cfg)
    _, _, b = full_context(cfg)
    try:
        names = admitted(case)
        r["case"], r["masks"], r["names"] = case, masks, names
        a.dia_select(names)
        assert a.step(0, 4) == 4
        r["A4"] = {nm: a.dia_get(nm) for nm in names}
        r["A4_nacc"] = a.dia_nacc()
        r["A4_state"] = {nm: a.get(nm) for nm in STATE_FIELDS if a.has_field(nm)}
        ref = Restated(case, masks, names)
        r["init"] = {nm: v.copy() for nm, v in ref.acc.items()}
        for ns in range(4):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
            if ns == 2:
                r["E3"] = {nm: v.copy() for nm, v in ref.acc.items()}
        r["E4"] = {nm: v.copy() for nm, v in ref.acc.items()}
        r["E4_nacc"] = ref.nacc
        r["B4_state"] = {nm: b.get(nm) for nm in STATE_FIELDS if b.has_field(nm)}
        r["E4_fin"] = ref.finlyr()
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
    finally:
        a.close()
        b.close()
    _RUNS[key] = r
    return r


CASES = ["chan_s_tke", "box_s", "tri_s_tke"]
EXTENDED = {"chan_s_tke"}


# ---- 1. the step accumulates what the reference's loops would -------------------------------------------------------------------
def check_step_accumulates(cfg):
    r = case_run(cfg, cfg in EXTENDED)
    bad = differing(r["A4"], r["E4"])
    assert not bad, f"{cfg}: accumulators that differ from the restated loops: {bad}"
    assert r["A4_nacc"] == 4 and r["E4_nacc"] == 4
    # the whole padded array was compared: in particular land under maxbld is -0.0
    land = r["masks"]["ip"].reshape(r["A4"]["maxbld"].shape[1:]) == 0
    if land.any():
        assert np.signbit(r["A4"]["maxbld"][0][land]).all() and (r["A4"]["maxbld"][0][land] == 0.0).all()


@pytest.mark.parametrize("cfg", CASES)
def test_step_accumulates_what_the_reference_loops_would(cfg):
    check_step_accumulates(cfg)


def check_dyncore_only():
    """the dynamical core alone (chan_s, cmnfld1 = 1): the accumulators whose sources that sequence maintains"""
    names = ("dp temp saln uvel vvel dpu dpv uflx vflx utflx vtflx usflx vsflx umfltd vmfltd dz sealv slvsq sst sss sstsq ssssq sigmx ub vb "
             "ubflxs vbflxs taux tauy bld maxbld psrf pbot").split()
    case, masks, a = dyncore_context("chan_s", cmnfld1=1)
    _, _, b = dyncore_context("chan_s", cmnfld1=1)
    try:
        a.dia_select(names)
        assert a.step(0, 4) == 4
        ref = Restated(case, masks, names)
        for ns in range(4):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
        got = {nm: a.dia_get(nm) for nm in names}
        assert not differing(got, ref.acc), differing(got, ref.acc)
        assert a.dia_nacc() == 4
        for nm in ("dp", "uvel", "sealv", "ub"):
            assert np.abs(got[nm]).max() > 0.0, nm
    finally:
        a.close()
        b.close()


def test_dynamical_core_alone_accumulates_what_it_maintains():
    check_dyncore_only()


# ---- 2. the test cannot pass on zeros ------------------------------------------------------------------------------------------
def check_not_zeros(cfg):
    r = case_run(cfg, cfg in EXTENDED)
    assert len(MAY_REST) <= len(TABLE) // 4 and not set(MAY_REST) & set(MUST_MOVE) and set(MAY_REST) <= set(TABLE)
    zero = [nm for nm in r["names"] if nm not in MAY_REST and not (np.abs(r["A4"][nm]) > 0.0).any()]
    still = [nm for nm in r["names"] if nm not in MAY_REST and same_bytes(r["A4"][nm], r["E3"][nm])]
    print(cfg, "of MAY_REST, moving all the same:", [nm for nm in r["names"] if nm in MAY_REST and not same_bytes(r["A4"][nm], r["E3"][nm])])
    assert not zero and not still, f"{cfg}: zero everywhere {zero}; unchanged by the fourth step {still}"


@pytest.mark.parametrize("cfg", CASES)
def test_accumulators_are_non_zero_and_still_moving(cfg):
    check_not_zeros(cfg)


# ---- 3. finalise and reset -----------------------------------------------------------------------------------------------------
def check_finalize(cfg):
    r = case_run(cfg, cfg in EXTENDED)
    want = dict(r["E4"])
    want.update(r["E4_fin"])                                         # the unweighted ones (dp, dpu, dpv among them) stay
    bad = differing(r["A4_fin"], want)
    assert not bad, f"{cfg}: finalised accumulators that differ from the restated finlyr: {bad}"
    if cfg == "chan_s_tke":
        # both branches of finlyr: massless layers (accumulated dp <= epsil) at owned wet points, and layers with mass
        nj, ni = r["E4"]["dp"].shape[1:]
        own = np.zeros((nj, ni), bool)
        own[4:-4, 4:-4] = True
        wet = own & (r["masks"]["ip"].reshape(nj, ni) > 0)
        dp = r["E4"]["dp"][:, wet]
        assert (dp <= EPSIL).any() and (dp > EPSIL).any()
        assert (r["A4_fin"]["temp"][:, wet][dp <= EPSIL] == FILL).all()


@pytest.mark.parametrize("cfg", CASES)
def test_finalize_is_the_restated_finlyr(cfg):
    check_finalize(cfg)


def check_reset():
    r = case_run("chan_s_tke", True)
    assert not differing(r["A_reset"], r["init"]) and r["A_reset_nacc"] == 0
    assert not differing(r["A8"], r["B8"]), differing(r["A8"], r["B8"])
    assert r["A8_nacc"] == 4 and r["B8_nacc"] == 4
    assert (np.abs(r["A8"]["temp"]) > 0.0).any()


def test_reset_restores_the_initial_value_and_four_more_steps_match_a_fresh_selection():
    check_reset()


# ---- 4. selection semantics ------------------------------------------------------------------------------------------------------
def check_selection_semantics():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = dyncore_context("chan_s")                       # no TKE tracers: itrtke < 1; cmnfld1 = 0
    try:
        assert g.dia_nacc() == 0
        g.dia_select("temp")
        zero_p = 0.0 * masks["ip"].reshape(1, case.jdm + 8, case.idm + 8).astype(np.float64)
        assert same_bytes(g.dia_get("dp"), np.repeat(zero_p, case.kdm, axis=0))      # the dependency is there
        with pytest.raises(BlomGpuError, match="saln"):
            g.dia_get("saln")
        assert g.step(0, 2) == 2
        temp2, dp2 = g.dia_get("temp"), g.dia_get("dp")
        assert g.dia_nacc() == 2 and np.abs(temp2).max() > 0.0
        with pytest.raises(BlomGpuError, match="nonsense"):
            g.dia_select("dp nonsense uvel")
        with pytest.raises(BlomGpuError, match="tke"):
            g.dia_select("dp tke")
        with pytest.raises(BlomGpuError, match="gls_psi"):
            g.dia_select("gls_psi")
        assert same_bytes(g.dia_get("temp"), temp2) and same_bytes(g.dia_get("dp"), dp2) and g.dia_nacc() == 2
        with pytest.raises(BlomGpuError, match="uvel"):
            g.dia_get("uvel")                                        # the refused lists selected nothing
        g.dia_select("temp")                                         # re-selecting re-initialises
        assert same_bytes(g.dia_get("temp"), np.repeat(zero_p, case.kdm, axis=0)) and g.dia_nacc() == 0
        g.dia_select("uvel vvel")
        assert np.abs(g.dia_get("dpu")).max() == 0.0 and np.abs(g.dia_get("dpv")).max() == 0.0
        g.dia_select("")                                             # an empty selection frees
        assert g.dia_nacc() == 0
        with pytest.raises(BlomGpuError, match="temp"):
            g.dia_get("temp")
        assert g.step(2, 1) == 3
        # z-based names: refused at the step while the sequence does not run cmnfld1
        g.dia_select("dp sealv dz")
        with pytest.raises(BlomGpuError, match="sealv dz"):
            g.step(3, 1)
        assert g.dia_nacc() == 0
        g.set("cmnfld1", 1)
        assert g.step(3, 1) == 4 and g.dia_nacc() == 1
        assert np.abs(g.dia_get("dz")).max() > 0.0
        # the stage on its own: counts, then accumulates
        g.stage("diaacc", *hostinit.step_indices(3, case.kdm))
        g.diaacc(*hostinit.step_indices(3, case.kdm))
        assert g.dia_nacc() == 3
    finally:
        g.close()


def test_selection_semantics():
    check_selection_semantics()


# ---- 5. no selection, no trace ---------------------------------------------------------------------------------------------------
def check_no_trace():
    r = case_run("chan_s_tke", True)
    # a context with the whole table selected ends in the state bytes of one without
    bad = [nm for nm in r["B4_state"] if not same_bytes(r["A4_state"][nm], r["B4_state"][nm])]
    assert not bad, bad
    # ... and so does one that selected, stepped twice, deselected and stepped twice more
    case, masks, c = full_context("chan_s_tke")
    try:
        c.dia_select(r["names"])
        assert c.step(0, 2) == 2
        c.dia_select("")
        assert c.step(2, 2) == 4 and c.dia_nacc() == 0
        bad = [nm for nm in r["B4_state"] if not same_bytes(c.get(nm), r["B4_state"][nm])]
        assert not bad, bad
    finally:
        c.close()


def test_no_selection_no_trace():
    check_no_trace()


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------------------
def check_graph_replay(expect_replays):
    r = case_run("chan_s_tke", True)
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


# ---- 7. tiles ----------------------------------------------------------------------------------------------------------------------
def check_tiles(cfg="chan_s_tke", npx=2, npy=1, nsteps=4):
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd.tiles import tile_extents, tile_window, scatter_state
    from test_gpu_tiles import _single, ALL, FORCING
    case, masks, fields, ref = _single(cfg, nsteps)
    names = admitted(case)
    hostinit.init_forcing(ref, case)
    forcing(ref, case)
    ii, jj = tile_extents(case, npx, npy)
    grp = TileGroup(npx, npy)
    tiles = {}
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
    scatter_state(ref, tiles, case, npx, npy, [f for f in ALL if f in fields] + [f for f in FORCING if ref.has_field(f)])
    # the ocean area is a global number (mod_grid: area = xcsum(scp2, ips))
    w = masks["ip"][4:-4, 4:-4] > 0
    area = float(np.sum(ref.get("scp2")[0][4:-4, 4:-4][w]))

    def setup(g):
        g.set("area", area)
        options(g)
        g.set("full_physics", 1)
        g.dia_select(names)
    errs = []

    def run(t):
        try:
            setup(t)
            assert t.step(0, nsteps) == nsteps
            t.sync()
        except Exception as e:          # a failing tile would leave the others at a barrier
            errs.append(e)
    try:
        setup(ref)
        assert ref.step(0, nsteps) == nsteps
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x_.start() for x_ in th]
        [x_.join(timeout=300) for x_ in th]
        assert not errs, errs
        bad = []
        for nm in names:
            whole = ref.dia_get(nm)
            for (px, py), t in tiles.items():
                mine = t.dia_get(nm)[:, 4:4 + jj, 4:4 + ii]
                if not same_bytes(mine, whole[:, 4 + py * jj:4 + (py + 1) * jj, 4 + px * ii:4 + (px + 1) * ii]):
                    bad.append((nm, px, py))
            assert t.dia_nacc() == nsteps
        assert not bad, bad
        assert np.abs(ref.dia_get("uvel")).max() > 0.0
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


def test_tiles_accumulate_their_window_of_the_single_tile():
    check_tiles()


# ---- 8. full size --------------------------------------------------------------------------------------------------------------------
def test_channel_size_layer_table():
    """208x512x53 with every layer accumulator the case admits and sealv selected: 35 slots of 53 planes of 216x520 doubles,
    1.67e9 bytes in one allocation (slot offsets are size_t in the kernels; a 32-bit ELEMENT offset would still hold, a 32-bit
    byte offset past 2^30 elements would not).  Two steps; the first and the last layer slot of the allocation and sealv against
    numpy from two single steps of a second context."""
    case, masks, a = full_context("channel_tke")
    _, _, b = full_context("channel_tke")
    try:
        layers = [nm for nm in admitted(case) if nm in LYR]
        a.dia_select(layers + ["sealv"])
        first, last = layers[0], layers[-1]
        check = [first, last, "sealv"] + sorted({WEIGHTED[nm] for nm in (first, last) if nm in WEIGHTED})
        assert a.step(0, 2) == 2
        ref = Restated(case, masks, check)
        for ns in range(2):
            assert b.step(ns, 1) == ns + 1
            ref.accumulate(b, ns)
        got = {nm: a.dia_get(nm) for nm in check}
        print("accumulator bytes:", (len(layers) * case.kdm + 1) * (case.idm + 8) * (case.jdm + 8) * 8)
        assert not differing(got, ref.acc), differing(got, ref.acc)
        assert a.dia_nacc() == 2
        for nm in check:
            assert np.abs(got[nm]).max() > 0.0, nm
    finally:
        a.close()
        b.close()
