"""The end of blom_step on the device (blom_amd/csrc/stage_stepend.hip: the clock of step_time, k_swa_fill, k_updswa, k_fwbbal_acc /
_scale / _zero, k_chkvar) against tests/stepend_ref.py, the numpy restatement of phy/mod_time.F90:182-219, phy/mod_swabs.F90:216-732,
phy/mod_forcing.F90:361-441 and phy/mod_chkvar.F90:77-141.  Every comparison is == on the bytes of whole padded arrays, the outputs
preset to a pattern so that a store to a land or halo point is seen; error texts are compared character for character.

chkvar's checks plant one NaN or Inf in the data of a fresh state and run the chkvar stage ALONE: the kernel compares and writes one
word, and a poisoned state is never stepped.  tests/test_hostemu_stepend.py runs the same functions on the host emulation."""
import contextlib

import numpy as np
import pytest

from blom_amd import hostinit, stepper
from blom_amd.cases import default_grid, make_case
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import same_bytes
import stepend_ref as R

pytestmark = pytest.mark.gpu

NB = 4
HYBRID = ("chan_s", "cntiso_hybrid", "nudge")
CLOCK = dict(nstep_in_day=4, nday_in_year=24)
# three positions in the year: the months around January wrap (11 12 1 2 3), mid-year, and the wrap at the other end (10 11 12 1 2)
TIMES = (((11, 12, 1, 2, 3), 0.3), ((4, 5, 6, 7, 8), 0.75), ((10, 11, 12, 1, 2), 0.0))


def pattern(shape, k):
    return 7.25 + 0.001 * k + 1.0e-6 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


def context(cfg, hybrid=False, grid=None):
    with default_grid(grid) if grid else contextlib.nullcontext():
        if hybrid:
            from test_gpu_dia_hybrid import hybrid_context
            case, masks, g = hybrid_context(*HYBRID)
            hostinit.init_forcing(g, case)
            lyr.forcing(g, case)
        else:
            case, masks, g = lyr.full_context(cfg)
    return case, masks, g


def set_time(g, lmi, xmi):
    for k, v in enumerate(lmi):
        g.set("l%dmi" % (k + 1), int(v))
    g.set("xmi", float(xmi))


def chl_of(case):
    return R.synthetic_chl(case.jdm + 2 * NB, case.idm + 2 * NB)


# ---- iniswa / updswa -----------------------------------------------------------------------------------------------------------------------
def check_updswa(cfg, method, hybrid=False, grid=None, seen=None):
    case, masks, g = context(cfg, hybrid, grid)
    try:
        sel = R.owned(masks, case.idm, case.jdm)["p"]
        shape = (1, case.jdm + 2 * NB, case.idm + 2 * NB)
        g.set("swamth", method)
        g.set("jwtype", 3)
        g.set("swamxd", 150.0)
        for k, nm in enumerate(R.BANDS):
            g.put(nm, pattern(shape, k))
        chlor = method.startswith("chlorophyll")
        assert not g.has_field("chl10c") and not g.has_field("chl10")
        before = {nm: g.get(nm) for nm in R.BANDS}
        g.iniswa(chl_of(case) if chlor else None)
        assert g.has_field("chl10c") == chlor and g.has_field("chl10") == chlor
        s = {nm: g.get(nm) for nm in R.BANDS}
        if method in ("top-layer", "jerlov"):
            R.iniswa_constant(before, method, sel, jwtype=3, swamxd=150.0)
            assert sel.any() and not sel.all()
        bad = [nm for nm in R.BANDS if not same_bytes(s[nm], before[nm])]
        assert not bad, f"{cfg} {method}: iniswa left {bad} different from the restated routine"
        if chlor:
            assert g.get("chl10c").shape[0] == 12 and same_bytes(g.get("chl10c"), R.log10_chl(chl_of(case)))
            g.put("chl10", pattern(shape, 9))
            lut = R.ohl03_tables() if method == "chlorophyll_ohl03" else None
        for lmi, xmi in TIMES:
            set_time(g, lmi, xmi)
            s = {nm: g.get(nm) for nm in R.BANDS + (("chl10c", "chl10") if chlor else ())}
            g.stage("updswa", *hostinit.step_indices(0, case.kdm))
            if chlor:
                R.updswa(s, method, lmi, xmi, sel, lut=lut, seen=seen)
            bad = [nm for nm in s if not same_bytes(g.get(nm), s[nm])]
            assert not bad, f"{cfg} {method} {lmi} {xmi}: {bad} differ from the restated updswa"
        if chlor:
            # csdiag's four lines (:722-730) are checksums of these planes: the device's against the host's of the restated planes
            from blom_amd.checksum import chksum
            for nm in R.BANDS:
                assert g.crc(nm, 1, 1) == chksum(nm, s[nm], masks, case.idm, case.jdm), nm
        return case
    finally:
        g.close()


def check_updswa_not_vacuous(cfg, method, **kw):
    seen = {}
    check_updswa(cfg, method, seen=seen, **kw)
    print(cfg, method, {k: (len(v) if isinstance(v, set) else v) for k, v in seen.items()})
    assert not R.missing(seen, method), (R.missing(seen, method), seen)
    return seen


@pytest.mark.parametrize("method", R.METHODS)
def test_updswa_equals_the_restated_routine(method):
    if method.startswith("chlorophyll"):
        check_updswa_not_vacuous("chan_s_tke", method)
    else:
        check_updswa("chan_s_tke", method)


@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke", "chan_b"])
@pytest.mark.parametrize("method", ["chlorophyll_ma94", "chlorophyll_ohl03"])
def test_updswa_on_the_closed_box_the_arctic_patch_and_long_rows(cfg, method):
    seen = check_updswa_not_vacuous(cfg, method)
    if cfg == "chan_b" and method == "chlorophyll_ohl03":
        assert len(seen["indices"]) >= 100, len(seen["indices"])


def test_updswa_on_the_warped_grid_and_under_the_hybrid_coordinate():
    check_updswa_not_vacuous("chan_s_tke", "chlorophyll_ohl03", grid="warped_eq")
    check_updswa_not_vacuous("chan_s", "chlorophyll_ma94", hybrid=True)


def check_swabs_refusals():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.dyncore_context("chan_s")
    try:
        with pytest.raises(BlomGpuError) as x:
            g.set("swamth", "chlorophyll")
        assert str(x.value) == " iniswa: swamth = chlorophyll is unsupported!"
        with pytest.raises(BlomGpuError, match="swamth has not been set"):
            g.iniswa()
        g.set("swamth", "jerlov")
        for jw in (0, 6):
            g.set("jwtype", jw)
            with pytest.raises(BlomGpuError) as x:
                g.iniswa()
            assert str(x.value) == " jwtype = %11d is outside the valid interval of [1,5]!" % jw
        g.set("swamth", "chlorophyll_ma94")
        g.set("chlopt", "model")
        with pytest.raises(BlomGpuError) as x:
            g.iniswa()
        assert str(x.value) == " iniswa: chlopt = model is unsupported!"
        assert not g.has_field("chl10c")
        # a chlorophyll method without iniswa: the stage and the step say so
        with pytest.raises(BlomGpuError, match="blomgpu_iniswa has not been called"):
            g.updswa()
        g.set("chlopt", "climatology")
        g.iniswa(chl_of(case))
        g.updswa()
        g.set("swamth", "chlorophyll_ohl03")             # another method: iniswa once more
        with pytest.raises(BlomGpuError, match="blomgpu_iniswa has not been called"):
            g.updswa()
    finally:
        g.close()


def test_swabs_refusals_word_for_word():
    check_swabs_refusals()


# ---- fwbbal --------------------------------------------------------------------------------------------------------------------------------
FWB_IN = "eva fmltfz lip sop rnf rfi scp2".split()


def ipwocn_of(case, masks):
    """the wet points but for a block in the middle of the domain: a part of the ocean that is not connected to the world ocean"""
    nj, ni = case.jdm + 2 * NB, case.idm + 2 * NB
    w = (np.asarray(masks["ip"]).reshape(nj, ni) > 0).astype(np.int32)
    w[nj // 3:nj // 2, ni // 4:ni // 2] = 0
    return w[None]


def fwb_setup(g, case, masks):
    nj, ni = case.jdm + 2 * NB, case.idm + 2 * NB
    g.set("sprfac", 1)
    g.put("fmltfz", (1.5e-5 * np.cos(np.linspace(0.0, 7.0, nj))[:, None] * np.ones(ni)[None, :])[None])
    g.put("ipwocn", ipwocn_of(case, masks))
    for nm, v in CLOCK.items():
        g.set(nm, v)


# (nday_of_year, incremented nstep): four steps that only accumulate, the end of a year, two more steps
FWB_STEPS = ((24, 1), (24, 2), (24, 3), (1, 5), (1, 4), (1, 5), (1, 6))


def check_fwbbal(cfg, grid=None, hybrid=False):
    case, masks, g = context(cfg, hybrid, grid)
    _, _, h = context(cfg, hybrid, grid)
    try:
        sel = R.owned(masks, case.idm, case.jdm)["p"]
        assert not g.has_field("eiacc")
        fwb_setup(g, case, masks)
        fwb_setup(h, case, masks)
        assert g.get_real("prfac") == 1.0 and not g.get("eiacc").any() and not g.get("pracc").any()
        shape = (1, case.jdm + 2 * NB, case.idm + 2 * NB)
        g.put("eiacc", pattern(shape, 1))                 # (land and halo points must stay as they are)
        g.put("pracc", pattern(shape, 2))
        s = {nm: g.get(nm) for nm in FWB_IN + ["eiacc", "pracc", "ipwocn"]}
        assert (s["ipwocn"][0][sel] == 0).any() and (s["ipwocn"][0][sel] == 1).any()
        prfac, baclin = 1.0, float(case.params["baclin"])
        for step, (day, ns1) in enumerate(FWB_STEPS):
            g.set("nday_of_year", day)
            g.set("nstep", ns1)
            g.stage("fwbbal", *hostinit.step_indices(ns1 - 1, case.kdm))
            new = R.fwbbal(s, dict(CLOCK, baclin=baclin, nday_of_year=day, nstep=ns1, prfac=prfac), sel, case.idm, case.jdm)
            year_end = day == 1 and ns1 % CLOCK["nstep_in_day"] == 0
            assert (new != prfac) == year_end
            prfac = new
            assert g.get_real("prfac") == prfac, (step, g.get_real("prfac"), prfac)
            for nm in ("eiacc", "pracc"):
                assert same_bytes(g.get(nm), s[nm]), (cfg, step, nm)
                assert bool(s[nm][0][sel].any()) != year_end
            if step == 2:
                # a restart: both planes down and up by name, prfac through its option; the second context goes on to the same bytes
                for nm in ("eiacc", "pracc"):
                    h.put(nm, g.get(nm))
                h.set("prfac", g.get_real("prfac"))
            if step >= 3:
                h.set("nday_of_year", day)
                h.set("nstep", ns1)
                h.stage("fwbbal", *hostinit.step_indices(ns1 - 1, case.kdm))
                assert h.get_real("prfac") == prfac
                assert all(same_bytes(h.get(nm), s[nm]) for nm in ("eiacc", "pracc"))
        assert prfac != 1.0 and np.isfinite(prfac)
    finally:
        g.close()
        h.close()


@pytest.mark.parametrize("cfg", ["chan_s_tke", "box_s", "tri_s_tke", "chan_b"])
def test_fwbbal_equals_the_restated_routine(cfg):
    check_fwbbal(cfg)


def test_fwbbal_on_the_warped_grid_and_under_the_hybrid_coordinate():
    check_fwbbal("chan_s_tke", grid="warped_eq")
    check_fwbbal("chan_s", hybrid=True)


def check_fwbbal_tiles(npx, npy, cfg="chan_s_tke", grid="warped_eq"):
    """tiles of one process run the stage to the single tile's bytes and factor: the sums of the year's end go through the one-plane
    global-order sums there"""
    import threading
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd.tiles import tile_extents, tile_window
    case, masks, ref = context(cfg, grid=grid)
    ii, jj = tile_extents(case, npx, npy)
    grp = TileGroup(npx, npy)
    tiles = {}
    try:
        fwb_setup(ref, case, masks)
        src = {nm: ref.get(nm) for nm in FWB_IN + ["ipwocn"]}
        for py in range(npy):
            for px in range(npx):
                tm = {k: tile_window(masks[k], case, npx, npy, px, py) for k in masks}
                t = BlomGpu(ii, jj, case.kdm, case.ntr, case.nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=px * ii, j0=py * jj)
                t.set("baclin", case.params["baclin"])
                grp.attach(t, px, py)
                t.set("sprfac", 1)
                for nm, v in CLOCK.items():
                    t.set(nm, v)
                for nm, a in src.items():
                    t.put(nm, tile_window(a, case, npx, npy, px, py))
                tiles[(px, py)] = t
        errs = []

        def run(g):
            try:
                for day, ns1 in FWB_STEPS:
                    g.set("nday_of_year", day)
                    g.set("nstep", ns1)
                    g.stage("fwbbal", *hostinit.step_indices(ns1 - 1, case.kdm))
                    if (day, ns1) == (1, 4):
                        got[id(g)] = g.get_real("prfac")
                g.sync()
            except Exception as e:          # a failing tile would leave the others at a barrier
                errs.append(e)
        got = {}
        run(ref)
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x_.start() for x_ in th]
        [x_.join(timeout=300) for x_ in th]
        assert not errs, errs
        assert got[id(ref)] != 1.0 and all(got[id(t)] == got[id(ref)] for t in tiles.values()), got
        for nm in ("eiacc", "pracc"):
            whole = ref.get(nm)
            assert whole.any()
            for (px, py), t in tiles.items():
                assert same_bytes(t.get(nm)[:, 4:4 + jj, 4:4 + ii], whole[:, 4 + py * jj:4 + (py + 1) * jj, 4 + px * ii:4 + (px + 1) * ii]), (nm, px, py)
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_fwbbal_on_two_tiles_equals_the_single_tile(npx, npy):
    check_fwbbal_tiles(npx, npy)


# ---- chkvar --------------------------------------------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
# (field, value, level k, (di, dj) of the point in units of a tenth of the tile) -- a different field, level and point per case
PLANTS = [("dp", NAN, 1, (3, 2)), ("dp", INF, 2, (7, 5)), ("temp", NAN, 3, (1, 8)), ("temp", -INF, 1, (9, 1)), ("saln", NAN, 2, (5, 5)),
          ("saln", INF, 3, (2, 7))]


def wet_point(sel, idm, jdm, frac):
    """the wet owned point nearest to the given fractions of the tile, as 0-based indices of the padded plane"""
    j0, i0 = NB + min(jdm - 1, frac[1] * jdm // 10), NB + min(idm - 1, frac[0] * idm // 10)
    jj, ii = np.nonzero(sel)
    q = np.argmin((jj - j0) ** 2 + (ii - i0) ** 2)
    return int(jj[q]), int(ii[q])


def run_chkvar(g, case, n_level):
    from blom_amd.gpu import BlomGpuError
    idx = hostinit.step_indices(n_level, case.kdm)           # (n_level 0: n = 2, nn = kk; 1: n = 1, nn = 0)
    try:
        g.stage("chkvar", *idx)
    except BlomGpuError as e:
        return idx[3], str(e)
    return idx[3], None


def check_chkvar(cfg="chan_s_tke", hybrid=False):
    case, masks, g = context(cfg, hybrid)
    try:
        kk = case.kdm
        sel = R.owned(masks, case.idm, case.jdm)["p"]
        clean = {nm: g.get(nm) for nm in ("dp", "temp", "saln")}
        six = hostinit.step_indices(0, kk)
        # undeclared: the stage returns at once, whatever the state holds
        bad = clean["temp"].copy()
        bad[:] = NAN
        g.put("temp", bad)
        g.stage("chkvar", *six)
        g.put("temp", clean["temp"])
        g.set("chkvar", 1)
        assert run_chkvar(g, case, 0)[1] is None and run_chkvar(g, case, 1)[1] is None, "a clean state passes"

        def planted(plants, n_level):
            s = {nm: a.copy() for nm, a in clean.items()}
            nn = hostinit.step_indices(n_level, kk)[3]
            for nm, v, k, (j, i) in plants:
                s[nm][nn + k - 1, j, i] = v
            for nm in s:
                g.put(nm, s[nm])
            nn_, msg = run_chkvar(g, case, n_level)
            assert nn_ == nn
            want = R.chkvar(s, nn, kk, sel, case.idm, case.jdm)
            return msg, want
        for q, (nm, v, k, frac) in enumerate(PLANTS):
            msg, want = planted([(nm, v, k, wet_point(sel, case.idm, case.jdm, frac))], q % 2)
            assert want is not None and msg == "blom:" + want, (msg, want)
            assert (" %s is %s at " % (nm, "NaN" if v != v else "Inf")) in msg and ("k =%4d)" % k) in msg
            # the word is cleared after the report: the same state is reported again, a clean one passes
            g.put(nm, clean[nm])
            assert run_chkvar(g, case, q % 2)[1] is None
        # two hits: the reference's order decides -- the smaller j wins over the smaller k, the smaller k over the smaller i, the
        # routine's order of the tests at one point
        ja, ia = wet_point(sel, case.idm, case.jdm, (8, 2))
        jb, ib = wet_point(sel, case.idm, case.jdm, (2, 8))
        ia = int(np.flatnonzero(sel[jb])[-1])             # (a second wet point of row jb, further along it)
        assert ja < jb and ia > ib and sel[ja, ia] or sel[ja].any()
        ia_a = ia if sel[ja, ia] else int(np.flatnonzero(sel[ja])[-1])
        pairs = [[("saln", INF, 3, (ja, ia_a)), ("dp", NAN, 1, (jb, ib))],            # j before k
                 [("temp", NAN, 3, (jb, ib)), ("dp", INF, 2, (jb, ia))],            # k before i
                 [("temp", INF, 2, (jb, ia)), ("saln", NAN, 2, (jb, ib))],          # i
                 [("saln", NAN, 2, (jb, ib)), ("temp", INF, 2, (jb, ib)), ("dp", INF, 2, (jb, ib))]]      # dp Inf before temp Inf before saln NaN
        firsts = ["saln is Inf", "dp is Inf", "saln is NaN", "dp is Inf"]
        for plants, first in zip(pairs, firsts):
            msg, want = planted(plants, 0)
            assert msg == "blom:" + want and first in msg, (msg, want, first)
        # the other time level, a land point and a halo point are not reported
        s = {nm: a.copy() for nm, a in clean.items()}
        nn = hostinit.step_indices(0, kk)[3]
        other = kk - nn
        s["dp"][other + 1, ja, ia_a] = NAN
        s["temp"][nn, 0, 0] = NAN
        s["saln"][nn + 1, NB + case.jdm, NB + 1] = INF
        land = np.argwhere(~sel[NB:NB + case.jdm, NB:NB + case.idm])
        if len(land):
            s["temp"][nn + 2, NB + land[0][0], NB + land[0][1]] = INF
        for nm in s:
            g.put(nm, s[nm])
        assert run_chkvar(g, case, 0)[1] is None and R.chkvar(s, nn, kk, sel, case.idm, case.jdm) is None
        return len(land)
    finally:
        g.close()


def test_chkvar_reports_the_first_hit_of_the_serial_reference():
    check_chkvar("chan_s_tke")


def test_chkvar_beside_land_and_under_the_hybrid_coordinate():
    assert check_chkvar("box_s") > 0
    check_chkvar("chan_s", hybrid=True)


def check_chkvar_tile():
    """a tile with i0 /= 0 and j0 /= 0 reports global indices"""
    from blom_amd.gpu import BlomGpu, BlomGpuError
    from blom_amd.tiles import tile_extents, tile_window
    case = make_case("chan_s_tke")
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    ii, jj = tile_extents(case, 2, 2)
    tm = {k: tile_window(masks[k], case, 2, 2, 1, 1) for k in masks}
    t = BlomGpu(ii, jj, case.kdm, case.ntr, nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=ii, j0=jj)
    try:
        kk = case.kdm
        sel = R.owned(tm, ii, jj)["p"]
        s = {nm: np.ones((2 * kk, jj + 2 * NB, ii + 2 * NB)) for nm in ("dp", "temp", "saln")}
        j, i = wet_point(sel, ii, jj, (6, 4))
        s["saln"][kk + 1, j, i] = NAN
        for nm in s:
            t.put(nm, s[nm])
        t.set("chkvar", 1)
        with pytest.raises(BlomGpuError) as x:
            t.stage("chkvar", *hostinit.step_indices(0, kk))
        want = R.chkvar(s, kk, kk, sel, ii, jj, i0=ii, j0=jj)
        assert str(x.value) == "blom:" + want
        assert "(i =%4d, j =%4d, k =   2)" % (ii + i - NB + 1, jj + j - NB + 1) in want
    finally:
        t.close()


def test_chkvar_on_a_tile_reports_global_indices():
    check_chkvar_tile()


# ---- the clock and the coupling interval ------------------------------------------------------------------------------------------------------
def check_clock():
    """step_time restated against the day rule written out: a year of 24 days of 4 steps, from its last day across its end"""
    clock = dict(CLOCK, nday_of_year=24)
    seen = []
    for ns1 in range(1, 13):
        clock = R.step_time(clock, ns1)
        seen.append((clock["nday_of_year"], clock["lmi"][2], clock["xmi"]))
    assert seen[2] == (24, 12, 0.875) and seen[3] == (1, 1, 0.0) and seen[4] == (1, 1, 0.125) and seen[11] == (3, 2, 0.0), seen
    assert R.step_time(dict(CLOCK, nday_of_year=1), 4)["lmi"] == (11, 12, 1, 2, 3)


def test_step_time_restated():
    check_clock()


EXTRA_OUT = ["surflx", "sswflx", "surrlx", "salflx", "brnflx", "salrlx", "hmltfz", "ustar", "taux", "tauy", "trflx", "t_rs_nonloc", "s_rs_nonloc",
             "swfc1", "swfc2", "swal1", "swal2", "chl10", "eiacc", "pracc", "rnf", "fmltfz", "sfl", "frzpot", "mltpot", "hicem", "ficem", "tsi_tda"]


def interval_context(config):
    """the four configurations of the interval check: (case, masks, g), declared and with the end of the step switched on"""
    import test_gpu_thermf_cesm as tc
    import test_gpu_thermf_ben02 as tb
    if config in ("cesm", "cesm_hybrid"):
        hybrid = config == "cesm_hybrid"
        case, masks, g = tc.context("chan_s" if hybrid else "chan_s_tke", dict(tc.BASE), hybrid=hybrid)
        g.set("swamth", "chlorophyll_ma94")
        g.iniswa(chl_of(case))
        g.set("sprfac", 1)
        g.put("ipwocn", ipwocn_of(case, masks))
    elif config == "ben02":
        case, masks, g = tb.context("chan_s_tke", dict(tb.BASE))
    else:
        case, masks, g = lyr.full_context("chan_s_tke")
        set_time(g, (11, 12, 1, 2, 3), 0.3)
    for nm, v in CLOCK.items():
        g.set(nm, v)
    g.set("chkvar", 1)
    return case, masks, g


def check_interval(config, calls=(1, 2, 3, 4, 5), **extra):
    """blomgpu_step(N) with step_time = 1, N = 1..5 one after the other, against N calls of one step with the host setting the scalars
    from the restated step_time: from the last day of the year, so that its end, a month's end and the days' ends fall inside calls"""
    case, masks, a = interval_context(config)
    _, _, b = interval_context(config)
    try:
        for nm, v in extra.items():
            a.set(nm, v)
        clock = dict(CLOCK, nday_of_year=24)
        for g in (a, b):
            g.set("nday_of_year", 24)
        ns, days = 1, set()
        for g in (a, b):                                  # (one step from rest first: the time step doubles behind it)
            set_time(g, (10, 11, 12, 1, 2), 0.5)
            g.set("step_time", 0)
            assert g.step(0, 1) == 1
        a.set("step_time", 1)
        for n in calls:
            assert a.step(ns, n) == ns + n
            for k in range(n):
                clock = R.step_time(clock, ns + k + 1)
                days.add((clock["nday_of_year"], clock["lmi"][2]))
                b.set("nday_of_year", clock["nday_of_year"])
                set_time(b, clock["lmi"], clock["xmi"])
                assert b.step(ns + k, 1) == ns + k + 1
            ns += n
            assert a.get_real("xmi") == clock["xmi"] and a.get_real("nday_of_year") == clock["nday_of_year"]
            assert tuple(int(a.get_real("l%dmi" % q)) for q in range(1, 6)) == clock["lmi"]
            names = [nm for nm in list(STATE_FIELDS) + EXTRA_OUT if a.has_field(nm)]
            bad = [nm for nm in names if not same_bytes(a.get(nm), b.get(nm))]
            assert not bad, f"{config}: a call of {n} steps with step_time differs from {n} calls with the host's clock: {bad}"
            if a.has_field("eiacc"):
                assert a.get_real("prfac") == b.get_real("prfac")
        assert {(24, 12), (1, 1)} <= days and ((3, 2) in days or ns < 12), days
        out = {nm: a.get(nm) for nm in names}
        out["prfac"] = a.get_real("prfac") if a.has_field("eiacc") else None
        return out
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("config", ["cesm", "cesm_hybrid", "ben02", "channel"])
def test_one_call_of_n_steps_equals_n_calls_with_the_hosts_clock(config):
    out = check_interval(config)
    assert np.isfinite(out["temp"]).all()
    if config.startswith("cesm"):
        assert out["prfac"] != 1.0 and out["chl10"].any() and out["eiacc"].any()


def check_staged(hybrid):
    """four steps in one call against the stages of the stepper's tuple one by one, with updswa, fwbbal and chkvar where blom_step calls
    them (the clock fixed on the year's first day with four steps a day: the fourth step ends a year for fwbbal)"""
    out = []
    for staged in (False, True):
        case, masks, g = interval_context("cesm_hybrid" if hybrid else "cesm")
        try:
            g.set("nday_of_year", 1)
            set_time(g, (11, 12, 1, 2, 3), 0.3)
            if staged:
                stages = stepper.HYBRID_STAGES_CESM_END if hybrid else stepper.FULL_STAGES_LIVE_CESM_END
                ns = 0
                for _ in range(4):
                    ns = stepper.dyncore_step(g, ns, case.params["baclin"], stages=stages)
            else:
                assert g.step(0, 4) == 4
            names = [nm for nm in list(STATE_FIELDS) + EXTRA_OUT if g.has_field(nm)]
            out.append(dict({nm: g.get(nm) for nm in names}, prfac=g.get_real("prfac")))
        finally:
            g.close()
    a, b = out
    bad = [nm for nm in a if nm != "prfac" and not same_bytes(a[nm], b[nm])]
    assert not bad, f"four steps in one call differ from the stages of the stepper's tuple: {bad}"
    assert a["prfac"] == b["prfac"] != 1.0 and not a["eiacc"].any() and a["chl10"].any()
    for tup in (stepper.FULL_STAGES_LIVE_CESM_END, stepper.HYBRID_STAGES_CESM_END, stepper.FULL_STAGES_LIVE_BEN02_END):
        assert tup[-2:] == ("fwbbal", "chkvar") and tup.count("updswa") == 1
    assert stepper.FULL_STAGES_LIVE_CESM_END[:3] == ("init_fluxes", "getfrc_cesm", "updswa")
    assert stepper.FULL_STAGES_LIVE_BEN02_END[:2] == ("init_fluxes", "updswa")


@pytest.mark.parametrize("hybrid", [False, True])
def test_step_equals_the_stages_of_the_steppers_tuple(hybrid):
    check_staged(hybrid)


def check_phys_dag():
    a = check_interval("cesm")
    b = check_interval("cesm", phys_dag=0)
    bad = [nm for nm in a if nm != "prfac" and not same_bytes(a[nm], b[nm])]
    assert not bad and a["prfac"] == b["prfac"], bad


def test_phys_dag_0_equals_the_default():
    check_phys_dag()


def check_refusals():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.dyncore_context("chan_s")
    try:
        g.set("step_time", 1)
        g.set("nstep_in_day", 0)
        with pytest.raises(BlomGpuError, match="step_time = 1 needs nstep_in_day >= 1 and nday_in_year >= 1"):
            g.step(0, 1)
        g.set("nstep_in_day", 4)
        g.set("nday_in_year", 0)
        with pytest.raises(BlomGpuError, match="step_time = 1 needs nstep_in_day >= 1 and nday_in_year >= 1"):
            g.step(0, 1)
        g.set("nday_in_year", 24)
        g.set("step_time", 0)
        g.set("use_graph", 1)
        for name, on, off in (("step_time", lambda: g.set("step_time", 1), lambda: g.set("step_time", 0)),
                              ("chkvar", lambda: g.set("chkvar", 1), lambda: g.set("chkvar", 0)),
                              ("sprfac", lambda: g.set("sprfac", 1), lambda: g.set("sprfac", 0)),
                              ("swamth", lambda: g.set("swamth", "chlorophyll_ma94"), lambda: g.set("swamth", "jerlov"))):
            on()
            with pytest.raises(BlomGpuError, match="use_graph"):
                g.step(0, 1)
            off()
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.set("swamth", "chlorophyll_ohl03")
            g.iniswa()
        # the new names are options of their own table: the pinned table does not list them
        import ctypes as C
        buf, k, listed = C.create_string_buffer(64), 0, []
        while g.lib.blomgpu_option_name(k, buf, 64, None) == 0:
            listed.append(buf.value.decode())
            k += 1
        assert not {"step_time", "chkvar", "sprfac", "prfac", "swamth", "jwtype", "chlopt"} & set(listed)
        # by name like the planes of the forced ocean-ice experiment
        g.set("use_graph", 0)
        g.set("swamth", "chlorophyll_ma94")
        g.iniswa()
        g.set("sprfac", 1)
        names = g.field_names()
        for nm, nlev in (("chl10c", 12), ("chl10", 1), ("eiacc", 1), ("pracc", 1)):
            assert nm in names and g.field_info(nm) == (nlev, False)
        assert g.field_info("ipwocn") == (1, True)
    finally:
        g.close()


def test_refusals_and_names():
    check_refusals()


@pytest.mark.parametrize("cfg", ["chan_s", "box_s"])
def test_undeclared_context_steps_to_the_committed_golden_checksums(cfg):
    from test_gpu_thermf_cesm import check_undeclared_golden
    check_undeclared_golden(cfg)
