"""The surface forcing of the forced ocean-ice experiment on the device (expcnf = 'ben02clim'; blom_amd/csrc/stage_thermf_ben02.hip:
k_sfcstr_ben02, k_thermf_ben02_flux, k_thermf_ben02_corr, and the batched sums of halo.hip) against tests/thermf_ben02_ref.py, the numpy
restatement of ben02/mod_sfcstr_ben02.F90:44-61 and ben02/mod_thermf_ben02.F90:96-671.  Every comparison is == on the bytes, over the
whole padded arrays: the outputs are preset to a pattern so that a store to a land or halo point is seen.

check_stage: a few declared steps from rest with the synthetic forcing of blom_amd.hostinit.ben02_forcing, then the forcing and ice state
once more (the steps have moved the ice), a third of the surface water put below the freezing point, and the two stages once more on the
device and in numpy from the same downloaded state.  The option sets: relaxation from the climatology / off, aptflx + apsflx, ditflx +
disflx over steps that change ntld once, srxbal with an ipwocn that leaves a part of the ocean out, gls = 1 (chan_s_tk2).  The inputs reach
every branch of the routine, and the checks assert that they do (thermf_ben02_ref.BRANCHES).  tests/test_hostemu_thermf_ben02.py runs the
same functions on the host emulation."""
import contextlib

import numpy as np
import pytest

from blom_amd import hostinit, stepper
from blom_amd.cases import default_grid, make_case
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import same_bytes
import thermf_ben02_ref as R

pytestmark = pytest.mark.gpu

NB = 4
HYBRID = ("chan_s", "cntiso_hybrid", "nudge")             # one of the cases tests/test_gpu_dia_hybrid.py uses
ICE = "ficem hicem hsnwm tsrfm ticem alb iagem rnfres".split() + R.TDA
FLUX = ("rnf fmltfz sfl brnflx salflx hmltfz surflx sswflx trflx surrlx salrlx util2 util3 salt_corr trc_corr ustar t_rs_nonloc s_rs_nonloc "
        "tflxdi sflxdi").split()
OUT = ICE + FLUX + ["taux", "tauy"]
PRESET = "ticem alb rnf fmltfz sfl brnflx salflx hmltfz surflx sswflx trflx surrlx salrlx util2 util3 ustar taux tauy t_rs_nonloc s_rs_nonloc".split()
INPUTS = ("dp temp saln p trc scp2 difdia plat swfc2 swal2 sstclm ricclm sssclm tflxap sflxap ipwocn eva lip rfi".split()
          + [f for f in hostinit.BEN02_FLUXES])

BASE = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, trxlim=1.5, srxlim=0.5, xmi=0.3, sref=34.65, aptflx=0, apsflx=0, ditflx=0,
            disflx=0, srxbal=0, nstep_in_day=4, nday_of_year=1, nday_in_year=24)
OPTION_SETS = {
    "clim": dict(),
    "off": dict(trxday=0.0, srxday=0.0),
    "ap": dict(aptflx=1, apsflx=1, nday_of_year=20),
    "di": dict(ditflx=1, disflx=1),                      # nstep = 1, 2, 3 of 4 a day, 24 days a year: ntld = 1, 2, 2
    "srxbal": dict(srxbal=1),
}
LMI = (11, 12, 1, 2, 3)
EXPCNF = "ben02clim"


def declare(g, case, opts, seed=3):
    g.set("expcnf", EXPCNF)
    for nm in ("ditflx", "disflx"):                       # (the declaration zeroes what they switch on)
        g.set(nm, int(opts[nm]))
    g.inifrc_ben02()
    f = hostinit.put_ben02_forcing(g, case, seed=seed)
    for nm, v in opts.items():
        g.set(nm, v)
    return f


def context(cfg, opts, hybrid=False, ntr=None):
    if hybrid:
        from test_gpu_dia_hybrid import hybrid_context
        case, masks, g = hybrid_context(*HYBRID)
        hostinit.init_forcing(g, case)
    elif ntr is not None:
        case = make_case(cfg, ntr=ntr)
        nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
        masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
        import bench
        g = bench.device_for_bench(case, nreg, masks, live=True)
    else:
        case, masks, g = lyr.full_context(cfg)
    declare(g, case, opts)
    return case, masks, g


def ref_options(g, case, opts, hybrid, nstep):
    p = case.params
    return dict(opts, lmi=LMI, area=g.get_real("area"), baclin=float(p["baclin"]), hybrid=hybrid, itrtke=int(p.get("itrtke", -1)),
                itrgls=int(p.get("itrgls", -1)), gls=int(p.get("gls", 0)), nstep=nstep, nreg=case.nreg, kdm=case.kdm, ntr=case.ntr)


def pattern(shape, k):
    return 7.25 + 0.001 * k + 1.0e-6 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


def cold_points(case):
    """the third of the plane whose surface water the checks put below the freezing point: every ice class of ben02_forcing, in both
    hemispheres"""
    nj, ni = case.jdm + 2 * NB, case.idm + 2 * NB
    return (np.arange(ni)[None, :] + np.arange(nj)[:, None]) % 3 == 0


def prepare(g, case, masks, idx, hybrid, seed=3):
    """the forcing and the ice state as generated, surface water below the freezing point at cold_points, outputs preset to a pattern,
    and under the hybrid coordinate four columns whose walks leave at k = 1, in the middle, at kk, and never"""
    kk = case.kdm
    nn, k1n = idx[3], idx[5]
    f = hostinit.put_ben02_forcing(g, case, seed=seed)
    sel = R.owned(masks, case.idm, case.jdm)["p"]
    temp, dp = g.get("temp"), g.get("dp")
    cold = cold_points(case)
    odd = cold & (np.arange(cold.shape[0])[:, None] % 2 == 1)
    for lev in (k1n - 1, (k1n - 1 + kk) % (2 * kk)):
        temp[lev][cold] = -3.0
        temp[lev][odd] = -13.0                                # (enough new ice to take a cover of 0.9949 past fice_max)
    if hybrid:
        jj = NB + case.jdm // 2
        cols = [i for i in range(NB, NB + case.idm) if sel[jj, i] and sel[jj + 1, i]]
        assert len(cols) >= 8
        onem = R.ONEM
        a, b, c, d = cols[4], cols[7], cols[5], cols[6]
        dp[nn:nn + kk, jj, a] = 50.0 * onem                  # leaves at k = 1
        dp[nn:nn + kk, jj, b] = 8.0 * onem                   # leaves in the middle
        dp[nn:nn + kk - 1, jj, c] = 0.5 * onem              # leaves at kk
        dp[nn + kk - 1, jj, c] = 100.0 * onem
        dp[nn:nn + kk, jj, d] = 0.0                           # never leaves: 2**13 Pa in all, the fractions are exact
        dp[nn:nn + 5, jj, d] = [4096.0, 2048.0, 1024.0, 512.0, 512.0]
        g.put("dp", dp)
    g.put("temp", temp)
    nj, ni = sel.shape
    for k, nm in enumerate(PRESET):
        nlev = max(case.ntr, 1) if nm == "trflx" else g.field_info(nm)[0]
        g.put(nm, pattern((nlev, nj, ni), k))
    return f


def download(g, names):
    return {nm: g.get(nm) for nm in names if g.has_field(nm)}


def halo1(case, vland=0.0):
    def halo(a):
        b = np.array(a, dtype=np.float64)[None].copy()
        hostinit.xctilr_np(b, 1, 1, 1, 1, case.nreg, case.idm, case.jdm, vland, 1)
        return b[0]
    return halo


def check_stage(cfg, optname, hybrid=False, grid=None, ntr=None, presteps=3):
    opts = dict(BASE, **OPTION_SETS[optname])
    with default_grid(grid) if grid else contextlib.nullcontext():
        case, masks, g = context(cfg, opts, hybrid=hybrid, ntr=ntr)
    try:
        kk = case.kdm
        assert g.step(0, presteps) == presteps                # the declared step, from rest
        assert g.ben02_ntda() == presteps
        ns = presteps
        calls = 3 if optname == "di" else 1
        if optname == "di":                                   # (the steps above have accumulated: the zeroing once more)
            g.inifrc_ben02()
        seen_all = []
        for call in range(calls):
            idx = hostinit.step_indices(ns, kk)
            if call == 0:
                prepare(g, case, masks, idx, hybrid)
            nstep = ns + 1 if optname != "di" else call + 1
            g.set("nstep", nstep)
            names = [nm for nm in set(INPUTS + OUT + ["thermf_util", "ztx", "mty", "tauxice", "tauyice"])]
            if not (opts["ditflx"] or opts["disflx"]):
                names = [nm for nm in names if nm not in ("tflxdi", "sflxdi")]
            if not (opts["aptflx"] or opts["apsflx"]):
                names = [nm for nm in names if nm not in ("tflxap", "sflxap")]
            s = download(g, names)
            o = ref_options(g, case, opts, hybrid, nstep)
            ntda = g.ben02_ntda()
            g.stage("sfcstr", *idx)
            launches = g.get_real("thermf_ben02_launches")
            g.stage("thermf", *idx)
            assert g.get_real("thermf_ben02_launches") - launches == 4, "thermf_ben02 is four launches (up to 32 planes in the batch)"
            assert g.ben02_ntda() == ntda + 1
            seen = {}
            R.sfcstr(s, masks, case.idm, case.jdm, case.nreg, halo=halo1(case, float(case.params.get("vland", 0.0))))
            res = R.thermf(s, o, idx, masks, case.idm, case.jdm, seen)
            seen_all.append((seen, res))
            got = download(g, [nm for nm in OUT if nm in s])
            bad = [nm for nm in got if not same_bytes(got[nm], s[nm])]
            assert not bad, f"{cfg} {optname} call {call}: {bad} differ from the restated routines"
            sel = R.owned(masks, case.idm, case.jdm)
            util = g.get("thermf_util")
            assert same_bytes(util[:len(res["util"])][:, sel["p"]], res["util"][:, sel["p"]])
            assert g.get_real("sflxc") == res["sflxc"], (g.get_real("sflxc"), res["sflxc"])
            if call == 0:                                     # the corrections are reset, from non-zero inputs
                assert not got["salt_corr"][0][sel["p"]].any()
                for nt in res["passive"]:
                    assert not got["trc_corr"][nt - 1][sel["p"]].any()
        return case, masks, opts, seen_all, g.cesm_nflxdi(), {nm: g.get(nm) for nm in ("tflxdi", "sflxdi")} if optname == "di" else None
    finally:
        g.close()


def check_not_vacuous(cfg, optname, hybrid=False, **kw):
    case, masks, opts, seen_all, nflxdi, di = check_stage(cfg, optname, hybrid=hybrid, **kw)
    seen, res = seen_all[0]
    print(cfg, optname, "hybrid" if hybrid else "isopycnic", "seen:", seen)
    relax = opts["trxday"] > 0.0
    assert not R.missing(seen, relax=relax), (R.missing(seen, relax=relax), seen)
    if opts["srxbal"]:
        assert seen["qp"] != 1.0 and seen["qn"] != 1.0, seen
        assert res["sums"]["totsrp"] > 0.0 > res["sums"]["totsrn"]
    if hybrid and relax:
        kk = case.kdm
        for key in ("t_exits", "s_exits"):
            e = seen[key]
            assert e[1] > 0 and e[kk] > 0 and e[0] > 0 and sum(e[k] for k in range(2, kk)) > 0, (key, e)
    if optname == "di":
        assert [r["ntld"] for _, r in seen_all] == [1, 2, 2]
        assert list(nflxdi[:3]) == [1, 2, 0] and not nflxdi[3:].any()
        sel = R.owned(masks, case.idm, case.jdm)["p"]
        for nm in ("tflxdi", "sflxdi"):
            assert di[nm][0][sel].any() and di[nm][1][sel].any() and not di[nm][2:].any(), nm


@pytest.mark.parametrize("optname", list(OPTION_SETS))
def test_stages_equal_the_restated_routines(optname):
    check_not_vacuous("chan_s_tke", optname)


@pytest.mark.parametrize("optname", ["clim", "di"])
def test_stages_equal_the_restated_routines_under_the_hybrid_coordinate(optname):
    check_not_vacuous("chan_s", optname, hybrid=True)


@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke", "chan_b"])
def test_stages_on_the_closed_box_across_the_arctic_seam_and_on_long_rows(cfg):
    check_stage(cfg, "srxbal")


def test_stages_with_the_generic_length_scale():
    case = make_case("chan_s_tk2")
    assert case.params["gls"] == 1
    check_stage("chan_s_tk2", "clim")


def test_stages_on_the_warped_grid():
    check_not_vacuous("chan_s_tke", "clim", grid="warped_eq")


def test_four_launches_with_24_tracers():
    """1 + 24 sums in one batch (chan_s, no turbulence tracers)"""
    check_stage("chan_s", "clim", ntr=24, presteps=2)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
FIELDS = [f for f in STATE_FIELDS] + ICE + ["surflx", "sswflx", "surrlx", "salflx", "brnflx", "salrlx", "hmltfz", "ustar", "taux", "tauy", "trflx",
                                             "t_rs_nonloc", "s_rs_nonloc", "rnf", "fmltfz", "sfl"]


def stepped(cfg, hybrid, nsteps=4, staged=False, **extra):
    opts = dict(BASE)
    case, masks, g = context(cfg, opts, hybrid=hybrid)
    try:
        for nm, v in extra.items():
            g.set(nm, v)
        if staged:
            stages = stepper.HYBRID_STAGES_BEN02 if hybrid else stepper.FULL_STAGES_LIVE_BEN02
            ns = 0
            for _ in range(nsteps):
                ns = stepper.dyncore_step(g, ns, case.params["baclin"], stages=stages)
        else:
            assert g.step(0, nsteps) == nsteps
        assert g.ben02_ntda() == nsteps
        return {nm: g.get(nm) for nm in FIELDS if g.has_field(nm)}
    finally:
        g.close()


def check_step(hybrid):
    cfg = "chan_s" if hybrid else "chan_s_tke"
    a = stepped(cfg, hybrid)
    b = stepped(cfg, hybrid, staged=True)
    bad = [nm for nm in a if not same_bytes(a[nm], b[nm])]
    assert not bad, f"four steps in one call differ from the stages of the stepper's tuple: {bad}"
    assert a["surflx"].any() and a["taux"].any() and a["hicem"].any() and a["fice_tda"].any()
    assert np.isfinite(a["temp"]).all() and np.isfinite(a["hicem"]).all()
    if hybrid:
        assert a["t_rs_nonloc"][1].any()
    else:
        c = stepped(cfg, hybrid, phys_dag=0)
        bad = [nm for nm in a if not same_bytes(a[nm], c[nm])]
        assert not bad, f"phys_dag = 0 differs from the default: {bad}"


def test_step_equals_the_stages_one_by_one():
    check_step(False)


def test_hybrid_step_equals_the_stages_one_by_one():
    check_step(True)


# ---- ntda and the accumulators -------------------------------------------------------------------------------------------------------------
def check_ntda():
    """one call of N = 1..3 steps leaves ntda = N and the five _tda planes equal to the sums of N single-step calls; the reset zeroes both"""
    case, masks, a = context("chan_s_tke", dict(BASE))
    _, _, b = context("chan_s_tke", dict(BASE))
    try:
        ns = 0
        for n in (1, 2, 3):
            assert a.step(ns, n) == ns + n and a.ben02_ntda() == n
            for k in range(n):
                assert b.step(ns + k, 1) == ns + k + 1
            assert b.ben02_ntda() == n
            for nm in R.TDA:
                assert same_bytes(a.get(nm), b.get(nm)), (n, nm)
                assert a.get(nm).any(), nm
            ns += n
            for g in (a, b):
                g.ben02_reset_tda()
                assert g.ben02_ntda() == 0 and not any(g.get(nm).any() for nm in R.TDA)
    finally:
        a.close()
        b.close()


def test_ntda_and_the_accumulated_planes():
    check_ntda()


# ---- tiles -------------------------------------------------------------------------------------------------------------------------------
TILE_CHECK = ["u", "v", "dp", "temp", "saln", "trc", "surflx", "sswflx", "surrlx", "salflx", "brnflx", "salrlx", "hmltfz", "ustar", "taux", "tauy",
              "trflx", "ficem", "hicem", "hsnwm", "tsrfm", "ticem", "iagem", "rnfres", "alb"] + R.TDA


def check_tiles(npx=2, npy=1, nsteps=3, cfg="chan_s_tke"):
    """tiles of one process step the declared full-physics step to the single tile's bytes: the sums of thermf_ben02 go through the
    one-plane paths there, sfcstr_ben02's halo of ficem and hicem through the group's gather; srxbal is refused"""
    import threading
    from blom_amd.gpu import BlomGpu, BlomGpuError, TileGroup
    from blom_amd.tiles import tile_extents, tile_window, scatter_state
    from test_gpu_tiles import _single, ALL, FORCING
    case, masks, fields, ref = _single(cfg, nsteps)
    hostinit.init_forcing(ref, case)
    lyr.forcing(ref, case)
    opts = dict(BASE)
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
        frc = declare(ref, case, opts)
        for t in tiles.values():
            t.set("expcnf", EXPCNF)
            t.inifrc_ben02()
        scatter_state(ref, tiles, case, npx, npy, [f for f in ALL if f in fields] + [f for f in FORCING if ref.has_field(f)]
                      + [f for f in frc if f not in ALL and f not in FORCING])
        w = masks["ip"][4:-4, 4:-4] > 0
        area = float(np.sum(ref.get("scp2")[0][4:-4, 4:-4][w]))

        def setup(g):
            g.set("area", area)
            lyr.options(g)
            g.set("full_physics", 1)
            for nm, v in opts.items():
                g.set(nm, v)
        errs = []

        def run(t):
            try:
                setup(t)
                assert t.step(0, nsteps) == nsteps
                t.sync()
            except Exception as e:          # a failing tile would leave the others at a barrier
                errs.append(e)
        setup(ref)
        assert ref.step(0, nsteps) == nsteps
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x_.start() for x_ in th]
        [x_.join(timeout=300) for x_ in th]
        assert not errs, errs
        bad = []
        for nm in TILE_CHECK:
            whole = ref.get(nm)
            for (px, py), t in tiles.items():
                mine = t.get(nm)[:, 4:4 + jj, 4:4 + ii]
                if not same_bytes(mine, whole[:, 4 + py * jj:4 + (py + 1) * jj, 4 + px * ii:4 + (px + 1) * ii]):
                    bad.append((nm, px, py))
        assert not bad, bad
        assert ref.get("salflx").any() and ref.get("surrlx").any() and ref.get("hicem").any()
        assert all(t.ben02_ntda() == nsteps for t in tiles.values())
        t0 = tiles[(0, 0)]
        t0.set("srxbal", 1)
        with pytest.raises(BlomGpuError, match="srxbal"):
            t0.stage("thermf", *hostinit.step_indices(nsteps, case.kdm))
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_two_tiles_in_one_process_equal_the_single_tile(npx, npy):
    check_tiles(npx, npy)


# ---- a context that never declares: the committed golden fixtures ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["chan_s", "box_s"])
def test_undeclared_context_steps_to_the_committed_golden_checksums(cfg):
    from test_gpu_thermf_cesm import check_undeclared_golden
    check_undeclared_golden(cfg)


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------
NEW_FIELDS = ("hicem hsnwm ustari tauxice tauyice iagem tsrfm ticem tsi dfl albw alb rnfins rnfres tsi_tda tml_tda sml_tda alb_tda fice_tda "
              "ztx mty thermf_util ipwocn tflxap sflxap tflxdi sflxdi").split()


def check_interface():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.full_context("chan_s_tke")
    _, _, h = lyr.full_context("chan_s_tke")
    try:
        six = hostinit.step_indices(0, case.kdm)
        # undeclared: the three refusals of before, word for word, and nothing of the experiment exists
        for e in ("ben02clim", "ben02syn", "single_column"):
            g.set("expcnf", e)
            with pytest.raises(BlomGpuError) as x:
                g.stage("thermf", *six)
            assert str(x.value) == "thermf: expcnf = %s is not built on the device" % e
            with pytest.raises(BlomGpuError) as x:
                g.stage("sfcstr", *six)
            assert str(x.value) == " sfcstr: expcnf = %s is not built on the device (sfcstr_cesm / sfcstr_ben02)" % e
            with pytest.raises(BlomGpuError) as x:
                g.step(0, 1)
            assert "is not built on the device" in str(x.value)
        for nm in NEW_FIELDS:
            assert not g.has_field(nm), nm
        assert "hicem" not in g.field_names()
        with pytest.raises(BlomGpuError, match="blomgpu_inifrc_ben02"):
            g.ben02_reset_tda()
        assert g.get_real("thermf_ben02_launches") == 0.0
        # a wrong expcnf at the declaration
        for e in ("channel", "cesm", "fuk95"):
            g.set("expcnf", e)
            with pytest.raises(BlomGpuError, match="is not an experiment of mod_ben02"):
                g.inifrc_ben02()
        assert not g.has_field("hicem")
        # use_graph at the declaration, in the step and in the stages
        g.set("expcnf", "ben02syn")
        g.set("use_graph", 1)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.inifrc_ben02()
        g.set("use_graph", 0)
        g.inifrc_ben02()
        names = g.field_names()
        for nm in NEW_FIELDS:
            assert g.has_field(nm) and nm in names, nm
        assert "swa_da" not in names and not g.has_field("hmlt")
        assert all(not g.get(nm).any() for nm in NEW_FIELDS if g.field_info(nm)[0] <= 1 + case.ntr)
        assert g.get("thermf_util").shape[0] == 1 + case.ntr and g.get("tflxdi").shape[0] == 48 and g.get("hicem").shape[0] == 1
        g.set("use_graph", 1)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.step(0, 1)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.stage("thermf", *six)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.stage("sfcstr", *six)
        g.set("use_graph", 0)
        # both declarations on one context, either way round
        with pytest.raises(BlomGpuError, match="blomgpu_inifrc_ben02"):
            g.inifrc_cesm()
        h.set("expcnf", "cesm")
        h.inifrc_cesm()
        h.set("expcnf", "ben02clim")
        with pytest.raises(BlomGpuError, match="blomgpu_inifrc_cesm"):
            h.inifrc_ben02()
        # declared, then expcnf = 'channel': the channel path
        g.set("expcnf", "channel")
        assert g.step(0, 2) == 2
        assert not g.get("hicem").any() and not g.get("fice_tda").any()
    finally:
        g.close()
        h.close()


def test_interface():
    check_interface()
