"""The surface forcing of the coupled experiment on the device (expcnf = 'cesm'; blom_amd/csrc/stage_thermf_cesm.hip: k_getfrc_cesm,
k_sfcstr_cesm, k_thermf_cesm_flux, k_thermf_cesm_corr; blom_amd/csrc/halo.hip: k_xcsum_rows_batch, k_xcsum_total_batch) against
tests/thermf_cesm_ref.py, the numpy restatement of cesm/mod_cesm.F90:213-262, cesm/mod_sfcstr_cesm.F90:43-55 and
cesm/mod_thermf_cesm.F90:74-410.  Every comparison is == on the bytes, over the whole padded arrays: the outputs are preset to a pattern
so that a store to a land or halo point is seen.

check_stage: a few steps from rest with the declaration and random coupler forcing, then the three stages once more (several times
where the option set needs it) on the device and in numpy from the same downloaded state.  The option sets: relaxation off / from the
climatologies / from the streams, aptflx + apsflx, ditflx + disflx over steps that change ntld once, srxbal with an ipwocn that
excludes a basin, smtfrc on and off with l1ci != l2ci, gls = 1 (chan_s_tk2).  The inputs are made so that every branch is taken, and
the checks assert that it is.  tests/test_hostemu_thermf_cesm.py runs the same functions on the host emulation."""
import contextlib

import numpy as np
import pytest

from blom_amd import hostinit, stepper
from blom_amd.cases import default_grid, make_case
from parity import STATE_FIELDS
import test_gpu_diaacc as lyr
from test_gpu_diaacc import same_bytes
import thermf_cesm_ref as R

pytestmark = pytest.mark.gpu

HYBRID = ("chan_s", "cntiso_hybrid", "nudge")             # one of the cases tests/test_gpu_dia_hybrid.py uses
DA = [nm + "_da" for nm in hostinit.CESM_DA]
GETFRC_OUT = hostinit.CESM_DA
THERMF_OUT = ("surflx sswflx surrlx salflx brnflx salrlx hmltfz trflx ustar frzpot mltpot salt_corr trc_corr util2 util3 "
              "t_rs_nonloc s_rs_nonloc tflxdi sflxdi").split()
OUT = list(GETFRC_OUT) + ["taux", "tauy"] + THERMF_OUT
INPUTS = ("dp temp saln p trc scp2 difdia sstclm ricclm sssclm sst_stream sss_stream ice_stream tflxap sflxap ipwocn").split() + DA

# (name, options on top of BASE, steps the stages are called for)
BASE = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, trxlim=1.5, srxlim=0.5, xmi=0.3, sref=34.65, smtfrc=1, nstep_in_cpl=4,
            l1ci=1, l2ci=2, use_stream_relaxation=0, aptflx=0, apsflx=0, ditflx=0, disflx=0, srxbal=0, nstep_in_day=4, nday_of_year=1,
            nday_in_year=24)
OPTION_SETS = {
    "clim": dict(),
    "stream": dict(use_stream_relaxation=1, smtfrc=0, l1ci=2, l2ci=1),
    "off": dict(trxday=0.0, srxday=0.0),
    "ap": dict(aptflx=1, apsflx=1, nday_of_year=20),
    "di": dict(ditflx=1, disflx=1),                      # nstep = 1, 2, 3 of 4 a day, 24 days a year: ntld = 1, 2, 2
    "srxbal": dict(srxbal=1),
}
LMI = (11, 12, 1, 2, 3)


def declare(g, case, opts, seed=3):
    g.set("expcnf", "cesm")
    for nm in ("ditflx", "disflx"):                       # (idarlx reads them)
        g.set(nm, int(opts[nm]))
    g.inifrc_cesm()
    f = hostinit.put_cesm_forcing(g, case, seed=seed)
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
    o = dict(opts, lmi=LMI, area=g.get_real("area"), baclin=float(p["baclin"]), hybrid=hybrid, itrtke=int(p.get("itrtke", -1)),
             itrgls=int(p.get("itrgls", -1)), gls=int(p.get("gls", 0)), nstep=nstep, nreg=case.nreg, kdm=case.kdm, ntr=case.ntr)
    return o


def pattern(shape, k):
    return 7.25 + 0.001 * k + 1.0e-6 * np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


def prepare(g, case, masks, idx, hybrid):
    """non-zero corrections, a patch of surface water below the freezing point, and under the hybrid coordinate four columns whose
    walks leave at k = 1, in the middle, at kk, and never (a column shallower than trxdpt whose fractions are exact)"""
    kk = case.kdm
    nn, k1n = idx[3], idx[5]
    sel = R.owned(masks, case.idm, case.jdm)["p"]
    temp, dp = g.get("temp"), g.get("dp")
    jj = NB + case.jdm // 2
    cols = [i for i in range(NB, NB + case.idm) if sel[jj, i] and sel[jj + 1, i]]
    assert len(cols) >= 8
    for lev in (k1n - 1, (k1n - 1 + kk) % (2 * kk)):
        temp[lev, jj + 1, cols[0]:cols[3]] = -3.0             # both time levels: frzpot > 0 here
    if hybrid:
        onem = R.ONEM
        a, b, c, d = cols[4], cols[7], cols[5], cols[6]
        dp[nn:nn + kk, jj, a] = 50.0 * onem                  # leaves at k = 1
        dp[nn:nn + kk, jj, b] = 8.0 * onem                   # leaves in the middle (k = 4 of the 30 m and of the 25 m)
        dp[nn:nn + kk - 1, jj, c] = 0.5 * onem              # leaves at kk
        dp[nn + kk - 1, jj, c] = 100.0 * onem
        dp[nn:nn + kk, jj, d] = 0.0                           # never leaves: 4096 + 2048 + 1024 + 512 + 512 = 2**13 Pa, fractions exact
        dp[nn:nn + 5, jj, d] = [4096.0, 2048.0, 1024.0, 512.0, 512.0]
        g.put("dp", dp)
    g.put("temp", temp)
    nj, ni = sel.shape
    for k, nm in enumerate(OUT):
        if nm in DA or not g.has_field(nm):
            continue
        if nm in ("salt_corr", "trc_corr"):
            continue                                          # (the generator's non-zero corrections stay)
        nlev = g.field_info(nm)[0]
        if nm == "trflx" or nm == "trc_corr":
            nlev = max(case.ntr, 1)
        if nm in ("tflxdi", "sflxdi"):
            continue                                          # accumulators: zeroed by inifrc_cesm
        g.put(nm, pattern((nlev, nj, ni), k))
    f = hostinit.cesm_forcing(case, seed=3)
    g.put("salt_corr", f["salt_corr"])
    if case.ntr:
        g.put("trc_corr", f["trc_corr"])


NB = 4


def download(g, names):
    return {nm: g.get(nm) for nm in names if g.has_field(nm)}


def check_stage(cfg, optname, hybrid=False, grid=None, ntr=None, presteps=3):
    opts = dict(BASE, **OPTION_SETS[optname])
    with default_grid(grid) if grid else contextlib.nullcontext():
        case, masks, g = context(cfg, opts, hybrid=hybrid, ntr=ntr)
    try:
        kk = case.kdm
        assert g.step(0, presteps) == presteps                # the declared step, from rest
        ns = presteps
        calls = 3 if optname == "di" else 1
        if optname == "di":                                   # (the steps above have accumulated: idarlx's zeroing once more)
            g.inifrc_cesm()
            g.set("l1ci", opts["l1ci"])
            g.set("l2ci", opts["l2ci"])
        seen_all = []
        for call in range(calls):
            idx = hostinit.step_indices(ns, kk)
            if call == 0:
                prepare(g, case, masks, idx, hybrid)
            nstep = ns + 1 if optname != "di" else call + 1
            g.set("nstep", nstep)
            names = [nm for nm in set(INPUTS + OUT + ["thermf_util"])]
            if not (opts["ditflx"] or opts["disflx"]):
                names = [nm for nm in names if nm not in ("tflxdi", "sflxdi")]
            if not (opts["aptflx"] or opts["apsflx"]):
                names = [nm for nm in names if nm not in ("tflxap", "sflxap")]
            s = download(g, names)
            o = ref_options(g, case, opts, hybrid, nstep)
            sel = R.owned(masks, case.idm, case.jdm)
            g.stage("getfrc_cesm", *idx)
            g.stage("sfcstr", *idx)
            launches = g.get_real("thermf_cesm_launches")
            g.stage("thermf", *idx)
            assert g.get_real("thermf_cesm_launches") - launches == 4, "thermf_cesm is four launches (up to 32 planes in the batch)"
            seen = {}
            R.getfrc(s, o, sel)
            R.sfcstr(s, sel)
            res = R.thermf(s, o, idx, masks, case.idm, case.jdm, seen)
            seen_all.append((seen, res))
            got = download(g, [nm for nm in OUT if nm in s])
            bad = [nm for nm in got if not same_bytes(got[nm], s[nm])]
            assert not bad, f"{cfg} {optname} call {call}: {bad} differ from the restated routines"
            util = g.get("thermf_util")
            assert same_bytes(util[:len(res["util"])][:, sel["p"]], res["util"][:, sel["p"]])
            assert g.get_real("sflxc") == res["sflxc"], (g.get_real("sflxc"), res["sflxc"])
            # every sum of the batch equals blomgpu_xcsum of the same plane
            nq = len(res["util"])
            batch = g.xcsum_batch("thermf_util", 1, nq)
            single = [g.xcsum("thermf_util", q + 1) for q in range(nq)]
            want = [res["sums"]["salt"]] + [res["sums"]["trc%d" % nt] for nt in res["passive"]]
            assert list(batch) == single == want, (list(batch), single, want)
            # the corrections are reset, from non-zero inputs
            if call == 0:
                assert not got["salt_corr"][0][sel["p"]].any()
                for nt in res["passive"]:
                    assert not got["trc_corr"][nt - 1][sel["p"]].any()
        return case, masks, opts, seen_all, g.cesm_nflxdi(), {nm: g.get(nm) for nm in ("tflxdi", "sflxdi")} if optname == "di" else None
    finally:
        g.close()


def check_not_vacuous(cfg, optname, hybrid=False):
    case, masks, opts, seen_all, nflxdi, di = check_stage(cfg, optname, hybrid=hybrid)
    seen, res = seen_all[0]
    print(cfg, optname, "hybrid" if hybrid else "isopycnic", "seen:", seen)
    assert seen["frzpot_pos"] > 0 and seen["frzpot_zero"] > 0, seen
    assert seen["mltpot_neg"] > 0, seen
    assert seen["brnflx_clipped"] > 0 and seen["brnflx_pos"] > 0, seen
    if opts["trxday"] > 0.0:
        assert seen["sstc_above"] > 0 and seen["sstc_below"] > 0, seen
        assert seen["trxlim_hi"] > 0 and seen["trxlim_lo"] > 0, seen
        assert seen["srxlim_hi"] > 0 and seen["srxlim_lo"] > 0, seen
    if opts["srxbal"]:
        assert seen["qp"] != 1.0 and seen["qn"] != 1.0, seen
        assert res["sums"]["totsrp"] > 0.0 > res["sums"]["totsrn"]
    if hybrid and opts["trxday"] > 0.0:
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


@pytest.mark.parametrize("optname", ["clim", "stream", "di"])
def test_stages_equal_the_restated_routines_under_the_hybrid_coordinate(optname):
    check_not_vacuous("chan_s", optname, hybrid=True)


@pytest.mark.parametrize("cfg", ["box_s", "tri_s_tke"])
def test_stages_on_the_closed_box_and_across_the_arctic_seam(cfg):
    check_stage(cfg, "srxbal")


def test_stages_with_the_generic_length_scale():
    case = make_case("chan_s_tk2")
    assert case.params["gls"] == 1
    check_stage("chan_s_tk2", "clim")


def test_stages_on_the_warped_grid():
    check_stage("chan_s_tke", "clim", grid="warped_eq")


# ---- the batched sums -------------------------------------------------------------------------------------------------------------------
def check_batch_second_round():
    """idm = 580: 65 strips of nine a row, one more than a wavefront takes in a round"""
    from blom_amd.gpu import BlomGpu
    idm, jdm, kdm = 580, 5, 3                                 # (kdm = 3: the smallest blomgpu_create takes)
    nj, ni = jdm + 8, idm + 8
    m = {k: np.ones((nj, ni), np.int32) for k in ("ip", "iu", "iv", "iq")}
    g = BlomGpu(idm, jdm, kdm, 1, 0, m)
    try:
        rng = np.random.default_rng(5)
        a = rng.standard_normal((2 * kdm, nj, ni)) * 10.0 ** rng.integers(-6, 6, (2 * kdm, nj, ni))
        g.put("temp", a)
        batch = list(g.xcsum_batch("temp", 1, 2 * kdm))
        assert batch == [g.xcsum("temp", l + 1) for l in range(2 * kdm)]
        assert batch == [R.xcsum(a[l], m["ip"], idm, jdm) for l in range(2 * kdm)]
        odd = (np.arange(nj * ni).reshape(nj, ni) % 3 == 1).astype(np.int32)
        g.put("kming", odd[None])                             # a mask of the caller's own
        assert list(g.xcsum_batch("temp", 2, 3, mask="kming")) == [R.xcsum(a[l], odd, idm, jdm) for l in (1, 2, 3)]
    finally:
        g.close()


def test_batched_sums_beyond_one_round_of_strips():
    check_batch_second_round()


def test_batched_sums_with_24_tracers():
    """1 + 24 sums in one batch (chan_s, no turbulence tracers), each equal to the single sum and to the restatement"""
    check_stage("chan_s", "clim", ntr=24, presteps=2)


# ---- the step -----------------------------------------------------------------------------------------------------------------------------
FIELDS = [f for f in STATE_FIELDS] + ["surflx", "sswflx", "surrlx", "salflx", "brnflx", "salrlx", "hmltfz", "ustar", "taux", "tauy", "frzpot",
                                      "mltpot", "trflx", "t_rs_nonloc", "s_rs_nonloc", "swa", "ztx"]


def stepped(cfg, hybrid, nsteps=4, staged=False, **extra):
    opts = dict(BASE)
    case, masks, g = context(cfg, opts, hybrid=hybrid)
    try:
        for nm, v in extra.items():
            g.set(nm, v)
        if staged:
            stages = stepper.HYBRID_STAGES_CESM if hybrid else stepper.FULL_STAGES_LIVE_CESM
            ns = 0
            for _ in range(nsteps):
                ns = stepper.dyncore_step(g, ns, case.params["baclin"], stages=stages)
        else:
            assert g.step(0, nsteps) == nsteps
        return {nm: g.get(nm) for nm in FIELDS if g.has_field(nm)}
    finally:
        g.close()


def check_step(hybrid):
    cfg = "chan_s" if hybrid else "chan_s_tke"
    a = stepped(cfg, hybrid)
    b = stepped(cfg, hybrid, staged=True)
    bad = [nm for nm in a if not same_bytes(a[nm], b[nm])]
    assert not bad, f"four steps in one call differ from the stages of the stepper's tuple: {bad}"
    assert a["surflx"].any() and a["taux"].any() and a["frzpot"].shape == a["mltpot"].shape
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


# ---- tiles -------------------------------------------------------------------------------------------------------------------------------
TILE_CHECK = ["u", "v", "dp", "temp", "saln", "trc", "surflx", "sswflx", "surrlx", "salflx", "brnflx", "salrlx", "hmltfz", "ustar", "taux", "tauy",
              "frzpot", "mltpot", "trflx", "swa", "ztx", "mty"]


def check_tiles(npx=2, npy=1, nsteps=3, cfg="chan_s_tke"):
    """tiles of one process (the in-process halo transport) step the declared full-physics step to the single tile's bytes: the sums
    of thermf_cesm go through the one-plane paths there, once per plane"""
    import threading
    from blom_amd.gpu import BlomGpu, TileGroup
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
        cesm = declare(ref, case, opts)
        for t in tiles.values():
            t.set("expcnf", "cesm")
            t.inifrc_cesm()
        scatter_state(ref, tiles, case, npx, npy, [f for f in ALL if f in fields] + [f for f in FORCING if ref.has_field(f)] + list(cesm))
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
        assert ref.get("salflx").any() and ref.get("surrlx").any()
        assert ref.get_real("sflxc") == tiles[(0, 0)].get_real("sflxc") != 0.0
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_two_tiles_in_one_process_equal_the_single_tile(npx, npy):
    check_tiles(npx, npy)


# ---- the step on the warped grid (tests/curvilinear.py) -----------------------------------------------------------------------------------------
def check_step_warped():
    from curvilinear import on_grid
    with on_grid("warped_eq"):
        check_step(False)
        check_step(True)


def check_tiles_warped():
    from curvilinear import on_grid
    with on_grid("warped_eq"):
        check_tiles(2, 1)


def test_step_equals_the_stages_on_the_warped_grid():
    check_step_warped()


def test_two_tiles_equal_the_single_tile_on_the_warped_grid():
    check_tiles_warped()


# ---- a context that never declares: the committed golden fixtures ---------------------------------------------------------------------------
def check_undeclared_golden(cfg="chan_s"):
    """tests/golden/<cfg>_init.npz stepped by blomgpu_step on a context that never declares the coupler's forcing: the reference's
    checksums of every recorded field after the last stage of every step (<cfg>_crc.json) and its final fields (<cfg>_final.npz) --
    what tests/test_gpu_golden.py checks stage by stage, here through the sequence that gained the coupled experiment's branches"""
    import json
    import os
    from blom_amd.checksum import chksum
    from blom_amd.gpu import BlomGpu
    from parity import load_golden_init, put_fields
    here = os.path.dirname(os.path.abspath(__file__))
    eddtra_out = {"umfltd", "vmfltd", "utfltd", "vtfltd", "usfltd", "vsfltd"}
    case = make_case(cfg)
    masks, fields = load_golden_init(cfg)
    gold = json.load(open(os.path.join(here, "golden", f"{cfg}_crc.json")))
    g = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, case.nreg, masks)
    try:
        for nm, v in case.params.items():
            if not nm.endswith("0"):
                g.set(nm, v)
        put_fields(g, fields)
        g.set("delt1", case.params["baclin"])
        assert not g.has_field("swa_da")
        bad, checked = [], 0
        for ns in range(gold["nsteps"]):
            assert g.step(ns, 1) == ns + 1
            for nm, want in gold["crc"][str(ns + 1)][stepper.DYNCORE_STAGES[-1]].items():
                if nm in eddtra_out or not g.has_field(nm):
                    continue
                got = chksum(nm, g.get(nm), masks, case.idm, case.jdm)
                checked += 1
                if got != want:
                    bad.append(f"step {ns + 1} {nm}: crc 0x{got:08x} != 0x{want:08x}")
        assert not bad, bad[:10]
        assert checked >= 10 * gold["nsteps"], checked
        z = np.load(os.path.join(here, "golden", f"{cfg}_final.npz"))
        J, I = slice(4, 4 + case.jdm), slice(4, 4 + case.idm)
        for nm in z.files:
            a = z[nm][:, J, I]
            assert np.array_equal(a, g.get(nm)[:a.shape[0], J, I], equal_nan=True), nm
        assert not g.has_field("swa_da") and "hmlt" not in g.field_names()
    finally:
        g.close()


@pytest.mark.parametrize("cfg", ["chan_s", "box_s"])
def test_undeclared_context_steps_to_the_committed_golden_checksums(cfg):
    check_undeclared_golden(cfg)


# ---- the 48-level arrays before they have memory ------------------------------------------------------------------------------------------------
def check_unallocated_fields():
    """after the declaration tflxap sflxap tflxdi sflxdi have names and no memory: every entry point that takes a field by name gives
    them memory (zeros) or refuses -- one array per entry point, so that each meets an unallocated one"""
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.dyncore_context("chan_s")
    try:
        for nm in ("tflxap", "sflxap", "tflxdi", "sflxdi"):
            with pytest.raises(BlomGpuError, match="unknown field"):
                g.crc(nm, 1, 1)
        g.set("expcnf", "cesm")
        g.inifrc_cesm()
        zero = g.crc("frzpot", 1, 1)
        assert g.crc("tflxap", 3, 1) == zero                       # blomgpu_crc
        l0, strips = g.crc_strips("sflxap", 48, 1)                  # blomgpu_crc_strips
        assert strips.shape[0] == case.jdm
        assert g.xcsum("tflxdi", 48) == 0.0                         # blomgpu_xcsum
        g.xctilr("sflxdi", 2, 1, 3, 2, 2, 1)                        # blomgpu_xctilr
        for nm in ("tflxap", "sflxap", "tflxdi", "sflxdi"):
            with pytest.raises(BlomGpuError, match="levels out of range"):
                g.crc(nm, 48, 2)
            assert not g.get(nm).any()
        _, _, h = lyr.dyncore_context("chan_s")
        try:
            h.set("expcnf", "cesm")
            h.inifrc_cesm()
            assert list(h.xcsum_batch("sflxdi", 47, 2)) == [0.0, 0.0]   # blomgpu_xcsum_batch
            plane = pattern((1, case.jdm + 8, case.idm + 8), 1)[0]
            h.put_level("tflxap", plane, 48)                        # blomgpu_upload_level
            a = h.get("tflxap")
            assert same_bytes(a[47], plane) and not a[:47].any()
            h.set("ditflx", 1)                                      # the option allocates its array
            assert not h.get("tflxdi").any()
            with pytest.raises(BlomGpuError, match="levels out of range"):
                h.put_level("swa_da", plane, 3)
            h.put_level("swa_da", plane, 2)
            a = h.get("swa_da")
            assert same_bytes(a[1], plane) and not a[0].any()
        finally:
            h.close()
    finally:
        g.close()


def test_named_entry_points_on_arrays_without_memory():
    check_unallocated_fields()


# ---- the interface ---------------------------------------------------------------------------------------------------------------------------
def check_interface():
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.full_context("chan_s_tke")
    _, _, h = lyr.full_context("chan_s_tke")
    try:
        six = hostinit.step_indices(0, case.kdm)
        # undeclared: the refusals of before, and nothing of the coupled experiment exists
        g.set("expcnf", "cesm")
        with pytest.raises(BlomGpuError, match="thermf: expcnf = cesm is not built on the device until blomgpu_inifrc_cesm has been called"):
            g.stage("thermf", *six)
        with pytest.raises(BlomGpuError, match="sfcstr: expcnf = cesm is not built on the device .* until blomgpu_inifrc_cesm has been called"):
            g.stage("sfcstr", *six)
        with pytest.raises(BlomGpuError):
            g.stage("getfrc_cesm", *six)
        for nm in ("swa_da", "frzpot", "tflxap", "ipwocn", "thermf_util"):
            assert not g.has_field(nm), nm
        assert "hmlt" not in g.field_names()
        with pytest.raises(BlomGpuError):
            g.get_real("sflxc")
        # declared with expcnf = 'channel': the channel path, byte for byte
        g.set("expcnf", "channel")
        g.inifrc_cesm()
        for nm in ("swa_da", "frzpot", "tflxap", "ipwocn", "thermf_util"):
            assert g.has_field(nm), nm
        assert g.get("swa_da").shape[0] == 2 and g.get("tflxdi").shape[0] == 48 and g.get("thermf_util").shape[0] == 1 + case.ntr
        assert g.step(0, 3) == 3 and h.step(0, 3) == 3
        bad = [nm for nm in STATE_FIELDS + ["surflx", "salflx", "ustar", "taux"] if h.has_field(nm) and not same_bytes(g.get(nm), h.get(nm))]
        assert not bad, bad
        assert not g.get("frzpot").any() and not g.get("swa_da").any()
        # declared, expcnf = 'cesm', use_graph = 1: refused
        g.set("expcnf", "cesm")
        g.set("use_graph", 1)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.step(3, 1)
        with pytest.raises(BlomGpuError, match="use_graph"):
            g.stage("thermf", *hostinit.step_indices(3, case.kdm))
        g.set("use_graph", 0)
        # inifrc_cesm again: l1ci = l2ci = 1 and idarlx's zeroing
        g.set("ditflx", 1)
        g.set("l1ci", 2)
        g.put("tflxdi", np.ones_like(g.get("tflxdi")))
        g.inifrc_cesm()
        assert not g.get("tflxdi").any() and not g.cesm_nflxdi().any()
        with pytest.raises(BlomGpuError, match="l1ci"):
            g.set("l1ci", 3), g.stage("getfrc_cesm", *six)
    finally:
        g.close()
        h.close()


def test_interface():
    check_interface()
