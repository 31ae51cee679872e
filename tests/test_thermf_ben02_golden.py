"""CROSS-CHECK (not a pin) of sfcstr_ben02 and thermf_ben02 against the reference's REAL ben02/mod_sfcstr_ben02.F90 and
ben02/mod_thermf_ben02.F90 (with its mod_thdysi and mod_seaice): tests/golden/thermf_ben02_*.npz hold what the modules, compiled behind
the stand-ins of tests/golden/thermf_ben02_standins.F90 (tests/golden/make_thermf_ben02_golden.py), compute from synthetic inputs on
chan_s_tke's grid, for the option sets relaxation from the climatology / off, aptflx + apsflx, ditflx + disflx, srxbal, and under the
hybrid coordinate.  The numpy restatement (tests/thermf_ben02_ref.py) is compared with them on the CPU, the device's sfcstr and thermf
stages on the GPU; both == on the bytes, over the whole padded arrays.  The inputs reach every branch of the routine (asserted)."""
import glob
import json
import os

import numpy as np
import pytest

import thermf_ben02_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(os.path.basename(f)[len("thermf_ben02_"):-4] for f in glob.glob(os.path.join(HERE, "golden", "thermf_ben02_*_*.npz")))
STATE_IN = ("scp2 plat dp temp saln p trc difdia swfc2 swal2 swa nsf dfl lip sop eva rfi rnfins ustarw tsi albw ztx mty ustari tauxice tauyice "
            "ficem hicem hsnwm tsrfm iagem rnfres tsi_tda tml_tda sml_tda alb_tda fice_tda salt_corr trc_corr sstclm ricclm sssclm tflxap sflxap "
            "tflxdi sflxdi ipwocn").split()
PRESET = ("ticem alb rnf fmltfz sfl brnflx salflx hmltfz surflx sswflx surrlx salrlx util2 util3 ustar taux tauy trflx t_rs_nonloc "
          "s_rs_nonloc").split()
NOT_FIELDS = ("nflxdi", "ntda")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def load(name):
    inp = dict(np.load(os.path.join(HERE, "golden", "thermf_ben02_inputs.npz")))
    out = dict(np.load(os.path.join(HERE, "golden", f"thermf_ben02_{name}.npz")))
    meta = json.loads(str(out.pop("meta")))
    return inp, out, meta


def nlevels(nm, kk, ntr):
    return dict(trflx=ntr, t_rs_nonloc=kk + 1, s_rs_nonloc=kk + 1).get(nm, 1)


def test_the_fixtures_are_there():
    assert FIXTURES == ["ap_iso", "clim_hyb", "clim_iso", "di_hyb", "di_iso", "off_iso", "srxbal_iso"], FIXTURES
    for f in glob.glob(os.path.join(HERE, "golden", "thermf_ben02_*.npz")):
        assert os.path.getsize(f) < 700 * 1024, f


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_real_modules(name):
    from blom_amd.cases import make_case
    from blom_amd import hostinit
    inp, want, meta = load(name)
    case = make_case(meta["cfg"])
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    s = {nm: inp[nm].copy() for nm in STATE_IN}
    for nm in PRESET:
        s[nm] = np.full((nlevels(nm, kk, ntr), nj, ni), meta["fill"])
    masks = {k: inp[k][0] for k in ("ip", "iu", "iv")}
    p = case.params
    o = dict(meta["options"], lmi=meta["lmi"], area=float(inp["area"]), baclin=float(p["baclin"]), hybrid=meta["hybrid"], itrtke=int(p["itrtke"]),
             itrgls=int(p["itrgls"]), gls=0, nreg=case.nreg, kdm=kk, ntr=ntr)

    def halo(a):
        b = np.array(a, dtype=np.float64)[None].copy()
        hostinit.xctilr_np(b, 1, 1, 1, 1, case.nreg, case.idm, case.jdm, 0.0, 1)
        return b[0]
    seen = {}
    R.sfcstr(s, masks, case.idm, case.jdm, case.nreg, halo=halo)
    R.thermf(s, o, tuple(meta["idx"]), masks, case.idm, case.jdm, seen)
    bad = [nm for nm in want if nm not in NOT_FIELDS and not same_bytes(s[nm][:want[nm].shape[0]], want[nm])]
    assert not bad, f"{name}: {bad} differ from the reference's compiled sfcstr_ben02 / thermf_ben02"
    relax = meta["options"]["trxday"] > 0.0
    assert not R.missing(seen, relax=relax), (R.missing(seen, relax=relax), seen)
    assert int(want["ntda"][0]) == meta["ntda0"] + 1
    assert not same_bytes(want["hicem"], inp["hicem"]) and not same_bytes(want["taux"], inp["ztx"])
    if meta["hybrid"]:
        e = seen["t_exits"]
        assert e[0] > 0 and e[1] > 0 and e[kk] > 0 and sum(e[k] for k in range(2, kk)) > 0, e
    if meta["options"]["ditflx"]:
        assert list(want["nflxdi"][:3]) == [0, 6, 0]          # (the generator starts level 2 at 5; nstep = 2 of 4 a day: ntld = 2)
        assert not same_bytes(want["tflxdi"][1], inp["tflxdi"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_real_modules(name):
    check_device(name)


def check_device(name):
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu
    inp, want, meta = load(name)
    case = make_case(meta["cfg"])
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    g = BlomGpu(case.idm, case.jdm, kk, ntr, case.nreg, {k: inp[k][0] for k in ("ip", "iu", "iv", "iq")})
    try:
        for nm, v in case.params.items():
            if not nm.endswith("0"):
                g.set(nm, v)
        o = meta["options"]
        g.set("expcnf", "ben02clim")
        g.set("ditflx", int(o["ditflx"]))
        g.set("disflx", int(o["disflx"]))
        g.inifrc_ben02()
        for nm in STATE_IN:
            if nm in ("tflxdi", "sflxdi") and not o["ditflx"]:
                continue
            g.put(nm, inp[nm])
        for nm in PRESET:
            g.put(nm, np.full((nlevels(nm, kk, ntr), nj, ni), meta["fill"]))
        for nm, v in o.items():
            g.set(nm, v)
        for k, v in enumerate(meta["lmi"]):
            g.set("l%dmi" % (k + 1), int(v))
        g.set("area", float(inp["area"]))
        if meta["hybrid"]:
            g.set("vcoord_type", "cntiso_hybrid")
        g.stage("sfcstr", *meta["idx"])
        g.stage("thermf", *meta["idx"])
        bad = [nm for nm in want if nm not in NOT_FIELDS and not same_bytes(g.get(nm)[:want[nm].shape[0]], want[nm])]
        assert not bad, f"{name}: {bad} differ from the reference's compiled sfcstr_ben02 / thermf_ben02"
        assert g.ben02_ntda() == 1                              # (the device's count starts at the declaration's zero)
        if o["ditflx"]:
            assert list(g.cesm_nflxdi()[:3]) == [0, 1, 0]
    finally:
        g.close()
