"""CROSS-CHECK (not a pin) of thermf_cesm against the reference's REAL cesm/mod_thermf_cesm.F90: tests/golden/thermf_cesm_*.npz hold what
the module, compiled behind the stand-ins of tests/golden/thermf_cesm_standins.F90 (tests/golden/make_thermf_cesm_golden.py), computes
from synthetic inputs on chan_s_tke's grid, for the option sets relaxation from the climatologies / from the streams / off, aptflx +
apsflx, ditflx + disflx, srxbal, and under the hybrid coordinate.  The numpy restatement (tests/thermf_cesm_ref.py) is compared with
them on the CPU, the device's thermf stage on the GPU; both == on the bytes, over the whole padded arrays."""
import glob
import json
import os

import numpy as np
import pytest

import thermf_cesm_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(os.path.basename(f)[len("thermf_cesm_"):-4] for f in glob.glob(os.path.join(HERE, "golden", "thermf_cesm_*_*.npz")))
STATE_IN = ("scp2 dp temp saln p trc difdia swa nsf hmlt lip sop eva rnf rfi fmltfz sfl ustarw sst_stream sss_stream ice_stream salt_corr trc_corr "
            "sstclm ricclm sssclm tflxap sflxap tflxdi sflxdi ipwocn").split()
PRESET = "surflx sswflx surrlx salflx brnflx salrlx hmltfz ustar frzpot mltpot util2 util3 trflx t_rs_nonloc s_rs_nonloc".split()


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def load(name):
    inp = dict(np.load(os.path.join(HERE, "golden", "thermf_cesm_inputs.npz")))
    out = dict(np.load(os.path.join(HERE, "golden", f"thermf_cesm_{name}.npz")))
    meta = json.loads(str(out.pop("meta")))
    return inp, out, meta


def nlevels(nm, kk, ntr):
    return dict(trflx=ntr, t_rs_nonloc=kk + 1, s_rs_nonloc=kk + 1).get(nm, 1)


def test_the_fixtures_are_there():
    assert len(FIXTURES) == 9 and "clim_hyb" in FIXTURES and "srxbal_iso" in FIXTURES, FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_real_module(name):
    from blom_amd.cases import make_case
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
    seen = {}
    R.thermf(s, o, tuple(meta["idx"]), masks, case.idm, case.jdm, seen)
    bad = [nm for nm in want if nm != "nflxdi" and not same_bytes(s[nm], want[nm])]
    assert not bad, f"{name}: {bad} differ from the reference's compiled thermf_cesm"
    assert seen["frzpot_pos"] > 0 and seen["brnflx_clipped"] > 0 and seen["brnflx_pos"] > 0
    if meta["hybrid"]:
        e = seen["t_exits"]
        assert e[0] > 0 and e[1] > 0 and e[kk] > 0 and sum(e[k] for k in range(2, kk)) > 0, e
    if meta["options"]["ditflx"]:
        assert list(want["nflxdi"][:3]) == [0, 6, 0]          # (the generator starts level 2 at 5; nstep = 2 of 4 a day: ntld = 2)
        assert not same_bytes(want["tflxdi"][1], inp["tflxdi"][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_the_real_module(name):
    check_device(name)


def check_device(name):
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu
    from blom_amd import hostinit
    inp, want, meta = load(name)
    case = make_case(meta["cfg"])
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    g = BlomGpu(case.idm, case.jdm, kk, ntr, case.nreg, {k: inp[k][0] for k in ("ip", "iu", "iv", "iq")})
    try:
        for nm, v in case.params.items():
            if not nm.endswith("0"):
                g.set(nm, v)
        o = meta["options"]
        g.set("expcnf", "cesm")
        g.set("ditflx", int(o["ditflx"]))
        g.set("disflx", int(o["disflx"]))
        g.inifrc_cesm()
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
        g.stage("thermf", *meta["idx"])
        bad = [nm for nm in want if nm != "nflxdi" and not same_bytes(g.get(nm)[:want[nm].shape[0]], want[nm])]
        assert not bad, f"{name}: {bad} differ from the reference's compiled thermf_cesm"
        if o["ditflx"]:
            assert list(g.cesm_nflxdi()[:3]) == [0, 1, 0]      # (the device's count starts at inifrc_cesm's zero)
    finally:
        g.close()
