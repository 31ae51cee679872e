"""CROSS-CHECK (not a pin) fixtures for sfcstr_ben02 and thermf_ben02: the reference's own ben02/mod_thermf_ben02.F90,
ben02/mod_sfcstr_ben02.F90, ben02/mod_thdysi.F90, phy/mod_seaice.F90, phy/mod_intp1d.F90 and drivers/nocoupler/mod_swtfrz.F (with
phy/mod_types.F90, phy/mod_constants.F90, phy/mod_ifdefs.F90) compiled in place from the reference tree into a temporary directory,
against the stand-in modules and the driver beside this file (thermf_ben02_standins.F90, thermf_ben02_driver.F90: this project's own
text; the stand-ins declare only the names the routines use, with an xcsum in the reference's order and an xctilr for a grid that is
periodic in i and closed in j).  The routines are run on chan_s_tke's grid and tracer set with synthetic inputs, for the option sets of
tests/test_gpu_thermf_ben02.py under both vertical coordinates; inputs and outputs are written as tests/golden/thermf_ben02_*.npz --
data only.  The inputs reach every branch of thermf_ben02: the numpy restatement counts them here, and an input set that misses one is
refused.  tests/test_thermf_ben02_golden.py compares the restatement and the device with the fixtures.

usage: python tests/golden/make_thermf_ben02_golden.py --reference /path/to/reference [--fc amdflang]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, ".."))

CFG = "chan_s_tke"
BASE = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, trxlim=1.5, srxlim=0.5, xmi=0.3, sref=34.65, aptflx=0, apsflx=0, ditflx=0,
            disflx=0, srxbal=0, nstep=2, nstep_in_day=4, nday_of_year=1, nday_in_year=24)
OPTION_SETS = dict(clim={}, off=dict(trxday=0.0, srxday=0.0), ap=dict(aptflx=1, apsflx=1, nday_of_year=20), di=dict(ditflx=1, disflx=1),
                   srxbal=dict(srxbal=1))
RUNS = [(o, False) for o in OPTION_SETS] + [(o, True) for o in ("clim", "di")]
LMI = (11, 12, 1, 2, 3)
FILL = 7.25
NTDA0 = 3
OUT2D = ("ficem hicem hsnwm tsrfm ticem alb iagem rnfres tsi_tda tml_tda sml_tda alb_tda fice_tda rnf fmltfz sfl brnflx salflx hmltfz surflx "
         "sswflx surrlx salrlx util2 util3 salt_corr ustar taux tauy").split()
IN_ORDER = ("scp2 plat dp temp saln p trc difdia swfc2 swal2 "
            "swa nsf dfl lip sop eva rfi rnfins ustarw tsi albw ztx mty ustari tauxice tauyice "
            "ficem hicem hsnwm tsrfm iagem rnfres tsi_tda tml_tda sml_tda alb_tda fice_tda "
            "salt_corr trc_corr sstclm ricclm sssclm tflxap sflxap tflxdi sflxdi").split()


def inputs(seed=7):
    """a synthetic state on the case's grid and masks: every array the two routines read, whole padded planes"""
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    import thermf_ben02_ref as R
    case = make_case(CFG)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    assert nreg == 1, "the stand-in xctilr is periodic in i and closed in j"
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    rng = np.random.default_rng(seed)
    f = hostinit.ben02_forcing(case, seed=seed)
    a = {nm: f[nm] for nm in hostinit.BEN02_FLUXES + hostinit.BEN02_ICE + ["plat", "salt_corr", "trc_corr"]}
    y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / case.idm
    a["scp2"] = (1.0e8 * (1.0 + 0.1 * np.sin(x) * (0.5 + y)))[None]
    a["dp"] = R.ONEM * (0.5 + 30.0 * rng.random((2 * kk, nj, ni)) ** 2)
    a["temp"] = 8.0 + 7.0 * np.sin(x + 3.0 * y)[None] * np.ones((2 * kk, 1, 1)) - np.arange(2 * kk)[:, None, None] % kk + rng.standard_normal((2 * kk, nj, ni))
    a["saln"] = 35.0 + 0.8 * np.cos(2 * x + y)[None] * np.ones((2 * kk, 1, 1)) + 0.2 * rng.standard_normal((2 * kk, nj, ni))
    a["p"] = np.zeros((kk + 1, nj, ni))
    a["difdia"] = np.zeros((kk, nj, ni))
    a["swfc2"] = 0.33 + 0.05 * rng.random((1, nj, ni))
    a["swal2"] = 17.0 + 6.0 * rng.random((1, nj, ni))
    a["trc"] = np.zeros((2 * kk * ntr, nj, ni))
    for nt in range(ntr):
        for lev in (0, kk):
            a["trc"][nt * 2 * kk + lev] = 1.0e-4 * (1.0 + rng.random((nj, ni))) * (1 + nt)
    for nm in R.TDA:                                          # (accumulators that have accumulated)
        a[nm] = 10.0 * rng.random((1, nj, ni))
    # the five months / five of the 48 levels a run reads, the rest zero
    for nm in ("sstclm", "ricclm", "sssclm"):
        a[nm] = np.zeros((12, nj, ni))
        for l in LMI:
            a[nm][l - 1] = f[nm][l - 1]
    for nm in ("tflxap", "sflxap"):
        a[nm] = np.zeros((48, nj, ni))
        for l in (37, 38, 39, 40, 41):                        # (nday_of_year = 20 of 24: m3 = 39)
            a[nm][l - 1] = f[nm][l - 1]
    a["tflxdi"], a["sflxdi"] = np.zeros((48, nj, ni)), np.zeros((48, nj, ni))
    a["tflxdi"][1], a["sflxdi"][1] = 3.0 + rng.random((nj, ni)), 1.0e-6 * rng.random((nj, ni))
    # a third of the surface water below the freezing point (every ice class of ben02_forcing, both hemispheres; the odd rows by enough to take a
    # cover of 0.9949 past fice_max), and four prepared columns for the walks of the hybrid coordinate (level nn = kk: n = 2)
    sel = R.owned(dict(ip=ip, iu=iu, iv=iv), case.idm, case.jdm)["p"]
    cold = (np.arange(ni)[None, :] + np.arange(nj)[:, None]) % 3 == 0
    odd = cold & (np.arange(nj)[:, None] % 2 == 1)
    for lev in (0, kk):
        a["temp"][lev][cold] = -3.0
        a["temp"][lev][odd] = -13.0
    jj = 4 + case.jdm // 2
    cols = [i for i in range(4, 4 + case.idm) if sel[jj, i] and sel[jj + 1, i]]
    dp = a["dp"]
    dp[kk:, jj, cols[4]] = 50.0 * R.ONEM
    dp[kk:, jj, cols[7]] = 8.0 * R.ONEM
    dp[kk:2 * kk - 1, jj, cols[5]] = 0.5 * R.ONEM
    dp[2 * kk - 1, jj, cols[5]] = 100.0 * R.ONEM
    dp[kk:, jj, cols[6]] = 0.0
    dp[kk:kk + 5, jj, cols[6]] = [4096.0, 2048.0, 1024.0, 512.0, 512.0]
    a["ip"] = ip.reshape(1, nj, ni).astype(np.int32)
    a["iu"], a["iv"], a["iq"] = (m.reshape(1, nj, ni).astype(np.int32) for m in (iu, iv, iq))
    a["ipwocn"] = (f["ipwocn"].reshape(1, nj, ni) * (a["ip"] > 0)).astype(np.int32)
    a["area"] = np.array(R.xcsum(a["scp2"][0], a["ip"][0], case.idm, case.jdm))
    return case, a


def check_branches(case, a):
    """the restatement on the inputs: every branch of thermf_ben02 is taken, under both vertical coordinates"""
    import thermf_ben02_ref as R
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    p = case.params
    for hybrid in (False, True):
        s = {nm: np.array(v, copy=True) for nm, v in a.items() if nm != "area"}
        for nm, nlev in (("ticem", 1), ("alb", 1), ("rnf", 1), ("fmltfz", 1), ("sfl", 1), ("brnflx", 1), ("salflx", 1), ("hmltfz", 1), ("surflx", 1),
                         ("sswflx", 1), ("surrlx", 1), ("salrlx", 1), ("util2", 1), ("util3", 1), ("ustar", 1), ("trflx", ntr),
                         ("t_rs_nonloc", kk + 1), ("s_rs_nonloc", kk + 1)):
            s[nm] = np.full((nlev, nj, ni), FILL)
        o = dict(BASE, srxbal=1, lmi=LMI, area=float(a["area"]), baclin=float(p["baclin"]), hybrid=hybrid, itrtke=int(p["itrtke"]),
                 itrgls=int(p["itrgls"]), gls=0, nreg=case.nreg, kdm=kk, ntr=ntr)
        seen = {}
        R.thermf(s, o, (1, 2, 0, kk, 1, 1 + kk), {k: a[k][0] for k in ("ip", "iu", "iv")}, case.idm, case.jdm, seen)
        assert not R.missing(seen), ("the inputs miss branches of thermf_ben02", R.missing(seen), seen)
        assert seen["qp"] != 1.0 and seen["qn"] != 1.0, seen
        if hybrid:
            for key in ("t_exits", "s_exits"):
                e = seen[key]
                assert e[0] > 0 and e[1] > 0 and e[kk] > 0 and sum(e[k] for k in range(2, kk)) > 0, (key, e)
        print("hybrid" if hybrid else "isopycnic", "branches:", {k: v for k, v in seen.items() if not isinstance(v, dict)})


def compile_reference(ref, fc, tmp, case):
    flags = ["-O2", "-fdefault-real-8", "-cpp", "-ffp-contract=off", "-DTRC", "-DTKE", f"-DIDM={case.idm}", f"-DJDM={case.jdm}",
             f"-DKDM={case.kdm}", f"-DNTR={case.ntr}", "-w"]
    srcs = [os.path.join(ref, "phy", "mod_types.F90"), os.path.join(ref, "phy", "mod_constants.F90"), os.path.join(ref, "phy", "mod_ifdefs.F90"),
            os.path.join(HERE, "thermf_ben02_standins.F90"), os.path.join(ref, "phy", "mod_intp1d.F90"),
            os.path.join(ref, "drivers", "nocoupler", "mod_swtfrz.F"), os.path.join(ref, "ben02", "mod_thdysi.F90"),
            os.path.join(ref, "phy", "mod_seaice.F90"), os.path.join(ref, "ben02", "mod_sfcstr_ben02.F90"),
            os.path.join(ref, "ben02", "mod_thermf_ben02.F90"), os.path.join(HERE, "thermf_ben02_driver.F90")]
    objs = []
    for k, s in enumerate(srcs):
        o = os.path.join(tmp, f"o{k}.o")
        subprocess.check_call([fc] + flags + ["-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    exe = os.path.join(tmp, "thermf_ben02_driver")
    subprocess.check_call([fc, "-o", exe] + objs, cwd=tmp)
    return exe


def run(exe, tmp, case, a, o, hybrid):
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    m, n = 1, 2
    idx = (m, n, (m - 1) * kk, (n - 1) * kk, 1 + (m - 1) * kk, 1 + (n - 1) * kk)
    p = case.params
    with open(os.path.join(tmp, "scalars.txt"), "w") as f:
        f.write(" ".join(str(v) for v in idx) + "\n")
        f.write(" ".join(str(int(v)) for v in (o["nstep"], o["nstep_in_day"], o["nday_in_year"], o["nday_of_year"]) + LMI) + "\n")
        f.write(" ".join(repr(float(v)) for v in (p["baclin"], o["xmi"], o["sref"], float(a["area"]), o["trxday"], o["srxday"], o["trxdpt"],
                                                  o["srxdpt"], o["trxlim"], o["srxlim"])) + "\n")
        f.write(" ".join(str(int(v)) for v in (o["aptflx"], o["apsflx"], o["ditflx"], o["disflx"], o["srxbal"], 2 if hybrid else 1, p["itrtke"],
                                               p["itrgls"], NTDA0)) + "\n")
    nflxdi = np.zeros(48, np.int32)
    nflxdi[1] = 5
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        for arr in (a["ip"], a["iu"], a["iv"], a["ipwocn"], nflxdi):
            f.write(np.ascontiguousarray(arr, np.int32).tobytes())
        for nm in IN_ORDER:
            f.write(np.ascontiguousarray(a[nm], np.float64).tobytes())
        f.write(np.full((nj, ni), FILL).tobytes())
    subprocess.check_call([exe], cwd=tmp)
    raw = open(os.path.join(tmp, "out.bin"), "rb").read()
    pos, out = 0, {}

    def take(nlev):
        nonlocal pos
        v = np.frombuffer(raw, np.float64, nlev * nj * ni, pos).reshape(nlev, nj, ni).copy()
        pos += v.nbytes
        return v
    for nm in OUT2D:
        out[nm] = take(1)
    out["trflx"], out["trc_corr"] = take(ntr), take(ntr)
    out["t_rs_nonloc"], out["s_rs_nonloc"] = take(kk + 1), take(kk + 1)
    tdi, sdi = take(48), take(48)
    tail = np.frombuffer(raw, np.int32, 49, pos).copy()
    assert pos + tail.nbytes == len(raw)
    out["nflxdi"], out["ntda"] = tail[:48], tail[48:]
    if o["ditflx"]:
        out["tflxdi"], out["sflxdi"] = tdi[:3], sdi[:3]        # (levels 1..3: ntld = 2, its neighbours untouched)
    if not hybrid:
        del out["t_rs_nonloc"], out["s_rs_nonloc"]
    return idx, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--fc", default="amdflang")
    a_ = ap.parse_args()
    case, a = inputs()
    check_branches(case, a)
    np.savez_compressed(os.path.join(HERE, "thermf_ben02_inputs.npz"), **a)
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_reference(a_.reference, a_.fc, tmp, case)
        for optname, hybrid in RUNS:
            o = dict(BASE, **OPTION_SETS[optname])
            idx, out = run(exe, tmp, case, a, o, hybrid)
            meta = dict(options=o, hybrid=hybrid, idx=idx, lmi=LMI, fill=FILL, cfg=CFG, ntda0=NTDA0)
            np.savez_compressed(os.path.join(HERE, f"thermf_ben02_{optname}_{'hyb' if hybrid else 'iso'}.npz"), meta=np.array(json.dumps(meta)), **out)
            print(optname, "hybrid" if hybrid else "isopycnic", {k: v.shape for k, v in out.items() if k in ("surflx", "trflx", "hicem")})


if __name__ == "__main__":
    main()
