"""CROSS-CHECK (not a pin) fixtures for thermf_cesm: the reference's own cesm/mod_thermf_cesm.F90, phy/mod_intp1d.F90 and
drivers/nocoupler/mod_swtfrz.F (with phy/mod_types.F90, phy/mod_constants.F90, phy/mod_ifdefs.F90) compiled in place from the reference
tree into a temporary directory, against the stand-in modules and the driver beside this file (thermf_cesm_standins.F90,
thermf_cesm_driver.F90: this project's own text; the stand-ins declare only the names the routine uses, with an xcsum in the
reference's order).  The routine is run on chan_s_tke's grid and tracer set with synthetic inputs, for the option sets of
tests/test_gpu_thermf_cesm.py under both vertical coordinates; inputs and outputs are written as tests/golden/thermf_cesm_*.npz --
data only.  tests/test_thermf_cesm_golden.py compares the numpy restatement and the device with them.

usage: python tests/golden/make_thermf_cesm_golden.py --reference /path/to/reference [--fc amdflang]"""
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
BASE = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, trxlim=1.5, srxlim=0.5, xmi=0.3, sref=34.65, use_stream_relaxation=0,
            aptflx=0, apsflx=0, ditflx=0, disflx=0, srxbal=0, nstep=2, nstep_in_day=4, nday_of_year=1, nday_in_year=24)
OPTION_SETS = dict(clim={}, stream=dict(use_stream_relaxation=1), off=dict(trxday=0.0, srxday=0.0), ap=dict(aptflx=1, apsflx=1, nday_of_year=20),
                   di=dict(ditflx=1, disflx=1), srxbal=dict(srxbal=1))
RUNS = [(o, False) for o in OPTION_SETS] + [(o, True) for o in ("clim", "stream", "di")]
LMI = (11, 12, 1, 2, 3)
FILL = 7.25
OUT2D = "surflx sswflx surrlx salflx brnflx salrlx hmltfz ustar frzpot mltpot util2 util3 salt_corr".split()
IN_ORDER = ("scp2 dp temp saln p trc difdia swa nsf hmlt lip sop eva rnf rfi fmltfz sfl ustarw sst_stream sss_stream ice_stream salt_corr "
            "trc_corr sstclm ricclm sssclm tflxap sflxap tflxdi sflxdi").split()


def inputs(seed=7):
    """a synthetic state on the case's grid and masks: every array thermf_cesm reads, whole padded planes"""
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    import thermf_cesm_ref as R
    case = make_case(CFG)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    kk, ntr, nj, ni = case.kdm, case.ntr, case.jdm + 8, case.idm + 8
    rng = np.random.default_rng(seed)
    f = hostinit.cesm_forcing(case, seed=seed)
    a = {nm: f[nm + "_da"][0:1].copy() for nm in "swa nsf hmlt lip sop eva rnf rfi fmltfz sfl ustarw".split()}
    for nm in "sst_stream sss_stream ice_stream salt_corr trc_corr".split():
        a[nm] = f[nm]
    y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / case.idm
    a["scp2"] = (1.0e8 * (1.0 + 0.1 * np.sin(x) * (0.5 + y)))[None]
    a["dp"] = R.ONEM * (0.5 + 30.0 * rng.random((2 * kk, nj, ni)) ** 2)
    a["temp"] = 12.0 + 9.0 * np.sin(x + 3.0 * y)[None] * np.ones((2 * kk, 1, 1)) - np.arange(2 * kk)[:, None, None] % kk + rng.standard_normal((2 * kk, nj, ni))
    a["saln"] = 35.0 + 0.8 * np.cos(2 * x + y)[None] * np.ones((2 * kk, 1, 1)) + 0.2 * rng.standard_normal((2 * kk, nj, ni))
    a["p"] = np.zeros((kk + 1, nj, ni))
    a["difdia"] = np.zeros((kk, nj, ni))
    a["trc"] = np.zeros((2 * kk * ntr, nj, ni))
    for nt in range(ntr):
        for lev in (0, kk):
            a["trc"][nt * 2 * kk + lev] = 1.0e-4 * (1.0 + rng.random((nj, ni))) * (1 + nt)
    # the five months / five of the 48 levels a run reads, the rest zero
    for nm in ("sstclm", "ricclm", "sssclm"):
        a[nm] = np.zeros((12, nj, ni))
        for l in LMI:
            a[nm][l - 1] = f[nm][l - 1]
    for nm in ("tflxap", "sflxap"):
        a[nm] = np.zeros((48, nj, ni))
        for l in (37, 38, 39, 40, 41, 47, 48, 1, 2, 3):
            a[nm][l - 1] = f[nm][l - 1]
    a["tflxdi"], a["sflxdi"] = np.zeros((48, nj, ni)), np.zeros((48, nj, ni))
    a["tflxdi"][1], a["sflxdi"][1] = 3.0 + rng.random((nj, ni)), 1.0e-6 * rng.random((nj, ni))
    # a patch below the freezing point, and four prepared columns for the walks of the hybrid coordinate (level nn = kk: n = 2)
    sel = R.owned(dict(ip=ip, iu=iu, iv=iv), case.idm, case.jdm)["p"]
    jj = 4 + case.jdm // 2
    cols = [i for i in range(4, 4 + case.idm) if sel[jj, i] and sel[jj + 1, i]]
    a["temp"][[0, kk], jj + 1, cols[0]:cols[3]] = -3.0
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


def compile_reference(ref, fc, tmp, case):
    flags = ["-O2", "-fdefault-real-8", "-cpp", "-ffp-contract=off", "-DTRC", "-DTKE", f"-DIDM={case.idm}", f"-DJDM={case.jdm}",
             f"-DKDM={case.kdm}", f"-DNTR={case.ntr}", "-w"]
    srcs = [os.path.join(ref, "phy", "mod_types.F90"), os.path.join(ref, "phy", "mod_constants.F90"), os.path.join(ref, "phy", "mod_ifdefs.F90"),
            os.path.join(HERE, "thermf_cesm_standins.F90"), os.path.join(ref, "phy", "mod_intp1d.F90"),
            os.path.join(ref, "drivers", "nocoupler", "mod_swtfrz.F"), os.path.join(ref, "cesm", "mod_thermf_cesm.F90"),
            os.path.join(HERE, "thermf_cesm_driver.F90")]
    objs = []
    for k, s in enumerate(srcs):
        o = os.path.join(tmp, f"o{k}.o")
        subprocess.check_call([fc] + flags + ["-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    exe = os.path.join(tmp, "thermf_cesm_driver")
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
        f.write(" ".join(str(int(v)) for v in (o["aptflx"], o["apsflx"], o["ditflx"], o["disflx"], o["srxbal"], o["use_stream_relaxation"],
                                               2 if hybrid else 1, p["itrtke"], p["itrgls"])) + "\n")
    nflxdi = np.zeros(48, np.int32)
    nflxdi[1] = 5
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        for arr in (a["ip"], a["ipwocn"], nflxdi):
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
    out["nflxdi"] = np.frombuffer(raw, np.int32, 48, pos).copy()
    if o["ditflx"]:
        out["tflxdi"], out["sflxdi"] = tdi, sdi
    if not hybrid:
        del out["t_rs_nonloc"], out["s_rs_nonloc"]
    return idx, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--fc", default="amdflang")
    a_ = ap.parse_args()
    case, a = inputs()
    np.savez_compressed(os.path.join(HERE, "thermf_cesm_inputs.npz"), **a)
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_reference(a_.reference, a_.fc, tmp, case)
        for optname, hybrid in RUNS:
            o = dict(BASE, **OPTION_SETS[optname])
            idx, out = run(exe, tmp, case, a, o, hybrid)
            meta = dict(options=o, hybrid=hybrid, idx=idx, lmi=LMI, fill=FILL, cfg=CFG)
            np.savez_compressed(os.path.join(HERE, f"thermf_cesm_{optname}_{'hyb' if hybrid else 'iso'}.npz"), meta=np.array(json.dumps(meta)), **out)
            print(optname, "hybrid" if hybrid else "isopycnic", {k: v.shape for k, v in out.items() if k in ("surflx", "trflx")})


if __name__ == "__main__":
    main()
