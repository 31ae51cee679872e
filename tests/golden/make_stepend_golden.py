"""CROSS-CHECK (not a pin) fixtures for iniswa / updswa, fwbbal and chkvar: the reference's own phy/mod_swabs.F90, phy/mod_forcing.F90,
phy/mod_chkvar.F90 and phy/mod_intp1d.F90 (with phy/mod_types.F90, phy/mod_constants.F90, phy/mod_ifdefs.F90) compiled in place from the
reference tree into a temporary directory, against the stand-in modules and the driver beside this file (stepend_standins.F90,
stepend_driver.F90: this project's own text).  Among the stand-ins is a netcdf module whose nf90_get_var hands iniswa the driver's
synthetic chlorophyll, so that the real iniswa fills its private chl10c and tables and the real updswa runs unchanged.  phy/mod_time.F90
is NOT compiled: its step_time moves a date of mod_calendar that init_timevars sets from a namelist file, so the clock keeps its
restatement (tests/stepend_ref.py: step_time) and the stand-in mod_time holds the scalars.

The routines run on chan_s_tke's grid; inputs and outputs are written as tests/golden/stepend_*.npz -- data only: both chlorophyll
methods at three (l?mi, xmi) settings, jerlov and top-layer, fwbbal over a run of steps that contains one year's end with an ipwocn that
excludes some wet points, and the line chkvar prints for a few planted values.  tests/test_stepend_golden.py compares the restatement
and the device with the fixtures.

usage: python tests/golden/make_stepend_golden.py --reference /path/to/reference [--fc amdflang]"""
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
FILL = 7.25
TIMES = (((11, 12, 1, 2, 3), 0.3), ((4, 5, 6, 7, 8), 0.75), ((10, 11, 12, 1, 2), 0.0))
SWABS = (("chlorophyll_ma94", 1), ("chlorophyll_ohl03", 1), ("jerlov", 3), ("top-layer", 1))
FWB_STEPS = ((24, 1), (24, 2), (24, 3), (1, 5), (1, 4), (1, 5), (1, 6))
NSTEP_IN_DAY = 4
NAN, INF = float("nan"), float("inf")
# (field, value, level k, (row, column) as 1-based interior indices); the last two hold two hits each
CHKVAR = ([("dp", NAN, 2, (5, 7))], [("temp", INF, 1, (9, 3))], [("saln", NAN, 3, (2, 11))], [("saln", -INF, 1, (6, 6))],
          [("saln", INF, 3, (4, 12)), ("dp", NAN, 1, (8, 2))], [("temp", INF, 2, (8, 9)), ("saln", NAN, 2, (8, 4)), ("dp", INF, 2, (8, 9))], [])


def grid():
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    case = make_case(CFG)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    assert nreg == 1, "the stand-in xctilr is periodic in i and closed in j"
    nj, ni = case.jdm + 8, case.idm + 8
    return case, ip.reshape(nj, ni).astype(np.int32)


def compile_reference(ref, fc, tmp, case):
    flags = ["-O2", "-fdefault-real-8", "-cpp", "-ffp-contract=off", "-DTRC", "-DTKE", f"-DIDM={case.idm}", f"-DJDM={case.jdm}",
             f"-DKDM={case.kdm}", f"-DNTR={case.ntr}", "-w"]
    srcs = [os.path.join(ref, "phy", "mod_types.F90"), os.path.join(ref, "phy", "mod_constants.F90"), os.path.join(ref, "phy", "mod_ifdefs.F90"),
            os.path.join(HERE, "stepend_standins.F90"), os.path.join(ref, "phy", "mod_intp1d.F90"), os.path.join(ref, "phy", "mod_swabs.F90"),
            os.path.join(ref, "phy", "mod_forcing.F90"), os.path.join(ref, "phy", "mod_chkvar.F90"), os.path.join(HERE, "stepend_driver.F90")]
    objs = []
    for k, s in enumerate(srcs):
        o = os.path.join(tmp, f"o{k}.o")
        subprocess.check_call([fc] + flags + ["-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    # which libm entries the reference's compiler calls for 10._r8**x and log10 in mod_swabs: the library's host code calls the same
    syms = subprocess.run(["nm", "-u", objs[5]], capture_output=True, text=True).stdout.split()
    print("mod_swabs.o calls:", sorted(s for s in syms if s in ("pow", "log10", "exp10", "exp", "log", "__exp10", "__log10_finite", "__pow_finite")))
    exe = os.path.join(tmp, "stepend_driver")
    subprocess.check_call([fc, "-o", exe] + objs, cwd=tmp)
    return exe


def drive(exe, tmp, control, arrays, check=True):
    with open(os.path.join(tmp, "control.txt"), "w") as f:
        f.write("\n".join(control) + "\n")
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe], cwd=tmp, capture_output=True, text=True)
    if check:
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return open(os.path.join(tmp, "out.bin"), "rb").read(), r.stdout


def main():
    import stepend_ref as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--fc", default="amdflang")
    a_ = ap.parse_args()
    case, ip = grid()
    nj, ni, kk = case.jdm + 8, case.idm + 8, case.kdm
    chl = R.synthetic_chl(nj, ni)
    with tempfile.TemporaryDirectory() as tmp:
        exe = compile_reference(a_.reference, a_.fc, tmp, case)
        # ---- iniswa / updswa
        out = dict(ip=ip[None], chl=chl)
        for method, jwtype in SWABS:
            control = ["1", method, f"{jwtype} {FILL!r} {len(TIMES)}"] + [" ".join(str(v) for v in lmi) + f" {xmi!r}" for lmi, xmi in TIMES]
            raw, _ = drive(exe, tmp, control, [ip, np.ascontiguousarray(chl[:, 4:-4, 4:-4])])
            v = np.frombuffer(raw, np.float64).reshape(1 + len(TIMES), 4, nj, ni)
            out[method.replace("-", "_")] = v.copy()
        meta = dict(cfg=CFG, fill=FILL, times=TIMES, swabs=SWABS, swamxd=200.0)
        np.savez_compressed(os.path.join(HERE, "stepend_swabs.npz"), meta=np.array(json.dumps(meta)), **out)
        print("swabs:", {k: v.shape for k, v in out.items()})
        # ---- fwbbal
        rng = np.random.default_rng(11)
        y, x = np.arange(nj)[:, None] / nj, 2 * np.pi * (np.arange(ni)[None, :] - 4) / case.idm
        f = dict(scp2=1.0e8 * (1.0 + 0.1 * np.sin(x) * (0.5 + y)), eva=-2e-5 * (1.0 + 0.5 * np.sin(2 * x)) + 0.0 * y,
                 fmltfz=1.5e-5 * np.cos(7.0 * y) * (1.0 + 0.2 * np.cos(x)), lip=3e-5 * (y > 0.5) * (1.0 + 0.1 * np.sin(x)),
                 sop=1e-5 * (y < 0.6) * (1.0 + np.sin(x)), rnf=2e-6 * (1.0 + np.cos(3 * x)) + 0.0 * y, rfi=1e-6 * (1.0 + np.sin(2 * x) * y),
                 eiacc=1.0e-3 * rng.random((nj, ni)), pracc=1.0e-3 * rng.random((nj, ni)))
        ipwocn = ip.copy()
        ipwocn[nj // 3:nj // 2, ni // 4:ni // 2] = 0
        order = "scp2 eva fmltfz lip sop rnf rfi eiacc pracc".split()
        baclin = float(case.params["baclin"])
        control = ["2", f"{NSTEP_IN_DAY} {baclin!r} {len(FWB_STEPS)}"] + [f"{d} {n}" for d, n in FWB_STEPS]
        raw, _ = drive(exe, tmp, control, [ip, ipwocn] + [f[nm] for nm in order])
        rec = np.frombuffer(raw, np.float64).reshape(len(FWB_STEPS), 2 * nj * ni + 1)
        steps = dict(eiacc=rec[:, :nj * ni].reshape(-1, nj, ni).copy(), pracc=rec[:, nj * ni:2 * nj * ni].reshape(-1, nj, ni).copy(),
                     prfac=rec[:, -1].copy())
        meta = dict(cfg=CFG, steps=FWB_STEPS, nstep_in_day=NSTEP_IN_DAY, baclin=baclin)
        np.savez_compressed(os.path.join(HERE, "stepend_fwbbal.npz"), meta=np.array(json.dumps(meta)), ip=ip[None], ipwocn=ipwocn[None],
                            **{"in_" + nm: f[nm][None] for nm in order}, **{"out_" + nm: v for nm, v in steps.items()})
        print("fwbbal: prfac", steps["prfac"])
        # ---- chkvar: the line the reference prints before it stops
        lines = []
        for q, plants in enumerate(CHKVAR):
            s = {nm: np.ones((2 * kk, nj, ni)) for nm in ("dp", "temp", "saln")}
            n = 2 - q % 2
            for nm, v, k, (j, i) in plants:
                s[nm][(n - 1) * kk + k - 1, 3 + j, 3 + i] = v
            _, text = drive(exe, tmp, ["3", str(n)], [ip, s["dp"], s["temp"], s["saln"]], check=False)
            line = [ln for ln in text.splitlines() if "chkvar:" in ln]
            assert len(line) == 1, text
            lines.append(dict(plants=[[nm, repr(v), k, [j, i]] for nm, v, k, (j, i) in plants], n=n, line=line[0]))
            print(lines[-1]["line"])
        np.savez_compressed(os.path.join(HERE, "stepend_chkvar.npz"), meta=np.array(json.dumps(dict(cfg=CFG, cases=lines))), ip=ip[None])


if __name__ == "__main__":
    main()
