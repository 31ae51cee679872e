"""What the end of blom_step costs on the device (blom_amd/csrc/stage_stepend.hip: updswa, fwbbal, chkvar and the clock of step_time;
bench.py's workload with swamth = 'chlorophyll_ma94' | 'chlorophyll_ohl03', sprfac, chkvar and step_time declared):

 1. each new launch's timer (HIP events around it, option "timing") over --steps steps after --warmup, beside the bytes it moves and
    the rate that makes;
 2. the step with updswa, fwbbal and chkvar declared against the step without, stepped alternately on the same frozen clock (wall clock
    around blomgpu_step + sync, three rounds).

Bytes, in planes of idm x jdm doubles:
  updswa   5 in (the five months of chl10c the interpolation reads; the mask rides along as an int plane), 5 out (chl10 and the four bands)
  fwbbal   8 in (eiacc pracc eva fmltfz lip sop rnf rfi), 2 out -- the accumulation; a year's end adds a pass over both planes, two masked
           sums and a zeroing, once a year
  chkvar   3 kk in (dp temp saln of time level n), nothing out

usage (GPU box): python3 tools/gpu_stepend_cost.py [--config channel] [--swamth chlorophyll_ma94] [--out profiles/stepend_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

CLOCK = dict(nstep_in_day=96, nday_of_year=40, nday_in_year=365)


def chlorophyll(case):
    nj, ni = case.jdm + 8, case.idm + 8
    x = np.linspace(0.0, 2.0 * np.pi, ni)[None, :]
    y = np.linspace(0.0, np.pi, nj)[:, None]
    return np.stack([10.0 ** (-0.4 + 1.8 * np.sin(x + 0.5 * k) * np.cos(y + 0.25 * k)) for k in range(12)])


def device(case, nreg, masks, declared, swamth, clock=True):
    g = bench.device_for_bench(case, nreg, masks)
    for nm, v in CLOCK.items():
        g.set(nm, v)
    if declared:
        g.set("swamth", swamth)
        g.iniswa(chlorophyll(case) if swamth.startswith("chlorophyll") else None)
        g.set("sprfac", 1)
        g.put("ipwocn", np.asarray(masks["ip"]).reshape(1, case.jdm + 8, case.idm + 8).astype(np.int32))
        g.set("chkvar", 1)
        g.set("step_time", int(clock))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="channel")
    ap.add_argument("--swamth", default="chlorophyll_ma94")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    case, nreg, masks = bench.build_case(a.config)
    plane = case.idm * case.jdm * 8
    planes = dict(updswa=10, fwbbal=10, chkvar=3 * case.kdm)
    res = dict(config=a.config, swamth=a.swamth, idm=case.idm, jdm=case.jdm, kdm=case.kdm, steps=a.steps, warmup=a.warmup, plane_bytes=plane,
               stages={})
    g = device(case, nreg, masks, True, a.swamth)
    ns = g.step(0, a.warmup)
    g.set("timing", 1)
    g.timer_reset()
    ns = g.step(ns, a.steps)
    g.sync()
    for lb in ("updswa", "fwbbal", "chkvar"):
        ms, n = g.timer_get(lb)
        byt = planes[lb] * plane
        row = dict(ms=ms / max(n, 1), launches=n, bytes=byt, TBps=byt / (ms / max(n, 1) * 1e-3) / 1e12 if ms > 0 else 0.0)
        res["stages"][lb] = row
        print(f"{lb:8s}: {row['ms']:8.4f} ms x {n}, {byt / 1e6:9.2f} MB, {row['TBps']:6.3f} TB/s")
    res["prfac"], res["xmi"] = g.get_real("prfac"), g.get_real("xmi")
    g.close()
    # (the clock stays off in this pair: a moving xmi changes thermf's relaxation and with it the state every other stage works on, and
    # the two contexts would not run the same workload; step_time itself is a few host instructions a step)
    with_, without = device(case, nreg, masks, True, a.swamth, clock=False), device(case, nreg, masks, False, a.swamth)
    t = {id(with_): [], id(without): []}
    ns = {id(with_): with_.step(0, a.warmup), id(without): without.step(0, a.warmup)}
    for _ in range(3):
        for g in (without, with_):
            g.sync()
            t0 = time.perf_counter()
            ns[id(g)] = g.step(ns[id(g)], a.steps)
            g.sync()
            t[id(g)].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step_ms_undeclared"], res["step_ms_declared"] = t[id(without)], t[id(with_)]
    res["adds_ms"] = statistics.median(t[id(with_)]) - statistics.median(t[id(without)])
    print("step undeclared [ms]:", " ".join(f"{x:.3f}" for x in t[id(without)]), " declared:", " ".join(f"{x:.3f}" for x in t[id(with_)]),
          f"-> adds {res['adds_ms']:.3f} ms")
    with_.close()
    without.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
