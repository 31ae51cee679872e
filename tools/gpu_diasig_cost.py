"""What the density-class mass fluxes (k_diasig, blom_amd/csrc/stage_diaacc.hip) cost on the channel (208x512x53, ntr = 3, the bench
workload) with the six names umfll umfltdl umflsml vmfll vmfltdl vmflsml selected and the case's reference densities as sigdia:

 1. each launch of the stage (the stage timers "diasig_int", "diasig_u", "diasig_v"), timed with HIP events over 20 steps after 5
    warm-up steps, with its bytes by the bound -- (2 + n_sel + 2 n_sel) kk planes per grid: sigint twice, the sources, the
    accumulators read and written; 2 kk planes for the sigint kernel -- and the rate that is, beside what
    tools/probes/stream_probe.hip reaches in the same job (the halo exchange of sigint between them is a few hundred points);
 2. what the set adds to a step: one context with it, one without, stepped alternately (wall clock around blomgpu_step + sync,
    medians of three rounds of 20 steps).

usage (GPU box): python3 tools/gpu_diasig_cost.py [--out profiles/diasig_cost.json] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from gpu_diaacc_cost import probe_rates  # noqa: E402

NAMES = "umfll umfltdl umflsml vmfll vmfltdl vmflsml".split()


def reference_densities(gpu, case, masks):
    """the column of sigmar at the first wet owned point"""
    nj, ni = case.jdm + 8, case.idm + 8
    wet = np.zeros((nj, ni), bool)
    wet[4:-4, 4:-4] = True
    wet &= np.asarray(masks["ip"]).reshape(nj, ni) > 0
    j, i = np.argwhere(wet)[0]
    return gpu.get("sigmar")[:case.kdm, j, i].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diasig_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    probe = rates.get((4, 2)) or max(rates.values())             # 5 planes in, 3 out per grid: the nearest line of the probe
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    plane = case.idm * case.jdm * 8
    kk = case.kdm
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=kk, steps=a.steps, warmup=a.warmup, names=NAMES,
               stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()}, probe_TBps=probe, launches={})
    gpu = bench.device_for_bench(case, nreg, masks, live=True)
    sigdia = reference_densities(gpu, case, masks)
    gpu.dia_set_sigdia(sigdia)
    gpu.dia_select(NAMES)
    ns = gpu.step(0, a.warmup)
    gpu.set("timing", 1)
    gpu.timer_reset()
    ns = gpu.step(ns, a.steps)
    gpu.sync()
    for label, byt in (("diasig_int", 2 * kk * plane), ("diasig_u", (2 + 3 + 2 * 3) * kk * plane), ("diasig_v", (2 + 3 + 2 * 3) * kk * plane)):
        ms, cnt = gpu.timer_get(label)
        b = dict(bytes=byt, ms=ms / max(cnt, 1), launches=cnt)
        b["TBps"] = byt / (b["ms"] * 1e-3) / 1e12 if cnt else 0.0
        b["of_probe"] = b["TBps"] / probe
        res["launches"][label] = b
        print(f"{label:10s}: {byt / 1e9:6.3f} GB, {b['ms']:7.4f} ms, {b['TBps']:5.2f} TB/s = {b['of_probe']:4.2f} of the probe's {probe:4.2f}")
    res["ms_total"] = sum(b["ms"] for b in res["launches"].values())
    gpu.close()
    # what the set adds to the step
    with_, without = (bench.device_for_bench(case, nreg, masks, live=True) for _ in range(2))
    with_.dia_set_sigdia(sigdia)
    with_.dia_select(NAMES)
    t = {id(with_): [], id(without): []}
    ns = {id(with_): with_.step(0, a.warmup), id(without): without.step(0, a.warmup)}
    for _ in range(3):
        for g in (without, with_):
            g.sync()
            t0 = time.perf_counter()
            ns[id(g)] = g.step(ns[id(g)], a.steps)
            g.sync()
            t[id(g)].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step_ms_without"], res["step_ms_with"] = t[id(without)], t[id(with_)]
    res["adds_ms"] = statistics.median(t[id(with_)]) - statistics.median(t[id(without)])
    print("step without [ms]:", " ".join(f"{x:.3f}" for x in t[id(without)]), " with:", " ".join(f"{x:.3f}" for x in t[id(with_)]),
          f"-> adds {res['adds_ms']:.3f} ms")
    with_.close()
    without.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
