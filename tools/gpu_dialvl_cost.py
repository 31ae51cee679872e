"""What the depth-level diagnostics (k_dialvl, blom_amd/csrc/stage_diaacc.hip) cost on the channel (208x512x53, ntr = 3, the bench workload):

 1. the three level launches (the stage timers "dialvl_u", "dialvl_v", "dialvl_p"), timed with HIP events over 20 steps after 5
    warm-up steps, for two selections -- the 13 names of tests/test_gpu_dialvl.py::test_channel_size_level_set, and all 33 names
    (gls_psilvl is refused without gls) -- with each launch's bytes by the bound (2 n_acc ddm + (n_src + 2) kk) planes and the rate
    that is, beside what tools/probes/stream_probe.hip reaches in the same job;
 2. what each set adds to a step: one context with it, one without, stepped alternately (wall clock around blomgpu_step + sync,
    medians of three rounds of 20 steps).

usage (GPU box): python3 tools/gpu_dialvl_cost.py [--out profiles/dialvl_cost.json] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from gpu_diaacc_cost import probe_rates  # noqa: E402

CHANNEL_SET = "templvl salnlvl uvellvl vvellvl uflxlvl vflxlvl utflxlvl vtflxlvl usflxlvl vsflxlvl difdialvl difisolvl dzlvl".split()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dialvl_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    probe = rates.get((24, 8)) or max(rates.values())
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    plane = case.idm * case.jdm * 8
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=case.kdm, steps=a.steps, warmup=a.warmup,
               stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()}, probe_TBps=probe, selections={})
    sets = {}
    for label in ("test8", "all"):
        gpu = bench.device_for_bench(case, nreg, masks, live=True)
        rows = gpu.dia_names()
        names = CHANNEL_SET if label == "test8" else [nm for nm, kind, _ in rows if kind == 2 and nm != "gls_psilvl"]
        sets[label] = names
        grid = {nm: g for nm, _, g in rows}
        ddm = len(gpu.dia_levels())
        gpu.dia_select(names)
        ns = gpu.step(0, a.warmup)
        gpu.set("timing", 1)
        gpu.timer_reset()
        ns = gpu.step(ns, a.steps)
        gpu.sync()
        b = dict(ddm=ddm, names=len(names))
        for g in "uvp":
            n = len([nm for nm in names if grid[nm] == g])
            ms, cnt = gpu.timer_get("dialvl_" + g)
            byt = (2 * n * ddm + (n + 2) * case.kdm) * plane if n else 0
            b[g] = dict(n_acc=n, bytes=byt, ms=ms / max(cnt, 1), launches=cnt)
            b[g]["TBps"] = byt / (b[g]["ms"] * 1e-3) / 1e12 if cnt and n else 0.0
            b[g]["of_probe"] = b[g]["TBps"] / probe
            print(f"{label:6s} {g}: {n:2d} accumulators x {ddm} levels, {byt / 1e9:6.3f} GB, {b[g]['ms']:7.4f} ms, {b[g]['TBps']:5.2f} TB/s = "
                  f"{b[g]['of_probe']:4.2f} of the probe's {probe:4.2f}")
        b["ms_total"] = sum(b[g]["ms"] for g in "uvp")
        res["selections"][label] = b
        gpu.close()
    # what each set adds to the step
    for label, names in sets.items():
        with_, without = (bench.device_for_bench(case, nreg, masks, live=True) for _ in range(2))
        with_.dia_select(names)
        t = {id(with_): [], id(without): []}
        ns = {id(with_): with_.step(0, a.warmup), id(without): without.step(0, a.warmup)}
        for _ in range(3):
            for g in (without, with_):
                g.sync()
                t0 = time.perf_counter()
                ns[id(g)] = g.step(ns[id(g)], a.steps)
                g.sync()
                t[id(g)].append((time.perf_counter() - t0) / a.steps * 1e3)
        r = res["selections"][label]
        r["step_ms_without"], r["step_ms_with"] = t[id(without)], t[id(with_)]
        r["adds_ms"] = statistics.median(t[id(with_)]) - statistics.median(t[id(without)])
        print(f"{label:6s} step without [ms]:", " ".join(f"{x:.3f}" for x in t[id(without)]), " with:", " ".join(f"{x:.3f}" for x in t[id(with_)]),
              f"-> adds {r['adds_ms']:.3f} ms")
        with_.close()
        without.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
