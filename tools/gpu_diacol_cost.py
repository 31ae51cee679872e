"""What the column-derived diagnostics (k_diacol, k_diapv, blom_amd/csrc/stage_diaacc.hip; k_cmn_mldl82<DIAG>, stage_cmnfld.hip) cost on
the channel (208x512x53, ntr = 3, the bench workload) with sbot tbot t20d t17d mldl82 mldl82mn mldl82mx mldl82sq avdsg dpvor selected:

 1. the new launches (the stage timers "diacol" and "diapv"; "cmn_mldl82", the launch cmnfld1 adds under isopyc_bulkml), timed with
    HIP events over 20 steps after 5 warm-up steps, with their bytes by the bound -- k_diacol: temp saln dp and p(2..kk+1) of every
    layer, p(1), at most 8 planes of z / dz, mldl82, and 8 accumulators read and written; k_diapv: absvor dpvor sigma and two
    accumulators read and written, per layer; the mldl82 launch: p temp saln dp z dz per layer and one plane out (every layer is
    counted; the search ends below the mixed layer and reads a fraction of that) -- and the rate that is, beside the nearest line
    of tools/probes/stream_probe.hip in the same job;
 2. what the ten names add to a step: one context with them, one without, stepped alternately (wall clock around blomgpu_step + sync,
    medians of three rounds of 20 steps).

usage (GPU box): python3 tools/gpu_diacol_cost.py [--out profiles/diacol_cost.json] [--steps 20] [--warmup 5]"""
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
from gpu_diavfl_cost import nearest  # noqa: E402

NAMES = "sbot tbot t20d t17d mldl82 mldl82mn mldl82mx mldl82sq avdsg dpvor".split()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diacol_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    plane = case.idm * case.jdm * 8
    kk = case.kdm
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=kk, steps=a.steps, warmup=a.warmup, names=NAMES,
               stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()}, launches={})
    ms = {}
    for label, names in (("with", NAMES), ("without", [])):
        gpu = bench.device_for_bench(case, nreg, masks, live=True)
        gpu.dia_select(names)
        ns = gpu.step(0, a.warmup)
        gpu.set("timing", 1)
        gpu.timer_reset()
        gpu.step(ns, a.steps)
        gpu.sync()
        ms[label] = {lb: gpu.timer_get(lb) for lb in ("diacol", "diapv", "cmn_mldl82", "cmnfld")}
        gpu.close()
    # (label, bytes, streams in, streams out of the probe line it is put beside)
    parts = (("diacol", (4 * kk + 1 + 8 + 1 + 2 * 8) * plane, 4, 1), ("diapv", (3 + 4) * kk * plane, 4, 2),
             ("cmn_mldl82", (6 * kk + 1) * plane, 4, 1))
    for label, byt, n_in, n_out in parts:
        t, cnt = ms["with"][label]
        key, probe = nearest(rates, n_in, n_out)
        b = dict(bytes=byt, ms=t / max(cnt, 1), launches=cnt, probe_line=f"{key[0]}in_{key[1]}out", probe_TBps=probe)
        b["TBps"] = byt / (b["ms"] * 1e-3) / 1e12 if cnt else 0.0
        b["of_probe"] = b["TBps"] / probe
        res["launches"][label] = b
        print(f"{label:10s}: {byt / 1e9:7.4f} GB, {b['ms']:7.4f} ms, {b['TBps']:6.3f} TB/s = {b['of_probe']:4.2f} of the probe's {probe:4.2f} ({b['probe_line']})")
    # (the bound of the mldl82 launch counts every layer; the search ends at the first layer below the mixed layer, so the launch
    # reads a fraction of it.)  The stage timer "cmnfld" brackets all of a step's cmnfld launches, this one among them
    res["cmnfld_ms_per_step"] = {lb: ms[lb]["cmnfld"][0] / a.steps for lb in ms}
    print("the stage timer 'cmnfld' per step [ms]:", {k: round(v, 4) for k, v in res["cmnfld_ms_per_step"].items()})
    res["ms_total"] = sum(b["ms"] for b in res["launches"].values())
    # what the ten names add to the step
    with_, without = (bench.device_for_bench(case, nreg, masks, live=True) for _ in range(2))
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
