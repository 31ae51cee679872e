"""What the vertical mass fluxes (diavfl: k_diavfl_lyr, k_diavfl_lvl, blom_amd/csrc/stage_diaacc.hip) cost on the channel (208x512x53,
ntr = 3, the bench workload) with wflx wflx2 wflxlvl wflx2lvl selected (the group: plus uflx vflx uflxlvl vflxlvl and the two old slots)
at the default 35 levels:

 1. each part of the stage (the stage timers "diavfl_copy", "diavfl_lyr", "diavfl_xctilr", "diavfl_lvl"), timed with HIP events over 20
    steps after 5 warm-up steps, with its bytes by the bound -- the copy 4 ddm planes (two slots read and written); the layer kernel
    (4 + 4) kk planes (uflx, vflx, dp, dpold -- a face is read by the two columns it separates and comes from memory once; two
    accumulators read and written); the level kernel (4 + 4) ddm planes; the two exchanges the halo ring of 2 ddm planes, read and
    written -- and the rate that is, beside the nearest line of tools/probes/stream_probe.hip in the same job.  Beside them the
    launches the group's dependencies bring (uflx vflx in "diaacc_lyr", uflxlvl in "dialvl_u", vflxlvl in "dialvl_v") and "tmsmt"
    (tmsmt1 + tmsmt2 of a step) with the group, where tmsmt1 stays a launch of its own, and without it, where it is folded;
 2. what the group adds to a step: one context with it, one without, stepped alternately (wall clock around blomgpu_step + sync,
    medians of three rounds of 20 steps).  The context with the group runs tmsmt1 as a launch of its own in every step; the one
    without folds it into tmsmt2 in all but the last step of a call.

usage (GPU box): python3 tools/gpu_diavfl_cost.py [--out profiles/diavfl_cost.json] [--steps 20] [--warmup 5]"""
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

NAMES = "wflx wflx2 wflxlvl wflx2lvl".split()


def nearest(rates, n_in, n_out):
    key = min(rates, key=lambda k: (abs(k[0] - n_in) + abs(k[1] - n_out), k))
    return key, rates[key]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diavfl_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    plane = case.idm * case.jdm * 8
    kk = case.kdm
    gpu = bench.device_for_bench(case, nreg, masks, live=True)
    gpu.dia_select(NAMES)
    ddm = len(gpu.dia_levels())
    ring = 2 * (case.idm + 2) + 2 * case.jdm
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=kk, ddm=ddm, steps=a.steps, warmup=a.warmup, names=NAMES,
               stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()}, launches={})
    ns = gpu.step(0, a.warmup)
    gpu.set("timing", 1)
    gpu.timer_reset()
    ns = gpu.step(ns, a.steps)
    gpu.sync()
    # (label, bytes, streams in, streams out of the probe line it is put beside)
    parts = (("diavfl_copy", 4 * ddm * plane, 2, 1), ("diavfl_lyr", (4 + 4) * kk * plane, 4, 2),
             ("diavfl_xctilr", 2 * 2 * ddm * ring * 8, 2, 1), ("diavfl_lvl", (4 + 4) * ddm * plane, 4, 2))
    for label, byt, n_in, n_out in parts:
        ms, cnt = gpu.timer_get(label)
        key, probe = nearest(rates, n_in, n_out)
        b = dict(bytes=byt, ms=ms / max(cnt, 1), launches=cnt, probe_line=f"{key[0]}in_{key[1]}out", probe_TBps=probe)
        b["TBps"] = byt / (b["ms"] * 1e-3) / 1e12 if cnt else 0.0
        b["of_probe"] = b["TBps"] / probe
        res["launches"][label] = b
        print(f"{label:14s}: {byt / 1e9:7.4f} GB, {b['ms']:7.4f} ms, {b['TBps']:6.3f} TB/s = {b['of_probe']:4.2f} of the probe's {probe:4.2f} ({b['probe_line']})")
    res["ms_total"] = sum(b["ms"] for b in res["launches"].values())
    res["ms_per_step_beside"] = {lb: gpu.timer_get(lb)[0] / a.steps for lb in ("diaacc_lyr", "dialvl_u", "dialvl_v", "tmsmt")}
    gpu.close()
    plain = bench.device_for_bench(case, nreg, masks, live=True)
    ns = plain.step(0, a.warmup)
    plain.set("timing", 1)
    plain.timer_reset()
    plain.step(ns, a.steps)
    plain.sync()
    res["tmsmt_ms_per_step_folded"] = plain.timer_get("tmsmt")[0] / a.steps
    plain.close()
    res["tmsmt1_unfolded_adds_ms"] = res["ms_per_step_beside"]["tmsmt"] - res["tmsmt_ms_per_step_folded"]
    print("per step [ms]:", {k: round(v, 4) for k, v in res["ms_per_step_beside"].items()}, "tmsmt folded:", round(res["tmsmt_ms_per_step_folded"], 4))
    # what the group adds to the step
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
