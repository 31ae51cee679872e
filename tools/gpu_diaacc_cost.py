"""What the device-side diagnostics (diaacc, blom_amd/csrc/stage_diaacc.hip) cost on the channel (208x512x53, ntr = 3, the bench workload):

 1. the layer launch and the 2-D launch of k_diaacc, timed with HIP events (the stage timers "diaacc_lyr", "diaacc_h2d") over 20 steps
    after 5 warm-up steps, for two selections -- the whole table, and a "monthly" set -- with each launch's bytes by the bound
    (2 n_acc + n_distinct_sources) F and the rate that is, beside what tools/probes/stream_probe.hip reaches in the same job;
 2. what the monthly selection adds to a step: one context with it, one without, stepped alternately (wall clock around
    blomgpu_step + sync, medians of three rounds of 20 steps).

usage (GPU box): python3 tools/gpu_diaacc_cost.py [--out profiles/diaacc_cost.json] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MONTHLY = ("dp temp saln uvel vvel uflx vflx utflx vtflx usflx vsflx umfltd vmfltd difdia difiso dz sealv sst sss ub vb bld maxbld surflx "
           "salflx ustar slvsq").split()
# 2-D names that read the same plane as another one (phy/mod_dia.F90:1589/1780, :1691/1783, :1694/1786, :1703/1752)
SHARED_2D = {"slvsq": "sealv", "ssssq": "sss", "sstsq": "sst", "maxbld": "bld"}
WEIGHT = dict(uvel="dpu", vvel="dpv", saln="dp", temp="dp", bfsq="dp", difint="dp", difiso="dp", difdia="dp", tke="dp", gls_psi="dp")


def probe_rates():
    """the stream probe's lines {(n_in, n_out): TB/s at 8 B per lane}, built on first use"""
    src = os.path.join(ROOT, "tools", "probes", "stream_probe.hip")
    exe = src[:-4]
    if not os.path.exists(exe):
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-o", exe, src])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, check=True).stdout
    rates = {}
    for ln in out.splitlines():
        m = re.match(r"in\s+(\d+) out (\d+): 8 B/lane\s+[\d.]+ us\s+([\d.]+) TB/s", ln)
        if m:
            rates[(int(m.group(1)), int(m.group(2)))] = float(m.group(3))
    return rates, out


def bound_bytes(rows, selected, case):
    """(2 n_acc + n_distinct_sources) F for the layer launch, the same with G for the 2-D launch"""
    F = case.idm * case.jdm * case.kdm * 8
    G = case.idm * case.jdm * 8
    lyr = [nm for nm, is_lyr, _ in rows if is_lyr == 1 and nm in selected]
    h2d = [nm for nm, is_lyr, _ in rows if not is_lyr and nm in selected]
    # a layer row reads its own 3-D source, except dp / dpu / dpv, whose source is the weight the point has loaded anyway
    src_l = len([nm for nm in lyr if nm not in ("dp", "dpu", "dpv")]) + len({"dp", "dpu", "dpv"} & (set(lyr) | {WEIGHT[nm] for nm in lyr if nm in WEIGHT}))
    src_h = len({SHARED_2D.get(nm, nm) for nm in h2d}) + (1 if {"bld", "maxbld"} & set(h2d) else 0)      # dpml is two planes of dp
    return dict(n_lyr=len(lyr), src_lyr=src_l, bytes_lyr=(2 * len(lyr) + src_l) * F, n_h2d=len(h2d), src_h2d=src_h, bytes_h2d=(2 * len(h2d) + src_h) * G)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diaacc_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    probe = rates.get((24, 8)) or max(rates.values())
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=case.kdm, steps=a.steps, warmup=a.warmup, stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()},
               probe_TBps=probe, selections={})
    for label in ("whole", "monthly"):
        gpu = bench.device_for_bench(case, nreg, masks, live=True)
        rows = gpu.dia_names()
        names = MONTHLY if label == "monthly" else [nm for nm, kind, _ in rows if nm != "gls_psi" and kind != 2]           # (the depth levels: tools/gpu_dialvl_cost.py)
        gpu.dia_select(names)
        selected = set(names) | {WEIGHT[nm] for nm in names if nm in WEIGHT}       # diaini's dependencies, phy/mod_dia.F90:598-608
        b = bound_bytes(rows, selected, case)
        ns = gpu.step(0, a.warmup)
        gpu.set("timing", 1)
        gpu.timer_reset()
        ns = gpu.step(ns, a.steps)
        gpu.sync()
        for k in ("lyr", "h2d"):
            ms, n = gpu.timer_get("diaacc_" + k)
            b["ms_" + k] = ms / max(n, 1)
            b["TBps_" + k] = b["bytes_" + k] / (b["ms_" + k] * 1e-3) / 1e12 if n else 0.0
            b["of_probe_" + k] = b["TBps_" + k] / probe
        res["selections"][label] = b
        print(f"{label:8s} layer launch: {b['n_lyr']:2d} accumulators + {b['src_lyr']:2d} sources, {b['bytes_lyr'] / 1e9:6.3f} GB, {b['ms_lyr']:7.4f} ms, "
              f"{b['TBps_lyr']:5.2f} TB/s = {b['of_probe_lyr']:4.2f} of the probe's {probe:4.2f}")
        print(f"{label:8s} 2-D launch  : {b['n_h2d']:2d} accumulators + {b['src_h2d']:2d} sources, {b['bytes_h2d'] / 1e6:6.3f} MB, {b['ms_h2d']:7.4f} ms, "
              f"{b['TBps_h2d']:5.2f} TB/s")
        gpu.close()
    # what the monthly selection adds to the step
    with_, without = (bench.device_for_bench(case, nreg, masks, live=True) for _ in range(2))
    with_.dia_select(MONTHLY)
    t = {id(with_): [], id(without): []}
    ns = {id(with_): with_.step(0, a.warmup), id(without): without.step(0, a.warmup)}
    for _ in range(3):
        for g in (without, with_):
            g.sync()
            t0 = time.perf_counter()
            ns[id(g)] = g.step(ns[id(g)], a.steps)
            g.sync()
            t[id(g)].append((time.perf_counter() - t0) / a.steps * 1e3)
    res["step_ms_without"] = t[id(without)]
    res["step_ms_monthly"] = t[id(with_)]
    res["monthly_adds_ms"] = statistics.median(t[id(with_)]) - statistics.median(t[id(without)])
    print("step without a selection [ms]:", " ".join(f"{x:.3f}" for x in t[id(without)]))
    print("step with the monthly set [ms]:", " ".join(f"{x:.3f}" for x in t[id(with_)]), f"-> adds {res['monthly_adds_ms']:.3f} ms")
    with_.close()
    without.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
