"""What templvl salnlvl uvellvl vvellvl cost under the hybrid coordinate (blom_amd/csrc/stage_ale.hip: k_ale_zl_edges, the engine's
prepare_remapping and remap on the maps with n_dst = ddm, k_ale_zl_add) on `bench.py --config hybrid`'s workload -- the channel
(208x512x53, ntr = 3), cntiso_hybrid, nudge, ppm 6/4, ltedtp = 'neutral' -- with the default 35 levels:

 1. the new launches inside ale_regrid_remap (alarm 0; the stage timers "ale_diazlv_trc" and "ale_diazlv_vel", each around its
    edge kernel, prepare_remapping, remap and the add), timed with HIP events over 20 steps after 5 warm-up steps, with their
    algorithmic bytes, beside the nearest line of tools/probes/stream_probe.hip in the same job; and the end-of-step call
    (alarm 1; "ale_remap_diazlv": both parts again plus a prepare_reconstruction and a reconstruction of each grid), timed over 20 calls;
 2. what the four names add to a step: one context with them (alarm 0), one without, stepped alternately (wall clock around
    blomgpu_step + sync, medians of three rounds of 20 steps).

Bytes of a part, in planes of idm x jdm doubles (F = fields of the part: 2; c = polynomial coefficients per layer: 3 for ppm):
  edges      2 (p_src(1), p_src(kk+1)) + 1 (depths) in, ddm + 1 out                    -- x 2 columns for the velocities
  prepare    (ddm + 1) + 3 kk + 1 in (the target edges; x_edge, h, 1/h of the grid), 3.5 (kk + ddm) + .5 kk out (limits, weights,
             destination indices and segment counts, the last two ints)
  remap      F ((c + 1) kk + ddm) + 3.5 (kk + ddm) + .5 kk in / out (the map again, means and coefficients in, ddm planes out)
  add        F 3 ddm (remapped plane and accumulator in, accumulator out) + 1 (ub | vb)
The two-pass form (remap to scratch, then add) moves F 2 ddm planes more than an engine entry that added into the slots would.

usage (GPU box): python3 tools/gpu_diahyb_cost.py [--out profiles/diahyb_cost.json] [--steps 20] [--warmup 5]"""
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

NAMES = "templvl salnlvl uvellvl vvellvl".split()


def hybrid_device(case, nreg, masks):
    """bench.bench_hybrid_step's context: the same fields, options and start"""
    import numpy as np
    from blom_amd.gpu import BlomGpu
    from blom_amd import hostinit
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(gpu, case)
    kk = case.kdm
    for nm, a in bench._hybrid_fields(case).items():
        gpu.put(nm, a)
    pbot = float(np.max(gpu.get("p")[kk][4:-4, 4:-4][masks["ip"][4:-4, 4:-4] > 0]))
    gpu.set("vcoord_type", "cntiso_hybrid")
    o = bench.HYB_OPTS
    gpu.set("ale_regrid_method", o["regrid_method"])
    gpu.set("ale_reconstruction_method", o["reconstruction_method"])
    gpu.set("ale_tracer_limiting", o["tracer_limiting"])
    gpu.set("ale_velocity_limiting", o["velocity_limiting"])
    for nm in ("upper_bndr_ord", "lower_bndr_ord"):
        gpu.set("ale_" + nm, int(o[nm]))
    for nm in ("tracer_pc_upper_bndr", "tracer_pc_lower_bndr", "velocity_pc_upper_bndr", "velocity_pc_lower_bndr"):
        gpu.set("ale_" + nm, 1 if o[nm] else 0)
    gpu.set("mlrmth", "fox08")
    gpu.set_vector("plevel", 0.05 * pbot * (np.arange(kk) / kk) ** 1.3)
    gpu.set("ltedtp_opt", 2)
    gpu.set("ndiff_surface_align", 1)
    gpu.stage("cmnfld1", *hostinit.init_indices(0, kk))
    return gpu


def part_planes(kk, ddm, ncoef, cols):
    """planes of one column set moved by the four launches of a part with two fields; cols = 1 (p) | 2 (u and v side by side)"""
    F = 2
    edges = 3 + ddm + 1
    prep = (ddm + 1) + 3 * kk + 1 + 3.5 * (kk + ddm) + .5 * kk
    remap = F * ((ncoef + 1) * kk + ddm) + 3.5 * (kk + ddm) + .5 * kk if cols == 1 else ((ncoef + 1) * kk + ddm) + 3.5 * (kk + ddm) + .5 * kk
    add = F * 3 * ddm + (0 if cols == 1 else 2)
    return dict(edges=edges * cols, prepare=prep * cols, remap=remap * cols, add=add)


def main():
    from blom_amd import hostinit
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diahyb_cost.json"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rates, raw = probe_rates()
    print(raw)
    case, nreg, masks = bench.build_case("channel")
    plane = case.idm * case.jdm * 8
    kk = case.kdm
    gpu = hybrid_device(case, nreg, masks)
    gpu.dia_alarm(0)
    gpu.dia_select(NAMES)
    ddm = len(gpu.dia_levels())
    res = dict(config="hybrid", idm=case.idm, jdm=case.jdm, kdm=kk, ddm=ddm, steps=a.steps, warmup=a.warmup, names=NAMES,
               stream_probe_TBps={f"{k[0]}in_{k[1]}out": v for k, v in rates.items()}, launches={})
    ns = gpu.step(0, a.warmup)
    gpu.set("timing", 1)
    gpu.timer_reset()
    ns = gpu.step(ns, a.steps)
    gpu.sync()
    tm = {lb: gpu.timer_get(lb) for lb in ("ale_diazlv_trc", "ale_diazlv_vel", "ale_regrid_remap")}
    gpu.dia_alarm(1)
    six = hostinit.step_indices(ns - 1, kk)
    gpu.timer_reset()
    for _ in range(a.steps):
        gpu.ale_remap_diazlv(*six)
    gpu.sync()
    tm["ale_remap_diazlv"] = gpu.timer_get("ale_remap_diazlv")
    gpu.close()
    trc, vel = part_planes(kk, ddm, 3, 1), part_planes(kk, ddm, 3, 2)
    # the end-of-step call adds, per grid: prepare_reconstruction (kk + 1 in, ~ (3 + ncoef + 2) kk out) and the reconstructions
    recon = (kk + 1) + 8 * kk + 2 * (kk + 5 * kk) + 2 * ((2 * kk + 1) + 8 * kk + (kk + 5 * kk))
    parts = (("ale_diazlv_trc", sum(trc.values()) * plane, 4, 2, trc), ("ale_diazlv_vel", sum(vel.values()) * plane, 4, 2, vel),
             ("ale_remap_diazlv", (sum(trc.values()) + sum(vel.values()) + recon) * plane, 4, 2, None))
    for label, byt, n_in, n_out, split in parts:
        t, cnt = tm[label]
        key, probe = nearest(rates, n_in, n_out)
        b = dict(bytes=byt, ms=t / max(cnt, 1), launches=cnt, probe_line=f"{key[0]}in_{key[1]}out", probe_TBps=probe)
        if split:
            b["planes"] = split
        b["TBps"] = byt / (b["ms"] * 1e-3) / 1e12 if cnt and b["ms"] > 0 else 0.0
        b["of_probe"] = b["TBps"] / probe
        res["launches"][label] = b
        print(f"{label:18s}: {byt / 1e9:7.4f} GB, {b['ms']:7.4f} ms x {cnt}, {b['TBps']:6.3f} TB/s = {b['of_probe']:4.2f} of the probe's {probe:4.2f} ({b['probe_line']})")
    res["ale_regrid_remap_ms_with"] = tm["ale_regrid_remap"][0] / max(tm["ale_regrid_remap"][1], 1)
    res["two_pass_extra_bytes"] = 2 * 2 * 2 * ddm * plane          # 2 parts x 2 fields x (ddm written + ddm read again)
    # what the four names add to the step
    with_, without = hybrid_device(case, nreg, masks), hybrid_device(case, nreg, masks)
    with_.dia_alarm(0)
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
