"""What the coupled experiment's surface forcing costs on the device (blom_amd/csrc/stage_thermf_cesm.hip: getfrc_cesm, sfcstr_cesm,
thermf_cesm; bench.py's workload with expcnf = 'cesm' declared and synthetic coupler forcing, blom_amd.hostinit.cesm_forcing):

 1. the three stages' timers (HIP events around each stage's launches, option "timing") over --steps steps after --warmup; thermf's
    three parts each with a timer of its own (flux kernel, the batched sums' two kernels, correction kernel) and its algorithmic
    bytes; the kernel launches of a thermf as the library counts them where it issues them (blomgpu_get_real "thermf_cesm_launches");
 2. the same thermf with its 1 + ntr' sums taken one xcsum at a time (option cesm_single_sums: 2 launches each), for what the batch buys;
 3. the step with the declaration against the step without, stepped alternately (wall clock around blomgpu_step + sync, medians of three
    rounds).

Bytes, in planes of idm x jdm doubles (ntr' = tracers that are not turbulence tracers):
  getfrc   14 x 2 in (the _da pairs; one level each when l1ci = l2ci), 14 out
  sfcstr   2 in, 2 out
  flux     ~28 + 2 ntr' in (forcing, two time levels of the top layer's dp temp saln, the mixed layer's two layers, the climatologies'
           five months x 3, scp2, corrections, tracers), ~19 + 3 ntr' out
  sums     1 + ntr' (+ 2) in
  corr     4 + ntr' in, 3 + ntr' out

usage (GPU box): python3 tools/gpu_thermf_cesm_cost.py [--config channel] [--tracers default|24] [--out profiles/thermf_cesm_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

OPTS = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, smtfrc=1, nstep_in_cpl=4, l1ci=1, l2ci=2, nstep_in_day=96, nday_of_year=1,
            nday_in_year=365)


def device(case, nreg, masks, declared):
    from blom_amd import hostinit
    g = bench.device_for_bench(case, nreg, masks)
    if declared:
        g.set("expcnf", "cesm")
        g.inifrc_cesm()
        hostinit.put_cesm_forcing(g, case, seed=1)
        for nm, v in OPTS.items():
            g.set(nm, v)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="channel")
    ap.add_argument("--tracers", default="default")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    case, nreg, masks = bench.build_case(a.config, tracers=a.tracers)
    p = case.params
    ntrp = case.ntr - (2 if p.get("itrtke", -1) >= 1 else 0)
    plane = case.idm * case.jdm * 8
    res = dict(config=a.config, idm=case.idm, jdm=case.jdm, kdm=case.kdm, ntr=case.ntr, ntr_passive=ntrp, steps=a.steps, warmup=a.warmup,
               plane_bytes=plane, stages={})
    parts = dict(thermf_cesm_flux=(28 + 2 * ntrp) + (19 + 3 * ntrp), thermf_cesm_sums=1 + ntrp, thermf_cesm_corr=(4 + ntrp) + (3 + ntrp))
    planes = dict(getfrc_cesm=14 * 2 + 14, sfcstr=4, thermf=sum(parts.values()), **parts)
    for single in (0, 1):
        g = device(case, nreg, masks, True)
        g.set("cesm_single_sums", single)
        ns = g.step(0, a.warmup)
        g.set("timing", 1)
        g.timer_reset()
        counted = g.get_real("thermf_cesm_launches")
        ns = g.step(ns, a.steps)
        g.sync()
        counted = g.get_real("thermf_cesm_launches") - counted
        for lb in ("getfrc_cesm", "sfcstr", "thermf") + tuple(parts):
            ms, n = g.timer_get(lb)
            key = lb + ("_single_sums" if single else "")
            if single and not lb.startswith("thermf"):
                continue
            calls = a.steps if lb in parts else n                 # (a part's timer counts its launch groups: one per sum when taken singly)
            byt = planes[lb] * plane
            row = dict(ms=ms / max(calls, 1), calls=calls, bytes=byt, TBps=byt / (ms / max(calls, 1) * 1e-3) / 1e12 if ms > 0 else 0.0)
            if lb == "thermf":
                row["launches_per_call_counted"] = counted / a.steps
            res["stages"][key] = row
            print(f"{key:30s}: {row['ms']:8.4f} ms x {calls}, {byt / 1e6:8.2f} MB, {row['TBps']:6.3f} TB/s"
                  + (f", {row['launches_per_call_counted']:.0f} launches a call (counted)" if lb == "thermf" else ""))
        g.close()
    # where the rest of the difference goes: the forcing is another workload for the stages behind it (the channel's own forcing is
    # zero but for the wind), so the other stages' timers of a declared and an undeclared context are put side by side
    classes = ["cmnfld", "difest", "eddtra", "remap", "diffus", "pgforc", "momtum", "convec", "diapfl", "thermf", "mxlayr", "barotp", "pbcor1",
               "pbcor2", "tmsmt", "init_fluxes", "updtrc", "getfrc_cesm", "sfcstr"]
    per = {}
    for declared in (False, True):
        g = device(case, nreg, masks, declared)
        ns = g.step(0, a.warmup)
        g.set("timing", 1)
        g.timer_reset()
        g.step(ns, a.steps)
        g.sync()
        per[declared] = {cl: g.timer_get(cl)[0] / a.steps for cl in classes}
        g.close()
    res["stage_ms_undeclared"], res["stage_ms_declared"] = per[False], per[True]
    print("stage timers [ms a step], undeclared -> declared: " + ", ".join(f"{cl} {per[False][cl]:.3f} -> {per[True][cl]:.3f}" for cl in classes
                                                                              if abs(per[True][cl] - per[False][cl]) > 0.005))
    print(f"sum of the stage timers: {sum(per[False].values()):.3f} -> {sum(per[True].values()):.3f}")
    with_, without = device(case, nreg, masks, True), device(case, nreg, masks, False)
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
