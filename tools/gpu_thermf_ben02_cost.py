"""What the forced ocean-ice experiment's surface forcing costs on the device (blom_amd/csrc/stage_thermf_ben02.hip: sfcstr_ben02,
thermf_ben02; bench.py's workload with expcnf = 'ben02clim' declared and the synthetic forcing of blom_amd.hostinit.ben02_forcing):

 1. the two stages' timers (HIP events around each stage's launches, option "timing") over --steps steps after --warmup; thermf's three
    parts each with a timer of its own (flux kernel, the batched sums' two kernels, correction kernel) and its algorithmic bytes; the
    kernel launches of a thermf as the library counts them where it issues them (blomgpu_get_real "thermf_ben02_launches");
 2. the step with the declaration against the step without, stepped alternately (wall clock around blomgpu_step + sync, three rounds).

Bytes, in planes of idm x jdm doubles (ntr' = tracers that are not turbulence tracers), with the relaxation from the climatology on:
  sfcstr   6 in (ficem hicem ztx mty tauxice tauyice), 2 out; in front of it two halo updates of one plane with a halo of one
  flux     ~53 + 2 ntr' in (the top layer's dp temp saln and p, the ice state, the fluxes asflux leaves, swfc2 swal2, the five accumulators,
           the runoff reservoir, the mixed layer's two layers, the climatologies' five months x 3, scp2, corrections, tracers),
           ~28 + 3 ntr' out
  sums     1 + ntr' in
  corr     4 + ntr' in, 3 + ntr' out

usage (GPU box): python3 tools/gpu_thermf_ben02_cost.py [--config channel] [--tracers default|24] [--out profiles/thermf_ben02_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import bench  # noqa: E402

OPTS = dict(trxday=20.0, srxday=40.0, trxdpt=30.0, srxdpt=25.0, nstep_in_day=96, nday_of_year=1, nday_in_year=365)


def device(case, nreg, masks, declared):
    from blom_amd import hostinit
    g = bench.device_for_bench(case, nreg, masks)
    if declared:
        g.set("expcnf", "ben02clim")
        g.inifrc_ben02()
        hostinit.put_ben02_forcing(g, case, seed=1)
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
    parts = dict(thermf_ben02_flux=(53 + 2 * ntrp) + (28 + 3 * ntrp), thermf_ben02_sums=1 + ntrp, thermf_ben02_corr=(4 + ntrp) + (3 + ntrp))
    planes = dict(sfcstr=8, thermf=sum(parts.values()), **parts)
    g = device(case, nreg, masks, True)
    ns = g.step(0, a.warmup)
    g.set("timing", 1)
    g.timer_reset()
    counted = g.get_real("thermf_ben02_launches")
    ns = g.step(ns, a.steps)
    g.sync()
    counted = g.get_real("thermf_ben02_launches") - counted
    assert g.ben02_ntda() == a.warmup + a.steps
    for lb in ("sfcstr", "thermf") + tuple(parts):
        ms, n = g.timer_get(lb)
        calls = a.steps
        byt = planes[lb] * plane
        row = dict(ms=ms / calls, calls=calls, bytes=byt, TBps=byt / (ms / calls * 1e-3) / 1e12 if ms > 0 else 0.0)
        if lb == "thermf":
            row["launches_per_call_counted"] = counted / a.steps
        res["stages"][lb] = row
        print(f"{lb:22s}: {row['ms']:8.4f} ms x {calls}, {byt / 1e6:8.2f} MB, {row['TBps']:6.3f} TB/s"
              + (f", {row['launches_per_call_counted']:.0f} launches a call (counted)" if lb == "thermf" else ""))
    res["ice_volume_after"] = float((g.get("hicem") * g.get("ficem")).sum())
    g.close()
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
