"""What the output-time reductions (blomgpu_dia_reduce: diamer, diasec, the global sums; blom_amd/csrc/stage_diaout.hip) cost on the
channel (208x512x53, ntr = 3, the bench workload) with every interior row a zonal section, three ocean regions, three meridional
regions, three named sections and all 23 msc names selected -- against the downloads they replace:

 1. dia_reduce, 20 calls after 5 (it is idempotent): each launch timed with HIP events (the stage timers "diaout_*"), with the bytes
    the launch reads -- 16 per section entry and source level plus 16 per entry for its table row; the column sums read their
    sources' planes once -- and the wall clock around the call plus a sync;
 2. in the same job, dia_get of every source accumulator the reductions read: the host path a caller without dia_reduce has to take
    before it can restate diamer itself.

usage (GPU box): python3 tools/gpu_diaout_cost.py [--out profiles/diaout_cost.json] [--calls 20] [--warmup 5]"""
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
from gpu_diasig_cost import reference_densities  # noqa: E402

# name -> (launch, u source, v source)
MSC = dict(
    mmflxl=("density", "umfll", "vmfll"), mmftdl=("density", "umfltdl", "vmfltdl"), mmfsml=("density", "umflsml", "vmflsml"),
    mmflxd=("depth", "uflxlvl", "vflxlvl"), mmftdd=("depth", "umfltdlvl", "vmfltdlvl"), mmfsmd=("depth", "umflsmlvl", "vmflsmlvl"),
    mhflx=("transports", "utflx", "vtflx"), mhftd=("transports", "utfltd", "vtfltd"), mhfsm=("transports", "utflsm", "vtflsm"),
    mhfld=("transports", "utflld", "vtflld"), msflx=("transports", "usflx", "vsflx"), msftd=("transports", "usfltd", "vsfltd"),
    msfsm=("transports", "usflsm", "vsflsm"), msfld=("transports", "usflld", "vsflld"),
    masstr=("diasec", "uflxlvl", "vflxlvl"), heattr=("diasec", "utflxlvl", "vtflxlvl"), salttr=("diasec", "usflxlvl", "vsflxlvl"),
    massgs=("columns", "dp", None), salnga=("columns", "dp", "saln"), tempga=("columns", "dp", "temp"), volgs=("columns", "dz", None),
    sssga=("columns", "sss", None), sstga=("columns", "sst", None))


def tables(case):
    idm, jdm = case.idm, case.jdm
    oflg = np.zeros((jdm, idm), np.int32)
    oflg[:, :idm // 3], oflg[:, idm // 3:2 * idm // 3], oflg[:, 2 * idm // 3:] = 1, 2, 3
    rows = list(range(2, jdm))
    pts = np.array([(i, j, 0, 1) for j in rows for i in range(1, idm + 1)], np.int32)
    regflg = np.zeros((3, 20), np.int32)
    regflg[1, :2], regflg[2, 0] = (1, 2), 3
    mer = dict(mtlat=np.array(rows, np.float64), nind=np.full(len(rows), idm, np.int32), pts=pts, oflg=oflg, ocn_nreg=3,
               nflg=np.array([1, 2, 1], np.int32), regflg=regflg, minlat=np.full(3, -1.0), maxlat=np.full(3, 1.0e4))
    secs = [[(idm // 2, j, 1, 0) for j in range(1, jdm + 1)], [(i, jdm // 2, 0, 1) for i in range(1, idm + 1)],
            [(1 + s, 1 + s, 1, 1) for s in range(min(idm, jdm))]]
    sec = dict(nsi=np.array([len(s) for s in secs], np.int32), pts=np.array([p for s in secs for p in s], np.int32), equat_sec=2)
    return mer, sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diaout_cost.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    case, nreg, masks = bench.build_case("channel", "remap", "default")
    kk, plane = case.kdm, (case.idm + 8) * (case.jdm + 8) * 8
    gpu = bench.device_for_bench(case, nreg, masks, live=True)
    gpu.dia_set_sigdia(reference_densities(gpu, case, masks))
    mer, sec = tables(case)
    gpu.dia_set_mertra(**mer)
    gpu.dia_set_sections(sec["nsi"], sec["pts"], sec["equat_sec"])
    if gpu.get_real("area") <= 0.:
        gpu.set("area", float(case.idm * case.jdm) * 1.0e8)
    gpu.dia_select(list(MSC))
    assert gpu.step(0, 4) == 4
    gpu.sync()
    ddm = len(gpu.dia_levels())
    nlev = lambda s: 1 if s in ("sss", "sst") else ddm if s.endswith("lvl") else kk
    # the bytes a launch reads
    ent = dict(transports=int(mer["nind"].sum()), density=int(mer["nind"].sum()), depth=int(mer["nind"].sum()), diasec=int(sec["nsi"].sum()))
    byt = dict.fromkeys(("transports", "density", "depth", "diasec", "columns"), 0)
    for nm, (launch, us, vs) in MSC.items():
        if launch != "columns":
            byt[launch] += ent[launch] * (16 * nlev(us) + 16)
    byt["columns"] = sum(nlev(s) for s in ("dp", "dz", "saln", "temp", "sss", "sst")) * plane + 6 * plane
    for _ in range(a.warmup):
        gpu.dia_reduce()
    gpu.sync()
    gpu.set("timing", 1)
    gpu.timer_reset()
    wall = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        gpu.dia_reduce()
        gpu.sync()
        wall.append((time.perf_counter() - t0) * 1e3)
    res = dict(config="channel", idm=case.idm, jdm=case.jdm, kdm=kk, ddm=ddm, calls=a.calls, warmup=a.warmup, names=list(MSC),
               sections=len(mer["mtlat"]), entries=int(mer["nind"].sum()), launches={})
    for label in ("transports", "density", "depth", "diasec", "columns", "xcsum"):
        ms, cnt = gpu.timer_get("diaout_" + label)
        res["launches"][label] = dict(ms=ms / max(cnt, 1), timed=cnt, bytes=byt.get(label, 0))
        print(f"diaout_{label:10s}: {res['launches'][label]['ms']:8.4f} ms, {byt.get(label, 0) / 1e6:9.2f} MB read")
    gpu.set("timing", 0)
    res["reduce_ms_events"] = sum(v["ms"] for v in res["launches"].values())
    res["reduce_ms_wall"] = wall
    # the downloads the reduction replaces
    srcs = sorted({s for v in MSC.values() for s in v[1:] if s})
    down = []
    for _ in range(3):
        gpu.sync()
        t0 = time.perf_counter()
        for s in srcs:
            gpu.dia_get(s)
        down.append((time.perf_counter() - t0) * 1e3)
    res["sources"] = srcs
    res["download_bytes"] = sum(nlev(s) for s in srcs) * plane
    res["download_ms"] = down
    print(f"dia_reduce: {res['reduce_ms_events']:.3f} ms by events, {statistics.median(wall):.3f} ms wall (median of {a.calls}); "
          f"dia_get of {len(srcs)} sources, {res['download_bytes'] / 1e9:.2f} GB: {statistics.median(down):.1f} ms (median of 3)")
    res["reduce_faster_than_downloads"] = bool(statistics.median(wall) < statistics.median(down))
    gpu.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    assert res["reduce_faster_than_downloads"], "the reduction takes longer than the downloads it replaces"


if __name__ == "__main__":
    main()
