"""HIP-event time of one 3-D halo update (dp, 2 x kdm levels, halo 3) per tile on the tnx1v4s grid cut by eliminate_land into
8 x 4 tiles (32 tiles, row 3 ragged: k_xctilr_tiles_ragged) beside the same on TileLayout.regular(360, 385, 8, 4)
(k_xctilr_tiles).  An in-process, one-GPU number: the tiles are threads of this process on one device and read each other's
memory; it says nothing about xGMI or the RCCL transport.  Usage: python tools/gpu_halo_ragged.py [repeats]"""
import os
import sys
import threading

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(lay, case, masks, nreg, reps):
    import numpy as np
    from blom_amd.gpu import BlomGpu, TileGroup
    grp = TileGroup.for_layout(lay)
    tiles = {}
    rng = np.random.default_rng(3)
    for px, py in lay.tiles():
        i0, j0, ii, jj = lay.tile(px, py)
        t = BlomGpu(ii, jj, case.kdm, case.ntr, nreg, {k: lay.window(masks[k], px, py) for k in masks},
                    itdm=case.idm, jtdm=case.jdm, i0=i0, j0=j0)
        t.put("dp", rng.random((2 * case.kdm, jj + 8, ii + 8)))
        grp.attach(t, px, py)
        tiles[(px, py)] = t
    out, errs = {}, []

    def run(k):
        t = tiles[k]
        try:
            for r in range(reps + 2):
                if r == 2:                       # two warm-up updates
                    t.set("timing", 1)
                    t.timer_reset()
                t.xctilr("dp", 1, 1, 2 * case.kdm, 3, 3, 1)
            t.sync()
            ms, n = t.timer_get("halo_gather")
            out[k] = ms / max(n, 1)
        except Exception as e:
            errs.append(e)
    th = [threading.Thread(target=run, args=(k,), daemon=True) for k in tiles]
    [x.start() for x in th]
    [x.join(timeout=120) for x in th]
    assert not errs and not any(x.is_alive() for x in th), errs
    for t in tiles.values():
        t.close()
    grp.destroy()
    return out


def main():
    import numpy as np
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    from blom_amd.tiles import TileLayout
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    case = make_case("tnx1v4s_tke")
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=True)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    for name, lay in (("regular 8x4", TileLayout.regular(case.idm, case.jdm, 8, 4)),
                      ("eliminate_land 8x4", TileLayout.eliminate_land(ip[4:-4, 4:-4], 8, 4, nreg))):
        v = np.array(list(measure(lay, case, masks, nreg, reps).values()))
        print(f"{name}: {len(v)} tiles, halo update of dp per tile [ms]: median {np.median(v):.4f}  min {v.min():.4f}  max {v.max():.4f}")


if __name__ == "__main__":
    main()
