"""Shared by tests/test_hostemu_ragged.py (emulated RCCL ranks on the CPU) and tests/test_gpu_ragged_tiles.py (in-process
group on the device): the small cases whose bathymetry is carved (make_case(..., carve=...)) so that land-tile elimination
(blom_amd.tiles.TileLayout.eliminate_land) yields what each case is for -- an eliminated tile, a row with an interior gap
that no longer wraps, a trimmed row under the uniform top row of an arctic grid -- and the runners of the two transports."""
import threading

import numpy as np

CHECK = ["u", "v", "dp", "temp", "saln", "sigma", "pb", "ub", "vb", "ubflxs_p", "pb_p", "trc", "uflx", "vflx",
         "pgfx", "pgfy", "dpu", "dpv", "pbu", "pbv", "ubflx", "vbflx", "pb_mn", "ubcors_p"]


# Every block of land reaches nbdy rows beyond the tile row it empties, so that no tile touches sea diagonally across an
# edge without a neighbour (TileLayout.corner_contacts: there the reference's exchange writes vland)
def _carve_box(d):            # box_s 24 x 20 as 3 x 2: the north-eastern cell all land, the northern middle one trimmed
    d[6:20, 12:24] = 0.0


def _carve_chan(d):           # chan_s 20 x 24 as 3 x 2: the northern row loses its western 3 columns and its middle
    d[8:24, 0:4] = 0.0        # (with column 20: a block across the periodic seam)
    d[8:24, 19:20] = 0.0
    d[8:24, 7:15] = 0.0


def _carve_tri(d):            # tri_s 24 x 20 as 4 x 2: a continent across the two middle cells of the southern row
    d[0:14, 5:19] = 0.0


CASES = {
    # name: (cfg, carve, npx, npy)
    "box_3x2_one_tile_eliminated": ("box_s", _carve_box, 3, 2),
    "chan_3x2_gap_row_does_not_wrap": ("chan_s", _carve_chan, 3, 2),
    "tri_4x2_trimmed_row_under_arctic_row": ("tri_s_tke", _carve_tri, 4, 2),
}


def build(name, advmth=None):
    """(case, masks, ref, layout): the carved case initialised on a single tile, and its land-eliminated layout"""
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu
    from blom_amd.tiles import TileLayout
    cfg, carve, npx, npy = CASES[name]
    case = make_case(cfg, carve=carve, **({"advmth": advmth} if advmth else {}))
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    ref = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(ref, case)
    ref.set("delt1", case.params["baclin"])
    lay = TileLayout.eliminate_land(ip[4:-4, 4:-4], npx, npy, nreg)
    assert_shape(name, lay)
    assert lay.corner_contacts(ip[4:-4, 4:-4], nreg) == []
    return case, masks, ref, lay


def assert_shape(name, lay):
    """the property each carved case exists for; a changed bathymetry must not turn it into a tensor-product one"""
    assert not lay.is_tensor_product
    if name.startswith("box_3x2"):
        assert lay.nranks == 5 and lay.rows[1][2][1] == 0                      # the north-eastern tile is gone ...
        assert lay.rows[0][0] == (1, 7) and lay.rows[1][1] == (8, 4)           # ... the tiles around it are trimmed
    elif name.startswith("chan_3x2"):
        assert lay.rows[0] == ((0, 7), (7, 7), (14, 6))                        # spans the domain: wraps in i
        assert lay.rows[1] == ((3, 4), (7, 0), (15, 4))                        # a gap, and the row starts beyond column 1:
        assert lay.rows[1][2][0] - sum(lay.rows[1][0]) >= lay.MIN_GAP          # no wrap there
    elif name.startswith("tri_4x2"):
        assert lay.rows[1] == ((0, 6), (6, 6), (12, 6), (18, 6))               # the arctic top row: uniform
        assert lay.rows[0] == ((0, 5), (6, 0), (12, 0), (19, 5))               # trimmed, two tiles eliminated


def new_tile(case, masks, ref, lay, px, py):
    from blom_amd.gpu import BlomGpu
    from blom_amd.tiles import scatter_to_tile
    i0, j0, ii, jj = lay.tile(px, py)
    t = BlomGpu(ii, jj, case.kdm, case.ntr, case.nreg, {k: lay.window(masks[k], px, py) for k in masks},
                itdm=case.idm, jtdm=case.jdm, i0=i0, j0=j0)
    for nm, v in case.params.items():
        if not nm.endswith("0"):
            t.set(nm, v)
    t.set("delt1", case.params["baclin"])
    scatter_to_tile(ref, t, lay, px, py)
    return t


def full_physics(ref, case, masks):
    """config 2's step as far as built (tests/test_hostemu_multirank.py): returns the per-context setup"""
    from blom_amd import hostinit
    hostinit.init_forcing(ref, case)
    nj, ni = case.jdm + 8, case.idm + 8
    yy = np.linspace(-1.0, 1.0, nj)[:, None] + 0.0 * np.arange(ni)[None, :]
    ref.put("nsf", (300.0 * yy)[None])
    ref.put("swa", (120.0 * (yy > -0.5))[None])
    ref.put("eva", (-2e-5 * np.ones((nj, ni)))[None])
    scp2 = ref.get("scp2")[0][4:-4, 4:-4]
    w = masks["ip"][4:-4, 4:-4] > 0
    if case.nreg == 2:
        w = w.copy()
        w[-1, :] = False
    area = float(np.sum(scp2[w]))

    def setup(g):
        g.set("area", area)
        g.set("niwgf", 0.4)
        g.set("full_physics", 1)
    return setup, ["kfpla", "surflx", "ustar", "mtkepe", "sfl", "uml"]


def compare_owned(ref, tiles, lay, masks, names):
    """every field on the points some tile owns (the others are land no tile holds: left out) -- [(name, differing points)]"""
    from blom_amd.tiles import gather_interior_layout
    own = lay.owned()
    bad = []
    for nm in names:
        a = ref.get(nm)[:, 4:4 + lay.jtdm, 4:4 + lay.itdm]
        b = gather_interior_layout(tiles, lay, nm, fill=a)
        ok = np.isfinite(a) & (np.abs(a) < 1e30) & own[None]          # land keeps whatever pattern it had
        if not np.array_equal(a[ok], b[ok]):
            bad.append((nm, int((a[ok] != b[ok]).sum())))
    return bad


def run_threads(targets, timeout):
    th = [threading.Thread(target=f, daemon=True) for f in targets]
    [x.start() for x in th]
    [x.join(timeout=timeout) for x in th]
    assert not any(x.is_alive() for x in th), "a tile did not finish"
