"""Ragged tile tables (land-tile elimination, phy/mod_xc.F90:1332-1990) through the library's RCCL transport on the CPU:
every non-empty tile of a land-eliminated layout is an emulated rank (tests/hostemu: the library's own sources compiled
for the host, RCCL replaced by mailboxes between threads) running the real blomgpu_rccl_init_table / segment pack /
ncclSend+Recv / unpack code of blom_amd/csrc/comm_rccl.hip.  Requirement: after 3 steps every field of CHECK equals the
single tile's on the points some tile owns, and blomgpu_rccl_crc on every rank equals the single tile's checksum.  Also:
the in-process group (halo.hip) and the RCCL ranks leave identical halos on a hand-written table whose gap is narrower
than the halo, and a tensor-product table through the new entries leaves the bits of the old ones."""
import os
import threading

import numpy as np
import pytest

import ragged_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
pytestmark = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    old = g.LIB_PATH
    g.LIB_PATH = EMU
    yield
    g.LIB_PATH = old


def _run_ranks(case, masks, ref, lay, nsteps=3, bt_global=False, setup=None, table_entries=True, final_halo=None):
    """one emulated rank per non-empty tile; returns (tiles, {rank: {field: rccl_crc}})"""
    from blom_amd.gpu import rccl_unique_id
    from blom_amd.tiles import make_barotp_global
    assert lay.nranks <= 8
    uid = rccl_unique_id()
    tiles, errs, crcs = {}, [], {}
    crc_fields = [("dp", 1, 2 * case.kdm, 1), ("u", 1, 2 * case.kdm, 3), ("v", 1, 2 * case.kdm, 4), ("pb", 1, 2, 1)]
    lock = threading.Lock()
    barrier = threading.Barrier(lay.nranks)

    def rank_main(rank):
        try:
            px, py = lay.rank_tile(rank)
            with lock:                                    # the whole-domain backend is shared: read it one rank at a time
                t = rc.new_tile(case, masks, ref, lay, px, py)
                glob = make_barotp_global(ref, case, masks) if bt_global else None
            if table_entries:
                t.rccl_init_layout(uid, rank, lay)
                if bt_global:
                    t.rccl_attach_barotp_layout(glob, lay)
            else:
                t.rccl_init_2d(uid, rank, lay.npx, lay.npy)
                if bt_global:
                    t.rccl_attach_barotp_global(glob, lay.isizes, lay.jsizes)
            with lock:
                tiles[(px, py)] = t
            barrier.wait()
            if setup:
                setup(t)
            assert t.step(0, nsteps) == nsteps
            if final_halo:
                final_halo(t)
            t.sync()
            crcs[rank] = {f[0]: t.rccl_crc(*f) for f in crc_fields}
        except Exception as e:                            # a failing rank would leave the others waiting
            errs.append(e)
            barrier.abort()

    rc.run_threads([lambda r=r: rank_main(r) for r in range(lay.nranks)], 600)
    assert not errs, errs
    return tiles, crcs, crc_fields


def _close(tiles, ref):
    for t in tiles.values():
        t.rccl_finalize()
        t.close()
    ref.close()


def _check_case(name, bt_global=False, full=False, nsteps=3):
    case, masks, ref, lay = rc.build(name)
    setup, check = None, list(rc.CHECK)
    if full:
        setup, extra = rc.full_physics(ref, case, masks)
        check += extra
    tiles, crcs, crc_fields = _run_ranks(case, masks, ref, lay, nsteps, bt_global, setup)
    if setup:
        setup(ref)
    assert ref.step(0, nsteps) == nsteps
    bad = rc.compare_owned(ref, tiles, lay, masks, check)
    want = {f[0]: ref.crc(*f) for f in crc_fields}
    crc_bad = [(r, nm, hex(v), hex(want[nm])) for r, d in crcs.items() for nm, v in d.items() if v != want[nm]]
    _close(tiles, ref)
    assert not bad, bad
    assert len(crcs) == lay.nranks and not crc_bad, crc_bad


@pytest.mark.parametrize("bt_global", [False, True], ids=["decomposed_barotp", "replicated_barotp"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_ragged_rccl_ranks_match_single_tile(emu_lib, name, bt_global):
    _check_case(name, bt_global=bt_global)


@pytest.mark.parametrize("name", ["tri_4x2_trimmed_row_under_arctic_row", "box_3x2_one_tile_eliminated"])
def test_ragged_rccl_ranks_with_the_full_physics_step(emu_lib, name):
    """thermf's two global sums (xcsum) are formed on the replicated solve's global context, which the tiles fill by the table"""
    _check_case(name, bt_global=True, full=True)


def test_tensor_product_table_through_the_new_entries_leaves_the_same_bits(emu_lib):
    """blomgpu_rccl_init_table / blomgpu_rccl_attach_barotp_table given a tensor-product layout are the old entries"""
    from blom_amd.tiles import TileLayout
    from test_gpu_tiles import _single
    got = {}
    for new in (False, True):
        case, masks, fields, ref = _single("chan_s", 3)
        lay = TileLayout((7, 7, 6), (13, 11))
        tiles, crcs, _ = _run_ranks(case, masks, ref, lay, 3, True, None, table_entries=new)
        got[new] = ({k: {nm: t.get(nm) for nm in ("dp", "temp", "u", "pb")} for k, t in tiles.items()}, crcs)
        _close(tiles, ref)
    assert got[False][1] == got[True][1]
    for k, d in got[False][0].items():
        for nm, a in d.items():
            assert np.array_equal(a, got[True][0][k][nm], equal_nan=True), (k, nm)


def _narrow_gap_layout():
    """chan_s 20 x 24 with two land columns (9, 10) in the northern half, as a table written by hand: the northern row is cut
    into (0,8) and (10,10) -- a gap of 2 columns, narrower than the halo, so each tile's halo would reach the other's sea"""
    from blom_amd.tiles import TileLayout

    def carve(d):
        d[12:24, 8:10] = 0.0
    lay = TileLayout.from_rows((((0, 10), (10, 10)), ((0, 8), (10, 10))), (12, 12), 20, nreg=1)
    return carve, lay


def test_narrow_gap_both_transports_leave_identical_halos(emu_lib):
    """Check 4 of the ragged-layout work: the in-process gather must apply the reference's touching rule, not read through a
    gap.  Whole padded arrays of dp, temp, u, tile by tile, after 3 steps through either transport and one last halo update
    of the three fields over the full halo width.  That last update is needed for the comparison to mean anything: the
    step itself does not leave the two transports' halos alike even on a tensor-product table through the unchanged paths
    (chan_s as 2 x 2 after one step: the E/W halo columns of u, v, dp, pb differ, e.g. 954 points of u in tile (0,0)),
    because they schedule their exchanges differently (overlapped and batched over RCCL); the interiors are the same."""
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    from blom_amd.gpu import BlomGpu, TileGroup
    carve, lay = _narrow_gap_layout()
    assert lay.rows[1][1][0] - sum(lay.rows[1][0]) == 2 and not lay.is_tensor_product
    res = {}

    def final_halo(t):
        for nm, itype in (("dp", 1), ("temp", 1), ("u", 3)):
            t.xctilr(nm, 1, 1, t.field_info(nm)[0], 4, 4, itype)
    for transport in ("rccl", "group"):
        case = make_case("chan_s", carve=carve)
        nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm)
        masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
        lay.validate(nreg, ip[4:-4, 4:-4])
        ref = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
        hostinit.init_state(ref, case)
        if transport == "rccl":
            tiles, _, _ = _run_ranks(case, masks, ref, lay, 3, final_halo=final_halo)
        else:
            grp = TileGroup.for_layout(lay)
            tiles, errs = {}, []
            for px, py in lay.tiles():
                tiles[(px, py)] = rc.new_tile(case, masks, ref, lay, px, py)
                grp.attach(tiles[(px, py)], px, py)

            def run(t):
                try:
                    t.step(0, 3)
                    final_halo(t)
                    t.sync()
                except Exception as e:
                    errs.append(e)
            rc.run_threads([lambda t=t: run(t) for t in tiles.values()], 600)
            assert not errs, errs
        res[transport] = {k: {nm: t.get(nm) for nm in ("dp", "temp", "u")} for k, t in tiles.items()}
        if transport == "rccl":
            _close(tiles, ref)
        else:
            for t in tiles.values():
                t.close()
            ref.close()
            grp.destroy()
    bad = [(k, nm) for k, d in res["rccl"].items() for nm, a in d.items()
           if not np.array_equal(a, res["group"][k][nm], equal_nan=True)]
    assert len(res["rccl"]) == 4 and not bad, bad
