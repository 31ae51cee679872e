"""The general tile table of xcspmd on the host (blom_amd/tiles.py: TileLayout), no library needed: the reference's own
ragged patch.input, land-tile elimination on the project's synthetic bathymetries, xcspmd's refusals."""
import os

import numpy as np
import pytest

from blom_amd import cases
from blom_amd.tiles import NBDY, TileLayout

HERE = os.path.dirname(os.path.abspath(__file__))


def one_based(row):
    return tuple((i0 + 1, ii) for i0, ii in row)


def test_reference_ragged_patch_input_round_trips(tmp_path):
    lay = TileLayout.from_patch_input(os.path.join(HERE, "golden", "tnx1v4_patch.input.32"))   # bld/tnx1v4/patch.input.32
    assert (lay.npx, lay.npy, lay.nranks) == (4, 8, 32) and not lay.is_tensor_product
    assert lay.rows[6] == ((15, 75), (90, 59), (246, 24), (270, 77))
    assert all(lay.rows[n] == ((0, 90), (90, 90), (180, 90), (270, 90)) for n in range(8) if n != 6)
    assert lay.jsizes == (48, 48, 48, 49, 48, 48, 48, 48)
    with pytest.raises(ValueError):
        lay.isizes
    dst = str(tmp_path / "patch.input")
    lay.write_patch_input(dst, 2)
    assert TileLayout.from_patch_input(dst) == lay
    assert lay.rank_tile(27) == (3, 6) and lay.tile_rank(2, 6) == 26 and lay.tile(2, 6) == (246, 289, 24, 48)


def _sea(name, idm, jdm):
    return cases._depth_for(name, idm, jdm, 1.0) > 0


def test_eliminate_land_on_tnx1v4s():
    sea = _sea("tnx1v4s", 360, 385)
    lay = TileLayout.eliminate_land(sea, 8, 4, 2)
    reg = TileLayout.regular(360, 385, 8, 4)
    assert one_based(lay.rows[2])[4:] == ((181, 20), (247, 24), (271, 45), (316, 45))
    assert lay.rows[0] == reg.rows[0] and lay.rows[1] == reg.rows[1]
    # the top row of the arctic grid stays untrimmed although its sea spans only part of tiles 5 and 6
    j0 = sum(lay.jsizes[:3])
    for px, want in ((4, (181, 28)), (5, (240, 31))):
        cols = np.flatnonzero(sea[j0:, reg.rows[3][px][0]:sum(reg.rows[3][px])].any(axis=0)) + reg.rows[3][px][0]
        assert (cols[0] + 1, cols[-1] - cols[0] + 1) == want
    assert lay.rows[3] == reg.rows[3]
    assert not (sea & ~lay.owned()).any()
    assert lay.nranks == 32 and [lay.rank_tile(r) for r in (0, 8, 21)] == [(0, 0), (0, 1), (5, 2)]


def test_eliminate_land_on_tnx2v1s():
    sea = _sea("tnx2v1s", 180, 193)
    lay = TileLayout.eliminate_land(sea, 6, 6, 2)
    reg = TileLayout.regular(180, 193, 6, 6)
    assert one_based(lay.rows[3]) == ((1, 27), (46, 15), (61, 30), (91, 10), (124, 27), (151, 30))
    assert [lay.rows[n] != reg.rows[n] for n in range(6)] == [False, False, True, True, True, False]
    assert not (sea & ~lay.owned()).any() and lay.nranks == 36
    # two tiles of a row are pulled apart by at least MIN_GAP >= nbdy land columns, or keep touching
    for row in lay.rows:
        live = [t for t in row if t[1]]
        for w, e in zip(live, live[1:]):
            assert e[0] == sum(w) or e[0] - sum(w) >= TileLayout.MIN_GAP >= NBDY


def test_eliminate_land_drops_all_land_tiles_and_skips_them_in_the_rank_numbering():
    sea = _sea("box_s", 24, 20)
    sea[6:20, 12:24] = False
    lay = TileLayout.eliminate_land(sea, 3, 2, 0)
    assert lay.rows == (((1, 7), (8, 8), (16, 7)), ((1, 7), (8, 4), (16, 0)))
    assert lay.nranks == 5 and lay.tile_rank(2, 1) == -1 and lay.rank_tile(4) == (1, 1)
    assert lay.tables()[1].tolist() == [7, 8, 7, 7, 4, 0]


@pytest.mark.parametrize("rows,jsizes,itdm,nreg,msg", [
    ((((0, 0), (10, 0)), ((0, 10), (10, 10))), (10, 10), 20, 0, "decomposition has an empty row"),
    ((((0, 10), (8, 12)),), (10,), 20, 0, "overlap or are out of order"),
    ((((0, 3), (10, 10)),), (10,), 20, 0, "narrower than nbdy"),
    ((((0, 5), (5, 5), (10, 5), (15, 5)), ((0, 5), (5, 4), (10, 5), (15, 5))), (10, 10), 20, 2, "arctic tiles are not the right size"),
    ((((0, 5), (5, 5), (10, 5), (15, 5)), ((0, 0), (5, 5), (10, 5), (15, 5))), (10, 10), 20, 2, "arctic empty tiles are not twins"),
])
def test_xcspmd_refusals(rows, jsizes, itdm, nreg, msg):
    with pytest.raises(ValueError, match=msg):
        TileLayout.from_rows(rows, jsizes, itdm, nreg=nreg)


def test_arctic_twin_empty_tiles_are_accepted_and_unowned_sea_is_refused():
    rows = (((0, 5), (5, 5), (10, 5), (15, 5)), ((0, 0), (5, 5), (10, 5), (15, 0)))
    lay = TileLayout.from_rows(rows, (10, 10), 20, nreg=2)
    assert lay.nranks == 6
    sea = np.zeros((20, 20), bool)
    sea[:, 5:15] = True
    lay.validate(2, sea)
    sea[15, 2] = True
    with pytest.raises(ValueError, match="owned by no tile"):
        lay.validate(2, sea)
