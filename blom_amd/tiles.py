"""2-D tile decomposition of a case in the reference's patch.input scheme (bld/blom_dimensions:104-148; xcspmd,
phy/mod_xc.F90:1332-1720): tile rows of heights jjpe(py), every row cut into tiles (ispt, iipe); tile (px,py) owns the global
points i0+1..i0+ii, j0+1..j0+jj.  A tile-local padded array is simply the window [j0 : j0+jj+8, i0 : i0+ii+8] of the global
padded array (local (i,j) <-> global (i0+i, j0+j)), halo included -- which is why a state scattered this way needs no halo
update before the first step.  `chain_crc` completes the decomposition-independent checksum xccrc (phy/mod_xc.F90:2195-2322)
from the strip CRCs of the tiles."""
import re
import zlib

import numpy as np

NBDY = 4


class TileLayout:
    """The tile table of xcspmd: npy tile rows of heights jj_pe(n) starting at j0_pe(n), every row cut into npx tiles
    (i0_pe(m,n), ii_pe(m,n)), ii_pe = 0 for a tile that land-tile elimination dropped.  Ranks number the non-empty tiles
    only, m fastest, then n (phy/mod_xc.F90:1545-1560).  `TileLayout(isizes, jsizes)` is the tensor-product case (every
    row cut into the same columns, no empty tile); `TileLayout.from_rows` takes the general table.  Indices are 0-based
    here: tile (px, py) owns the global points i0+1..i0+ii, j0+1..j0+jj."""

    def __init__(self, isizes, jsizes, rows=None, itdm=None):
        self._jsizes = tuple(int(v) for v in jsizes)
        if rows is None:
            isizes = tuple(int(v) for v in isizes)
            off = [int(sum(isizes[:k])) for k in range(len(isizes))]
            rows = tuple(tuple(zip(off, isizes)) for _ in self._jsizes)
            itdm = int(sum(isizes))
        self.rows = tuple(tuple((int(a), int(b)) for a, b in r) for r in rows)      # rows[py][px] = (i0, ii)
        self._itdm = int(itdm)
        self._ranks = {}
        self._tiles = []
        for py, r in enumerate(self.rows):
            for px, (_, ii) in enumerate(r):
                if ii > 0:
                    self._ranks[(px, py)] = len(self._tiles)
                    self._tiles.append((px, py))

    @classmethod
    def from_rows(cls, rows, jsizes, itdm, nreg=None, ip_mask=None):
        """the general table: rows[n] = ((i0, ii), ...) of tile row n (0-based i0; ii = 0: eliminated), jsizes the row
        heights, itdm the width of the domain.  With nreg the table is checked as xcspmd checks it (`validate`)."""
        lay = cls(None, jsizes, rows=rows, itdm=itdm)
        if nreg is not None:
            lay.validate(nreg, ip_mask)
        return lay

    def __eq__(self, other):
        return isinstance(other, TileLayout) and \
            (self.rows, self._jsizes, self._itdm) == (other.rows, other._jsizes, other._itdm)

    def __repr__(self):
        if self.is_tensor_product:
            return f"TileLayout(isizes={self.isizes}, jsizes={self.jsizes})"
        return f"TileLayout.from_rows({self.rows}, {self._jsizes}, {self._itdm})"

    @property
    def is_tensor_product(self):
        """every tile row cut into the same columns, which cover the domain without a gap, and no tile eliminated"""
        r0 = self.rows[0]
        if any(r != r0 for r in self.rows) or any(ii <= 0 for _, ii in r0):
            return False
        return r0[0][0] == 0 and all(r0[k][0] + r0[k][1] == r0[k + 1][0] for k in range(len(r0) - 1)) \
            and r0[-1][0] + r0[-1][1] == self._itdm

    @property
    def isizes(self):
        """widths of the tile columns (tensor-product layouts only: a ragged table has no such thing)"""
        if not self.is_tensor_product:
            raise ValueError("isizes: the tile rows are cut differently; read the table (rows) instead")
        return tuple(ii for _, ii in self.rows[0])

    @property
    def jsizes(self):
        return self._jsizes

    @property
    def npx(self):
        return len(self.rows[0])

    @property
    def npy(self):
        return len(self._jsizes)

    @property
    def itdm(self):
        return self._itdm

    @property
    def jtdm(self):
        return int(sum(self._jsizes))

    @property
    def nranks(self):
        """number of non-empty tiles"""
        return len(self._tiles)

    def tile(self, px, py):
        """(i0, j0, ii, jj) of tile (px, py)"""
        i0, ii = self.rows[py][px]
        return i0, int(sum(self._jsizes[:py])), ii, self._jsizes[py]

    def rank_tile(self, rank):
        """(px, py) of rank `rank`: the rank-th non-empty tile, m fastest (phy/mod_xc.F90:1545-1560); without eliminated
        tiles that is rank = px + npx*py"""
        return self._tiles[rank]

    def tile_rank(self, px, py):
        """rank of tile (px, py), -1 for an eliminated tile"""
        return self._ranks.get((px, py), -1)

    def tiles(self):
        """the non-empty tiles (px, py) in rank order"""
        return list(self._tiles)

    def window(self, a, px, py):
        i0, j0, ii, jj = self.tile(px, py)
        return np.ascontiguousarray(a[..., j0:j0 + jj + 2 * NBDY, i0:i0 + ii + 2 * NBDY])

    def tables(self):
        """(i0_pe, ii_pe, j0_pe, jj_pe) as the C entries take them: int32 arrays, i0_pe / ii_pe of npy*npx entries with
        m fastest, j0_pe / jj_pe of npy entries"""
        i0 = np.array([t[0] for r in self.rows for t in r], dtype=np.int32)
        ii = np.array([t[1] for r in self.rows for t in r], dtype=np.int32)
        jj = np.array(self._jsizes, dtype=np.int32)
        j0 = np.array([sum(self._jsizes[:k]) for k in range(self.npy)], dtype=np.int32)
        return i0, ii, j0, jj

    def owned(self):
        """bool (jtdm, itdm): the points some tile owns (all of them on a tensor-product layout)"""
        m = np.zeros((self.jtdm, self.itdm), dtype=bool)
        for px, py in self._tiles:
            i0, j0, ii, jj = self.tile(px, py)
            m[j0:j0 + jj, i0:i0 + ii] = True
        return m

    def validate(self, nreg, ip_mask=None):
        """The checks xcspmd makes on a table, with its messages (phy/mod_xc.F90:1470-1530), the ordering of a row's
        tiles its neighbour logic relies on (:1726-1745), and -- given the p-mask of the interior, (jtdm, itdm), sea > 0 --
        the one the reference leaves to its table generator: every sea point is owned by a tile."""
        npx, npy = self.npx, self.npy
        if any(len(r) != npx for r in self.rows) or len(self.rows) != npy:
            raise ValueError("xcspmd: every tile row needs the same number of tiles")
        if any(jj <= 0 for jj in self._jsizes):
            raise ValueError("xcspmd: decomposition has wrong jj_pe")
        for n, r in enumerate(self.rows):
            if max(ii for _, ii in r) <= 0:
                raise ValueError("xcspmd: decomposition has an empty row")
            end = 0
            for m, (i0, ii) in enumerate(r):
                if ii == 0:
                    continue
                if ii < NBDY:
                    raise ValueError(f"xcspmd: tile {m + 1},{n + 1} is narrower than nbdy = {NBDY}")
                if i0 < end:
                    raise ValueError(f"xcspmd: the tiles of row {n + 1} overlap or are out of order")
                end = i0 + ii
            if end > self._itdm:
                raise ValueError(f"xcspmd: row {n + 1} reaches beyond itdm = {self._itdm}")
        if nreg == 2 and npx > 1:
            top = self.rows[-1]
            for m, (i0, ii) in enumerate(top):
                if ii == 0:
                    if top[npx - 1 - m][1] != 0:
                        raise ValueError("xcspmd: arctic empty tiles are not twins")
                elif ii != self._itdm // npx or i0 != m * (self._itdm // npx):
                    raise ValueError("xcspmd: arctic tiles are not the right size")
            if npx % 2:
                raise ValueError("xcspmd (arctic) - ipr must be even")
        if ip_mask is not None:
            sea = np.asarray(ip_mask) > 0
            if sea.shape != (self.jtdm, self._itdm):
                raise ValueError(f"p-mask of shape {sea.shape}, domain is {(self.jtdm, self._itdm)}")
            lost = sea & ~self.owned()
            if lost.any():
                j, i = np.argwhere(lost)[0]
                raise ValueError(f"tile table: {int(lost.sum())} sea points are owned by no tile "
                                 f"(first: i = {i + 1}, j = {j + 1})")
        return self

    def corner_contacts(self, ip_mask, nreg):
        """[(px, py, side, sea points)]: the corner pieces of a tile's halo -- nbdy columns beyond an edge without a
        touching neighbour, nbdy rows below / above the tile -- that hold sea.  The reference's exchange brings corners
        with the E-W strips only (phy/mod_xc.F90:3131-3178), so there it writes vland where the undivided domain holds the
        sea of a tile that touches this one diagonally.  A property of the reference's rule: on such a
        table a run need not reproduce the single tile bit for bit."""
        sea = np.asarray(ip_mask) > 0
        jtdm, itdm = sea.shape
        per_i = nreg not in (0, 4)
        out = []
        for px, py in self._tiles:
            i0, j0, ii, jj = self.tile(px, py)
            live = [t for t in self.rows[py] if t[1] > 0]
            wraps = per_i and live[0][0] == 0 and sum(live[-1]) == itdm
            sides = (("W", any(sum(t) == i0 for t in live) or (wraps and i0 == 0), range(i0 - NBDY, i0)),
                     ("E", any(t[0] == i0 + ii for t in live) or (wraps and i0 + ii == itdm), range(i0 + ii, i0 + ii + NBDY)))
            for side, touching, cols in sides:
                if touching:
                    continue
                cols = [c % itdm for c in cols] if per_i else [c for c in cols if 0 <= c < itdm]
                rows = [r for r in list(range(j0 - NBDY, j0)) + list(range(j0 + jj, j0 + jj + NBDY)) if 0 <= r < jtdm]
                n = int(sea[np.ix_(rows, cols)].sum()) if rows and cols else 0
                if n:
                    out.append((px, py, side, n))
        return out

    @staticmethod
    def split(n, parts):
        """sizes of `parts` tiles covering n points the way bld/blom_dimensions cuts them: the first tiles one longer"""
        q, r = divmod(n, parts)
        return tuple(q + (1 if k < r else 0) for k in range(parts))

    @classmethod
    def regular(cls, idm, jdm, npx, npy):
        return cls(cls.split(idm, npx), cls.split(jdm, npy))

    # eliminate_land pulls two neighbours of a row apart only by at least this many land columns: then a halo (nbdy) never
    # reaches across the gap, and no 9-column strip of xcsum / xccrc holds sea of both ("Ragged tile tables")
    MIN_GAP = 2 * NBDY

    @classmethod
    def eliminate_land(cls, ip_mask, npx, npy, nreg):
        """Land-tile elimination for the p-mask `ip_mask` of the interior, (jtdm, itdm), sea > 0: regular(itdm, jtdm, npx,
        npy) with every tile shrunk in i to the first..last column that holds a sea point in its rows, and tiles without
        sea dropped.  The top row of an arctic grid (nreg = 2) is not trimmed (the fold pairs equal tiles) and loses twin
        pairs only.  A tile is not shrunk below nbdy columns, and two neighbours are not pulled apart by fewer than
        MIN_GAP columns: they keep their common edge instead."""
        sea = np.asarray(ip_mask) > 0
        jtdm, itdm = sea.shape
        reg = cls.regular(itdm, jtdm, npx, npy)
        rows = []
        for py in range(npy):
            row = []                                                     # [i0, ii, regular i0, regular ii]
            for px in range(npx):
                i0, j0, ii, jj = reg.tile(px, py)
                cols = np.flatnonzero(sea[j0:j0 + jj, i0:i0 + ii].any(axis=0))
                if cols.size == 0:
                    row.append([i0, 0, i0, ii])
                    continue
                a, b = i0 + int(cols[0]), i0 + int(cols[-1]) + 1          # [a, b)
                if b - a < NBDY:                                         # widen inside the regular tile
                    a = max(i0, min(a, i0 + ii - NBDY))
                    b = a + NBDY
                row.append([a, b - a, i0, ii])
            if nreg == 2 and py == npy - 1:
                for t, twin in zip(row, [list(x) for x in reversed(row)]):
                    t[:2] = [t[2], 0] if t[1] == 0 and twin[1] == 0 else [t[2], t[3]]
            else:
                for px in range(npx - 1):                                # a gap narrower than MIN_GAP: keep the common edge
                    w, e = row[px], row[px + 1]
                    if w[1] and e[1] and 0 < e[0] - (w[0] + w[1]) < cls.MIN_GAP:
                        edge, e_end = e[2], e[0] + e[1]
                        w[1] = edge - w[0]
                        e[0], e[1] = edge, e_end - edge
            rows.append(tuple((t[0], t[1]) for t in row))
        return cls.from_rows(rows, reg.jsizes, itdm, nreg=nreg, ip_mask=sea)

    @classmethod
    def from_patch_input(cls, path, nreg=None):
        """the tile table of a reference patch.input file (the format xcspmd reads, phy/mod_xc.F90:1405-1430): ispt / iipe
        of every tile row, jspt / jjpe of the first tile column; ragged rows and eliminated tiles (iipe = 0) included.
        The table is checked (`validate`) with the nreg of the file's header, or the one given."""
        txt = open(path).read()
        head = None
        for line in txt.splitlines():
            w = line.split()
            if len(w) >= 8 and all(re.fullmatch(r"-?\d+", x) for x in w[:8]):
                head = [int(x) for x in w[:8]]
                break
        if head is None:
            raise ValueError(f"{path}: no header line (npes npe mpe idm jdm ibig jbig nreg)")
        npes, npx, npy, itdm, jtdm, _, _, nreg_file = head

        def table(name):
            return {int(m.group(1)): [int(x) for x in m.group(2).split()]
                    for m in re.finditer(name + r"\(\s*(\d+)\)\s*=\s*([\d\s]+)", txt)}
        ispt, iipe, jspt, jjpe = table("ispt"), table("iipe"), table("jspt"), table("jjpe")
        if sorted(iipe) != list(range(1, npy + 1)) or sorted(ispt) != sorted(iipe) or 1 not in jjpe or 1 not in jspt:
            raise ValueError(f"{path}: the tables do not list {npy} tile rows")
        if any(len(iipe[n]) != npx or len(ispt[n]) != npx for n in iipe) or len(jjpe[1]) != npy or len(jspt[1]) != npy:
            raise ValueError(f"{path}: the tables do not list {npx} x {npy} tiles")
        if jspt[1][0] != 1:
            raise ValueError("xcspmd: decomposition has wrong j0_pe")
        if [v - 1 for v in jspt[1]] != [sum(jjpe[1][:k]) for k in range(npy)]:
            raise ValueError("xcspmd: decomposition is non-contiguous")
        if sum(jjpe[1]) != jtdm:
            raise ValueError("xcspmd: decomposition has wrong jj_pe")
        rows = [tuple((max(ispt[n][m] - 1, 0), iipe[n][m]) for m in range(npx)) for n in range(1, npy + 1)]
        lay = cls.from_rows(rows, jjpe[1], itdm, nreg=nreg_file if nreg is None else nreg)
        if lay.nranks != npes:
            raise ValueError("xcspmd: wrong number of sea tiles")
        return lay

    def write_patch_input(self, path, nreg):
        """this layout as a reference patch.input file (the format xcspmd reads, phy/mod_xc.F90:1405-1430): the header line
        npes npe mpe idm jdm ibig jbig nreg, then ispt / iipe of every tile row, then jspt / jjpe"""
        jspt = [1 + sum(self._jsizes[:k]) for k in range(self.npy)]
        ibig = max(ii for r in self.rows for _, ii in r)
        head = (self.nranks, self.npx, self.npy, self.itdm, self.jtdm, ibig, max(self._jsizes), nreg)
        lines = ["".join(f"{h:>6}" for h in ("npes", "npe", "mpe", "idm", "jdm", "ibig", "jbig", "nreg")),
                 "".join(f"{int(v):6d}" for v in head), ""]
        for n in range(self.npy):
            lines.append(f"ispt({n + 1:3d}) = " + "".join(f"{i0 + 1:6d}" for i0, _ in self.rows[n]))
            lines.append(f"iipe({n + 1:3d}) = " + "".join(f"{ii:6d}" for _, ii in self.rows[n]))
        lines += ["", "jspt(  1) = " + "".join(f"{v:6d}" for v in jspt),
                  "jjpe(  1) = " + "".join(f"{int(v):6d}" for v in self._jsizes)]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def tile_extents(case, npx, npy):
    assert case.idm % npx == 0 and case.jdm % npy == 0, "uniform tiles only"
    return case.idm // npx, case.jdm // npy


def tile_window(a, case, npx, npy, px, py):
    ii, jj = tile_extents(case, npx, npy)
    i0, j0 = px * ii, py * jj
    return np.ascontiguousarray(a[..., j0:j0 + jj + 8, i0:i0 + ii + 8])


def scatter_state(src, tiles, case, npx, npy, fields):
    """Copy `fields` of the single-tile backend `src` into the tile backends (dict (px,py)->backend)."""
    for nm in fields:
        try:
            a = src.get(nm)
        except KeyError:
            continue
        for (px, py), t in tiles.items():
            if t.has_field(nm):
                t.put(nm, tile_window(a, case, npx, npy, px, py))


def scatter_to_tile(src, tile, layout, px, py, fields=None, skip=("mpack",)):
    """Copy every field (default: all the library registers) of the whole-domain backend `src` into tile (px,py)."""
    for nm in (fields or src.field_names()):
        if nm in skip or nm.startswith("wkp"):
            continue
        tile.put(nm, layout.window(src.get(nm), px, py))


def gather_interior(tiles, case, npx, npy, name):
    """Assemble the global interior (nlev, jdm, idm) of field `name` from the tiles."""
    ii, jj = tile_extents(case, npx, npy)
    out = None
    for (px, py), t in tiles.items():
        a = t.get(name)
        if out is None:
            out = np.zeros((a.shape[0], case.jdm, case.idm), a.dtype)
        out[:, py * jj:(py + 1) * jj, px * ii:(px + 1) * ii] = a[:, 4:4 + jj, 4:4 + ii]
    return out


def gather_interior_layout(tiles, layout, name, fill=None):
    """Assemble the global interior (nlev, jtdm, itdm) of field `name` from the tiles.  Points no tile owns (a ragged
    layout: land between and beside the tiles, `~layout.owned()`) are taken from `fill`, an array of the same interior
    shape -- the source's own values, so that a comparison with it leaves them out -- or stay zero."""
    out = None
    for (px, py), t in tiles.items():
        i0, j0, ii, jj = layout.tile(px, py)
        a = t.get(name)
        if out is None:
            out = np.zeros((a.shape[0], layout.jtdm, layout.itdm), a.dtype)
            if fill is not None:
                out[...] = fill
        out[:, j0:j0 + jj, i0:i0 + ii] = a[:, 4:4 + jj, 4:4 + ii]
    return out


def chain_crc(parts, layout):
    """xccrc of the whole domain from the tiles' strip CRCs.  parts[(px,py)] = (l0, strips[jj, ns]) as returned by
    BlomGpu.crc_strips: a row's CRC chains its strips in global order, the result chains the rows in global order
    (phy/mod_xc.F90:2262-2300).  A strip no tile owns lies in the land of a ragged layout: its CRC is that of no wet
    point, 0, and it is chained like the others."""
    ntot = (layout.itdm + 2 * NBDY) // (2 * NBDY + 1)
    rows = []
    for py in range(layout.npy):
        jj = layout.jsizes[py]
        table = np.zeros((jj, ntot), dtype="<u4")
        for px in range(layout.npx):
            if layout.tile_rank(px, py) < 0:
                continue
            l0, strips = parts[(px, py)]
            table[:, l0:l0 + strips.shape[1]] = strips
        for j in range(jj):
            crc8 = 0
            for v in table[j]:
                crc8 = zlib.crc32(np.array([v], dtype="<u4").tobytes(), crc8)
            rows.append(crc8)
    return zlib.crc32(np.array(rows, dtype="<u4").tobytes()) & 0xFFFFFFFF


def make_barotp_global(src, case, masks, device=0):
    """The second context of an RCCL tile that solves the whole 2-D barotropic domain (blomgpu_rccl_attach_barotp_global):
    global dimensions, kdm = 3 (it holds 2-D fields only), no tracers, the global masks, and every 2-D field of the
    whole-domain backend `src` (grid metrics, the barotropic state at start).  Points no tile of a ragged layout owns keep
    these values -- they are land."""
    from .gpu import BlomGpu
    g = BlomGpu(case.idm, case.jdm, 3, 0, case.nreg, masks, device=device)
    for nm in src.field_names():
        if nm == "mpack" or nm.startswith("wkp") or nm in masks:
            continue
        nlev, isint = src.field_info(nm)
        if nlev <= 3 and not isint and g.has_field(nm) and g.field_info(nm)[0] == nlev:
            g.put(nm, src.get(nm))
    return g
