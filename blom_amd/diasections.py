"""The two text tables that the reference's diamer and diasec read at their first call, for BlomGpu.dia_set_mertra and
BlomGpu.dia_set_sections: readers that follow the reference's own read statements, and writers for both.

The index file of the meridional sections (mer_mifile, phy/mod_dia.F90:4045-4095).  Every line is read into 20 characters
(`read(nfu,'(a)') c20`), so nothing behind column 20 counts.  A header line starts with `Section`; columns 9-15 are the section's
latitude, read with f7.3, columns 16-20 the number of point lines that follow.  A point line holds `i j uflg vflg`, list-directed.

The file of the named sections (sec_sifile, :3838-3866).  Lines of up to 120 characters; one that starts with `Name` opens a section
whose name is columns 7-120, and the section whose line holds `equatorial_undercurrent` takes the upper-350 m sums; every other
line holds `i j usi vsi` of the section that is open.

ocean_regions.nc (mer_orfile) is not read here: the region array is the caller's.
"""
import numpy as np


class SectionFileError(ValueError):
    pass


def _f73(field, where):
    """a field read with f7.3: blanks do not count; without a decimal point the last three digits are the fraction"""
    s = field.replace(" ", "")
    if not s:
        return 0.0
    try:
        if any(ch in s for ch in ".eEdD"):
            return float(s.replace("d", "e").replace("D", "e"))
        return int(s) / 1000.0
    except ValueError:
        raise SectionFileError(f"{where}: latitude field {field!r} is not a number") from None


def _ints(text, n, where):
    """list-directed read of n integers: blanks or commas separate, a slash ends the list, what follows the n-th is not looked at"""
    out = []
    for tok in text.split("/")[0].replace(",", " ").split():
        try:
            out.append(int(tok))
        except ValueError:
            raise SectionFileError(f"{where}: {tok!r} is not an integer") from None
        if len(out) == n:
            return out
    raise SectionFileError(f"{where}: {n} integers expected, {len(out)} found")


def _check_range(i, j, itdm, jtdm, where):
    if itdm is not None and not (1 <= i <= itdm and 1 <= j <= jtdm):
        raise SectionFileError(f"{where}: indices out of range! i = {i} itdm = {itdm} j = {j} jtdm = {jtdm}")


def read_metra_index(path, itdm=None, jtdm=None):
    """-> mtlat (lmax,) float64, nind (lmax,) int32, pts (sum nind, 4) int32 = (i, j, uflg, vflg), every point of the file (the filter
    on the ocean regions is filter_ocean_points's, and the library applies the same).  With itdm, jtdm an index outside the domain
    raises, as do a line that is not a header where one is due (:4057) and a section with fewer point lines than its header says (:4065)."""
    mtlat, nind, pts = [], [], []
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f]
    k = 0
    while k < len(lines):
        c20 = lines[k][:20].ljust(20)
        where = f"{path}:{k + 1}"
        k += 1
        if c20[:7] != "Section":
            raise SectionFileError(f"{where}: problem in the section index: a line that starts with 'Section' expected, found {c20.rstrip()!r}")
        lat = _f73(c20[8:15], where)
        count = c20[15:20].replace(" ", "")
        try:
            n = int(count) if count else 0
        except ValueError:
            raise SectionFileError(f"{where}: point count {c20[15:20]!r} is not an integer") from None
        if n < 0:
            raise SectionFileError(f"{where}: negative point count")
        for _ in range(n):
            if k >= len(lines):
                raise SectionFileError(f"{path}: section too short? section {len(mtlat) + 1} announces {n} points")
            i, j, u, v = _ints(lines[k][:20], 4, f"{path}:{k + 1}")
            _check_range(i, j, itdm, jtdm, f"{path}:{k + 1}")
            pts.append((i, j, u, v))
            k += 1
        mtlat.append(lat)
        nind.append(n)
    if itdm is not None and len(mtlat) > itdm + jtdm:
        raise SectionFileError(f"{path}: too many or too long sections! {len(mtlat)} > itdm+jtdm = {itdm + jtdm}")
    return np.array(mtlat, np.float64), np.array(nind, np.int32), np.array(pts, np.int32).reshape(-1, 4)


def filter_ocean_points(nind, pts, oflg):
    """the points diamer keeps (:4070): those whose ocean region flag oflg[j-1, i-1] is positive.  -> nind, pts of the kept points"""
    oflg = np.asarray(oflg)
    pts = np.asarray(pts, np.int32).reshape(-1, 4)
    keep = oflg[pts[:, 1] - 1, pts[:, 0] - 1] > 0
    sec = np.repeat(np.arange(len(nind)), np.asarray(nind))
    return np.bincount(sec[keep], minlength=len(nind)).astype(np.int32), pts[keep]


def write_metra_index(path, mtlat, nind, pts):
    pts = np.asarray(pts).reshape(-1, 4)
    if int(np.sum(nind)) != pts.shape[0]:
        raise ValueError("write_metra_index: the counts do not add up to the points")
    k = 0
    with open(path, "w") as f:
        for lat, n in zip(mtlat, nind):
            head = "Section %7.3f%5d" % (lat, n)
            if len(head) != 20:
                raise ValueError(f"write_metra_index: latitude {lat} or count {n} does not fit its field")
            f.write(head + "\n")
            for i, j, u, v in pts[k:k + n]:
                line = "%5d%5d%3d%3d" % (i, j, u, v)
                if len(line) > 20:
                    raise ValueError(f"write_metra_index: point {(i, j, u, v)} does not fit 20 columns")
                f.write(line + "\n")
            k += n


def read_section_index(path, itdm=None, jtdm=None):
    """-> names (list), nsi (sec_num,) int32, pts (sum nsi, 4) int32 = (i, j, usi, vsi), equat_sec (1-based, -1: none)"""
    names, nsi, pts, equat = [], [], [], -1
    with open(path) as f:
        for k, ln in enumerate(f):
            c120 = ln.rstrip("\n")[:120]
            where = f"{path}:{k + 1}"
            if c120[:4] == "Name":
                names.append(c120[6:].rstrip())
                nsi.append(0)
                if "equatorial_undercurrent" in c120:
                    equat = len(names)
            else:
                if not names:
                    raise SectionFileError(f"{where}: a point line in front of the first 'Name' line")
                i, j, u, v = _ints(c120, 4, where)
                _check_range(i, j, itdm, jtdm, where)
                pts.append((i, j, u, v))
                nsi[-1] += 1
    return names, np.array(nsi, np.int32), np.array(pts, np.int32).reshape(-1, 4), equat


def write_section_index(path, names, nsi, pts):
    pts = np.asarray(pts).reshape(-1, 4)
    if int(np.sum(nsi)) != pts.shape[0] or len(names) != len(nsi):
        raise ValueError("write_section_index: the counts do not add up to the points")
    k = 0
    with open(path, "w") as f:
        for name, n in zip(names, nsi):
            f.write("Name: %s\n" % name)
            for i, j, u, v in pts[k:k + n]:
                f.write("%6d%6d%4d%4d\n" % (i, j, u, v))
            k += n
