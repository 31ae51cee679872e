"""The end of blom_step restated in numpy, for the checks of tests/test_gpu_stepend.py: step_time (phy/mod_time.F90:182-219), iniswa's
table build and its two constant methods (phy/mod_swabs.F90:216-271, :407-441), updswa (:611-732), fwbbal (phy/mod_forcing.F90:361-441)
and the first hit of chkvar in the serial reference's loop order with its line (phy/mod_chkvar.F90:77-141).  Every operation in the
reference's order and association (numpy does not contract; max / min are `a > b ? a : b` / `a < b ? a : b` as amdflang lowers them).
log10 and 10**x come from the C library, element by element (math.log10, math.pow: the reference's compiler calls log10 and pow).  The
constants are written out here once more, from the papers the reference cites, so that a slip in the library's table shows.

`seen` counts the points that take each branch of updswa -- clamped below, clamped above, inside; for chlorophyll_ohl03 the lookup
indices: the lowest reachable one (101: the clamp at -2 lies 100 table steps above log10 of Table 1a's first entry, so the indices
1..100 cannot occur), 401, and those between -- and the tests assert on it."""
import math

import numpy as np

from thermf_cesm_ref import NBDY, fmax, fmin, intp1d, owned, xcsum

METHODS = ("top-layer", "jerlov", "chlorophyll_ma94", "chlorophyll_ohl03", "spatial_frac_attlen")
BANDS = ("swfc1", "swfc2", "swal1", "swal2")
# Paulson and Simpson (1977), Jerlov (1968) water types I, IA, IB, II, III
PS77_IRFC = (.58, .62, .67, .77, .78)
PS77_AL1 = (.35, .60, 1.00, 1.50, 1.40)
PS77_AL2 = (23.00, 20.00, 17.00, 14.00, 7.90)
# Morel and Antoine (1994) as modified; the infrared fraction of Sweeney et al. (2005)
MA94_IRFC = .43
MA94_V2 = (.679, -.008, -.132, -.038, .017, .007)
MA94_Z1 = (1.540, -.197, .166, -.252, -.055, .042)
MA94_Z2 = (7.925, -6.644, 3.662, -1.815, -.218, .502)
# Ohlmann (2003), Table 1a
CHL_TAB1A = (.001, .005, .01, .02, .03, .05, .10, .15, .20, .25, .30, .35, .40, .45, .50, .60, .70, .80, .90, 1.00, 1.50, 2.00, 2.50, 3.00,
             4.00, 5.00, 6.00, 7.00, 8.00, 9.00, 10.00)
A1_TAB1A = (0.4421, 0.4451, 0.4488, 0.4563, 0.4622, 0.4715, 0.4877, 0.4993, 0.5084, 0.5159, 0.5223, 0.5278, 0.5326, 0.5369, 0.5408, 0.5474,
            0.5529, 0.5576, 0.5615, 0.5649, 0.5757, 0.5802, 0.5808, 0.5788, 0.56965, 0.55638, 0.54091, 0.52442, 0.50766, 0.49110, 0.47505)
A2_TAB1A = (0.2981, 0.2963, 0.2940, 0.2894, 0.2858, 0.2800, 0.2703, 0.2628, 0.2571, 0.2523, 0.2481, 0.2444, 0.2411, 0.2382, 0.2356, 0.2309,
            0.2269, 0.2235, 0.2206, 0.2181, 0.2106, 0.2089, 0.2113, 0.2167, 0.23357, 0.25504, 0.27829, 0.30274, 0.32698, 0.35056, 0.37303)
B1_TAB1A = (0.0287, 0.0301, 0.0319, 0.0355, 0.0384, 0.0434, 0.0532, 0.0612, 0.0681, 0.0743, 0.0800, 0.0853, 0.0902, 0.0949, 0.0993, 0.1077,
            0.1154, 0.1227, 0.1294, 0.1359, 0.1640, 0.1876, 0.2082, 0.2264, 0.25808, 0.28498, 0.30844, 0.32932, 0.34817, 0.36540, 0.38132)
B2_TAB1A = (0.3192, 0.3243, 0.3306, 0.3433, 0.3537, 0.3705, 0.4031, 0.4262, 0.4456, 0.4621, 0.4763, 0.4889, 0.4999, 0.5100, 0.5191, 0.5347,
            0.5477, 0.5588, 0.5682, 0.5764, 0.6042, 0.6206, 0.6324, 0.6425, 0.66172, 0.68144, 0.70086, 0.72144, 0.74178, 0.76190, 0.78155)
NVAL_LUT = 401
CHL10_MIN, CHL10_MAX = -2.0, 1.0
LOWEST_INDEX = 101


# ---- step_time -------------------------------------------------------------------------------------------------------------------------
def step_time(clock, ns1):
    """clock: dict(nday_of_year, nstep_in_day, nday_in_year); ns1: the incremented step number.  Returns the clock after the step with
    xmi and lmi = (l1mi .. l5mi), :193-217"""
    sd, nd = clock["nstep_in_day"], clock["nday_in_year"]
    day = clock["nday_of_year"]
    if ns1 % sd == 0:
        day = day % nd + 1
    xmi = (float(day - 1) + float(ns1 % sd) / float(sd)) * 12.0 / float(nd)
    l3 = int(xmi) + 1
    xmi = xmi - float(l3 - 1)
    lmi = ((l3 + 9) % 12 + 1, (l3 + 10) % 12 + 1, l3, l3 % 12 + 1, (l3 + 1) % 12 + 1)
    return dict(clock, nday_of_year=day, xmi=xmi, lmi=lmi)


# ---- iniswa ------------------------------------------------------------------------------------------------------------------------------
def ohl03_tables():
    """a1_lut a2_lut b1_lut b2_lut (401 each), log10chl_min, dlog10chl: :407-441"""
    lo = math.log10(CHL_TAB1A[0])
    hi = math.log10(CHL_TAB1A[-1])
    d = (hi - lo) / float(NVAL_LUT - 1)
    lut = np.zeros((4, NVAL_LUT))
    m = 2
    for n in range(1, NVAL_LUT + 1):
        chl = math.pow(10.0, lo + float(n - 1) * d)
        chl = max(CHL_TAB1A[0], min(chl, CHL_TAB1A[-1]))
        while chl > CHL_TAB1A[m - 1]:
            m += 1
        w2 = (chl - CHL_TAB1A[m - 2]) / (CHL_TAB1A[m - 1] - CHL_TAB1A[m - 2])
        w1 = 1.0 - w2
        for r, tab in enumerate((A1_TAB1A, A2_TAB1A, B1_TAB1A, B2_TAB1A)):
            lut[r, n - 1] = w1 * tab[m - 2] + w2 * tab[m - 1]
    return lut, lo, d


def log10_chl(chl):
    """iniswa's conversion, :391-402, element by element from the C library"""
    a = np.array(chl, dtype=np.float64)
    flat = a.reshape(-1)
    for q in range(flat.size):
        flat[q] = math.log10(flat[q])
    return a


def iniswa_constant(s, method, sel, jwtype=1, swamxd=200.0):
    """'top-layer' (:229-245) and 'jerlov' (:247-271) on the four planes of s at the points sel"""
    if method == "top-layer":
        v = (0.0, 0.0, swamxd, swamxd)
    else:
        w = jwtype - 1
        v = (PS77_IRFC[w], 1.0 - PS77_IRFC[w], PS77_AL1[w], PS77_AL2[w])
    for nm, x in zip(BANDS, v):
        s[nm][0][sel] = x


def synthetic_chl(nj, ni, i0=0, j0=0, itdm=None, jtdm=None):
    """a smooth monthly chlorophyll concentration from about 0.005 to 30 mg m-3 (log10 from below -2 to above 1), every month different:
    (12, nj, ni) with halos, a function of the global indices"""
    itdm, jtdm = itdm or ni - 2 * NBDY, jtdm or nj - 2 * NBDY
    x = (np.arange(ni)[None, :] - NBDY + i0 + 0.5) / itdm
    y = (np.arange(nj)[:, None] - NBDY + j0 + 0.5) / jtdm
    out = np.zeros((12, nj, ni))
    for k in range(12):
        ph = 2.0 * np.pi * k / 12.0
        e = -0.41 + 1.89 * np.sin(2.0 * np.pi * x + ph) * np.cos(np.pi * y + 0.5 * ph) + 0.07 * (k - 5.5) / 5.5 * np.cos(4.0 * np.pi * y)
        out[k] = 10.0 ** e
    return out


# ---- updswa ------------------------------------------------------------------------------------------------------------------------------
def nint(x):
    """Fortran's nint, half away from zero, element by element (floor(x + .5) would round x + .5 first)"""
    out = np.empty(x.shape, dtype=np.int64)
    flat, o = x.reshape(-1), out.reshape(-1)
    for q in range(flat.size):
        v = float(flat[q])
        f = math.floor(abs(v))
        r = f + 1 if abs(v) - f >= 0.5 else f
        o[q] = int(math.copysign(r, v))
    return out


def updswa(s, method, lmi, xmi, sel, lut=None, seen=None):
    """s: chl10c (12, nj, ni), chl10 and the four band planes (1, nj, ni), modified in place at the points sel"""
    if method not in ("chlorophyll_ma94", "chlorophyll_ohl03"):
        return
    c = s["chl10c"]
    chl10 = intp1d(c[lmi[0] - 1], c[lmi[1] - 1], c[lmi[2] - 1], c[lmi[3] - 1], c[lmi[4] - 1], xmi)
    s["chl10"][0][sel] = chl10[sel]
    q = fmax(CHL10_MIN, fmin(CHL10_MAX, chl10))
    if seen is not None:
        seen["below"] = seen.get("below", 0) + int((chl10[sel] < CHL10_MIN).sum())
        seen["above"] = seen.get("above", 0) + int((chl10[sel] > CHL10_MAX).sum())
        seen["inside"] = seen.get("inside", 0) + int(((chl10[sel] >= CHL10_MIN) & (chl10[sel] <= CHL10_MAX)).sum())
    if method == "chlorophyll_ma94":
        def poly(p):
            return ((((p[5] * q + p[4]) * q + p[3]) * q + p[2]) * q + p[1]) * q + p[0]
        v2 = poly(MA94_V2)
        out = ((1.0 - MA94_IRFC) * (1.0 - v2), (1.0 - MA94_IRFC) * v2, poly(MA94_Z1), poly(MA94_Z2))
    else:
        tab, lo, d = lut if lut is not None else ohl03_tables()
        n = nint((q - lo) / d) + 1
        if seen is not None:
            seen["n_lowest"] = seen.get("n_lowest", 0) + int((n[sel] == LOWEST_INDEX).sum())
            seen["n_401"] = seen.get("n_401", 0) + int((n[sel] == NVAL_LUT).sum())
            seen["n_interior"] = seen.get("n_interior", 0) + int(((n[sel] > LOWEST_INDEX) & (n[sel] < NVAL_LUT)).sum())
            seen.setdefault("indices", set()).update(int(v) for v in np.unique(n[sel]))
            assert n[sel].min() >= LOWEST_INDEX and n[sel].max() <= NVAL_LUT
        n = np.clip(n, 1, NVAL_LUT)
        out = (tab[1][n - 1], tab[0][n - 1], 1.0 / tab[3][n - 1], 1.0 / tab[2][n - 1])
    for nm, v in zip(BANDS, out):
        s[nm][0][sel] = v[sel]


def missing(seen, method):
    keys = ["below", "above", "inside"] + (["n_lowest", "n_401", "n_interior"] if method == "chlorophyll_ohl03" else [])
    return [k for k in keys if seen.get(k, 0) <= 0]


# ---- fwbbal ------------------------------------------------------------------------------------------------------------------------------
def fwbbal(s, o, sel, idm, jdm):
    """s: eiacc pracc eva fmltfz lip sop rnf rfi scp2 (1, nj, ni) and ipwocn; o: baclin, nday_of_year, nstep (incremented), nstep_in_day,
    prfac.  Returns the new prfac; eiacc and pracc are modified in place"""
    ei, pr = s["eiacc"][0], s["pracc"][0]
    ei[sel] = (ei + (s["eva"][0] + s["fmltfz"][0]) * o["baclin"])[sel]
    pr[sel] = (pr + (((s["lip"][0] + s["sop"][0]) + s["rnf"][0]) + s["rfi"][0]) * o["baclin"])[sel]
    prfac = o["prfac"]
    if o["nday_of_year"] == 1 and o["nstep"] % o["nstep_in_day"] == 0:
        ei[sel] = (ei * s["scp2"][0])[sel]
        pr[sel] = (pr * s["scp2"][0])[sel]
        totei = xcsum(ei, s["ipwocn"][0], idm, jdm)
        totpr = xcsum(pr, s["ipwocn"][0], idm, jdm)
        prfac = -prfac * totei / totpr
        ei[sel] = 0.0
        pr[sel] = 0.0
    return prfac


# ---- chkvar ------------------------------------------------------------------------------------------------------------------------------
def chkvar(s, nn, kk, sel, idm, jdm, i0=0, j0=0):
    """the line the serial reference prints first, or None: j, then k, then i (the wet points of the row in ascending i), then dp NaN, dp Inf,
    temp NaN, temp Inf, saln NaN, saln Inf"""
    with np.errstate(invalid="ignore"):
        for j in range(1, jdm + 1):
            for k in range(1, kk + 1):
                row = {nm: s[nm][nn + k - 1, NBDY + j - 1] for nm in ("dp", "temp", "saln")}
                bad = np.zeros(row["dp"].shape, bool)
                for a in row.values():
                    bad |= (a != a) | (a * 0 != 0)
                bad &= sel[NBDY + j - 1]
                if not bad.any():
                    continue
                x = int(np.flatnonzero(bad)[0])
                for nm in ("dp", "temp", "saln"):
                    a = row[nm][x]
                    what = "NaN" if a != a else "Inf" if a * 0 != 0 else None
                    if what:
                        return " chkvar: %s is %s at (i =%4d, j =%4d, k =%4d)" % (nm, what, i0 + x - NBDY + 1, j0 + j, k)
    return None
