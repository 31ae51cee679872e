"""What diaout_iogrp forms from the accumulators at output time, on the device (blomgpu_dia_reduce, blom_amd/csrc/stage_diaout.hip):
diamer (phy/mod_dia.F90:4004-4629), diasec (:3814-4001) and the global sums and means (:2427-2588).

The expected values are those routines restated in numpy below -- float64, the running sums vectorised over the plane (every point
sees the reference's operations in the reference's order), the section sums as serial Python loops over the entries in the table's
order -- and applied to the accumulators that dia_get downloads from the same context just before dia_reduce.  xcsum is
tests/thermf_cesm_ref.py's.  Everything is compared with ==, byte for byte, fill values included.

The section and region tables are generated here (make_tables): every interior row as a zonal section, a staircase with flags of
both signs, a section that lies wholly where oflg = 0, one whose latitude lies outside every region's bounds; three ocean regions as
stripes in i plus a stripe of 0; four meridional regions, two with latitude bounds that cut the rows; three named sections for diasec,
one of them equatorial.

tests/test_hostemu_diaout.py runs the same functions on the host emulation of the library."""
import contextlib

import numpy as np
import pytest

from blom_amd import hostinit
from blom_amd.cases import default_grid
from parity import STATE_FIELDS
from thermf_cesm_ref import xcsum
from test_gpu_diaacc import full_context, same_bytes

pytestmark = pytest.mark.gpu

GRAV, SPCIFH, G2KG = 9.806, 3990.0, 1.0e-3          # phy/mod_constants.F90
FILL = 9.9692099683868690e+36                       # nf90_fill_double
# name -> (kind, factor, u source, v source), in the library's order
MSC = dict(
    mmflxl=("dens", "mass", "umfll", "vmfll"), mmftdl=("dens", "mass", "umfltdl", "vmfltdl"), mmfsml=("dens", "mass", "umflsml", "vmflsml"),
    mmflxd=("depth", "mass", "uflxlvl", "vflxlvl"), mmftdd=("depth", "mass", "umfltdlvl", "vmfltdlvl"),
    mmfsmd=("depth", "mass", "umflsmlvl", "vmflsmlvl"),
    mhflx=("tr", "heat", "utflx", "vtflx"), mhftd=("tr", "heat", "utfltd", "vtfltd"), mhfsm=("tr", "heat", "utflsm", "vtflsm"),
    mhfld=("tr", "heat", "utflld", "vtflld"),
    msflx=("tr", "salt", "usflx", "vsflx"), msftd=("tr", "salt", "usfltd", "vsfltd"), msfsm=("tr", "salt", "usflsm", "vsflsm"),
    msfld=("tr", "salt", "usflld", "vsflld"),
    masstr=("sec", "mass", "uflxlvl", "vflxlvl"), heattr=("sec", "heat", "utflxlvl", "vtflxlvl"), salttr=("sec", "salt", "usflxlvl", "vsflxlvl"),
    massgs=("glb", None, "dp", None), salnga=("glb", None, "dp", "saln"), tempga=("glb", None, "dp", "temp"),
    volgs=("glb", None, "dz", None), sssga=("glb", None, "sss", None), sstga=("glb", None, "sst", None))
NAMES = list(MSC)
SOURCES = sorted({s for v in MSC.values() for s in v[2:] if s})
# eddtra leaves the submesoscale fluxes zero under isopyc_bulkml (test_gpu_diaacc.MAY_REST: umflsm ...), so what is formed from them may rest
MAY_REST = ("mmfsml", "mmfsmd", "mhfsm", "msfsm")


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def make_tables(case):
    idm, jdm = case.idm, case.jdm
    b1, b2, b3 = idm * 3 // 10, idm * 11 // 20, idm * 8 // 10
    oflg = np.zeros((jdm, idm), np.int32)
    oflg[:, :b1], oflg[:, b1:b2], oflg[:, b2:b3] = 1, 2, 3                       # ... and a stripe of 0 east of b3
    mtlat, nind, pts = [], [], []

    def section(lat, p):
        mtlat.append(float(lat)); nind.append(len(p)); pts.extend(p)
    for j in range(2, jdm):
        section(j, [(i, j, 0, 1) for i in range(1, idm + 1)])
    n = min(idm, jdm) - 2
    section(2.5, [(1 + s, 2 + s, 1 if s % 2 == 0 else -1, -1 if s % 3 == 0 else 1) for s in range(n)])      # a staircase, both signs on u and v
    section(3.25, [(i, jdm // 2, 0, 1) for i in range(b3 + 1, idm + 1)])         # wholly where oflg = 0: the count is 0
    section(999.0, [(i, 3, 0, 1) for i in range(1, idm + 1)])                   # outside every region's latitude bounds
    regflg = np.zeros((4, 20), np.int32)
    regflg[1, :2], regflg[2, 0], regflg[3, 0] = (1, 2), 3, 2
    mer = dict(mtlat=np.array(mtlat), nind=np.array(nind, np.int32), pts=np.array(pts, np.int32), oflg=oflg, ocn_nreg=3,
               nflg=np.array([1, 2, 1, 1], np.int32), regflg=regflg,
               minlat=np.array([-10.0, jdm / 3.0, -10.0, -10.0]), maxlat=np.array([500.0, 500.0, 2.0 * jdm / 3.0, 500.0]))
    names = ["drake_passage", "equatorial_undercurrent", "zigzag"]
    secs = [[(idm // 3, j, 1, 0) for j in range(1, jdm + 1)],
            [(i, jdm // 2, 1 if i % 2 else 0, 1) for i in range(1, idm + 1)],
            [(2 + s, 1 + s, -1, 1 if s % 2 else -1) for s in range(n)]]
    sec = dict(names=names, nsi=np.array([len(s) for s in secs], np.int32), pts=np.array([p for s in secs for p in s], np.int32), equat_sec=2)
    return mer, sec


def kept(mer):
    """the entries diamer keeps (:4070), per section: lists of (i, j, uflg, vflg, o)"""
    out, k = [], 0
    for n in mer["nind"]:
        sec = []
        for i, j, u, v in mer["pts"][k:k + n]:
            o = int(mer["oflg"][j - 1, i - 1])
            if o > 0:
                sec.append((int(i), int(j), int(u), int(v), o))
        out.append(sec)
        k += n
    return out


# ---- diamer, diasec and the global sums, restated -----------------------------------------------------------------------------------------
def factor(fac, baclin, nacc):
    den = (GRAV * baclin) * float(nacc)
    return dict(mass=.5, heat=.5 * SPCIFH, salt=.5 * G2KG)[fac] / den


def running(kind, a, wet, r, k350=None, w350=None, equat=False):
    """the running sum of one source down its levels: a (nlev, nj, ni), wet the owned points where the grid's mask is set.  -> the
    (nout, nj, ni) planes the section sums read: every level for the stream functions, the last for the transports; equat: ucum350"""
    n = a.shape[0]
    cum = np.zeros(a.shape[1:])                                    # ucum = 0. at 1..ii, 1..jj (:4131-4137); only wet points are written
    c350 = np.zeros(a.shape[1:])
    out = []
    for k in range(1, n + 1):
        if kind == "dens":                                         # :4340-4371
            new = np.zeros_like(cum) if k == 1 else cum + r * a[k - 2]
        elif kind == "depth":                                      # :4492-4559, in the reference's branch order
            if k == 1:
                new = np.zeros_like(cum)
            elif k == 2:
                new = r * (a[0] + .5 * a[1])
            elif k == n:
                new = cum + r * (.5 * a[n - 2] + a[n - 1])
            else:
                new = cum + (.5 * r) * (a[k - 2] + a[k - 1])
        else:                                                      # :4188-4212 | :3903-3953
            new = a[0] * r if k == 1 else cum + a[k - 1] * r
        cum = np.where(wet, new, cum)
        if kind == "sec" and k >= 2:
            if k == k350 - 1:
                c350 = np.where(wet, cum, c350)
            elif k == k350:
                c350 = np.where(wet, c350 + w350 * (cum - c350), c350)
        if kind in ("dens", "depth"):
            out.append(cum)
    if kind == "tr":
        out = [cum]
    if kind == "sec":
        out = [c350 if equat else cum]
    return np.stack(out)


def kmax_of(mer, entries, depths, bnds1):
    """:4449-4467 as written"""
    nm = len(mer["nflg"])
    kmax = np.zeros((len(entries), nm), np.int64)
    for k in range(1, len(bnds1) + 1):
        for l, sec in enumerate(entries):
            for i, j, _, _, o in sec:
                if bnds1[k - 1] < depths[j + 3, i + 3]:
                    for m in range(nm):
                        if mer["regflg"][m, 0] == 0:
                            kmax[l, m] = k
                        else:
                            for n in range(mer["nflg"][m]):
                                if mer["regflg"][m, n] == o:
                                    kmax[l, m] = k
    return kmax


def mer_sums(mer, entries, U, V, kind, kmax=None, sens=None):
    """the serial sums over a section's entries, one per ocean region (:4219-4230), the region sums and the fill rules (:4235-4256);
    vectorised over the levels only.  -> (mer_nreg, nout, lmax).  sens: a list that receives one flag per (section, region): the sum
    taken in the reversed order differs somewhere"""
    nout, no, nm, lmax = U.shape[0], mer["ocn_nreg"], len(mer["nflg"]), len(entries)
    out = np.empty((nm, nout, lmax))
    k1 = np.arange(1, nout + 1)
    for l, sec in enumerate(entries):
        mor, cnt = np.zeros((no + 1, nout)), np.zeros(no + 1, np.int64)
        for i, j, uf, vf, o in sec:
            mor[o] = (mor[o] + float(uf) * U[:, j + 3, i + 3]) + float(vf) * V[:, j + 3, i + 3]
            cnt[o] += 1
        if sens is not None:
            rev = np.zeros((no + 1, nout))
            for i, j, uf, vf, o in reversed(sec):
                rev[o] = (rev[o] + float(uf) * U[:, j + 3, i + 3]) + float(vf) * V[:, j + 3, i + 3]
            sens.append(bool((rev != mor).any()))
        for m in range(nm):
            if mer["mtlat"][l] < mer["minlat"][m] or mer["mtlat"][l] > mer["maxlat"][m]:
                out[m, :, l] = FILL
                continue
            s, c = np.zeros(nout), 0
            for o in (range(1, no + 1) if mer["regflg"][m, 0] == 0 else mer["regflg"][m, :mer["nflg"][m]]):
                s = s + mor[o]
                c += cnt[o]
            if kind == "tr" and c == 0:
                s = np.full(nout, FILL)
            if kind == "depth":
                s = np.where(kmax[l, m] < k1, FILL, s)
            out[m, :, l] = s
    return out


def restate(case, masks, mer, sec, acc, nacc, depths, scp2, bnds, area, names=NAMES, sens=None):
    """every name of `names` from the downloaded accumulators acc[source] (nlev, nj, ni)"""
    nj, ni = case.jdm + 8, case.idm + 8
    own = np.zeros((nj, ni), bool)
    own[4:4 + case.jdm, 4:4 + case.idm] = True
    wet = {g: own & (masks["i" + g].reshape(nj, ni) > 0) for g in "puv"}
    baclin = case.params["baclin"]
    ddm = len(bnds)
    k350, w350 = (25, .5) if ddm == 70 else (12, 1.)              # :131-132 | :112-113
    entries = kept(mer) if mer else None
    kmax = None
    out = {}
    for nm in names:
        kind, fac, us, vs = MSC[nm]
        if kind == "glb":
            continue
        r = factor(fac, baclin, nacc)
        if kind == "sec":
            tr, k = np.zeros(len(sec["nsi"])), 0
            for s, n in enumerate(sec["nsi"]):
                eq = s + 1 == sec["equat_sec"]
                U = running("sec", acc[us], wet["u"], r, k350, w350, eq)[0]
                V = running("sec", acc[vs], wet["v"], r, k350, w350, eq)[0]
                t = 0.0
                for i, j, usi, vsi in sec["pts"][k:k + n]:
                    t = (t + float(U[j + 3, i + 3]) * float(usi)) + float(V[j + 3, i + 3]) * float(vsi)      # :3970 | :3976
                tr[s] = t
                k += n
            out[nm] = tr
            continue
        U, V = running(kind, acc[us], wet["u"], r), running(kind, acc[vs], wet["v"], r)
        if kind == "depth" and kmax is None:
            kmax = kmax_of(mer, entries, depths, bnds[:, 0])
        res = mer_sums(mer, entries, U, V, kind, kmax, sens)
        out[nm] = res[:, 0, :].copy() if kind == "tr" else res

    def colsum(a):                                                 # :2429-2457
        util = a[0].copy()
        for k in range(1, a.shape[0]):
            util = util + a[k]
        return xcsum(util * scp2, masks["ip"].reshape(nj, ni), case.idm, case.jdm, skip_seam=case.nreg == 2)
    rnacc = 1. / float(nacc)
    if {"massgs", "salnga", "tempga"} & set(names):
        massgs = colsum(acc["dp"])
    if "volgs" in names:
        out["volgs"] = np.array([rnacc * colsum(acc["dz"])])
    if "salnga" in names:
        out["salnga"] = np.array([colsum(acc["saln"]) / massgs])
    if "tempga" in names:
        out["tempga"] = np.array([colsum(acc["temp"]) / massgs])
    if "massgs" in names:
        out["massgs"] = np.array([rnacc * massgs / GRAV])
    for nm, src in (("sssga", "sss"), ("sstga", "sst")):
        if nm in names:
            out[nm] = np.array([rnacc * colsum(acc[src]) / area])
    return out


# ---- contexts and runs ---------------------------------------------------------------------------------------------------------------------
def sigdia_of(g, case, masks):
    """the case's reference densities: the column of sigmar at its first wet point (tests/test_gpu_diasig.py: tables_for, "ref")"""
    nj, ni = case.jdm + 8, case.idm + 8
    wet = np.zeros((nj, ni), bool)
    wet[4:-4, 4:-4] = True
    wet &= masks["ip"].reshape(nj, ni) > 0
    j, i = np.argwhere(wet)[0]
    return g.get("sigmar")[:case.kdm, j, i].astype(np.float64).copy()


def context(cfg, grid=None, levitus2x=False, tables=True, **opts):
    with default_grid(grid) if grid else contextlib.nullcontext():
        case, masks, g = full_context(cfg)
    g.dia_set_sigdia(sigdia_of(g, case, masks))
    if levitus2x:
        g.dia_set_levels(levitus2x=True)
    if g.get_real("area") <= 0.:
        g.set("area", float(np.sum(g.get("scp2")[0][masks["ip"].reshape(case.jdm + 8, case.idm + 8) > 0])))
    for k, v in opts.items():
        g.set(k, v)
    mer, sec = make_tables(case)
    if tables:
        g.dia_set_mertra(**mer)
        g.dia_set_sections(sec["nsi"], sec["pts"], sec["equat_sec"])
    return case, masks, g, mer, sec


def reduce_and_restate(g, case, masks, mer, sec, names=NAMES, sens=None):
    """-> (got, want): dia_msc of every name after dia_reduce, and the restatement on the accumulators downloaded just before it"""
    srcs = sorted({s for nm in names for s in MSC[nm][2:] if s})
    acc = {s: g.dia_get(s) for s in srcs}
    g.dia_reduce()
    got = {nm: g.dia_msc(nm) for nm in names}
    want = restate(case, masks, mer, sec, acc, g.dia_nacc(), g.get("depths")[0], g.get("scp2")[0], g.dia_levels(), g.get_real("area"), names, sens)
    return got, want


def differing(got, want):
    return [nm for nm in want if got[nm].shape != want[nm].shape or not same_bytes(got[nm], want[nm])]


_RUNS = {}


def run(cfg, grid=None, levitus2x=False, **opts):
    """four steps, all 23 names, reduce and restate; one more step and again (r changes with nacc)"""
    key = (cfg, grid, levitus2x, tuple(sorted(opts.items())))
    if key in _RUNS:
        return _RUNS[key]
    case, masks, g, mer, sec = context(cfg, grid, levitus2x, **opts)
    try:
        g.dia_select(NAMES)
        assert g.step(0, 4) == 4
        sens = []
        got4, want4 = reduce_and_restate(g, case, masks, mer, sec, sens=sens)
        assert g.step(4, 1) == 5
        got5, want5 = reduce_and_restate(g, case, masks, mer, sec)
    finally:
        g.close()
    _RUNS[key] = dict(case=case, mer=mer, sec=sec, got4=got4, want4=want4, got5=got5, want5=want5, sens=sens)
    return _RUNS[key]


CASES = ["chan_s_tke", "box_s", "tri_s_tke"]


# ---- 1. the results are the reference's -----------------------------------------------------------------------------------------------------
def speaks(a):
    """a finite, non-fill, non-zero value somewhere"""
    return bool((np.isfinite(a) & (a != FILL) & (a != 0.)).any())


def check_run(r):
    """what holds on every run: the restated bytes after four and after five steps, no result silent but the four that may rest, and
    inputs that tell summation orders apart"""
    for tag in ("4", "5"):
        got, want = r["got" + tag], r["want" + tag]
        assert sorted(got) == sorted(NAMES)
        bad = differing(got, want)
        assert not bad, (tag, bad)
        silent = [nm for nm in NAMES if nm not in MAY_REST and not speaks(got[nm])]
        assert not silent, (tag, silent)
    assert [nm for nm in NAMES if not same_bytes(r["got4"][nm], r["got5"][nm])], "nacc = 5 gave what nacc = 4 gave"
    assert any(r["sens"]), "no section sum depends on the order of its entries: lengthen the sections"


def check_reduce(cfg, grid=None, levitus2x=False):
    r = run(cfg, grid, levitus2x)
    check_run(r)
    lmax, nm_ = len(r["mer"]["mtlat"]), len(r["mer"]["nflg"])
    assert r["got4"]["mmflxl"].shape == (nm_, r["case"].kdm, lmax) and r["got4"]["mhflx"].shape == (nm_, lmax)
    assert r["got4"]["masstr"].shape == (3,) and r["got4"]["massgs"].shape == (1,)
    # the section that lies where oflg = 0: the transports give fill, the stream functions 0. (inside the regions' bounds)
    dead = lmax - 2
    assert (r["got4"]["mhflx"][0, dead] == FILL) and (r["got4"]["msflx"][3, dead] == FILL)
    assert (r["got4"]["mmflxl"][0, :, dead] == 0.).all()
    # ... and the one outside every region's bounds: fill everywhere
    for nm in ("mmflxl", "mmflxd"):
        assert (r["got4"][nm][:, :, lmax - 1] == FILL).all()
    assert (r["got4"]["mhflx"][:, lmax - 1] == FILL).all()


def check_fill_below_the_bottom(cfg="chan_s_tke"):
    """the cases are 200-800 m deep under levels that reach 8000 m: mmflxd holds fill below the bottom and values above it"""
    r = run(cfg)
    d = r["got4"]["mmflxd"][0, :, 0]                               # all ocean regions, the first zonal row
    assert (d[-1] == FILL) and (d[0] != FILL)
    first = int(np.argmax(d == FILL))
    assert (d[first:] == FILL).all() and (d[:first] != FILL).all() and 0 < first < len(d)


def check_chunks_and_passes():
    """chan_m: a row of 80 entries crosses a pass of 64, 8 layers and 35 levels cross chunks of 4 -- and equal the default sizes"""
    a, b = run("chan_m"), run("chan_m", diaout_entries=64, diaout_levels=4)
    check_run(a)
    check_run(b)
    for tag in ("got4", "got5"):
        bad = differing(b[tag], a[tag])
        assert not bad, bad
    assert max(a["mer"]["nind"]) == 80


def check_equatorial_tables():
    """k350 = 12, w350 = 1. on the 35 levels, 25 and .5 on LEVITUS2X; a table of the caller's is refused"""
    from blom_amd.gpu import BlomGpuError
    a, b = run("chan_s_tke"), run("chan_s_tke", levitus2x=True)
    check_run(a)
    check_run(b)
    assert b["got4"]["mmflxd"].shape[1] == 70
    assert not same_bytes(a["got4"]["masstr"][1:2], b["got4"]["masstr"][1:2])
    case, masks, g, mer, sec = context("chan_s_tke", tables=False)
    try:
        g.dia_set_levels(np.array([[0., 100.], [100., 400.], [400., 9000.]]))
        with pytest.raises(BlomGpuError, match="blomgpu_dia_set_sections: the upper-350 m sums of section 2 need k350 and w350"):
            g.dia_set_sections(sec["nsi"], sec["pts"], sec["equat_sec"])
        g.dia_set_sections(sec["nsi"], sec["pts"], -1)              # without an equatorial section any table will do
        g.dia_select(["masstr"])
        assert g.step(0, 2) == 2
        got, want = reduce_and_restate(g, case, masks, None, dict(sec, equat_sec=-1), names=["masstr"])
        assert not differing(got, want)
        # the table changed behind an equatorial section's back: the reduce refuses
        g.dia_select([])
        g.dia_set_levels()
        g.dia_set_sections(sec["nsi"], sec["pts"], 2)
        g.dia_set_levels(np.array([[0., 100.], [100., 400.], [400., 9000.]]))
        g.dia_select(["masstr"])
        assert g.step(2, 1) == 3
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: the upper-350 m sums of section 2"):
            g.dia_reduce()
    finally:
        g.close()


def check_resting_names_under_the_hybrid_coordinate():
    """mmfsml mmfsmd mhfsm msfsm rest under isopyc_bulkml; under cntiso_hybrid the mixed layer restratification (fox08) drives them once
    an interface lies inside the time-filtered mixed layer depth, which on this case takes six steps: eight are run"""
    from test_gpu_dia_hybrid import hybrid_context
    case, masks, g = hybrid_context("chan_s", "cntiso_hybrid", "nudge")
    try:
        mer, sec = make_tables(case)
        g.dia_set_sigdia(sigdia_of(g, case, masks))
        g.dia_set_mertra(**mer)
        g.dia_select(list(MAY_REST))
        assert g.step(0, 8) == 8
        got, want = reduce_and_restate(g, case, masks, mer, sec, names=MAY_REST)
        assert not differing(got, want)
        silent = [nm for nm in MAY_REST if not speaks(got[nm])]
        assert not silent, silent
    finally:
        g.close()


# ---- 2. the interface ------------------------------------------------------------------------------------------------------------------------
def check_interface():
    from blom_amd.gpu import BlomGpuError
    case, masks, g, mer, sec = context("chan_s_tke", tables=False)
    try:
        # the enumerators: the older ones as they were, the new one ends with the 23 names
        ext, msc = g.dia_names_ext(), g.dia_names_msc()
        assert (len(g.dia_names()), len(g.dia_names_all()), len(g.dia_names_full()), len(ext)) == (111, 117, 123, 133)
        assert msc[:133] == ext and [n for n, _, _ in msc[133:]] == NAMES and {k for _, k, _ in msc[133:]} == {5}
        assert not {n for n, _, _ in ext} & set(NAMES)
        # the selection adds the sources
        for nm in NAMES:
            g.dia_select([nm])
            for s in MSC[nm][2:]:
                if s:
                    assert g.dia_get(s).shape[0] >= 1
        g.dia_set_sigdia(None)
        with pytest.raises(BlomGpuError, match="umfll needs the diagnostic density classes sigdia"):
            g.dia_select(["mmflxl"])
        g.dia_set_sigdia(sigdia_of(g, case, masks))
        # refusals of the reduce and of the get, each with its reason
        g.dia_select(NAMES)
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: nacc = 0"):
            g.dia_reduce()
        with pytest.raises(BlomGpuError, match="blomgpu_dia_msc_get: mhflx: no blomgpu_dia_reduce since"):
            g.dia_msc("mhflx")
        assert g.step(0, 2) == 2
        with pytest.raises(BlomGpuError, match="mmflxl is selected, which needs the sections and regions of diamer .blomgpu_dia_set_mertra."):
            g.dia_reduce()
        g.dia_set_mertra(**mer)
        with pytest.raises(BlomGpuError, match="masstr is selected, which needs the sections of diasec .blomgpu_dia_set_sections."):
            g.dia_reduce()
        g.dia_set_sections(sec["nsi"], sec["pts"], sec["equat_sec"])
        area = g.get_real("area")
        g.set("area", 0.)
        with pytest.raises(BlomGpuError, match="sssga / sstga: the ocean area .mod_grid: area. has not been set"):
            g.dia_reduce()
        g.set("area", area)
        with pytest.raises(BlomGpuError, match="unknown msc name temp"):
            g.dia_msc("temp")
        # reduce reads only: every accumulator and every model field keeps its bytes, and twice gives the same results
        accs = [n for n, _, _ in ext if n in SOURCES]
        before = {n: g.dia_get(n) for n in accs}
        state = {n: g.get(n) for n in STATE_FIELDS if g.has_field(n)}
        got, want = reduce_and_restate(g, case, masks, mer, sec)
        assert not differing(got, want)
        g.dia_reduce()
        assert not differing({nm: g.dia_msc(nm) for nm in NAMES}, got)
        assert not [n for n in accs if not same_bytes(before[n], g.dia_get(n))]
        assert not [n for n in state if not same_bytes(state[n], g.get(n))]
        assert g.dia_nacc() == 2
        # a table set anew invalidates the results; a name that is not selected is refused
        g.dia_set_sections(sec["nsi"], sec["pts"], sec["equat_sec"])
        with pytest.raises(BlomGpuError, match="no blomgpu_dia_reduce since"):
            g.dia_msc("masstr")
        # finalize writes fill values into the level rows: no reduce until a reset, and then not before a step has run
        g.dia_reduce()
        g.dia_finalize()
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: blomgpu_dia_finalize has run"):
            g.dia_reduce()
        g.dia_reset()
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: nacc = 0"):
            g.dia_reduce()
        with pytest.raises(BlomGpuError, match="no blomgpu_dia_reduce since"):
            g.dia_msc("mhflx")
        assert g.step(2, 1) == 3
        got, want = reduce_and_restate(g, case, masks, mer, sec)
        assert not differing(got, want)
        # massgs is formed for salnga but handed out only when selected itself
        g.dia_select(["salnga", "mhflx"])
        assert g.step(3, 1) == 4
        got, want = reduce_and_restate(g, case, masks, mer, sec, names=["salnga", "mhflx"])
        assert not differing(got, want)
        with pytest.raises(BlomGpuError, match="blomgpu_dia_msc_get: massgs is not selected"):
            g.dia_msc("massgs")
        g.dia_select(["temp"])
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: no msc name is selected"):
            g.dia_reduce()
        # the tables' own refusals
        bad = dict(mer, pts=mer["pts"].copy())
        bad["pts"][3, 0] = case.idm + 1
        with pytest.raises(BlomGpuError, match="blomgpu_dia_set_mertra: indices out of range! section 1: iind = %d" % (case.idm + 1)):
            g.dia_set_mertra(**bad)
        with pytest.raises(BlomGpuError, match="blomgpu_dia_set_mertra: oflg.* > ocn_nreg = 2"):
            g.dia_set_mertra(**dict(mer, ocn_nreg=2))
        flg = mer["regflg"].copy()
        flg[1, 1] = 4
        with pytest.raises(BlomGpuError, match=r"mer_regflg\(2,2\) = 4 outside 0..ocn_nreg = 3"):
            g.dia_set_mertra(**dict(mer, regflg=flg))
        many = case.idm + case.jdm + 1
        with pytest.raises(BlomGpuError, match="too many or too long sections! lmax = %d" % many):
            g.dia_set_mertra(**dict(mer, mtlat=np.zeros(many), nind=np.ones(many, np.int32), pts=np.tile(np.array([[1, 1, 0, 1]], np.int32), (many, 1))))
        with pytest.raises(BlomGpuError, match="too many or too long sections! section 1 keeps %d" % many):
            g.dia_set_mertra(**dict(mer, mtlat=np.zeros(1), nind=np.array([many], np.int32), pts=np.tile(np.array([[1, 1, 0, 1]], np.int32), (many, 1))))
        with pytest.raises(BlomGpuError, match="blomgpu_dia_set_sections: indices out of range"):
            g.dia_set_sections(np.array([1], np.int32), np.array([[1, case.jdm + 1, 1, 0]], np.int32), -1)
        # cleared tables are missing tables
        g.dia_set_mertra()
        g.dia_select(["mhflx"])
        assert g.step(4, 1) == 5
        with pytest.raises(BlomGpuError, match="needs the sections and regions of diamer"):
            g.dia_reduce()
    finally:
        g.close()


def check_tile_refuses():
    from blom_amd.gpu import BlomGpu, BlomGpuError, TileGroup
    from blom_amd.cases import make_case
    from blom_amd.tiles import tile_extents, tile_window
    case = make_case("chan_s_tke")
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    ii, jj = tile_extents(case, 2, 1)
    grp = TileGroup(2, 1)
    tiles = []
    try:
        for px in range(2):
            tm = {k: tile_window(masks[k], case, 2, 1, px, 0) for k in masks}
            t = BlomGpu(ii, jj, case.kdm, case.ntr, case.nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=px * ii, j0=0)
            grp.attach(t, px, 0)
            tiles.append(t)
        tiles[0].dia_select(["massgs", "sstga"])
        with pytest.raises(BlomGpuError, match="blomgpu_dia_reduce: this context is a tile of a group or an RCCL rank"):
            tiles[0].dia_reduce()
    finally:
        for t in tiles:
            t.close()
        grp.destroy()


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CASES)
def test_reduce_gives_what_the_restated_routines_give(cfg):
    check_reduce(cfg)


def test_reduce_on_the_warped_grid():
    """scp2 is not a constant in the global means"""
    check_reduce("chan_s_tke", grid="warped")


def test_depth_space_holds_fill_below_the_bottom():
    check_fill_below_the_bottom()


def test_passes_and_chunks_give_the_default_sizes_results():
    check_chunks_and_passes()


def test_equatorial_section_on_both_level_tables():
    check_equatorial_tables()


def test_resting_names_move_under_the_hybrid_coordinate():
    check_resting_names_under_the_hybrid_coordinate()


def test_interface_and_refusals():
    check_interface()


def test_a_tile_of_a_group_refuses():
    check_tile_refuses()
