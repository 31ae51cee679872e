"""The readers of diamer's and diasec's text tables (blom_amd/diasections.py) and the numpy restatement of both routines
(tests/test_gpu_diaout.py) on values made up here.  CPU only; the comparison of the oflg <= 0 filter with the library's runs on the host
emulation where it is built."""
import os

import numpy as np
import pytest

from blom_amd import diasections as ds
from blom_amd.cases import make_case

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
needs_emu = pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")


def _tables():
    import test_gpu_diaout as t
    case = make_case("chan_s_tke")
    return t, case, t.make_tables(case)


def test_write_then_read_returns_the_same_tables(tmp_path):
    t, case, (mer, sec) = _tables()
    a, b = str(tmp_path / "metra_index.dat"), str(tmp_path / "section_index.dat")
    ds.write_metra_index(a, mer["mtlat"], mer["nind"], mer["pts"])
    mtlat, nind, pts = ds.read_metra_index(a, case.idm, case.jdm)
    assert mtlat.tobytes() == mer["mtlat"].tobytes() and (nind == mer["nind"]).all() and (pts == mer["pts"]).all()
    assert pts.dtype == np.int32 and nind.dtype == np.int32
    ds.write_section_index(b, sec["names"], sec["nsi"], sec["pts"])
    names, nsi, spts, equat = ds.read_section_index(b, case.idm, case.jdm)
    assert names == sec["names"] and (nsi == sec["nsi"]).all() and (spts == sec["pts"]).all() and equat == sec["equat_sec"] == 2


def test_header_fields_are_read_as_the_reference_reads_them(tmp_path):
    """c20(9:15) with f7.3 -- without a decimal point the last three digits are the fraction --, c20(16:20) the count, and nothing
    behind column 20 counts"""
    p = str(tmp_path / "m.dat")
    with open(p, "w") as f:
        f.write("Section   45250    2 trailing words\n    3    4  0  1\n 5 6 -1 1 ignored\nSection -12.500    0\n")
    mtlat, nind, pts = ds.read_metra_index(p)
    assert list(mtlat) == [45.25, -12.5] and list(nind) == [2, 0]
    assert pts.tolist() == [[3, 4, 0, 1], [5, 6, -1, 1]]
    q = str(tmp_path / "s.dat")
    with open(q, "w") as f:
        f.write("Name: a\n1 2 1 0\nName: the equatorial_undercurrent at 170W\n 2, 3, 0, -1\nName: c\n")
    names, nsi, spts, equat = ds.read_section_index(q)
    assert names == ["a", "the equatorial_undercurrent at 170W", "c"] and list(nsi) == [1, 1, 0] and equat == 2
    assert spts.tolist() == [[1, 2, 1, 0], [2, 3, 0, -1]]


def test_malformed_files_raise(tmp_path):
    p = str(tmp_path / "m.dat")

    def metra(text, **kw):
        with open(p, "w") as f:
            f.write(text)
        return ds.read_metra_index(p, **kw)
    with pytest.raises(ds.SectionFileError, match="a line that starts with 'Section' expected"):
        metra("section   1.000    1\n1 1 0 1\n")
    with pytest.raises(ds.SectionFileError, match="a line that starts with 'Section' expected"):
        metra("Section   1.000    1\n1 1 0 1\n2 1 0 1\n")                      # one point line more than announced
    with pytest.raises(ds.SectionFileError, match="section too short"):
        metra("Section   1.000    3\n1 1 0 1\n2 1 0 1\n")
    with pytest.raises(ds.SectionFileError, match="4 integers expected, 3 found"):
        metra("Section   1.000    1\n1 1 0\n")
    with pytest.raises(ds.SectionFileError, match="indices out of range! i = 21 itdm = 20"):
        metra("Section   1.000    1\n21 1 0 1\n", itdm=20, jtdm=24)
    with pytest.raises(ds.SectionFileError, match="latitude field"):
        metra("Section   x.000    0\n")
    with open(p, "w") as f:
        f.write("1 1 1 0\nName: a\n")
    with pytest.raises(ds.SectionFileError, match="in front of the first 'Name' line"):
        ds.read_section_index(p)
    with open(p, "w") as f:
        f.write("Name: a\n1 25 1 0\n")
    with pytest.raises(ds.SectionFileError, match="indices out of range"):
        ds.read_section_index(p, 20, 24)


def test_filter_keeps_the_points_of_positive_ocean_regions():
    t, case, (mer, sec) = _tables()
    nind, pts = ds.filter_ocean_points(mer["nind"], mer["pts"], mer["oflg"])
    want = t.kept(mer)
    assert list(nind) == [len(s) for s in want]
    assert pts.tolist() == [list(e[:4]) for s in want for e in s]
    assert nind[-2] == 0 and nind[0] == case.idm * 8 // 10              # the section in the stripe of 0; a row loses that stripe


def test_restatement_on_made_up_accumulators():
    """the fill rules, the shapes, the dependence on the order of the entries and on nacc, without any library"""
    t, case, (mer, sec) = _tables()
    rng = np.random.default_rng(5)
    nj, ni, kk = case.jdm + 8, case.idm + 8, case.kdm
    masks = {k: np.ones((nj, ni), np.int32) for k in ("ip", "iu", "iv")}
    bnds = np.array([[0., 100.], [100., 300.], [300., 600.], [600., 8000.]])
    acc = {s: rng.normal(size=(len(bnds) if s.endswith("lvl") else 1 if s in ("sss", "sst") else kk, nj, ni)) * 1e9 for s in t.SOURCES}
    acc["dp"] = np.abs(acc["dp"])
    depths = np.full((nj, ni), 450.0)
    sens = []
    a = t.restate(case, masks, mer, sec, acc, 4, depths, np.full((nj, ni), 1.0e8), bnds, 3.0e12, sens=sens)
    b = t.restate(case, masks, mer, sec, acc, 5, depths, np.full((nj, ni), 1.0e8), bnds, 3.0e12)
    lmax, nm = len(mer["mtlat"]), 4
    assert sorted(a) == sorted(t.NAMES) and any(sens)
    assert a["mmflxl"].shape == (nm, kk, lmax) and a["mmflxd"].shape == (nm, 4, lmax) and a["mhflx"].shape == (nm, lmax) and a["masstr"].shape == (3,)
    assert (a["mmflxl"][:, 0, :-1][a["mmflxl"][:, 0, :-1] != t.FILL] == 0.).all()          # the exclusive sum starts at 0.
    assert (a["mmflxd"][0, :3, 0] != t.FILL).all() and a["mmflxd"][0, 3, 0] == t.FILL          # 450 m deep: the level from 600 m on is below the bottom
    assert (a["mhflx"][:, -1] == t.FILL).all() and a["mhflx"][0, -2] == t.FILL and (a["mmflxl"][0, :, -2] == 0.).all()
    assert a["mhflx"][1, 0] == t.FILL and a["mhflx"][2, -4] == t.FILL                          # the latitude bounds cut the rows
    assert a["mhflx"][1, -4] != t.FILL and a["mhflx"][2, 0] != t.FILL
    for nm_ in ("mhflx", "mmflxd", "masstr", "massgs", "sssga"):
        assert a[nm_].tobytes() != b[nm_].tobytes(), nm_
    assert a["salnga"].tobytes() == b["salnga"].tobytes()                                      # a ratio of two sums: nacc drops out


@needs_emu
def test_the_library_filters_as_the_reader_does():
    """dia_set_mertra with every point of the file and with the points filter_ocean_points keeps: the same results"""
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    import test_gpu_diaout as t
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = h._LIB = EMU
    try:
        case, masks, gpu, mer, sec = t.context("chan_s_tke", tables=False)
        try:
            names = ["mhflx", "mmflxd", "msfld"]
            gpu.dia_select(names)
            assert gpu.step(0, 2) == 2
            gpu.dia_set_mertra(**mer)
            gpu.dia_reduce()
            a = {nm: gpu.dia_msc(nm) for nm in names}
            nind, pts = ds.filter_ocean_points(mer["nind"], mer["pts"], mer["oflg"])
            assert int(nind.sum()) < int(mer["nind"].sum())
            gpu.dia_set_mertra(**dict(mer, nind=nind, pts=pts))
            gpu.dia_reduce()
            assert not [nm for nm in names if a[nm].tobytes() != gpu.dia_msc(nm).tobytes()]
        finally:
            gpu.close()
    finally:
        g.LIB_PATH, h._LIB = old, oldh
