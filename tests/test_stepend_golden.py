"""CROSS-CHECK, not a pin: the numpy restatement of tests/stepend_ref.py, the device stages (marked gpu) and the device library compiled
for the host (tests/hostemu) against tests/golden/stepend_*.npz -- what the reference's own phy/mod_swabs.F90, phy/mod_forcing.F90 and
phy/mod_chkvar.F90 computed behind stand-ins on chan_s_tke's grid (tests/golden/make_stepend_golden.py): both chlorophyll methods at
three positions in the year, jerlov and top-layer, fwbbal over steps that contain one year's end, and the line chkvar prints.  == on the
bytes of whole padded planes, character for character on the lines."""
import json
import os

import numpy as np
import pytest

import stepend_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
NB = 4


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def load(name):
    z = np.load(os.path.join(GOLD, f"stepend_{name}.npz"))
    return z, json.loads(str(z["meta"]))


def geometry(z):
    ip = z["ip"][0]
    nj, ni = ip.shape
    jdm, idm = nj - 2 * NB, ni - 2 * NB
    return ip, idm, jdm, R.owned(dict(ip=ip, iu=ip, iv=ip), idm, jdm)["p"]


def preset(meta, shape):
    return {nm: np.full(shape, meta["fill"] + k) for k, nm in enumerate(R.BANDS)}


def planted(case_, kk, shape):
    s = {nm: np.ones((2 * kk,) + shape) for nm in ("dp", "temp", "saln")}
    nn = (case_["n"] - 1) * kk
    for nm, v, k, (j, i) in case_["plants"]:
        s[nm][nn + k - 1, NB - 1 + j, NB - 1 + i] = float(v)
    return s, nn


# ---- the restatement (CPU) ----------------------------------------------------------------------------------------------------------------
def test_restated_swabs_equal_the_references_module():
    z, meta = load("swabs")
    ip, idm, jdm, sel = geometry(z)
    chl10c = R.log10_chl(z["chl"])
    lut = R.ohl03_tables()
    for method, jwtype in meta["swabs"]:
        want = z[method.replace("-", "_")]
        s = preset(meta, (1,) + ip.shape)
        s["chl10c"], s["chl10"] = chl10c, np.zeros((1,) + ip.shape)
        if not method.startswith("chlorophyll"):
            R.iniswa_constant(s, method, sel, jwtype=jwtype, swamxd=meta["swamxd"])
        for q in range(1 + len(meta["times"])):
            if q:
                lmi, xmi = meta["times"][q - 1]
                R.updswa(s, method, lmi, xmi, sel, lut=lut)
            bad = [nm for k, nm in enumerate(R.BANDS) if not same_bytes(s[nm][0], want[q, k])]
            assert not bad, (method, q, bad)
        assert not same_bytes(want[0], want[1]) or not method.startswith("chlorophyll")


def test_restated_fwbbal_equals_the_references_module():
    z, meta = load("fwbbal")
    ip, idm, jdm, sel = geometry(z)
    s = {nm[3:]: z[nm].copy() for nm in z.files if nm.startswith("in_")}
    s["ipwocn"] = z["ipwocn"]
    prfac = 1.0
    for q, (day, ns1) in enumerate(meta["steps"]):
        prfac = R.fwbbal(s, dict(baclin=meta["baclin"], nday_of_year=day, nstep=ns1, nstep_in_day=meta["nstep_in_day"], prfac=prfac), sel, idm, jdm)
        assert prfac == z["out_prfac"][q], (q, prfac, z["out_prfac"][q])
        assert same_bytes(s["eiacc"][0], z["out_eiacc"][q]) and same_bytes(s["pracc"][0], z["out_pracc"][q]), q
    assert prfac != 1.0


def test_restated_chkvar_prints_the_references_line():
    z, meta = load("chkvar")
    ip, idm, jdm, sel = geometry(z)
    from blom_amd.cases import make_case
    kk = make_case(meta["cfg"]).kdm
    for c in meta["cases"]:
        s, nn = planted(c, kk, ip.shape)
        got = R.chkvar(s, nn, kk, sel, idm, jdm)
        assert (got if got is not None else " chkvar: clean") == c["line"], (got, c["line"])


# ---- the device stages ------------------------------------------------------------------------------------------------------------------------
def check_device():
    import test_gpu_diaacc as lyr
    from blom_amd import hostinit
    from blom_amd.gpu import BlomGpuError
    case, masks, g = lyr.full_context("chan_s_tke")
    try:
        kk = case.kdm
        six = hostinit.step_indices(0, kk)
        # iniswa / updswa
        z, meta = load("swabs")
        ip, idm, jdm, sel = geometry(z)
        assert np.array_equal(np.asarray(masks["ip"]).reshape(ip.shape) > 0, ip > 0)
        g.set("swamxd", meta["swamxd"])
        for method, jwtype in meta["swabs"]:
            want = z[method.replace("-", "_")]
            for nm, a in preset(meta, (1,) + ip.shape).items():
                g.put(nm, a)
            g.set("swamth", method)
            g.set("jwtype", jwtype)
            g.iniswa(z["chl"] if method.startswith("chlorophyll") else None)
            for q in range(1 + len(meta["times"])):
                if q:
                    lmi, xmi = meta["times"][q - 1]
                    for k, v in enumerate(lmi):
                        g.set("l%dmi" % (k + 1), int(v))
                    g.set("xmi", float(xmi))
                    g.stage("updswa", *six)
                bad = [nm for k, nm in enumerate(R.BANDS) if not same_bytes(g.get(nm)[0], want[q, k])]
                assert not bad, (method, q, bad)
        # fwbbal
        z, meta = load("fwbbal")
        g.set("sprfac", 1)
        g.set("baclin", meta["baclin"])
        g.set("nstep_in_day", meta["nstep_in_day"])
        for nm in z.files:
            if nm.startswith("in_"):
                g.put(nm[3:], z[nm])
        g.put("ipwocn", z["ipwocn"])
        for q, (day, ns1) in enumerate(meta["steps"]):
            g.set("nday_of_year", day)
            g.set("nstep", ns1)
            g.stage("fwbbal", *six)
            assert g.get_real("prfac") == z["out_prfac"][q], q
            assert same_bytes(g.get("eiacc")[0], z["out_eiacc"][q]) and same_bytes(g.get("pracc")[0], z["out_pracc"][q]), q
        # chkvar: the stage alone on planted data
        z, meta = load("chkvar")
        g.set("chkvar", 1)
        for c in meta["cases"]:
            s, nn = planted(c, kk, ip.shape)
            for nm in s:
                g.put(nm, s[nm])
            idx = hostinit.step_indices(0 if nn else 1, kk)
            assert idx[3] == nn
            try:
                g.stage("chkvar", *idx)
                got = " chkvar: clean"
            except BlomGpuError as e:
                got = str(e)[len("blom:"):]
                assert str(e).startswith("blom:")
            assert got == c["line"], (got, c["line"])
    finally:
        g.close()


@pytest.mark.gpu
def test_device_stages_equal_the_references_modules():
    check_device()


@pytest.mark.skipif(not os.path.exists(EMU), reason="tests/hostemu/libblomgpu_hostemu.so not built")
def test_device_stages_equal_the_references_modules_on_the_host_emulation():
    import blom_amd.gpu as g
    import blom_amd.hor3map as h
    old, oldh = g.LIB_PATH, h._LIB
    g.LIB_PATH = h._LIB = EMU
    try:
        check_device()
    finally:
        g.LIB_PATH, h._LIB = old, oldh
