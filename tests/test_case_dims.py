"""make_case with sizes of the caller's choosing (blom_amd.cases: dims=, or the name <family>@<idm>x<jdm>x<kdm><suffix>) leaves the families as
they were."""
import numpy as np

from blom_amd.cases import make_case


def test_dims_none_builds_the_families_as_before():
    """make_case without dims: the arrays of every family of _DIMS (and a few with the tracer suffixes) as they were before
    make_case took sizes -- sha256 of the bytes of depth, dp, temp, trc and scux, recorded then -- and a sized case differs from
    its family in nothing but the three sizes and the name that carries them"""
    import hashlib
    import json
    import os
    from blom_amd.cases import _DIMS
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_case_sha256.json")) as f:
        want = json.load(f)
    assert set(_DIMS) <= set(want) and any(nm.endswith("_tke") for nm in want)
    for nm, rec in want.items():
        case = make_case(nm)
        got = {f: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
               for f, a in (("depth", case.depth), ("dp", case.ic["dp"]), ("temp", case.ic["temp"]), ("trc", case.ic["trc"]), ("scux", case.grid["scux"]))}
        assert got == rec["sha256"], nm
        assert [case.name, case.idm, case.jdm, case.kdm, case.nreg, case.ntr] == rec["head"], nm
    a, b = make_case("chan_s_tke"), make_case("chan_s_tke", dims=(20, 24, 6))
    assert b.name == "chan_s@20x24x6_tke" and (b.idm, b.jdm, b.kdm, b.nreg, b.ntr) == (a.idm, a.jdm, a.kdm, a.nreg, a.ntr)
    assert b.params == a.params
    for f in a.ic:
        assert a.ic[f].tobytes() == b.ic[f].tobytes(), f
    c = make_case("chan_s@33x17x3_tke", ntr=5)
    assert (c.name, c.idm, c.jdm, c.kdm, c.ntr, c.params["itrtke"]) == ("chan_s@33x17x3_tke", 33, 17, 3, 5, 1)
    assert c.ic["trc"].shape == (5, 3, 25, 41) and c.depth.shape == (25, 41)
