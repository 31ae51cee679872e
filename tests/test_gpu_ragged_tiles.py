"""Ragged tile tables (land-tile elimination, phy/mod_xc.F90:1332-1990) on the device: every non-empty tile of a
land-eliminated layout is a context of one in-process group (halo.hip: k_xctilr_tiles_ragged, the ragged xcsum and strip
ownership), one host thread per tile, all on one GPU in one process.  Requirement: the single tile's bits on every point a
tile owns, and -- at full size -- the reference's own single-tile checksums (tests/golden/tnx1v4s_tke_edf_crc.json)."""
import json
import os
import threading

import numpy as np
import pytest

import ragged_cases as rc

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run_group(name, nsteps=4, advmth=None, hybrid=None):
    from blom_amd.gpu import TileGroup
    case, masks, ref, lay = rc.build(name, advmth=advmth)
    setup, check = None, list(rc.CHECK)
    if hybrid:                # (vcoord_type, regrid_method): the step of the hybrid coordinate, as tests/test_hostemu_multirank.py
        from test_gpu_tiles import hybrid_inputs
        from blom_amd.hostinit import step_indices
        for nm, a in hybrid_inputs(case).items():
            ref.put(nm, a)
        kk = case.kdm
        pbot = float(np.max(ref.get("p")[kk][masks["ip"] > 0]))
        plevel = 0.3 * pbot * (np.arange(kk) / kk) ** 1.3
        check += ["umfltd", "vmfltd", "umflsm", "vmflsm", "hml_tf", "mld", "bfsqi", "nslpx", "nslpy", "salt_corr", "buoyfl"]

        def setup(g):
            g.set("vcoord_type", hybrid[0])
            g.set("ale_regrid_method", hybrid[1])
            g.set("mlrmth", "fox08")
            g.set("swamxd", 200.0)
            g.set("brine_mlbase_frac", 0.4)
            g.set_vector("plevel", plevel)
            g.stage("cmnfld1", *step_indices(0, kk))
    grp = TileGroup.for_layout(lay)
    tiles, errs = {}, []
    for px, py in lay.tiles():
        tiles[(px, py)] = rc.new_tile(case, masks, ref, lay, px, py)
        grp.attach(tiles[(px, py)], px, py)

    def run(t):
        try:
            if advmth == "cppm":
                t.stage("init_cppm", 2, 1, case.kdm, 0, case.kdm + 1, 1)
            if setup:
                setup(t)
            t.step(0, nsteps)
            t.sync()
        except Exception as e:          # a failing tile would leave the others at a barrier
            errs.append(e)
    rc.run_threads([lambda t=t: run(t) for t in tiles.values()], 300)
    assert not errs, errs
    if advmth == "cppm":
        ref.stage("init_cppm", 2, 1, case.kdm, 0, case.kdm + 1, 1)
    if setup:
        setup(ref)
    assert ref.step(0, nsteps) == nsteps
    bad = rc.compare_owned(ref, tiles, lay, masks, check)
    for t in tiles.values():
        t.close()
    ref.close()
    grp.destroy()
    assert not bad, bad


@pytest.mark.parametrize("name", list(rc.CASES))
def test_ragged_tiles_match_single_tile(name):
    _run_group(name)


@pytest.mark.parametrize("name", ["box_3x2_one_tile_eliminated", "tri_4x2_trimmed_row_under_arctic_row"])
def test_ragged_tiles_with_cppm(name):
    _run_group(name, advmth="cppm")


@pytest.mark.parametrize("name,vcoord,method", [("chan_3x2_gap_row_does_not_wrap", "cntiso_hybrid", "nudge"),
                                                ("tri_4x2_trimmed_row_under_arctic_row", "plevel", "direct")])
def test_ragged_tiles_with_the_hybrid_step(name, vcoord, method):
    _run_group(name, hybrid=(vcoord, method))


def test_full_size_tnx1v4s_as_32_land_eliminated_tiles_reproduces_the_reference_checksums():
    """BASELINE config 5's grid (360 x 385 x 53, arctic patch, ntr = 3, frozen eddy fluxes) cut by eliminate_land into
    8 x 4 tiles -- row 3 ragged: .. (181,20) (247,24) .. -- on one device.  After each recorded step the checksum chained
    over the tiles must be the one the reference's own Fortran produced on ONE tile."""
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd import hostinit
    from blom_amd.cases import make_case
    from blom_amd.checksum import grid_of
    from blom_amd.tiles import TileLayout, scatter_to_tile, chain_crc
    cfg = "tnx1v4s_tke"
    case = make_case(cfg)
    gold = json.load(open(os.path.join(HERE, "golden", f"{cfg}_edf_crc.json")))
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    whole = BlomGpu(case.idm, case.jdm, case.kdm, case.ntr, nreg, masks)
    hostinit.init_state(whole, case)
    hostinit.frozen_eddy_fluxes(whole, case)
    lay = TileLayout.eliminate_land(ip[4:-4, 4:-4], 8, 4, nreg)
    assert lay.nranks == 32 and not lay.is_tensor_product
    assert lay.rows[2][4:6] == ((180, 20), (246, 24)) and lay.rows[3] == TileLayout.regular(360, 385, 8, 4).rows[3]
    grp = TileGroup.for_layout(lay)
    tiles = {}
    for px, py in lay.tiles():
        i0, j0, ii, jj = lay.tile(px, py)
        t = BlomGpu(ii, jj, case.kdm, case.ntr, nreg, {k: lay.window(masks[k], px, py) for k in masks},
                    itdm=case.idm, jtdm=case.jdm, i0=i0, j0=j0)
        for nm, v in case.params.items():
            if not nm.endswith("0"):
                t.set(nm, v)
        scatter_to_tile(whole, t, lay, px, py)
        t.set("delt1", case.params["baclin"])
        t.set("eddtra_frozen", 1)
        grp.attach(t, px, py)
        tiles[(px, py)] = t
    whole.close()
    names = list(gold["crc"]["1"]["tmsmt2"])
    parts, errs = {}, []

    def run(key):
        t = tiles[key]
        try:
            ns = 0
            for step in range(1, gold["nsteps"] + 1):
                ns = t.step(ns, 1)
                for nm in names:
                    if t.has_field(nm):
                        parts[(step, nm, key)] = t.crc_strips(nm, 1, t.field_info(nm)[0], grid_of(nm))
            t.sync()
        except Exception as e:
            errs.append(e)
    th = [threading.Thread(target=run, args=(k,), daemon=True) for k in tiles]
    [x.start() for x in th]
    [x.join(timeout=400) for x in th]
    assert not errs, errs
    assert not any(x.is_alive() for x in th), "a tile did not finish"
    bad, checked = [], 0
    for step in range(1, gold["nsteps"] + 1):
        for nm in names:
            if (step, nm, (0, 0)) not in parts:
                continue
            got = chain_crc({k: parts[(step, nm, k)] for k in tiles}, lay)
            want = gold["crc"][str(step)]["tmsmt2"][nm]
            checked += 1
            if got != want:
                bad.append(f"step {step} {nm}: 0x{got:08x} != 0x{want:08x}")
    for t in tiles.values():
        t.close()
    grp.destroy()
    assert not bad, bad[:20]
    assert checked >= 45
