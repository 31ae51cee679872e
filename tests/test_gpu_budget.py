"""mod_budget inside blomgpu_step (blom_amd/csrc/stage_budget.hip; the options cnsvdi and budget_step): the record of every step and the
lines of salbud tembud tkebud glsbud trcbud trcbudtot against the reference's own sums.

Expected values never come from the code under test: the planes mod_budget sums are restated in numpy (tests/budget_ref.py, pinned on
the compiled routine's util planes by tests/test_budget_ref.py) from the state of the REFERENCE's run at each of the seven calls, and
summed by the reference's compiled xcsum -- or, at sizes the reference has no build for, by the C restatement's (pinned on the
reference by tests/test_oracle_vs_reference.py, tests/test_xcsum.py).  Every comparison is == on doubles.

The checks are functions so that tests/test_hostemu_budget.py runs them on the host emulation."""
import threading

import numpy as np
import pytest

from blom_amd import hostinit, stepper
from blom_amd.cases import make_case
from parity import STATE_FIELDS, GRID_FIELDS, INT_FIELDS, copy_state
import budget_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = ["chan_s", "box_s", "fuk95", "tri_s", "chan_s_tke", "tri_s_tke", "chan_s_tk2"]
# 65 strips (a second round of the strip loop, a last strip of 7 points); a row wider than a workgroup; more rows than the total kernel
# has threads; the arctic seam with a ragged last strip
SIZES = ["chan_s@583x9x3_tke", "chan_s@1030x9x3", "chan_s@20x261x3_tke", "tri_s@31x12x3"]
MODEL_FIELDS = [nm for nm in STATE_FIELDS if not nm.startswith("util")]


def device(case, ntr, nreg, masks, **opts):
    from blom_amd.gpu import BlomGpu
    gpu = BlomGpu(case.idm, case.jdm, case.kdm, ntr, nreg, masks)
    for nm, v in case.params.items():
        if not nm.endswith("0"):
            gpu.set(nm, v)
    for nm, v in opts.items():
        gpu.set(nm, v)
    return gpu


def oracle_for(cfg, which):
    """(case, backend at nstep = 0, its xcsum of a plane): the compiled reference, or the C restatement"""
    case = make_case(cfg)
    if which == "ref":
        from oracle.refblom import get_ref_backend, have_ref
        if not have_ref(cfg):
            pytest.skip(f"oracle/_ref/{cfg}/libblomref.so not built")
        be = get_ref_backend(cfg, case.depth)
        xc = lambda a: be.xcsum(a, 1)
    else:
        from oracle.coracle import COracle, have_coracle
        if not have_coracle():
            pytest.skip("oracle/_ref/liboracle_c.so not built")
        nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
        be = COracle(case.idm, case.jdm, case.kdm, case.ntr, nreg, dict(ip=ip, iu=iu, iv=iv, iq=iq))
        for nm, v in case.params.items():
            if not nm.endswith("0"):
                be.set(nm, v)

        def xc(a):
            be.put("util3", np.asarray(a)[None])
            return be.xcsum("util3", 1, 1)
    hostinit.init_state(be, case)
    return case, be, xc


def same_record(got, want):
    return [nm for nm in want if not np.array_equal(np.asarray(got[nm]), np.asarray(want[nm]))]


def tdp_differences(prev, cur):
    x = list(prev["tdp"][:5]) + list(cur["tdp"][5:])
    return [x[k + 1] - x[k] for k in range(6)]


# ---- a, b: records and lines against the reference ---------------------------------------------------------------------------------------
def check_records(cfg, which="ref", nsteps=5):
    from blom_amd.gpu import BlomGpuError
    case, be, xc = oracle_for(cfg, which)
    nt = R.tracer_set(be.ntr, case.params)
    frc = R.seeded_forcing(case, be.ntr)
    gpu = device(case, be.ntr, be.nreg, be.masks, cnsvdi=1, budget_step=1)
    try:
        copy_state(be, gpu)
        for nm, a in frc.items():
            gpu.put(nm, a)
            if be.has_field(nm):
                be.put(nm, a)
        gpu.set("delt1", case.params["baclin"])
        gpu.budget_init()
        assert gpu.step(0, nsteps) == nsteps                          # ONE call
        mass0, want = R.reference_run(R.WithPlanes(be, frc), xc, case, nsteps, nt)
        assert gpu.budget_mass0() == mass0 != 0.0
        assert gpu.budget_steps() == (1, nsteps)
        got = [gpu.budget_record(s + 1) for s in range(nsteps)]
        for s in range(nsteps):
            print(cfg, "step", s + 1, "tdp", got[s]["tdp"], "sc sf tf trf", got[s]["sc"], got[s]["sf"], got[s]["tf"], got[s]["trf"])
            assert not same_record(got[s], want[s]), (cfg, s + 1, same_record(got[s], want[s]))
            # not vacuous
            for nm in ("sdp", "tdp") + (("trdp",) if nt >= 1 else ()) + (("tkedp",) if nt >= 2 else ()) + (("glsdp",) if nt >= 3 else ()):
                assert np.all(want[s][nm] != 0.0), (cfg, s + 1, nm)
            assert want[s]["sc"] != 0.0 and want[s]["sf"] != 0.0 and want[s]["tf"] != 0.0 and (want[s]["trf"] != 0.0) == (nt >= 1)
        with pytest.raises(BlomGpuError, match="has no line"):
            gpu.budget_line(1, "salbud")
        lines = gpu.budget_lines()
        assert sorted(lines) == sorted(R.files_of(nt))
        for f in R.files_of(nt):
            assert list(lines[f][0]) == list(range(1, nsteps))
            for s in range(2, nsteps + 1):
                terms = R.line_terms(want[s - 2], want[s - 1], mass0, f)
                assert list(gpu.budget_line(s, f)) == terms == list(lines[f][1][s - 2]), (cfg, s, f)
        for s in range(2, nsteps + 1 if which == "ref" else 0):     # (the families' five steps; two steps from rest at the other sizes do not move every term)
            d = tdp_differences(want[s - 2], want[s - 1])
            assert d[0] != 0.0 and d[4] != 0.0 and d[5] != 0.0, (cfg, s, d)
        if case.nreg == 2:
            # the seam row holds data that the sum leaves out
            seam = R.column_planes(R.WithPlanes(be, frc), case, 0, nt)["tdp"][R.NB + case.jdm - 1]
            assert seam.any()
        # what budget_get sees: the last step's calls under its time levels
        m, n = (nsteps - 1) % 2 + 1, nsteps % 2 + 1
        assert gpu.budget_get("tdp", 3, n) == want[-1]["tdp"][2] and gpu.budget_get("sdp", 7, m) == want[-1]["sdp"][6]
        return got
    finally:
        gpu.close()


@pytest.mark.parametrize("cfg", FAMILIES)
def test_records_and_lines_of_five_steps_in_one_call_equal_the_reference(cfg):
    check_records(cfg)


@pytest.mark.parametrize("cfg", SIZES)
def test_row_shapes_the_families_do_not_reach(cfg):
    check_records(cfg, which="c", nsteps=2)


# ---- c: placement ------------------------------------------------------------------------------------------------------------------------
def placement_context(config):
    if config == "hybrid":
        from test_gpu_stepend import context
        case, masks, g = context("chan_s", hybrid=True)
        # (this step has no thermf: the heat and salt fluxes ale_forcing applies are uploaded, of both signs)
        nj, ni = case.jdm + 2 * R.NB, case.idm + 2 * R.NB
        y = np.linspace(-1.0, 1.0, nj)[:, None] + np.zeros((1, ni))
        x = np.linspace(0.0, 2 * np.pi, ni)[None, :] + np.zeros((nj, 1))
        swa, nsf = 120.0 * (1.0 + np.cos(x)), 300.0 * (y + 0.3 * np.sin(x))
        g.put("surflx", -(swa + nsf)[None])
        g.put("sswflx", -swa[None])
        g.put("salflx", (2.0e-3 * np.sin(x) * y)[None])
        return case, g, stepper.HYBRID_STAGES
    import test_gpu_diaacc as lyr
    case, masks, g = lyr.full_context("chan_s_tke")
    destabilise(g, case, masks)
    return case, g, stepper.FULL_STAGES_LIVE


def destabilise(g, case, masks, dtemp=12.0):
    """the case strengthened: the two mixed layers start up to `dtemp` K colder than at rest, colder than the layers below them (both time
    levels, halos included, sigma kept consistent), so that convec finds unstable columns and diapfl layers to mix from the first step on.
    Both stages conserve heat: what they leave in the 2nd and 3rd difference of tdp is the rounding of the columns they rewrite, and it
    takes this many rewritten columns for it to reach the last bits of a total of 5e17."""
    from blom_amd.cases import sig
    kk = case.kdm
    temp, saln, sigma = g.get("temp"), g.get("saln"), g.get("sigma")
    nj, ni = temp.shape[1:]
    wet = np.asarray(masks["ip"]).reshape(nj, ni) > 0
    y = np.linspace(0.0, 1.0, nj)[:, None] + np.zeros((1, ni))
    dt = dtemp * np.exp(-(y - 0.5) ** 2)
    for lev in (0, 1, kk, kk + 1):
        temp[lev] = np.where(wet, temp[lev] - dt, temp[lev])
        sigma[lev] = np.where(wet, sig(temp[lev], saln[lev], case.params.get("pref", 2000.0e4)), sigma[lev])
    g.put("temp", temp)
    g.put("sigma", sigma)


def check_placement(config, nsteps=5):
    """full physics with live diffusivities / the hybrid step: one call of five steps == five calls of one == the stages of
    with_budget(...) one by one, in records, lines and model fields; the model fields also == a run without the option"""
    runs = {}
    for mode in ("one", "five", "staged", "off"):
        case, g, stages = placement_context(config)
        try:
            g.set("cnsvdi", 1)
            g.set("budget_step", 0 if mode in ("off", "staged") else 1)
            g.budget_init()
            recs, lines = {}, {}

            def collect():
                first, count = g.budget_steps()
                for s in range(first, first + count):
                    recs[s] = g.budget_record(s)
                for f, (steps, terms) in g.budget_lines().items():
                    for s, t in zip(steps, terms):
                        lines[(int(s) + 1, f)] = list(t)
            if mode == "one" or mode == "off":
                assert g.step(0, nsteps) == nsteps
                collect()
            elif mode == "five":
                for s in range(nsteps):
                    assert g.step(s, 1) == s + 1
                    collect()
            else:
                ns = 0
                for _ in range(nsteps):
                    ns = stepper.dyncore_step(g, ns, case.params["baclin"], stages=stepper.with_budget(stages))
                collect()
            runs[mode] = (recs, lines, {nm: g.get(nm) for nm in MODEL_FIELDS if g.has_field(nm)})
        finally:
            g.close()
    recs, lines, fields = runs["one"]
    assert sorted(recs) == list(range(1, nsteps + 1)) and not runs["off"][0] and not runs["off"][1]
    nfiles = len({f for _, f in lines})
    assert len(lines) == (nsteps - 1) * nfiles and nfiles >= 2
    for mode in ("five", "staged"):
        r2, l2, f2 = runs[mode]
        assert sorted(r2) == sorted(recs), (config, mode, sorted(r2))
        for s in recs:
            assert not same_record(r2[s], recs[s]), (config, mode, s, same_record(r2[s], recs[s]))
        assert l2 == lines, (config, mode)
    for mode in ("five", "staged", "off"):
        bad = [nm for nm in fields if not np.array_equal(fields[nm], runs[mode][2][nm], equal_nan=True)]
        assert not bad, (config, mode, bad)
    # here thermf, mxlayr, diapfl and convec (ale_forcing, ale_vdifft) change the sums: every difference is nonzero in some line
    diffs = np.array([tdp_differences(recs[s - 1], recs[s]) for s in range(2, nsteps + 1)])
    print(config, "tdp differences of the lines 2..%d:\n" % nsteps, diffs)
    moved = (diffs != 0.0).any(axis=0)
    if config == "hybrid":
        # blom_step has nothing but updtrc between the calls 4 and 5 of this coordinate (phy/mod_blom_step.F90:205-215), and updtrc writes
        # no temperature: the 4th difference of tdp is 0 in every line by the reference's own placement, whatever the forcing.  The
        # other five move.
        assert list(moved) == [True, True, True, False, True, True], diffs
    else:
        assert moved.all(), diffs
    return recs


@pytest.mark.parametrize("config", ["full", "hybrid"])
def test_one_call_equals_single_steps_equals_the_staged_run(config):
    check_placement(config)


# ---- d: the coupled context: sc, sf, tf, trf from live stages ------------------------------------------------------------------------------
def coupled_context():
    """the coupled experiment's context of tests/test_gpu_thermf_cesm.py on chan_s, made to produce all four sums: tracer 1 is a passive
    tracer there once the ideal-age step is off (thermf_cesm gives the TKE tracer of the _tke cases a zero flux by definition,
    cesm/mod_thermf_cesm.F90:165-186), and a patch of the coupler's salt flux is strong enough to take the mixed layer's salt out within
    a step, so that mxlayr's copy-back rule books a correction in salt_corr in every step"""
    import test_gpu_thermf_cesm as tc
    case, masks, g = tc.context("chan_s", dict(tc.BASE))
    g.set("itriag", 0)
    sfl = g.get("sfl_da")
    sfl[:, 10:14, 8:13] = -0.2
    g.put("sfl_da", sfl)
    return case, masks, g


def check_coupled(nsteps=3):
    """The coupled context: salt_corr (thermf_cesm, mxlayr), salflx salrlx surflx surrlx trflx are written by the step's own stages.  A RESTATEMENT CHECK, not a pin: a stage-by-stage run stops in front of every budget
    pseudo-stage, the planes are restated in numpy from the device's own fields at that place and summed by the C restatement's xcsum;
    the staged run's records and the records of ONE blomgpu_step call of `nsteps` steps must both == those numbers -- so the in-step
    launches read what the live writers have left at the reference's places."""
    from oracle.coracle import COracle, have_coracle
    if not have_coracle():
        pytest.skip("oracle/_ref/liboracle_c.so not built")
    case, masks, a = coupled_context()
    _, _, b = coupled_context()
    orc = COracle(case.idm, case.jdm, case.kdm, case.ntr, case.nreg, masks)

    def xc(plane):
        orc.put("util3", np.asarray(plane)[None])
        return orc.xcsum("util3", 1, 1)
    try:
        nt = R.tracer_set(case.ntr, case.params)
        baclin = case.params["baclin"]
        for g in (a, b):
            g.set("cnsvdi", 1)
            g.budget_init()
        assert a.budget_mass0() == b.budget_mass0() == xc(R.mass_plane(b, case)) != 0.0
        a.set("budget_step", 1)
        assert a.step(0, nsteps) == nsteps
        stages = stepper.with_budget(stepper.FULL_STAGES_LIVE_CESM)
        ns, delt1, want = 0, b.get_real("delt1"), []
        for _ in range(nsteps):
            rec = R.new_record()

            def hook(st, six, rec=rec, delt1=delt1):
                if st.startswith("budget_sums"):
                    ncall = int(st[-1])
                    R.fill_call(rec, b, xc, case, ncall, six[3] if ncall <= 5 else six[2], nt)
                elif st == "budget_output":
                    R.fill_output(rec, b, xc, case, delt1, nt)
            ns = stepper.dyncore_step(b, ns, baclin, stages=stages, hook=hook)
            delt1 = baclin + baclin
            want.append(rec)
        for s in range(1, nsteps + 1):
            w = want[s - 1]
            print("coupled step", s, "sc sf tf trf", w["sc"], w["sf"], w["tf"], w["trf"])
            assert w["sc"] != 0.0 and w["sf"] != 0.0 and w["tf"] != 0.0 and w["trf"] != 0.0, (s, w)
            assert np.all(w["tdp"] != 0.0) and np.all(w["sdp"] != 0.0) and np.all(w["trdp"] != 0.0)
            assert not same_record(b.budget_record(s), w), ("staged", s, same_record(b.budget_record(s), w))
            assert not same_record(a.budget_record(s), w), ("one call", s, same_record(a.budget_record(s), w))
        for f in R.files_of(nt):
            for s in range(2, nsteps + 1):
                assert list(a.budget_line(s, f)) == R.line_terms(want[s - 2], want[s - 1], a.budget_mass0(), f), (f, s)
        # the live stages did write the planes between the steps
        assert want[0]["sc"] != want[1]["sc"] and want[0]["tf"] != want[1]["tf"]
    finally:
        a.close()
        b.close()


def test_coupled_context_live_fluxes_equal_the_restatement():
    check_coupled()


# ---- e: tiles ----------------------------------------------------------------------------------------------------------------------------
def check_tiles(npx, npy, cfg="chan_s_tke", nsteps=3):
    from blom_amd.gpu import BlomGpu, TileGroup
    from blom_amd.tiles import tile_extents, tile_window, scatter_state
    case = make_case(cfg)
    nreg, _, ip, iu, iv, iq = hostinit.bigrid_np(case.depth, case.idm, case.jdm, arctic=case.nreg == 2)
    masks = dict(ip=ip, iu=iu, iv=iv, iq=iq)
    opts = dict(cnsvdi=1, budget_step=1, delt1=case.params["baclin"])
    ref = device(case, case.ntr, nreg, masks, **opts)
    hostinit.init_state(ref, case)
    frc = R.seeded_forcing(case, case.ntr)
    ii, jj = tile_extents(case, npx, npy)
    grp = TileGroup(npx, npy)
    tiles = {}
    try:
        for nm, a in frc.items():
            ref.put(nm, a)
        for py in range(npy):
            for px in range(npx):
                tm = {k: tile_window(masks[k], case, npx, npy, px, py) for k in masks}
                t = BlomGpu(ii, jj, case.kdm, case.ntr, nreg, tm, itdm=case.idm, jtdm=case.jdm, i0=px * ii, j0=py * jj)
                for nm, v in list(case.params.items()) + list(opts.items()):
                    if not nm.endswith("0"):
                        t.set(nm, v)
                grp.attach(t, px, py)
                for nm, a in frc.items():
                    t.put(nm, tile_window(a, case, npx, npy, px, py))
                tiles[(px, py)] = t
        scatter_state(ref, tiles, case, npx, npy, [f for f in STATE_FIELDS + GRID_FIELDS + INT_FIELDS if ref.has_field(f)])
        errs = []

        def run(g):
            try:
                g.budget_init()
                g.step(0, nsteps)
                g.sync()
            except Exception as e:          # a failing tile would leave the others at a barrier
                errs.append(e)
        run(ref)
        th = [threading.Thread(target=run, args=(t,), daemon=True) for t in tiles.values()]
        [x.start() for x in th]
        [x.join(timeout=300) for x in th]
        assert not errs, errs
        want = [ref.budget_record(s) for s in range(1, nsteps + 1)]
        assert all(np.all(r["tdp"] != 0.0) and r["sf"] != 0.0 for r in want)
        for key, t in tiles.items():
            assert t.budget_mass0() == ref.budget_mass0(), key
            for s in range(1, nsteps + 1):
                assert not same_record(t.budget_record(s), want[s - 1]), (key, s)
            assert {f: [list(x) for x in v[1]] for f, v in t.budget_lines().items()} == \
                   {f: [list(x) for x in v[1]] for f, v in ref.budget_lines().items()}
    finally:
        for t in tiles.values():
            t.close()
        ref.close()
        grp.destroy()


@pytest.mark.parametrize("npx,npy", [(2, 1), (1, 2)])
def test_every_tile_of_a_group_holds_the_single_tiles_records(npx, npy):
    check_tiles(npx, npy)


# ---- f: off and refusals -----------------------------------------------------------------------------------------------------------------
def check_off_and_refusals():
    from blom_amd.gpu import BlomGpuError
    import ctypes as C
    import test_gpu_diaacc as lyr
    case, masks, g = lyr.dyncore_context("chan_s_tke", delt1=make_case("chan_s_tke").params["baclin"])
    try:
        # the option without cnsvdi: nothing is launched, nothing recorded (phy/mod_budget.F90:105)
        g.set("budget_step", 1)
        g.set("cnsvdi", 0)
        g.set("timing", 1)
        g.budget_init()
        assert g.step(0, 2) == 2
        assert g.timer_get("budget")[1] == 0 and g.timer_get("budget_output")[1] == 0
        assert g.timer_get("tmsmt")[1] > 0
        assert g.budget_steps()[1] == 0 and not g.budget_lines()
        with pytest.raises(BlomGpuError, match="blomgpu_budget_record: no record of step 2"):
            g.budget_record(2)
        with pytest.raises(BlomGpuError, match="blomgpu_budget_line: no record of step 2"):
            g.budget_line(2, "tembud")
        with pytest.raises(BlomGpuError, match="budget_init has not run"):
            g.budget_mass0()
        # on: call 1 of the first step of a call, calls 2..7 of every step, budget_output every step
        g.set("cnsvdi", 1)
        g.budget_init()
        assert g.step(2, 3) == 5
        assert g.timer_get("budget")[1] == 1 + 6 * 3 and g.timer_get("budget_output")[1] == 3
        g.set("timing", 0)
        assert g.budget_steps() == (3, 3)
        with pytest.raises(BlomGpuError, match="step 3 has no line: no record of step 2"):
            g.budget_line(3, "tembud")
        with pytest.raises(BlomGpuError, match="does not call for glsbud"):
            g.budget_line(4, "glsbud")
        assert g.budget_files() == ["salbud", "tembud", "tkebud", "trcbud", "trcbudtot"]
        plain = [g.budget_record(s) for s in (3, 4, 5)]
        # the step before a call stays: a line for the call's first step
        assert g.step(5, 1) == 6 and g.budget_steps() == (5, 2) and len(g.budget_line(6, "tembud")) == 6
        # glsdp through budget_get; a sixth quantity is refused
        assert g.budget_get("glsdp", 2, 1) == 0.0 and g.budget_get("tkedp", 2, 1) != 0.0
        v = C.c_double(0.0)
        assert g.lib.blomgpu_budget_get(g.ctx, 5, 1, 1, C.byref(v)) != 0
        # the option is one of a table of its own
        buf, k, listed = C.create_string_buffer(64), 0, []
        while g.lib.blomgpu_option_name(k, buf, 64, None) == 0:
            listed.append(buf.value.decode())
            k += 1
        assert "budget_step" not in listed and "cnsvdi" in listed
    finally:
        g.close()
    # use_graph = 1: the budgeted step runs as plain launches, to the same records
    case, masks, g = lyr.dyncore_context("chan_s_tke", delt1=case.params["baclin"], cnsvdi=1, budget_step=1, use_graph=1)
    try:
        g.budget_init()
        assert g.step(0, 2) == 2 and g.step(2, 3) == 5
        assert g.get_real("graph_steps") == 0
        for s, want in zip((3, 4, 5), plain):
            assert not same_record(g.budget_record(s), want), s
    finally:
        g.close()


def test_off_refusals_and_graphs():
    check_off_and_refusals()


# ---- g: the Fortran host ------------------------------------------------------------------------------------------------------------------
def fortran_exe():
    import os
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "blom_amd", "lib", "blom_dyncore")
    if not os.path.exists(exe):
        pytest.skip("Fortran driver not built")
    return exe


@pytest.mark.parametrize("cnsvdi", [True, False])
def test_fortran_host_on_a_limits_file_writes_the_files_only_with_cnsvdi(tmp_path, cnsvdi):
    from blom_amd.gpu import BlomGpu
    from test_fortran_budget_host import run_limits
    run_limits(tmp_path, fortran_exe(), BlomGpu, cnsvdi)


@pytest.mark.parametrize("cfg,full", [("chan_s_tke", True), ("chan_s_tke", False), ("chan_s", False)])
def test_fortran_host_writes_the_six_files_on_the_device(tmp_path, cfg, full):
    from test_fortran_budget_host import run_host, check_files
    nt, lines = run_host(tmp_path, cfg, full, 1, exe=fortran_exe(), lib=None)
    check_files(tmp_path, nt, lines)
