"""`program blom_dyncore` as N ranks (blom_amd/fortran): every process reads the same state file and the tile table
`patch.input` (the reference's format, xcspmd), keeps its window, joins the RCCL transport through the id file rank 0
writes, runs the stage sequence on its tile and takes part in the checksums (blomgpu_rccl_crc), which rank 0 prints.
Here the processes run the program linked against the host emulation of the device library (tests/hostemu), whose RCCL
stand-in carries messages between processes as files (BLOM_HOSTEMU_RCCL_DIR).  Requirement: rank 0's chksum lines equal
the single tile's after the same steps, and setups xcspmd would refuse end every process at once with the reason."""
import os
import re
import subprocess
import threading
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "hostemu", "libblomgpu_hostemu.so")
EXE = os.path.join(HERE, "hostemu", "blom_dyncore_hostemu")
pytestmark = pytest.mark.skipif(not (os.path.exists(EMU) and os.path.exists(EXE)), reason="tests/hostemu not built")

CRC_RE = re.compile(r"chksum: (\w+): 0x([0-9A-Fa-f]+)")


@pytest.fixture()
def emu_lib():
    import blom_amd.gpu as g
    old = g.LIB_PATH
    g.LIB_PATH = EMU
    yield
    g.LIB_PATH = old


def _state_names(be):
    return [n for n in be.field_names() if n not in ("mpack", "ip", "iu", "iv", "iq") and not n.startswith("wkp")]


def write_case(path, cfg, nsteps, full=False):
    """state file of case `cfg` (every registered field) for `nsteps` steps; returns the single tile's checksums after them
    (BlomGpu.crc of the backend LIB_PATH names), as the host prints them.  full: config 2's step (option record full_physics)
    with a surface forcing, thermf's ocean area the whole domain's as in test_hostemu_multirank._run_case"""
    from blom_amd.statefile import write_state
    from test_gpu_tiles import _single
    case, masks, fields, ref = _single(cfg, nsteps)
    if full:
        from blom_amd import hostinit
        hostinit.init_forcing(ref, case)
        nj, ni = case.jdm + 8, case.idm + 8
        yy = np.linspace(-1.0, 1.0, nj)[:, None] + 0.0 * np.arange(ni)[None, :]
        ref.put("nsf", (300.0 * yy)[None])
        ref.put("swa", (120.0 * (yy > -0.5))[None])
        ref.put("eva", (-2e-5 * np.ones((nj, ni)))[None])
        w = masks["ip"][4:-4, 4:-4] > 0
        if case.nreg == 2:
            w = w.copy()
            w[-1, :] = False
        case.params["area"] = float(np.sum(ref.get("scp2")[0][4:-4, 4:-4][w]))
        case.params["niwgf"] = 0.4
        case.params["full_physics"] = 1
        for nm in ("area", "niwgf", "full_physics"):
            ref.set(nm, case.params[nm])
    write_state(path, ref, case, nsteps, _state_names(ref))
    ref.set("delt1", case.params["baclin"])
    assert ref.step(0, nsteps) == nsteps
    kk = case.kdm
    want = {"dp": ref.crc("dp", 1, 2 * kk, 1), "temp": ref.crc("temp", 1, 2 * kk, 1), "u": ref.crc("u", 1, 2 * kk, 13)}
    ref.close()
    return case, want


def run_ranks(exe, cwd, n, timeout, stop_on_failure=True, local_rank=lambda r: 0, emulated=True):
    """start n processes of `exe` in `cwd` with torchrun's rank variables; every one under `timeout` seconds, the others
    killed when one fails (stop_on_failure).  emulated: the host emulation's RCCL mailbox between the processes.  Returns
    [(returncode, output)] by rank and the seconds it took."""
    env0 = {k: v for k, v in os.environ.items() if k not in ("BLOM_RUN_TOKEN", "RANK", "WORLD_SIZE", "LOCAL_RANK")}
    if emulated:
        env0["BLOM_HOSTEMU_RCCL_DIR"] = os.path.join(cwd, "rccl_box")
        os.makedirs(env0["BLOM_HOSTEMU_RCCL_DIR"], exist_ok=True)
    procs, logs = [], []
    t0 = time.monotonic()
    for r in range(n):
        env = dict(env0, RANK=str(r), WORLD_SIZE=str(n), LOCAL_RANK=str(local_rank(r)), BLOM_RCCL_ID_FILE=os.path.join(cwd, "rccl_id"))
        log = open(os.path.join(cwd, f"rank{r}.log"), "w")
        logs.append(log)
        procs.append(subprocess.Popen([exe, "blom_state.bin"], cwd=cwd, env=env, stdout=log, stderr=subprocess.STDOUT))
    try:
        while any(p.poll() is None for p in procs):
            if time.monotonic() - t0 > timeout or (stop_on_failure and any(p.poll() not in (None, 0) for p in procs)):
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for log in logs:
            log.close()
    took = time.monotonic() - t0
    outs = [(p.returncode, open(os.path.join(cwd, f"rank{r}.log")).read()) for r, p in enumerate(procs)]
    return outs, took


def checksums(out):
    return {m.group(1): int(m.group(2), 16) for m in CRC_RE.finditer(out)}


def run_tiled(tmp_path, cfg, isizes, jsizes, nsteps=2, full=False, timeout=900, exe=EXE, local_rank=lambda r: 0, emulated=True):
    """state file + patch.input of the layout isizes x jsizes in tmp_path, one process per tile: rank 0's checksums must be
    the single tile's"""
    from blom_amd.tiles import TileLayout
    case, want = write_case(str(tmp_path / "blom_state.bin"), cfg, nsteps, full)
    lay = TileLayout(tuple(isizes), tuple(jsizes))
    assert (lay.itdm, lay.jtdm) == (case.idm, case.jdm)
    lay.write_patch_input(str(tmp_path / "patch.input"), case.nreg)
    outs, _ = run_ranks(exe, str(tmp_path), lay.npx * lay.npy, timeout, local_rank=local_rank, emulated=emulated)
    for r, (rc, out) in enumerate(outs):
        assert rc == 0, f"rank {r} exited with {rc}:\n{out[-3000:]}"
    got = checksums(outs[0][1])
    assert got == want, (got, want)
    # only rank 0 prints them, once
    assert len(CRC_RE.findall(outs[0][1])) == len(want)
    assert all(not CRC_RE.search(out) for _, out in outs[1:])
    assert open(tmp_path / "run.status").read().strip() == "success"
    assert not os.path.exists(tmp_path / "rccl_id"), "rank 0 leaves the id file behind"
    return got


@pytest.mark.parametrize("cfg,isizes,jsizes", [
    ("chan_s", (10, 10), (24,)),                 # 2 x 1
    ("chan_s", (10, 10), (12, 12)),              # 2 x 2
    ("tri_s_tke", (6, 6, 6, 6), (10, 10)),       # the shape of the reference's tnx2v1 patch.input.8, arctic fold
])
def test_ranks_match_single_tile(emu_lib, tmp_path, cfg, isizes, jsizes):
    run_tiled(tmp_path, cfg, isizes, jsizes)


def test_ranks_run_the_full_physics_step(emu_lib, tmp_path):
    """option record full_physics: thermf's two global sums across the processes (on the global context of the replicated
    barotropic solve), mxlayr, the front of difest_isobml, cmnfld1/2"""
    run_tiled(tmp_path, "chan_s_tke", (10, 10), (13, 11), nsteps=2, full=True)


def test_one_rank_with_a_1x1_table_equals_the_run_without_one(emu_lib, tmp_path):
    """a 1x1 patch.input on one rank takes the whole tiled path (tile context, global context, RCCL with itself,
    blomgpu_rccl_crc) and must print what the single-context path prints"""
    tiled = tmp_path / "tiled"
    plain = tmp_path / "plain"
    tiled.mkdir()
    plain.mkdir()
    got = run_tiled(tiled, "chan_s", (20,), (24,))
    write_case(str(plain / "blom_state.bin"), "chan_s", 2)
    outs, _ = run_ranks(EXE, str(plain), 1, 600)
    assert outs[0][0] == 0, outs[0][1][-3000:]
    assert checksums(outs[0][1]) == got


def _edit_rows(txt):
    """cut tile row 2 differently: (12, 8) instead of (10, 10)"""
    txt = re.sub(r"(?m)^ispt\(  2\) =.*$", "ispt(  2) = " + "".join(f"{v:6d}" for v in (1, 13)), txt)
    return re.sub(r"(?m)^iipe\(  2\) =.*$", "iipe(  2) = " + "".join(f"{v:6d}" for v in (12, 8)), txt)


@pytest.mark.parametrize("what,nranks,isizes,jsizes,edit,message", [
    ("rows cut differently", 4, (10, 10), (12, 12), _edit_rows, "tile rows are cut differently"),
    ("npes is not WORLD_SIZE", 2, (10, 10), (12, 12), None, "npes = 4 ranks but WORLD_SIZE = 2"),
    ("tiles do not cover the state", 4, (10, 12), (12, 12), None, "the tiles cover 22 x 24 points but the state is idm x jdm = 20 x 24"),
])
def test_refused_layouts_end_every_rank(emu_lib, tmp_path, what, nranks, isizes, jsizes, edit, message):
    from blom_amd.tiles import TileLayout
    case, _ = write_case(str(tmp_path / "blom_state.bin"), "chan_s", 1)
    lay = TileLayout(tuple(isizes), tuple(jsizes))
    lay.write_patch_input(str(tmp_path / "patch.input"), case.nreg)
    if edit:
        txt = open(tmp_path / "patch.input").read()
        open(tmp_path / "patch.input", "w").write(edit(txt))
    outs, took = run_ranks(EXE, str(tmp_path), nranks, 60, stop_on_failure=False)
    for r, (rc, out) in enumerate(outs):
        assert rc != 0 and message in out, (what, r, rc, out[-2000:])
    assert took < 30, f"{what}: the ranks took {took:.0f} s to give up"
    assert not os.path.exists(tmp_path / "rccl_id") and not os.path.exists(tmp_path / "run.status")


def test_several_ranks_without_a_table_are_refused(emu_lib, tmp_path):
    write_case(str(tmp_path / "blom_state.bin"), "chan_s", 1)
    outs, took = run_ranks(EXE, str(tmp_path), 2, 60, stop_on_failure=False)
    for rc, out in outs:
        assert rc != 0 and "no patch.input" in out, out[-2000:]
    assert took < 30


@pytest.mark.parametrize("cfg,isizes,jsizes", [("chan_s", (10, 10), (12, 12)), ("tri_s", (12, 12), (11, 9))])
def test_rccl_crc_on_thread_ranks_equals_the_single_tile(emu_lib, cfg, isizes, jsizes):
    """BlomGpu.rccl_crc (blomgpu_rccl_crc) on ranks that are threads of this process, set up as in
    test_hostemu_multirank._run_case: every rank gets the single tile's checksum"""
    from blom_amd.gpu import BlomGpu, rccl_unique_id
    from blom_amd.tiles import TileLayout, scatter_to_tile
    from test_gpu_tiles import _single
    nsteps = 2
    case, masks, fields, ref = _single(cfg, nsteps)
    lay = TileLayout(tuple(isizes), tuple(jsizes))
    uid = rccl_unique_id()
    kk = case.kdm
    crc_fields = [("dp", 1, 2 * kk, 1), ("u", 1, 2 * kk, 3), ("v", 1, 2 * kk, 4), ("pb", 1, 2, 1)]
    n = lay.npx * lay.npy
    got, errs, tiles = {}, [], []
    lock = threading.Lock()
    barrier = threading.Barrier(n)

    def rank_main(rank):
        try:
            px, py = lay.rank_tile(rank)
            i0, j0, ii, jj = lay.tile(px, py)
            t = BlomGpu(ii, jj, kk, case.ntr, case.nreg, {k: lay.window(masks[k], px, py) for k in masks},
                        itdm=case.idm, jtdm=case.jdm, i0=i0, j0=j0)
            with lock:
                tiles.append(t)
            for nm, v in case.params.items():
                if not nm.endswith("0"):
                    t.set(nm, v)
            t.set("delt1", case.params["baclin"])
            with lock:
                scatter_to_tile(ref, t, lay, px, py)
            t.rccl_init_2d(uid, rank, lay.npx, lay.npy)
            barrier.wait()
            assert t.step(0, nsteps) == nsteps
            got[rank] = {f[0]: t.rccl_crc(*f) for f in crc_fields}
        except Exception as e:                            # a failing rank would leave the others waiting
            errs.append(e)
            barrier.abort()

    th = [threading.Thread(target=rank_main, args=(r,)) for r in range(n)]
    [x.start() for x in th]
    [x.join(timeout=600) for x in th]
    assert not errs, errs
    assert ref.step(0, nsteps) == nsteps
    want = {f[0]: ref.crc(*f) for f in crc_fields}
    assert ref.rccl_crc(*crc_fields[0]) == want["dp"]       # no RCCL on the context: blomgpu_crc
    for t in tiles:
        t.rccl_finalize()
        t.close()
    ref.close()
    assert len(got) == n
    for rank, g in got.items():
        assert g == want, (rank, g, want)


def test_write_patch_input_round_trips_the_reference_layout(tmp_path):
    from blom_amd.tiles import TileLayout
    src = os.path.join(HERE, "golden", "tnx2v1_patch.input.8")
    lay = TileLayout.from_patch_input(src)
    dst = str(tmp_path / "patch.input")
    lay.write_patch_input(dst, 2)
    back = TileLayout.from_patch_input(dst)
    assert back == lay and back.isizes == (45, 45, 45, 45) and back.jsizes == (97, 96)
    mine, ref = open(dst).read().splitlines(), open(src).read().splitlines()
    assert mine[1].split() == ref[1].split()[:8]            # npes npe mpe idm jdm ibig jbig nreg
    assert mine[2:] == ref[2:]                              # the tile rows and columns, character for character
