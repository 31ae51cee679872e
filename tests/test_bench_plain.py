"""bench.py with and without --full, end to end on the CPU: the same command the driver runs (`bench.py --gpus 1 --steps K
--warmup W`) with `--backend gloo` (no torch.cuda call) and BLOMGPU_LIB pointing at the host emulation of the library
(tests/hostemu).  A plain run stops after the timed steps and --dump-outputs; --full goes on with the measurements and checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "hostemu", "libblomgpu_hostemu.so")

# what --full adds to the line (chan_s on one tile: no spunup beyond --spunup-steps 0, no CPU baseline with --no-cpu-baseline)
EXTRAS = ("roofline", "class_roofline", "step_roofline", "stages_ms", "ms_per_step_blocks", "ms_per_step_median", "cpu_baseline", "spunup",
          "dyncore_only")


def _bench(tmp_path, name, extra):
    if not os.path.exists(EMU):
        pytest.skip("tests/hostemu/libblomgpu_hostemu.so not built")
    box = tmp_path / f"mail_{name}"
    box.mkdir()
    env = dict(os.environ, BLOMGPU_LIB=EMU, BLOM_HOSTEMU_RCCL_DIR=str(box), OMP_NUM_THREADS="1")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--config", "chan_s", "--steps", "3", "--warmup", "2", "--backend", "gloo",
           "--dump-outputs", str(tmp_path / f"dump_{name}"), *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    return json.loads(lines[0])


def test_a_plain_bench_run_prints_the_headline_only(tmp_path):
    """Without --full the line carries the headline and no figure of the measurements --full adds; with --full (or an option that
    shapes those measurements) they are there.  All three runs write the same state, and the headline's keys mean the same."""
    plain = _bench(tmp_path, "plain", ())
    full = _bench(tmp_path, "full", ("--full", "--no-cpu-baseline", "--no-dyncore-compare", "--spunup-steps", "0"))
    implied = _bench(tmp_path, "implied", ("--blocks", "2", "--no-cpu-baseline", "--no-dyncore-compare", "--spunup-steps", "0"))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "scaling"):
        for d in (full, implied):
            assert k in plain and k in d, k
            if k not in ("value", "ms_per_step"):
                assert plain[k] == d[k], (k, plain[k], d[k])
    # value = baclin / 86400 / (ms_per_step / 1e3) in every run
    assert plain["ms_per_step"] > 0.0 and plain["value"] * plain["ms_per_step"] == pytest.approx(full["value"] * full["ms_per_step"])
    for k in EXTRAS:
        assert k not in plain, k
    assert "state_crc" not in plain["config"]
    for d in (full, implied):
        assert "stages_ms" in d and "roofline" in d and "ms_per_step_median" in d
    assert len(full["ms_per_step_blocks"]) == 5 and len(implied["ms_per_step_blocks"]) == 2
    assert full["config"]["state_crc"] == implied["config"]["state_crc"]
    files = sorted(os.listdir(tmp_path / "dump_plain"))
    assert files
    for other in ("dump_full", "dump_implied"):
        assert files == sorted(os.listdir(tmp_path / other))
        for f in files:
            assert np.array_equal(np.load(tmp_path / "dump_plain" / f), np.load(tmp_path / other / f)), (other, f)
