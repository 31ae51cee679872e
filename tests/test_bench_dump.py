"""bench.py --dump-outputs: what it writes for a state, checked on the host with a stand-in for the device context (the
flag itself runs on the GPU: `python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`)."""
import os

import numpy as np

import bench


class _State:
    """Stand-in for BlomGpu.get: every field a distinct, known pattern of the library's (nlev, nj, ni) layout."""

    def __init__(self, shapes):
        self.shapes = shapes

    def get(self, name):
        n = int(np.prod(self.shapes[name]))
        return (np.arange(n, dtype=np.float64) + 1e6 * bench.DUMP_FIELDS.index(name)).reshape(self.shapes[name])


def test_dump_writes_every_field_whole_or_as_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 500)
    shapes = {nm: ((12, 20, 30) if nm in ("u", "trc", "dp") else (3, 10, 12)) for nm in bench.DUMP_FIELDS}
    st = _State(shapes)
    bench.dump_outputs(st, str(tmp_path / "a"))
    bench.dump_outputs(st, str(tmp_path / "b"))
    for nm in bench.DUMP_FIELDS:
        a = np.load(tmp_path / "a" / f"{nm}.npy")
        b = np.load(tmp_path / "b" / f"{nm}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b), nm          # the same arguments: the same elements
        full = st.get(nm).ravel()
        if full.size <= 500:
            assert np.array_equal(a, full), nm
        else:
            # a sample of distinct elements of the field, in array order
            assert a.size == 500 and np.all(np.diff(a) > 0) and np.isin(a, full).all(), nm
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{nm}.npy" for nm in bench.DUMP_FIELDS)


def test_dump_stays_within_64_mb():
    assert len(bench.DUMP_FIELDS) * bench.DUMP_MAX_ELEMS * 8 <= 64 * 10**6
