"""bench.py --dump-outputs: the out-batch -> .npy encoding is lossless,
float64, and capped at 64 MB by a fixed seeded row sample; the plain run
keeps the legs beyond the headline figure behind --full."""
import os
import sys

import numpy as np

import bench


def _batch(n, kw=2, vb=24, seed=5):
    rng = np.random.default_rng(seed)
    keys = rng.integers(-2**63, 2**63 - 1, n * kw, dtype=np.int64)
    vals = rng.integers(0, 256, n * vb, dtype=np.uint8)
    times = np.full(n, 7, np.uint64)
    diffs = rng.choice(np.array([-1, 1], np.int64), n)
    return keys, vals, times, diffs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _unwords(a):
    return a.astype("<u4").reshape(-1).view(np.uint8)


def test_dump_roundtrips_exactly(tmp_path):
    keys, vals, times, diffs = _batch(1000)
    bench.dump_outputs(str(tmp_path), (keys, vals, times, diffs))
    got = _load(str(tmp_path))
    assert set(got) == {"keys", "vals", "times", "diffs", "n_rows"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["keys"].shape == (1000, 4) and got["vals"].shape == (1000, 6)
    assert np.array_equal(_unwords(got["keys"]), keys.view(np.uint8))
    assert np.array_equal(_unwords(got["vals"]), vals)
    assert np.array_equal(got["times"], times.astype(np.float64))
    assert np.array_equal(got["diffs"], diffs.astype(np.float64))
    assert got["n_rows"][0] == 1000


def test_dump_empty_and_none(tmp_path):
    for i, cols in enumerate((None, _batch(0))):
        d = str(tmp_path / str(i))
        bench.dump_outputs(d, cols)
        got = _load(d)
        assert got["n_rows"][0] == 0
        assert len(got["times"]) == 0 and len(got["diffs"]) == 0


def test_dump_caps_total_size_with_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    cols = _batch(5000)
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        bench.dump_outputs(d, cols)
        total = sum(os.path.getsize(os.path.join(d, f))
                    for f in os.listdir(d))
        assert total <= 64 << 10
    a, b = _load(dirs[0]), _load(dirs[1])
    assert all(np.array_equal(a[k], b[k]) for k in a)  # same sample
    pick = a["sample_rows"].astype(np.int64)
    assert 0 < len(pick) < 5000 and np.all(np.diff(pick) > 0)
    assert a["n_rows"][0] == 5000
    assert np.array_equal(a["diffs"], cols[3][pick].astype(np.float64))
    assert np.array_equal(_unwords(a["vals"]),
                          cols[1].reshape(5000, 24)[pick].reshape(-1))


def test_full_is_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1",
                                      "--steps", "3", "--warmup", "1"])
    a = bench.parse_args()
    assert a.full is False and a.dump_outputs is None
    assert (a.steps, a.warmup) == (3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full",
                                      "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "out"
