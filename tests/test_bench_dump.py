"""``bench.py --dump-outputs``: what the files hold (no GPU: the writer on its own)."""
import os

import numpy as np

import bench


def _table(n, seed=1):
    rng = np.random.default_rng(seed)
    return rng.random((n, 8)), rng.integers(0, 2, (n, 2)).astype(np.uint8)


def test_small_outputs_are_written_whole(tmp_path):
    final, colocs = _table(100)
    got = bench.dump_outputs(str(tmp_path / "out"), {"final": final, "colocs": colocs})
    back = np.load(tmp_path / "out" / "final.npy")
    flags = np.load(tmp_path / "out" / "colocs.npy")
    assert back.dtype == np.float64 and flags.dtype == np.float32
    np.testing.assert_array_equal(back, final)
    np.testing.assert_array_equal(flags, colocs.astype(np.float32))
    assert got["final"] == {"shape": [100, 8], "dtype": "float64", "rows_of": 100}


def test_large_outputs_keep_one_seeded_sample_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40_000)
    final, colocs = _table(5000)
    runs = []
    for k in range(2):
        d = str(tmp_path / f"out{k}")
        got = bench.dump_outputs(d, {"final": final, "colocs": colocs})
        assert sum(os.path.getsize(os.path.join(d, f)) - 128 for f in os.listdir(d)) <= 40_000
        assert got["final"]["rows_of"] == 5000 and 0 < got["final"]["shape"][0] < 5000
        runs.append((np.load(os.path.join(d, "final.npy")), np.load(os.path.join(d, "colocs.npy"))))
    (f0, c0), (f1, c1) = runs
    np.testing.assert_array_equal(f0, f1)                  # the same rows from run to run
    np.testing.assert_array_equal(c0, c1)
    rows = np.flatnonzero(np.isin(final[:, 0], f0[:, 0]))  # (random floats: column 0 identifies a row)
    np.testing.assert_array_equal(final[rows], f0)         # rows in their order, the table's and the flags' the same
    np.testing.assert_array_equal(colocs[rows].astype(np.float32), c0)
