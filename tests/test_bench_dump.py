"""bench.py --dump-outputs on the host: float64 files that hold the integers exactly, at most 64 MB in all, an array over its share cut
to a seeded sample of its rows (the same rows every run) with the row numbers beside it."""
import numpy as np

import bench


def test_dump_outputs_budget_and_sample(tmp_path):
    big = np.arange(3_000_000 * 4, dtype=np.int64).reshape(-1, 4)          # 96 MB as float64: over the budget
    small = np.array([0xFFFFFFFF, 0, 7], dtype=np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small})
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_BUDGET
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small)
    assert not (tmp_path / "a" / "small_rows.npy").exists()
    rows = np.load(tmp_path / "a" / "big_rows.npy").astype(np.int64)
    b = np.load(tmp_path / "a" / "big.npy")
    assert b.dtype == np.float64 and len(rows) > 1_000_000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(b, big[rows])
    bench.dump_outputs(str(tmp_path / "b"), {"big": big, "small": small})
    assert np.array_equal(np.load(tmp_path / "b" / "big_rows.npy"), rows.astype(np.float64))
