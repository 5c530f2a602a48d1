"""bench.py's --dump-outputs writer on host arrays (no GPU): small outputs whole and in their shape, large ones as the same seeded sample in every run,
float32, within the dump budget."""
import numpy as np

import bench


def test_dump_outputs_whole_small_sampled_large(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_ELEMS", 2000)
    small = np.arange(12, dtype=np.float32).reshape(3, 4)
    large = np.arange(5000, dtype=np.float64).reshape(50, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("large", large)])
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    s = np.load(tmp_path / "a" / "large.npy")
    assert s.dtype == np.float32 and s.shape == (1000,)
    assert np.all(np.diff(s) > 0) and np.array_equal(s, large.reshape(-1)[s.astype(np.int64)])   # distinct positions, in order, values from the array
    assert np.array_equal(s, np.load(tmp_path / "b" / "large.npy"))                            # the same sample in every run
