"""bench.py --dump-outputs (bench.dump_outputs): float64 .npy files, and above
the size limit a fixed sample of each oversized array, the same elements on
every run."""
import numpy as np

import bench


def test_dump_outputs_writes_float64_arrays(tmp_path):
    a = np.arange(10, dtype=np.int32).reshape(2, 5)
    b = np.linspace(0.0, 1.0, 7, dtype=np.float32)
    bench.dump_outputs(tmp_path / "o", {"a": a, "b": b})
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == ["a.npy", "b.npy"]
    for k, v in (("a", a), ("b", b)):
        x = np.load(tmp_path / "o" / (k + ".npy"))
        assert x.dtype == np.float64 and x.shape == v.shape
        np.testing.assert_array_equal(x, v.astype(np.float64))


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_OUTPUTS_MAX_BYTES", 8 * 64)
    big = np.random.default_rng(1).random((50, 20))
    small = np.arange(5.0)
    for d in ("o1", "o2"):
        bench.dump_outputs(tmp_path / d, {"big": big, "small": small})
    x1, x2 = np.load(tmp_path / "o1" / "big.npy"), np.load(tmp_path / "o2" / "big.npy")
    np.testing.assert_array_equal(x1, x2)                      # the same sample every run
    assert x1.shape == (32,) and np.isin(x1, big).all()        # an equal share of the limit
    np.testing.assert_array_equal(np.load(tmp_path / "o1" / "small.npy"), small)
    assert x1.nbytes + small.nbytes <= 8 * 64
