"""bench.py --dump-outputs: the arrays of the last timed step are stored as float32 / float64
.npy files, at most DUMP_MAX_BYTES in all (a fixed seeded sample of a larger output)."""
import os

import numpy as np
import torch

import bench


def test_dump_writes_float32_and_float64(tmp_path):
    a = torch.arange(12, dtype=torch.float32).reshape(3, 4) / 7
    outs = {"lo": a.to(torch.bfloat16), "single": a, "double": a.double()}
    bench.dump_outputs(str(tmp_path / "d"), outs)
    assert sorted(os.listdir(tmp_path / "d")) == ["double.npy", "lo.npy", "single.npy"]
    lo, single, double = (np.load(tmp_path / "d" / f"{n}.npy") for n in ("lo", "single", "double"))
    assert lo.dtype == np.float32 and single.dtype == np.float32 and double.dtype == np.float64
    np.testing.assert_array_equal(lo, a.to(torch.bfloat16).float().numpy())
    np.testing.assert_array_equal(single, a.numpy())
    np.testing.assert_array_equal(double, a.double().numpy())


def test_dump_only_on_the_writing_rank(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"x": torch.ones(2, 2)}, write=False)
    assert not (tmp_path / "d").exists()


def test_dump_samples_large_outputs_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2 * 400)      # 100 float32 cells per array
    x = torch.arange(1000, dtype=torch.float32).reshape(100, 10)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": -x})
    xa, xb = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    ya = np.load(tmp_path / "a" / "y.npy")
    assert xa.shape == (100,) and xa.nbytes + ya.nbytes <= 2 * 400
    np.testing.assert_array_equal(xa, xb)                        # same cells every run
    np.testing.assert_array_equal(ya, -xa)                       # same cells in every array of one size
    assert len(np.unique(xa)) == 100 and np.all(np.diff(xa) > 0)  # distinct cells, in order
