"""bench.py's --dump-outputs writer (runs without a GPU): float arrays only, small arrays whole, a fixed sample of the rows of an
array beyond what is left of the budget, the same files from run to run."""
import os

import numpy as np
import torch

import bench


def _dump(d, big):
    bench.dump_outputs(str(d), {"loss": torch.tensor([0.25]), "log_probs": big, "params": torch.arange(10, dtype=torch.float64),
                                "grads": torch.ones(7, 3, dtype=torch.float16)})


def test_dump_outputs_float_arrays_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 1 << 20)
    big = torch.randn(100_000, 8, generator=torch.Generator().manual_seed(1))          # 3.2 MB: beyond the (patched) 1 MB budget
    _dump(tmp_path / "a", big)
    _dump(tmp_path / "b", big)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["grads.npy", "log_probs.npy", "log_probs_rows.npy", "loss.npy", "params.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 1 << 20
    arrs = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert arrs["params.npy"].dtype == np.float64 and arrs["grads.npy"].dtype == np.float32 and arrs["grads.npy"].shape == (7, 3)
    rows = arrs["log_probs_rows.npy"].astype(np.int64)
    assert 0 < len(rows) < big.shape[0] and np.all(np.diff(rows) > 0)
    assert np.array_equal(arrs["log_probs.npy"], big.numpy()[rows])
    for f in files:                                      # the sample is fixed: two runs write the same files
        assert np.array_equal(arrs[f], np.load(tmp_path / "b" / f)), f


def test_arrays_within_the_budget_are_written_whole(tmp_path):
    x = torch.randn(400_000, 8)                                                         # 12.8 MB: the default flagship's size
    _dump(tmp_path, x)
    assert not os.path.exists(tmp_path / "log_probs_rows.npy")
    assert np.array_equal(np.load(tmp_path / "log_probs.npy"), x.numpy())
    assert np.load(tmp_path / "loss.npy").tolist() == [0.25]
