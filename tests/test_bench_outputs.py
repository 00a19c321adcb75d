"""bench.py --dump-outputs / --full (CPU only): the options parse, arrays are written whole as float32
while they fit the budget, and above it every large array becomes the same seeded sample on every call."""
import os

import numpy as np
import torch

from conftest import ROOT  # noqa: F401  (puts the repository root on sys.path)


def test_options_default_off():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


def _arrays():
    g = torch.Generator().manual_seed(3)
    return {"small": torch.arange(10, dtype=torch.int32), "flag": torch.tensor([True, False]),
            "big": torch.randn((1000, 7), generator=g), "big64": torch.randn((5001,), generator=g, dtype=torch.float64)}


def test_dump_whole_when_it_fits(tmp_path):
    import bench
    arrays = _arrays()
    bench.dump_outputs(str(tmp_path / "o"), arrays)
    assert sorted(os.listdir(tmp_path / "o")) == ["big.npy", "big64.npy", "flag.npy", "small.npy"]
    for k, v in arrays.items():
        a = np.load(tmp_path / "o" / (k + ".npy"))
        assert a.dtype == np.float32 and a.shape == tuple(v.shape)
        assert np.array_equal(a, v.to(torch.float32).numpy())


def test_dump_samples_large_arrays_over_budget(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 12000)
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 1000)
    arrays = _arrays()
    out = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
        out.append({k: np.load(tmp_path / d / (k + ".npy")) for k in arrays})
    a, b = out
    assert sum(v.nbytes for v in a.values()) <= 12000
    assert np.array_equal(a["small"], np.arange(10, dtype=np.float32)) and np.array_equal(a["flag"], [1.0, 0.0])
    for k in ("big", "big64"):
        assert a[k].ndim == 1 and 0 < a[k].size < arrays[k].numel()
        assert np.array_equal(a[k], b[k])
        # a sample of the array's own elements, in their order
        flat = arrays[k].to(torch.float32).reshape(-1).numpy()
        idx = np.sort(np.random.default_rng(0).choice(flat.size, a[k].size, replace=False))
        assert np.array_equal(a[k], flat[idx])
