"""bench.py --dump-outputs: float32 files, the size budget, and the same sample of a large output in every run (CPU only)."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_budget_and_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    named = {"y": torch.randn(4096, 256, generator=g).bfloat16(), "dw": torch.randn(40, 8, 8, generator=g)}
    budget = 1 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), named, budget=budget)
    a = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in named}
    b = {n: np.load(str(tmp_path / "b" / (n + ".npy"))) for n in named}
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= budget
    np.testing.assert_array_equal(a["dw"], named["dw"].numpy())                 # small enough: written whole
    y = named["y"].float().numpy()
    assert a["y"].shape[1] == 256 and 0 < a["y"].shape[0] < 4096                 # too large: a sample of whole rows
    rows = [int(np.nonzero((y == r).all(axis=1))[0][0]) for r in a["y"]]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    np.testing.assert_array_equal(a["y"], b["y"])
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["dw.npy", "y.npy"]
