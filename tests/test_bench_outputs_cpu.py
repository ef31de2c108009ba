"""bench.py --dump-outputs on the host side: which tensors of a step count as its outputs, and how they are
written -- float32 .npy files that share a 64 MB budget, an array above its share as a fixed sample of its
elements that is the same from run to run.  CPU only: the step objects here are stand-ins."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_step_outputs_of_paired_and_cycle_steps():
    losses, fake, mask = torch.arange(4.0), torch.zeros(2, 3, 4, 4), torch.ones(2, 1, 4, 4)
    paired = types.SimpleNamespace(last_output=fake, last_mask=mask)
    assert list(bench.step_outputs(paired, losses)) == ["losses", "output", "mask"]
    p2p = types.SimpleNamespace(last_output=fake, last_mask=None)             # Pix2Pix has no attention mask
    assert list(bench.step_outputs(p2p, losses)) == ["losses", "output"]
    cyc = types.SimpleNamespace(last=dict(synthetic_post=fake, mask_pre_to_post=mask))
    outs = bench.step_outputs(cyc, losses)
    assert sorted(outs) == ["losses", "mask_pre_to_post", "synthetic_post"] and outs["synthetic_post"] is fake


def test_dump_outputs_whole_arrays(tmp_path):
    g = torch.Generator().manual_seed(3)
    outs = {"losses": torch.rand(4, generator=g, dtype=torch.float64),
            "output": torch.rand((2, 3, 5, 7), generator=g).permute(0, 1, 3, 2)}       # not contiguous
    bench.dump_outputs(str(tmp_path / "d"), outs)
    assert sorted(os.listdir(tmp_path / "d")) == ["losses.npy", "output.npy"]
    for k, t in outs.items():
        a = np.load(tmp_path / "d" / f"{k}.npy", allow_pickle=False)
        assert a.dtype == np.float32 and a.shape == tuple(t.shape)
        assert np.array_equal(a, t.float().numpy())


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 8192)        # 8 KiB per file, header included
    big = torch.arange(10000, dtype=torch.float32).reshape(10, 10, 100)
    outs = {"a": big, "b": big * 2, "small": torch.ones(5)}
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), outs)
    one = {k: np.load(tmp_path / "one" / f"{k}.npy") for k in outs}
    two = {k: np.load(tmp_path / "two" / f"{k}.npy") for k in outs}
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")) <= 3 * 8192
    assert one["small"].shape == (5,)
    n = (8192 - 1024) // 4
    assert one["a"].shape == (n,) and one["a"].dtype == np.float32
    # a sample of the flattened array: distinct elements, in index order, the same indices for every array and run
    assert np.all(np.diff(one["a"]) > 0) and np.array_equal(one["b"], 2 * one["a"])
    assert all(np.array_equal(one[k], two[k]) for k in outs)
