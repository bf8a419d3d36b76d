"""bench.py's host side: the --dump-outputs writer and argument checks (the timed GPU path is bench.py itself)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _outputs():
    g = torch.Generator().manual_seed(0)
    return {"probs": torch.rand((64, 400), generator=g), "loss": torch.full((1,), 4.5),
            "params": torch.randn(250_003, generator=g)}


def test_dump_outputs_writes_every_array_whole_within_the_budget(tmp_path):
    outs = _outputs()
    bench.dump_outputs(outs, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == ["loss.npy", "params.npy", "probs.npy"]
    for k, v in outs.items():
        a = np.load(tmp_path / "d" / f"{k}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(v.shape) and np.array_equal(a, v.numpy())


def test_dump_outputs_samples_the_same_elements_over_the_budget(tmp_path, monkeypatch):
    budget = 400_000
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    outs = _outputs()
    for d in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / d))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= budget + 4096   # + .npy headers
    for k, v in outs.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.dtype == np.float32 and 1 <= a.size <= v.numel() and np.array_equal(a, b)
        assert np.isin(a, v.numpy()).all()
    assert np.load(tmp_path / "a" / "params.npy").size < outs["params"].numel()


def test_steps_must_be_positive(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
