"""CPU: bench.py's command line (--full, --dump-outputs) and its output writer."""
import sys

import numpy as np
import pytest
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_only(monkeypatch):
    """Without --full every leg beside the timed steps is off, for N = 1 and N > 1."""
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "3")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    assert a.no_cpu_baseline and a.no_hot and a.no_extra


def test_full_keeps_every_leg_and_its_switches(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not (a.no_cpu_baseline or a.no_hot or a.no_extra)
    a = _parse(monkeypatch, "--full", "--no-hot", "--dump-outputs", "d")
    assert a.no_hot and not a.no_cpu_baseline and a.dump_outputs == "d"


@pytest.mark.parametrize("tdt", [torch.float32, torch.float16, torch.bfloat16])
def test_dump_outputs_small_tensor_is_written_whole(tmp_path, tdt):
    t = (torch.arange(1001, dtype=torch.float32) / 7 - 50).to(tdt)
    bench.dump_outputs(str(tmp_path / "d"), {"x": t})
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float32 and got.shape == (1001,)
    assert np.array_equal(got, t.float().numpy())  # float32 holds all three exactly


def test_dump_outputs_samples_a_large_tensor_the_same_way_each_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    t = torch.arange(1000, dtype=torch.float32)
    bench.dump_outputs(str(tmp_path / "a"), {"x": t})
    bench.dump_outputs(str(tmp_path / "b"), {"x": t})
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (64,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < 1000  # sorted indices of t itself
    assert len(np.unique(a)) > 32  # spread over the tensor, not one spot
