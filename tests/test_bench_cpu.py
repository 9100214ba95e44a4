"""bench.py's command line and its --dump-outputs writer (CPU only: no step is run)."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def _model():
    """Two layers whose first weight holds its own flat positions (exact in float32), so a
    sample of it shows which positions were taken."""
    model = torch.nn.Sequential(torch.nn.Linear(300, 300), torch.nn.Linear(300, 4))
    with torch.no_grad():
        model[0].weight.copy_(torch.arange(90000.0).reshape(300, 300))
    return model


def _positions(i, n, cap):
    """The documented sample of parameter i (n elements): cap draws of
    default_rng([i, n]).integers(0, n), sorted."""
    return np.sort(np.random.default_rng([i, n]).integers(0, n, cap)).astype(np.float32)


def test_dump_outputs_is_a_fixed_sample(tmp_path):
    model = _model()
    losses = [torch.tensor(2.5), torch.tensor(1.25)]
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(d1, model, losses)
    bench.dump_outputs(d2, model, losses)
    names = sorted(os.listdir(d1))
    assert names == sorted(["loss.npy", "losses.npy"] +
                           [f"param.{k}.npy" for k, _ in model.named_parameters()])
    assert sum(os.path.getsize(os.path.join(d1, n)) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert x.dtype in (np.float32, np.float64)
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(np.load(os.path.join(d1, "loss.npy")), [1.25])
    np.testing.assert_array_equal(np.load(os.path.join(d1, "losses.npy")), [2.5, 1.25])
    # the 90000-element weight (parameter 0) is sampled at the seeded positions, the rest whole
    np.testing.assert_array_equal(np.load(os.path.join(d1, "param.0.weight.npy")),
                                  _positions(0, 90000, 1 << 16))
    np.testing.assert_array_equal(np.load(os.path.join(d1, "param.1.weight.npy")),
                                  model[1].weight.detach().reshape(-1).numpy())


def test_dump_outputs_halves_the_cap_to_fit_the_budget(tmp_path, monkeypatch):
    """91508 parameters at a 100 KB budget: the per-tensor cap halves from 65536 to 16384
    (16384 + 300 + 1200 + 4 elements = 71552 bytes; at 32768 it would be 137088)."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    model = _model()
    d = str(tmp_path / "d")
    bench.dump_outputs(d, model, [torch.tensor(1.0)])
    params = {k: np.load(os.path.join(d, f"param.{k}.npy")) for k, _ in model.named_parameters()}
    assert sum(v.nbytes for v in params.values()) == 71552
    np.testing.assert_array_equal(params["0.weight"], _positions(0, 90000, 16384))
    np.testing.assert_array_equal(params["1.weight"],
                                  model[1].weight.detach().reshape(-1).numpy())
