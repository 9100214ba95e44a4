"""bench.py end to end on a small image: what a plain run and a --full run print and dump.

Two runs of the benchmark, shared by the tests below: plain at --warmup 2 and --full at
--warmup 1.  --full's launch-counting step is one more training step on the next batch, so
the two reach the timed region in the same state and must dump the same arrays; per-launch
timing events change no arithmetic."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--height", "192", "--width", "320"]


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    plain = _bench("--warmup", "2", "--dump-outputs", str(d / "plain"))
    full = _bench("--warmup", "1", "--full", "--cpu-baseline-steps", "1",
                  "--dump-outputs", str(d / "full"))
    return plain, full, d


def _headline(r):
    assert r["unit"] == "img/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
    assert r["steps"] == 2 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0
    # value = images/s of the timed steps: 1000 / ms_per_step, both rounded in the line
    assert r["value"] == pytest.approx(1e3 / r["ms_per_step"], rel=1e-3)
    assert "DAF VGG16" in r["metric"]


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(runs):
    plain, _, _ = runs
    _headline(plain)
    assert plain["warmup"] == 2
    assert plain["roofline"] is None and plain["cpu_baseline"] is None


@pytest.mark.gpu
def test_full_run_fills_roofline_and_cpu_baseline(runs):
    _, full, _ = runs
    _headline(full)
    assert full["warmup"] == 1
    roof = full["roofline"]
    assert roof["profiled_steps"] == 1 and roof["peak"] > 0
    assert 0 < roof["frac"] < 1 and roof["kernel_ms_per_step"] > 0
    assert roof["families"] and roof["by_kind"] and roof["all_conv_gemm"]["launches"] > 0
    base = full["cpu_baseline"]
    assert base["value"] > 0 and base["unit"] == "img/s"


@pytest.mark.gpu
def test_dumps_hold_the_timed_steps_and_full_adds_exactly_one_step(runs):
    _, _, d = runs
    names = sorted(os.listdir(d / "plain"))
    assert names == sorted(os.listdir(d / "full"))
    assert "loss.npy" in names and "losses.npy" in names
    assert sum(n.startswith("param.") for n in names) == len(names) - 2 > 0
    assert sum(os.path.getsize(d / "plain" / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(d / "plain" / n), np.load(d / "full" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        np.testing.assert_array_equal(x, y, err_msg=n)
    losses = np.load(d / "plain" / "losses.npy")
    assert losses.shape == (2,)
    np.testing.assert_array_equal(np.load(d / "plain" / "loss.npy"), losses[-1:])
