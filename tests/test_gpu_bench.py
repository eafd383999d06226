"""GPU: a plain bench.py run (no --full) prints the headline line only, and --dump-outputs writes what the last timed step
computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "4", "--points", "512", "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_headline_and_dump(tmp_path):
    out_dir = os.path.join(tmp_path, "out")
    d = _plain_run(out_dir)
    assert d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and "pairs/sec" in d["metric"]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(4 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert not {"roofline", "stages", "kernels_one_stream", "cpu_baseline"} & set(d)      # those are --full's

    names = sorted(os.listdir(out_dir))
    assert names == ["bn_running_stats.npy", "grads.npy", "loss.npy", "params.npy"]
    arrays = {n[:-4]: np.load(os.path.join(out_dir, n)) for n in names}
    assert sum(os.path.getsize(os.path.join(out_dir, n)) for n in names) <= 64 << 20
    for a in arrays.values():
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert float(arrays["loss"][0]) == pytest.approx(d["loss"], rel=1e-6)
    assert arrays["params"].shape == arrays["grads"].shape and np.abs(arrays["grads"]).max() > 0


def test_two_plain_runs_compute_the_same(tmp_path):
    """Same arguments, same inputs: two runs' dumps of the last timed step (which starts from the seeded initial state)
    agree to the rounding of one step's atomic sums.  Parameters: Adam's first update is lr * g / (|g| + eps), so an entry
    whose gradient is rounding noise (mathematically zero) may move by up to lr either way; those entries are few."""
    dirs = [os.path.join(tmp_path, k) for k in ("a", "b")]
    for d in dirs:
        _plain_run(d)
    got = [{n: np.load(os.path.join(d, n + ".npy")).astype(np.float64) for n in ("loss", "params", "grads", "bn_running_stats")}
           for d in dirs]
    for name in ("loss", "grads", "bn_running_stats"):
        a, b = got[0][name], got[1][name]
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max() + 1e-12, name
    import bench
    a, b = got[0]["params"], got[1]["params"]
    assert np.abs(a - b).max() <= 2 * bench.Cfg.lr * (1 + 1e-3)
    assert np.mean(np.abs(a - b) > 1e-5 * np.abs(a).max()) <= 1e-3
