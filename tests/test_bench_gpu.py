"""bench.py as it is run for every change: a plain `--gpus 1 --steps K --warmup W` run times K steps and prints the line without the legs
that --full adds, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    """Two runs with the same arguments compute the same step (seeded parameters, inputs and DropPath draws): their dumps are equal."""
    out_dir = tmp_path / "outputs"
    line = _plain_run(out_dir)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "bf16" and line["higher_is_better"] is True
    assert line["unit"] == "images/sec" and line["metric"].startswith("images/sec")
    assert abs(line["value"] - 8 * 1e3 / line["ms_per_step"]) < 1e-2 * line["value"]
    for leg in ("cpu_baseline", "secondary", "reference_gpu", "optimizer_step"):
        assert leg not in line, leg
    assert line["sustained"] is None and line["roofline"]["kernels"] == {}
    files = {f: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}
    assert set(files) == {"loss.npy", "pred.npy", "grad_norm.npy", "grad_sample.npy"}
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    assert files["pred.npy"].shape == (8, 1568, 768) and np.isfinite(files["pred.npy"]).all()
    assert abs(float(files["loss.npy"][0]) - line["loss"]) <= 1e-6 * max(1.0, abs(line["loss"]))
    assert np.isfinite(files["grad_norm.npy"]).all() and files["grad_norm.npy"].sum() > 0 and np.isfinite(files["grad_sample.npy"]).all()
    again = _plain_run(tmp_path / "again")
    assert again["loss"] == line["loss"]
    for f, a in files.items():
        assert np.array_equal(np.load(tmp_path / "again" / f), a), f
