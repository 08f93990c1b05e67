"""`python bench.py --gpus 1 --steps K --warmup W` as it is run for every change: the plain run prints the headline alone (the side
measurements are --full's), times exactly K steps, and --dump-outputs writes what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"].startswith("MPC plan-steps/sec") and d["unit"] == "plan-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["steps"] == 7 and d["warmup"] == 2 and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1e-2 * 1e3  # (one GPU: plan steps per second = 1000 / ms per step)
    assert not {"latency_ms", "roofline", "cpu_baseline", "parity", "closed_loop", "c5", "c3"} & set(d)

    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert {"sample_action", "eval_action", "p", "expect_return", "argmax", "sample_idx"} <= set(files)
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    N = 1024
    assert files["sample_action"].shape == (1, 3) and files["eval_action"].shape == (3,)
    assert files["p"].shape == (N,) and files["expect_return"].shape == (N,)
    assert abs(float(files["p"].sum()) - 1.0) < 1e-3
    assert 0 <= int(files["argmax"].reshape(-1)[0]) < N and 0 <= int(files["sample_idx"].reshape(-1)[0]) < N
