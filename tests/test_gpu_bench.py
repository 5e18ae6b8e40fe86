"""bench.py without --full: the headline line and nothing beside it (one rank, a small index)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_alone(tmp_path):
    """A plain run sets up, warms up, times its steps, writes --dump-outputs and prints one line: the headline fields,
    no roofline, strong-scaling set, CPU baseline, other configurations or large indexes (those are --full)."""
    n, nq, steps = 20000, 2000, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--n", str(n), "--nq", str(nq), "--max-batch", "4096", "--dump-outputs", str(tmp_path / "out")]
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "queries/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["n_gpus"] == 1 and out["steps"] == steps and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["value"] == pytest.approx(nq * 1e3 / out["ms_per_step"], rel=1e-9)
    assert out["config"]["recall_at_10"] >= 0.95 and out["config"]["L"] > 0
    assert not {"roofline", "other_configs", "cpu_baseline", "mfma"} & set(out)
    assert not [key for key in out if key.startswith("roofline_large")]
    dumped = {name: np.load(tmp_path / "out" / f"{name}.npy") for name in ("ids", "distances", "stats")}
    assert dumped["ids"].shape == dumped["distances"].shape == (nq, 10) and dumped["stats"].shape == (nq, 5)
    assert (dumped["stats"][:, 3] == 0).all()  # (status: no query overflowed its scratch)
