"""A plain `bench.py` run: exactly --steps timed steps, the headline record only, and --dump-outputs writing what the last timed
step computed -- the same inputs in every run, so two runs' outputs agree up to the fp32 atomics of the backward."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    r = _run(tmp_path / "a", 3)
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "molecules/s" and r["higher_is_better"] is True
    assert abs(r["value"] - 256 / (r["ms_per_step"] * 1e-3)) < 1e-2 * r["value"]
    assert r["workloads"] == {} and r["rooflines"] == [] and r["roofline"] is None and r["cpu_baseline"] is None      # (--full only)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["ct_loss.npy", "infonce_loss.npy", "logits.npy", "loss.npy", "params_sample.npy", "task_loss.npy"], files
    a = {f[:-4]: np.load(tmp_path / "a" / f, allow_pickle=False) for f in files}
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    assert a["logits"].shape == (256, 2) and a["params_sample"].shape == (1 << 20,)
    for k, name in (("loss", "loss"), ("task", "task_loss"), ("infonce", "infonce_loss"), ("ct", "ct_loss")):
        assert float(a[name]) == pytest.approx(r["losses_last_step"][k], rel=1e-6)
    _run(tmp_path / "b", 3)
    b = {f[:-4]: np.load(tmp_path / "b" / f, allow_pickle=False) for f in files}
    for name in ("loss", "task_loss", "infonce_loss", "ct_loss"):
        assert float(b[name]) == pytest.approx(float(a[name]), rel=1e-4), name
    np.testing.assert_allclose(b["logits"], a["logits"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(b["params_sample"], a["params_sample"], rtol=1e-4, atol=1e-6)
