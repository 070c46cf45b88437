"""bench.py's host side: what --dump-outputs writes, and the arguments it refuses before touching the GPU."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench
from mmdti_hip.trainer import StepOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _step(B=6):
    logits = torch.randn(B, 2, generator=torch.Generator().manual_seed(1))
    return StepOutput(torch.tensor(1.5), torch.tensor(0.5), torch.tensor(5.5, dtype=torch.float64), None, logits)


def test_step_outputs_are_float32_and_the_weight_sample_is_fixed(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 200), torch.nn.Linear(200, 7))
    out = _step()
    a = bench.step_outputs(out, model, sample=4096)
    assert set(a) == {"logits", "loss", "task_loss", "infonce_loss", "params_sample"}          # (ct_loss None: not written)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["logits"].shape == (6, 2) and np.array_equal(a["logits"], out.logits.numpy())
    assert a["loss"] == np.float32(1.5) and a["infonce_loss"] == np.float32(5.5)
    # the sample: the same positions every time, drawn from every parameter in named_parameters() order
    flat = torch.cat([p.detach().reshape(-1) for _, p in model.named_parameters()]).numpy()
    idx = torch.randint(flat.size, (4096,), generator=torch.Generator().manual_seed(0)).sort().values.numpy()
    assert np.array_equal(a["params_sample"], flat[idx])
    assert np.array_equal(bench.step_outputs(out, model, sample=4096)["params_sample"], a["params_sample"])
    # fewer weights than the sample size: one value per drawn position, never more positions than weights
    assert bench.step_outputs(out, torch.nn.Linear(3, 2), sample=4096)["params_sample"].shape == (8,)
    bench.dump_outputs(a, str(tmp_path / "d"))
    for name, v in a.items():
        got = np.load(tmp_path / "d" / (name + ".npy"), allow_pickle=False)
        assert got.dtype == np.float32 and np.array_equal(got, v)


def test_default_dump_fits_the_size_limit():
    assert bench.PARAM_SAMPLE * 4 + 256 * 2 * 4 + 4 * 4 <= 64 << 20


def test_options_and_refused_arguments():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stderr[-2000:]
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, (bad, r.stderr[-2000:])
