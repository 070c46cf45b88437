"""Measurements behind profiles/param_groups.txt (DESIGN.md "Parameter groups").

    python scratch/param_groups_measure.py kernel    alone on the chip, median of 20 launches (the method of scratch/det_measure.py), at the bench
                                                     model's arena size with both 16-bit shadows: mmdti_adam_step against
                                                     mmdti_adam_step_grouped with 4 groups (coupled and decoupled)
    python scratch/param_groups_measure.py steps     the headline step (bench.py's model and batch) in fresh processes, arms alternated, 2 rounds:
                                                     the default engine against FineTuner(weight_decay=0.01, param_groups=no_decay(model))
    python scratch/param_groups_measure.py arm NAME  one arm of `steps` in this process (default | no_decay)
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
    sys.path.insert(0, p)


def _time(fn, n=20):
    import torch
    for _ in range(3):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def kernel():
    import torch
    import bench
    from mmdti_hip import ops
    model, _ = bench.build_model()
    n = sum((p.numel() + 7) // 8 * 8 for p in model.parameters())
    g = torch.Generator(device="cuda").manual_seed(0)
    R = lambda: torch.randn(n, device="cuda", generator=g)
    p, grad, m, v = R(), R() * 0.1, R() * 0.01, (R() * 0.01) ** 2
    pb, ph = torch.empty(n, device="cuda", dtype=torch.bfloat16), torch.empty(n, device="cuda", dtype=torch.float16)
    scale = torch.tensor([0.5], device="cuda")
    nb = (n + 7) // 8
    ids = (torch.arange(nb, device="cuda") * 4 // nb).to(torch.uint8)           # four long runs, as parameters lie in the arena
    table = torch.tensor([[1.0, 0.01], [0.5, 0.0], [0.25, 0.01], [0.1, 0.0]], device="cuda")
    one = torch.tensor([[1.0, 0.01]], device="cuda")
    zeros = torch.zeros(nb, device="cuda", dtype=torch.uint8)
    cases = {
        "mmdti_adam_step (wd 0.01, by value)": lambda: ops.adam_step(p, grad, m, v, pb, 1e-4, 0.9, 0.999, 1e-6, 0.01, 5, scale, None, p_f16=ph),
        "mmdti_adam_step_grouped, 1 group, coupled": lambda: ops.adam_step_grouped(p, grad, m, v, pb, 1e-4, 0.9, 0.999, 1e-6, 5, zeros, one, False, None, None, scale, None, p_f16=ph),
        "mmdti_adam_step_grouped, 4 groups, coupled": lambda: ops.adam_step_grouped(p, grad, m, v, pb, 1e-4, 0.9, 0.999, 1e-6, 5, ids, table, False, None, None, scale, None, p_f16=ph),
        "mmdti_adam_step_grouped, 4 groups, decoupled": lambda: ops.adam_step_grouped(p, grad, m, v, pb, 1e-4, 0.9, 0.999, 1e-6, 5, ids, table, True, None, None, scale, None, p_f16=ph),
    }
    print(f"arena: {n} elements ({n * 4 / 2 ** 20:.1f} MiB fp32); bytes moved per launch: {n * 32 / 1e9:.3f} GB", flush=True)
    for name, fn in cases.items():
        t = _time(fn)
        print(f"{name:50s} {t:8.1f} us   {n * 32 / t / 1e3:7.1f} GB/s", flush=True)


def arm(name, steps=10, warmup=3):
    import torch
    import bench
    from mmdti_hip.param_groups import no_decay
    from mmdti_hip.trainer import FineTuner
    model, _ = bench.build_model()
    model = model.cuda().train()
    kw = dict(weight_decay=0.01, param_groups=no_decay(model)) if name == "no_decay" else {}
    tuner = FineTuner(model, "classification", total_steps=10_000, **kw)
    _, b, y = bench.synth(256, 128, 256, seed=1234)
    b, y = {k: v.cuda() for k, v in b.items()}, y.cuda()
    for _ in range(warmup):
        tuner.step(b, y, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tuner.step(b, y, epoch=0)
    torch.cuda.synchronize()
    print(f"{name} {(time.perf_counter() - t0) / steps * 1e3:.3f} ms/step", flush=True)


def steps():
    for k in range(2):
        for name in ("default", "no_decay"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "arm", name], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit(f"arm {name} failed ({r.returncode}): {r.stderr[-600:]}")
            print(f"round {k} {r.stdout.strip().splitlines()[-1]}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernel":
        kernel()
    elif what == "steps":
        steps()
    elif what == "arm":
        arm(sys.argv[2])
    else:
        raise SystemExit(__doc__)
