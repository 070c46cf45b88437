"""Measurements behind profiles/ema.txt (DESIGN.md "Weight averaging (EMA)").

    python scratch/ema_measure.py kernel       alone on the chip, median of 20 launches (the method of scratch/det_measure.py), at the bench
                                               model's arena size: the Adam pass with both shadows, mmdti_ema_update (t by value, from the
                                               step state, from the guard) and mmdti_ema_swap with both shadows
    python scratch/ema_measure.py steps        the headline step (256 molecules) and the 32-molecule mixed-length step in fresh processes,
                                               arms alternated, 2 rounds: the default engine against FineTuner(ema_decay=0.999)
    python scratch/ema_measure.py arm NAME     one arm of `steps` in this process (off | ema | off32 | ema32)
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
    p, grad, m, v, ema = R(), R() * 0.1, R() * 0.01, (R() * 0.01) ** 2, R()
    pb, ph = torch.empty(n, device="cuda", dtype=torch.bfloat16), torch.empty(n, device="cuda", dtype=torch.float16)
    scale = torch.tensor([0.5], device="cuda")
    state = torch.tensor([5.0, 1e-4, 0.4, 0.07], device="cuda")
    guard = torch.tensor([5.0, 0.0, 0.0, 0.4, 0.07, 0.0, 0.0, 0.0], device="cuda")
    cases = {
        "mmdti_adam_step (both shadows)": (32, lambda: ops.adam_step(p, grad, m, v, pb, 1e-4, 0.9, 0.999, 1e-6, 0.0, 5, scale, None, p_f16=ph)),
        "mmdti_ema_update, t by value": (12, lambda: ops.ema_update(p, ema, 0.999, True, 5)),
        "mmdti_ema_update, t from the step state": (12, lambda: ops.ema_update(p, ema, 0.999, True, 0, None, state)),
        "mmdti_ema_update, t from the guard": (12, lambda: ops.ema_update(p, ema, 0.999, True, 0, guard, None)),
        "mmdti_ema_swap (both shadows)": (20, lambda: ops.ema_swap(p, ema, pb, ph)),
        "mmdti_ema_swap (bf16 shadow only)": (18, lambda: ops.ema_swap(p, ema, pb, None)),
    }
    print(f"arena: {n} elements ({n * 4 / 2 ** 20:.1f} MiB fp32)", flush=True)
    for name, (bytes_per, fn) in cases.items():
        t = _time(fn)
        print(f"{name:42s} {t:8.1f} us   {bytes_per:2d} B/element   {n * bytes_per / t / 1e3:7.1f} GB/s", flush=True)


def arm(name, steps=10, warmup=3):
    import torch
    import bench
    from mmdti_hip.trainer import FineTuner
    model, _ = bench.build_model()
    model = model.cuda().train()
    kw = dict(ema_decay=0.999) if name.startswith("ema") else {}
    tuner = FineTuner(model, "classification", total_steps=10_000, **kw)
    small = name.endswith("32")
    _, b, y = bench.synth(32, 128, 256, seed=1234, ragged=True) if small else bench.synth(256, 128, 256, seed=1234)
    b, y = {k: v.cuda() for k, v in b.items()}, y.cuda()
    if small:
        steps, warmup = 50, 10
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
        for name in ("off", "ema", "off32", "ema32"):
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
