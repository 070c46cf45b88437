"""Measurements behind profiles/fds_streaming.txt (DESIGN.md "Streaming FDS statistics").

    python scratch/fds_stream_measure.py kernels
        the accumulate launch alone on the chip at B = 256, D = 512, nb = 30 / 200 (median of 50), the finish kernel, and for scale the
        one-shot mmdti_fds_update_stats over a 20 x 256-row epoch
    python scratch/fds_stream_measure.py epoch MODE [--tree DIR] [--steps 20]
        ONE process, one arm: a C3-like epoch (regression + ConR + FDS, reference architecture, dropout live, mixed-length batches of
        256) with the statistics from MODE = epoch_pass | streaming | none; prints one JSON line {epoch_ms, step_ms} (medians over the
        measured epochs 1..3, smoothing live).  --tree DIR imports the package of another checkout (the parent commit's build).
    python scratch/fds_stream_measure.py ab PARENT_TREE
        fresh process per arm, arms alternated, 3 rounds: PARENT_TREE's epoch_pass against this tree's streaming (and this tree's
        epoch_pass), then bench.py of both trees (parent, parent again, this; 2 rounds): the default-mode headline step against the
        parent's own spread
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _use_tree(tree):
    for p in (tree, os.path.join(tree, "mm-dti_amd")):
        sys.path.insert(0, p)


def _median_us(fn, n=50):
    import torch
    for _ in range(5):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def kernels():
    import torch
    _use_tree(ROOT)
    from mmdti_hip import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    B, D = 256, 512
    for nb in (30, 200):
        feats = torch.randn(B, D, device="cuda", generator=g)
        labels = torch.rand(B, device="cuda", generator=g) * (nb + 2) - 1          # a few rows below and above the range
        bins, flags = ops.fds_bins(labels, 0.0, 1.0, 0, nb)
        acc = ops.fds_stream_new(nb, D, "cuda")
        rm, rv, tr = torch.zeros(nb, D, device="cuda"), torch.ones(nb, D, device="cuda"), torch.zeros(nb, device="cuda")
        t_acc = _median_us(lambda: ops.fds_stream_accumulate(feats, bins, 0, nb, acc))
        t_bins = _median_us(lambda: ops.fds_bins(labels, 0.0, 1.0, 0, nb))
        t_fin = _median_us(lambda: ops.fds_stream_finish(acc, 0, nb, 0.9, rm, rv, tr))
        big_f = torch.randn(20 * B, D, device="cuda", generator=g)
        big_l = torch.rand(20 * B, device="cuda", generator=g) * (nb + 2) - 1
        bb, bf = ops.fds_bins(big_l, 0.0, 1.0, 0, nb)
        t_one = _median_us(lambda: ops.fds_update_stats(big_f, bb, bf, 0, nb, 0.9, rm, rv, tr), n=10)
        print(f"nb {nb:3d}: accumulate (256 x 512) {t_acc:7.1f} us | bins (with its two allocations) {t_bins:6.1f} us | finish {t_fin:6.1f} us | "
              f"one-shot update over 5120 rows {t_one:8.1f} us", flush=True)


def epoch(mode, tree, steps):
    import numpy as np
    import torch
    _use_tree(tree)
    import bench                      # (the tree's own: bench.py puts its tree's package on the path)
    from types import SimpleNamespace
    from mmdti_hip.models import mm_model as mm
    from mmdti_hip.trainer import FineTuner
    rcfg = SimpleNamespace(layers=6, dim=512, heads=8, ffn=2048, vocab=600, max_pos=514, type_vocab=1, pad_idx=1, ln_eps=1e-12,
                           hidden_dropout=0.1, attn_dropout=0.1)
    torch.manual_seed(1234)
    raw = np.random.default_rng(5).normal(0, 1, 4000)
    model = mm.MM_Model.from_configs(1, "regression", roberta_cfg=rcfg, fds=mode != "none", fds_num=30, _fds_raw_values=raw,
                                     use_scaler=False).cuda().train()
    distinct = []
    for s in range(4):                # four distinct mixed-length batches of 256, cycled
        _, b, _ = bench.synth(256, 128, 256, 100 + s, ragged=True)
        y = torch.from_numpy(np.random.default_rng(s).normal(0, 1, (256, 1)).astype(np.float32))
        distinct.append(({k: v.cuda() for k, v in b.items()}, y.cuda()))
    batches = [distinct[i % 4] for i in range(steps)]
    kw = dict(fds_stats="streaming") if mode == "streaming" else {}
    tuner = FineTuner(model, "regression", learning_rate=1e-4, total_steps=100 * steps, **kw)
    epoch_ms, step_ms = [], []
    for ep in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "streaming":
            tuner.fds_epoch_begin(ep)
        for dev, y in batches:
            tuner.step(dev, y, epoch=ep)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if mode == "streaming":
            tuner.fds_epoch_finish(ep)
        elif mode == "epoch_pass":
            tuner.fds_epoch_pass(batches, ep)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if ep >= 1:
            epoch_ms.append((t2 - t0) * 1e3)
            step_ms.append((t1 - t0) * 1e3 / steps)
    print(json.dumps(dict(mode=mode, tree=os.path.abspath(tree), steps=steps, epoch_ms=statistics.median(epoch_ms),
                          step_ms=statistics.median(step_ms), epochs_ms=epoch_ms)), flush=True)


def _run(cmd, timeout=400):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def ab(parent):
    me = os.path.abspath(__file__)
    arms = (("parent epoch_pass", parent, "epoch_pass"), ("this   streaming ", ROOT, "streaming"), ("this   epoch_pass", ROOT, "epoch_pass"))
    got = {name: [] for name, _, _ in arms}
    for k in range(3):
        for name, tree, mode in arms:
            r = _run([sys.executable, me, "epoch", mode, "--tree", tree])
            got[name].append(r)
            print(f"round {k} {name}: epoch {r['epoch_ms']:8.1f} ms, step {r['step_ms']:6.2f} ms", flush=True)
    for name, rs in got.items():
        print(f"median of 3 {name}: epoch {statistics.median(r['epoch_ms'] for r in rs):8.1f} ms, step "
              f"{statistics.median(r['step_ms'] for r in rs):6.2f} ms", flush=True)
    for k in range(2):
        for name, tree in (("parent", parent), ("parent-again", parent), ("this", ROOT)):
            r = _run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
                      "--no-rooflines"])
            print(f"round {k} headline {name:12s} {r['ms_per_step']:.3f} ms/step", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "kernels":
        kernels()
    elif what == "epoch":
        a = sys.argv[2:]
        tree = a[a.index("--tree") + 1] if "--tree" in a else ROOT
        steps = int(a[a.index("--steps") + 1]) if "--steps" in a else 20
        epoch(a[0], tree, steps)
    elif what == "ab":
        ab(os.path.abspath(sys.argv[2]))
    else:
        raise SystemExit(__doc__)
