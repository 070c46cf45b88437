"""Measurements behind profiles/lora.txt (DESIGN.md "LoRA adapters"), one arm per fresh process.

    python scratch/lora_measure.py all [OUT] [--parent DIR]
        every arm, 2 rounds alternating, written to OUT (default profiles/lora.txt).  --parent DIR: a directory holding the PARENT
        commit's ``include/`` and ``mm-dti_amd/mmdti_hip`` package with its built library -- the full fine-tune of the headline step then
        also runs from it (the default path must not have moved).
    python scratch/lora_measure.py seq [OUT] --parent DIR [--shape small|head]
        the measurements behind profiles/lora_seq.txt (adapted layers issued from the library's sequencers): per shape the full fine-tune
        and the LoRA step of this tree and of the parent commit's package, and this tree's LoRA step with MMDTI_LORA_SEQ=0 (op by op);
        2 rounds alternating, written to OUT (default profiles/lora_seq.txt; with --shape the other shape's lines in OUT are kept).
    python scratch/lora_measure.py arm NAME
        one arm in this process: kernels | {head,small}_{full,frozen,lora}
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LORA_MEASURE_PACKAGE") or os.path.join(ROOT, "mm-dti_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

STEP_ARMS = tuple(f"{s}_{m}" for s in ("head", "small") for m in ("full", "frozen", "lora"))
TOWER_PREFIXES = ("embed_tokens.", "encoder.", "gbf.", "gbf_proj.", "bert.")


def kernels(T=65536, n=512):
    """device events round 100 back-to-back calls (after 10) of each kernel alone at T x 512 -> 512, beside the bytes it must move"""
    import torch
    from mmdti_hip import ops
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731

    def timed(call, reps=100):
        for _ in range(10):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps * 1e3

    for r in (8, 16, 32):
        x16, x = rnd(T, n).half().cuda(), rnd(T, n).bfloat16().cuda()
        A, B = (rnd(r, n) * n ** -0.5), rnd(n, r) * 0.1
        Ab, Bb, Ah, Bh = A.bfloat16().cuda(), B.bfloat16().cuda(), A.half().cuda(), B.half().cuda()
        y16, y = rnd(T, n).half().cuda(), rnd(T, n).bfloat16().cuda()
        dy, t = (rnd(T, n) * 0.1).bfloat16().cuda(), rnd(T, r).bfloat16().cuda()
        dA, dB = torch.zeros(r, n, device="cuda"), torch.zeros(n, r, device="cuda")
        dx32, dx16 = torch.zeros(T, n, device="cuda"), torch.zeros(T, n, device="cuda", dtype=torch.bfloat16)
        u = ops.lora_bwd(x, dy, t, Bb, dA, dB, 2.0)
        small = 2 * r * n * 2
        rows = [
            ("lora_fwd bf16", timed(lambda: ops.lora_fwd(x, Ab, Bb, y, 1e-3)), T * n * 2 * 3 + T * r * 2 + small),
            ("lora_fwd fp16", timed(lambda: ops.lora_fwd(x16, Ah, Bh, y16, 1e-3)), T * n * 2 * 3 + T * r * 2 + small),
            ("lora_bwd", timed(lambda: ops.lora_bwd(x, dy, t, Bb, dA, dB, 2.0)), T * n * 2 * 2 + T * r * 2 * 2 + small * 3),
            ("lora_bwd fp16 x", timed(lambda: ops.lora_bwd(x16, dy, t, Bb, dA, dB, 2.0)), T * n * 2 * 2 + T * r * 2 * 2 + small * 3),
            ("lora_dx fp32", timed(lambda: ops.lora_dx(u, Ab, dx32)), T * n * 4 * 2 + T * r * 2 + small // 2),
            ("lora_dx bf16", timed(lambda: ops.lora_dx(u, Ab, dx16)), T * n * 2 * 2 + T * r * 2 + small // 2),
        ]
        for name, us, nbytes in rows:
            print(f"T {T} in {n} out {n} r {r:2d}  {name:16s} {us:8.1f} us   {nbytes / 2 ** 20:7.1f} MiB to move   {nbytes / us / 1e6:6.2f} TB/s",
                  flush=True)


def step(name, warmup=5, steps=30):
    import torch
    import mmdti_hip          # (before bench, which puts this tree's package first on sys.path: the parent arm must keep the parent's)
    assert os.path.abspath(mmdti_hip.__file__).startswith(os.path.abspath(PKG)), mmdti_hip.__file__
    import bench
    from mmdti_hip.trainer import FineTuner
    shape, mode = name.split("_")
    model, _ = bench.build_model()
    model = model.cuda().train()
    if mode == "frozen":
        for n, p in model.named_parameters():
            if n.startswith(TOWER_PREFIXES):
                p.requires_grad = False
    elif mode == "lora":
        from mmdti_hip import lora
        lora.apply_lora(model, lora.LoRAConfig(rank=16, alpha=32.0, targets=("q", "v"), towers=("bert", "unimol")))
    tuner = FineTuner(model, "classification", total_steps=10_000)
    small = shape == "small"
    _, b, y = bench.synth(32 if small else 256, 128, 256, seed=8765 if small else 1234, ragged=small)
    b, y = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}, y.cuda()
    steps = steps * 3 if small else steps
    for _ in range(warmup):
        tuner.step(b, y, epoch=0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        tuner.step(b, y, epoch=0)
    host = (time.perf_counter() - t0) / steps * 1e3          # the host's share: all steps enqueued, the device not yet waited for
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    what = "32 mixed-length molecules" if small else "headline, 256 molecules"
    label = {"full": "full fine-tune", "frozen": "both towers frozen", "lora": "both towers LoRA r=16 q,v"}[mode]
    print(f"{name:12s} {what:26s} {label:26s}: {ms:8.3f} ms / step over {steps} steps, peak {torch.cuda.max_memory_allocated() / 2 ** 30:6.2f} GiB, "
          f"{tuner.arena.numel} trainable elements, host enqueue {host:.3f} ms / step", flush=True)


def _arm(name, pkg=None, env_extra=None):
    """one arm in a fresh process -> its result lines (nothing more is started on the device after a failure)"""
    env = dict(os.environ, **(env_extra or {}))
    if pkg:
        env["LORA_MEASURE_PACKAGE"] = pkg
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "arm", name], capture_output=True, text=True, timeout=300, env=env)
    if r.returncode != 0:
        raise SystemExit(f"arm {name} failed ({r.returncode}): {r.stderr[-1500:]}")
    return [l for l in r.stdout.strip().splitlines() if " us " in l or " ms " in l]


SEQ_HEAD = ["Adapted layers from the library's sequencers (reference architecture, 128 atoms x 256 tokens, train mode, one MI355X); one fresh",
            "process per arm, arms alternating over 2 rounds; host clock round a synchronised loop of engine.step on a resident batch (5",
            "warm-up steps).  LoRA: r = 16 on q and v of tower 1 and tower 2, both towers frozen; the cross block and the heads train in every",
            "arm.  'parent commit': the package of the commit before this change; 'op by op': this tree with MMDTI_LORA_SEQ=0.", ""]


def run_seq(out_path, parent, shapes):
    assert parent, "seq needs --parent DIR"
    kept = []
    if os.path.exists(out_path):                # (a run of one shape keeps the other shape's lines)
        kept = [l for l in open(out_path).read().splitlines() if l.startswith("round ") and not any(f" {s}_" in l for s in shapes)]
    lines = []
    for rnd in range(2):
        for shape in shapes:
            for tag, name, pkg, env in (("this tree      ", f"{shape}_full", None, None), ("parent commit  ", f"{shape}_full", parent, None),
                                        ("this tree      ", f"{shape}_lora", None, None), ("parent commit  ", f"{shape}_lora", parent, None),
                                        ("this, op by op ", f"{shape}_lora", None, {"MMDTI_LORA_SEQ": "0"})):
                for ln in _arm(name, pkg, env):
                    line = f"round {rnd}  {tag} {ln}"
                    print(line, flush=True)
                    lines.append(line)
                with open(out_path, "w") as f:
                    f.write("\n".join(SEQ_HEAD + kept + lines) + "\n")


def run_all(out_path, parent):
    lines = ["LoRA adapters (reference architecture, 128 atoms x 256 tokens, train mode, one MI355X); one fresh process per arm, arms",
             "alternating over 2 rounds.  kernels: each kernel alone, device events round 100 back-to-back calls (10 warm-up); 'to move': the",
             "bytes of every operand read or written once.  steps: host clock round a synchronised loop of engine.step on a resident batch",
             "(5 warm-up steps); frozen / LoRA: tower 1 (embed_tokens, encoder, gbf, gbf_proj) and tower 2 (bert); the cross block and the",
             "heads train in every arm.", ""]
    arms = [("kernels", None)]
    for a in STEP_ARMS:
        if parent and a == "head_full":
            arms.append((a, parent))
        arms.append((a, None))
    for rnd in range(2):
        for name, pkg in arms:
            if name == "kernels" and rnd:
                continue
            tag = "parent commit  " if pkg else "this tree      "
            for ln in _arm(name, pkg):
                line = f"round {rnd}  {tag} {ln}"
                print(line, flush=True)
                lines.append(line)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "arm" and len(sys.argv) > 2 and sys.argv[2] == "kernels":
        kernels()
    elif what == "arm" and len(sys.argv) > 2 and sys.argv[2] in STEP_ARMS:
        step(sys.argv[2])
    elif what in ("all", "seq"):
        rest = sys.argv[2:]
        parent = None
        shapes = ("small", "head")
        if "--shape" in rest:
            i = rest.index("--shape")
            shapes = (rest[i + 1],)
            del rest[i:i + 2]
        if "--parent" in rest:
            i = rest.index("--parent")
            parent = os.path.join(os.path.abspath(rest[i + 1]), "mm-dti_amd")
            del rest[i:i + 2]
        if what == "seq":
            run_seq(rest[0] if rest else os.path.join(ROOT, "profiles", "lora_seq.txt"), parent, shapes)
        else:
            run_all(rest[0] if rest else os.path.join(ROOT, "profiles", "lora.txt"), parent)
    else:
        raise SystemExit(__doc__)
