"""Measurements behind profiles/infonce_bank.txt (DESIGN.md "Memory bank of InfoNCE negatives"), one arm per fresh process.

    python scratch/infonce_bank_measure.py all [OUT] [--parent DIR] [--one-split LIB]
        every arm, 2 rounds alternating, written to OUT (default profiles/infonce_bank.txt).  --parent DIR: a directory holding the PARENT
        commit's ``mmdti_hip`` package with its built library -- the two bank-less step arms then also run from it.  --one-split LIB: a
        libmmdti_hip.so of this tree built with EXTRA=-DMMDTI_NCE_BANK_ONE_SPLIT (the same kernels, never split) -- the kernel arm then
        also runs on it.
    python scratch/infonce_bank_measure.py arm NAME
        one arm in this process: kernels | small0 | small4096 | head0 | head4096
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("BANK_MEASURE_PACKAGE") or os.path.join(ROOT, "mm-dti_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

STEP_ARMS = ("small0", "small4096", "head0", "head4096")
SHAPES = ((32, 32, 4096), (256, 256, 4096), (2048, 256, 16384))          # (Bg, Bl, Q)


def kernels():
    """device events round 200 back-to-back calls of one direction (after 20): mmdti_infonce_bank_dir beside mmdti_infonce_dir"""
    import torch
    from mmdti_hip import ops
    unit = lambda n, s: torch.nn.functional.normalize(torch.randn(n, 50, generator=torch.Generator().manual_seed(s)), dim=-1).cuda()

    def timed(call, n=200):
        for _ in range(20):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3

    for Bg, Bl, Q in SHAPES:
        q, k, bank = unit(Bg, 1), unit(Bg, 2), unit(Q, 3)
        valid = torch.ones(Q, device="cuda", dtype=torch.uint8)
        loss, dq, dk = torch.zeros(1, device="cuda"), torch.zeros(Bg, 50, device="cuda"), torch.zeros(Bg, 50, device="cuda")
        row0 = Bg - Bl
        plain = timed(lambda: ops.infonce_dir(q, k, row0, Bl, 0.1, loss, dq, dk))
        banked = timed(lambda: ops.infonce_bank_dir(q, k, row0, Bl, 0.1, loss, dq, dk, bank, valid))
        plan = ops.infonce_bank_plan(Bg, Bl, Q)
        print(f"Bg {Bg:5d} Bl {Bl:4d} Q {Q:6d}: infonce_dir {plain:8.1f} us   infonce_bank_dir {banked:8.1f} us   "
              f"({plan['splits']} splits, {plan['grid']} workgroups of one wave, {plan['tiles']} key tiles)", flush=True)


def step(name, warmup=5, steps=40):
    import torch
    import mmdti_hip          # (before bench, which puts this tree's package first on sys.path: the parent arm must keep the parent's)
    assert os.path.abspath(mmdti_hip.__file__).startswith(os.path.abspath(PKG)), mmdti_hip.__file__
    import bench
    from mmdti_hip.trainer import FineTuner
    model, _ = bench.build_model()
    model = model.cuda().train()
    Q = int(name.lstrip("smalhed"))
    tuner = FineTuner(model, "classification", total_steps=10_000, **(dict(memory_bank=Q) if Q else {}))
    small = name.startswith("small")
    _, b, y = bench.synth(32 if small else 256, 128, 256, seed=8765 if small else 1234, ragged=small)
    b, y = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}, y.cuda()
    steps = steps * 3 if small else steps
    for _ in range(warmup):
        tuner.step(b, y, epoch=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tuner.step(b, y, epoch=0)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    what = "32 mixed-length molecules" if small else "headline, 256 molecules"
    print(f"{name:10s} {what:26s} memory_bank {Q:5d}: {ms:8.3f} ms / step over {steps} steps", flush=True)


def run_all(out_path, parent, one_split):
    lines = ["InfoNCE memory bank (reference architecture, 128 atoms x 256 tokens, train mode, one MI355X); one fresh process per arm, arms",
             "alternating over 2 rounds.  kernels: one direction alone, device events round 200 back-to-back calls, all Q slots valid, D = 50.",
             "steps: host clock round a synchronised loop of engine.step on a resident batch (5 warm-up steps).", ""]
    arms = [("kernels", None, None)]
    if one_split:
        arms.append(("kernels", None, one_split))
    for a in STEP_ARMS:
        if parent and a.endswith("0") and not a.endswith("4096"):
            arms.append((a, parent, None))
        arms.append((a, None, None))
    for rnd in range(2):
        for name, pkg, lib in arms:
            env = dict(os.environ)
            if pkg:
                env["BANK_MEASURE_PACKAGE"] = pkg
            if lib:
                env["MMDTI_HIP_LIB"] = lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "arm", name], capture_output=True, text=True, timeout=300, env=env)
            if r.returncode != 0:          # (nothing more is started on the device after a failure)
                raise SystemExit(f"arm {name} failed ({r.returncode}): {r.stderr[-1500:]}")
            tag = "parent commit  " if pkg else "forced 1 split " if lib else "this tree      "
            for ln in [l for l in r.stdout.strip().splitlines() if " us " in l or " ms " in l]:
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
    elif what == "all":
        rest = sys.argv[2:]
        opt = {}
        for flag in ("--parent", "--one-split"):
            if flag in rest:
                i = rest.index(flag)
                opt[flag] = os.path.abspath(rest[i + 1])
                del rest[i:i + 2]
        run_all(rest[0] if rest else os.path.join(ROOT, "profiles", "infonce_bank.txt"), opt.get("--parent"), opt.get("--one-split"))
    else:
        raise SystemExit(__doc__)
