"""Measurements behind profiles/accum_union.txt (DESIGN.md "Accumulated steps"): ms per optimizer step and peak device memory at the
bench shape (reference architecture, 128 atoms x 256 tokens, train mode), one arm per fresh process.

    python scratch/accum_measure.py all [OUT] [--parent DIR]   every arm, 2 rounds, written to OUT (default profiles/accum_union.txt);
                                                               --parent DIR: a directory holding the PARENT commit's ``mmdti_hip``
                                                               package (with the built library) -- the step(256) arm then also runs
                                                               from it
    python scratch/accum_measure.py arm NAME                   one arm in this process:
                                                               step256 | union4x64 | micro4x64 | union4x256 | micro4x256
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("ACCUM_MEASURE_PACKAGE") or os.path.join(ROOT, "mm-dti_amd")
for p in (ROOT, PKG):
    sys.path.insert(0, p)

ARMS = ("step256", "union4x64", "micro4x64", "union4x256", "micro4x256")


def arm(name, warmup=3):
    steps = 6 if name.endswith("x256") else 20          # (a timed window of a second or more)
    import torch
    import bench
    from mmdti_hip.trainer import FineTuner
    model, _ = bench.build_model()
    model = model.cuda().train()
    tuner = FineTuner(model, "classification", total_steps=10_000)
    if name == "step256":
        _, b, y = bench.synth(256, 128, 256, seed=1234)
        b, y = {k: v.cuda() for k, v in b.items()}, y.cuda()
        call = lambda: tuner.step(b, y, epoch=0)
    else:
        mode, shape = name[:5], name[5:]
        k, per = (int(v) for v in shape.split("x"))
        micro = []
        for i in range(k):
            _, b, y = bench.synth(per, 128, 256, seed=1234 + i)
            micro.append(({kk: v.cuda() for kk, v in b.items()}, y.cuda()))
        call = lambda: tuner.step_accumulated(micro, epoch=0, negatives=mode)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    print(f"{name:12s} {ms:9.2f} ms / optimizer step over {steps:2d} steps   peak {torch.cuda.max_memory_allocated() / 2 ** 30:6.2f} GiB allocated "
          f"({torch.cuda.max_memory_reserved() / 2 ** 30:.2f} GiB reserved)", flush=True)


def run_all(out_path, parent):
    lines = ["accumulated steps at the bench shape (reference architecture, 128 atoms x 256 tokens, train mode, one MI355X);",
             "one fresh process per arm, 3 warm-up optimizer steps, then 20 timed ones (6 for 4 x 256), host clock round a synchronised loop;",
             "<mode>K x b: step_accumulated over K micro-batches of b molecules, negatives = union | micro", ""]
    arms = [(a, None) for a in ARMS]
    if parent:
        arms.insert(0, ("step256", parent))
    for rnd in range(2):
        for name, pkg in arms:
            env = dict(os.environ)
            if pkg:
                env["ACCUM_MEASURE_PACKAGE"] = pkg
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "arm", name], capture_output=True, text=True, timeout=420, env=env)
            if r.returncode != 0:          # (nothing more is started on the device after a failure)
                raise SystemExit(f"arm {name} failed ({r.returncode}): {r.stderr[-1500:]}")
            line = f"round {rnd}  {'parent commit' if pkg else 'this tree    '}  {r.stdout.strip().splitlines()[-1]}"
            print(line, flush=True)
            lines.append(line)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else ""
    if what == "arm" and len(sys.argv) > 2 and sys.argv[2] in ARMS:
        arm(sys.argv[2])
    elif what == "all":
        rest = sys.argv[2:]
        parent = None
        if "--parent" in rest:
            i = rest.index("--parent")
            parent = os.path.abspath(rest[i + 1])
            del rest[i:i + 2]
        run_all(rest[0] if rest else os.path.join(ROOT, "profiles", "accum_union.txt"), parent)
    else:
        raise SystemExit(__doc__)
