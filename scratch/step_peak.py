"""bench.py's step with the peak of allocated device memory printed behind its JSON line: every argument goes to bench.py.

    python scratch/step_peak.py --gpus 1 --batch 64 --tokens 512 --steps 20 --warmup 5 --no-rooflines --no-cpu-baseline
"""
import os, runpy, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
try:
    runpy.run_path(sys.argv[0], run_name="__main__")
except SystemExit as e:
    if e.code not in (None, 0):
        raise
import torch
print(f"peak allocated {torch.cuda.max_memory_allocated() / 2 ** 30:.3f} GiB, reserved {torch.cuda.max_memory_reserved() / 2 ** 30:.3f} GiB")
