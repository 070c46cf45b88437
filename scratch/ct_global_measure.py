"""profiles/ct_global.txt: the row-block ConR / SupCon kernels (global negatives under data parallelism) on one chip.

  distances   per mode and shape, the distance from the float64 reference (tests/ct_rows_ref.py) of the loss and of dfhat: the row
              blocks of the virtual ranks summed, beside the square kernels on the same inputs (the figures of
              tests/test_ct_global_gpu.py::test_virtual_ranks_partition_the_square_result)
  times       forward and backward alone on the chip at D = 512, device events, median of 20 after warm-up, arms alternated in one
              process: the square pair at B = 256, rows at (rows, Bg) = (256, 256) -- the same code -- and at (256, 2048), the
              8-rank shape

usage: python scratch/ct_global_measure.py [out.txt]   (default: ./ct_global.txt)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mm-dti_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import torch

from mmdti_hip import ops
import ct_rows_ref as R
import test_ct_global_gpu as TG

HEADLINE_MS = (50.7, 51.8)          # README: the headline step of the parent commit


def main(out):
    lines = ["# Global ConR / SupCon negatives: the row-block kernels on one MI355X (scratch/ct_global_measure.py)", ""]
    lines += ["## distance from the float64 reference: virtual ranks summed (rows) / the square kernels, same inputs", "",
              f"{'mode':8s} {'world x Bl x D':>15s} {'loss rows':>11s} {'loss square':>11s} {'dfhat rows':>11s} {'dfhat square':>12s} {'max|dfhat|':>11s}"]
    for world, Bl, D in ((2, 3, 24), (4, 65, 512)):
        for mode in R.MODES:
            d = TG.virtual_rank_distances(ops, mode, world, Bl, D)
            lines.append(f"{mode:8s} {f'{world} x {Bl} x {D}':>15s} {d['loss_rows']:11.3e} {d['loss_square']:11.3e} {d['dfhat_rows']:11.3e} "
                         f"{d['dfhat_square']:12.3e} {float(d['ref_df'].abs().max()):11.3e}")
    lines += ["", "## kernels alone, D = 512: median of 20 [min .. max] in microseconds, arms alternated", ""]
    D = 512
    for mode in R.MODES:
        arms = {}
        for name, rows, Bg in (("square B=256", None, 256), ("rows (256, 256)", 256, 256), ("rows (256, 2048)", 256, 2048)):
            c = R.ct_inputs(mode, Bg, D, seed=5 + Bg, use_w=True, C=12)
            fh, _ = ops.l2norm_fwd(c["f"].cuda())
            kw = TG._kw(mode, c)
            m = TG.MODE_ID[mode]
            if rows is None:
                fwd = lambda fh=fh, kw=kw, m=m: ops.ct_loss_fwd(m, fh, **kw)
                G = fwd()[1]
                bwd = lambda fh=fh, G=G: ops.ct_loss_bwd(fh, G, TG.T)
            else:
                fwd = lambda fh=fh, kw=kw, m=m, rows=rows: ops.ct_loss_rows_fwd(m, fh, 0, rows, **kw)
                G = fwd()[1]
                bwd = lambda fh=fh, G=G: ops.ct_loss_rows_bwd(fh, G, 0, TG.T)
            arms[name + " fwd"], arms[name + " bwd"] = fwd, bwd
        for fn in arms.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in arms}
        for _ in range(20):
            for k, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                t[k].append(a.elapsed_time(b) * 1e3)
        for k, v in t.items():
            lines.append(f"{mode:8s} {k:22s} {statistics.median(v):9.1f}  [{min(v):.1f} .. {max(v):.1f}]")
        pair = statistics.median(t["rows (256, 2048) fwd"]) + statistics.median(t["rows (256, 2048) bwd"])
        lines.append(f"{mode:8s} 8-rank pair {pair:.1f} us = {100 * pair / 1e3 / HEADLINE_MS[1]:.2f} .. {100 * pair / 1e3 / HEADLINE_MS[0]:.2f} % of the "
                     f"headline step ({HEADLINE_MS[0]} .. {HEADLINE_MS[1]} ms)")
        lines.append("")
    lines += ["## collectives: not measured (one GPU).  Message sizes per step and rank at B_loc = 32, D = 512, 8 ranks:",
              f"gathered  B_loc (D + 3) 4 = {32 * (D + 3) * 4} bytes sent per rank ({8 * 32 * (D + 3) * 4} received); multilabel adds B_loc C 8 bytes",
              f"reduced   B_glob D 4      = {8 * 32 * D * 4} bytes (all-reduce SUM, own rows kept)", ""]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    open(out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "ct_global.txt")
