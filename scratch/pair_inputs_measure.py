"""pair_inputs="coords" against "planes": the two hot pair-bias kernels alone on the chip, bytes per batch and host collate time.

    python scratch/pair_inputs_measure.py [--baseline-lib /path/to/the/parent/commit's/libmmdti_hip.so] [--out profiles/pair_inputs.txt]

Kernel times: HIP events around one launch, median of 20 after 3 warm-up launches, at the bench shape (256 molecules x 130 tokens; all
at full length, and the mixed-length batch on packed rows with its tile prefixes), compact tiled planes as on the hot path.
--baseline-lib: the planes kernels of another build of the library (the parent commit's), loaded side by side in this process and
driven with the same pointers -- the header of this tree declares symbols an older library lacks, so it cannot go through MMDTI_HIP_LIB.
Collate times and byte counts need no GPU (--cpu-only).  --step: the whole fine-tune step of bench.py's model in both modes."""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

V, PAD, E = 31, 0, 31 * 31


def samples(B, max_atoms, ragged, seed=1234):
    from mmdti_hip.synth import molecule
    rng = np.random.default_rng(seed)
    elem_p = np.zeros(V)
    elem_p[8], elem_p[4], elem_p[5], elem_p[6] = 0.5, 0.3, 0.075, 0.075
    rest = [i for i in range(4, V - 1) if i not in (4, 5, 6, 8)]
    elem_p[rest] = 0.05 / len(rest)
    out = []
    for _ in range(B):
        na = int(np.clip(round(rng.normal(0.375 * max_atoms, 0.16 * max_atoms)), max(2, max_atoms // 16), max_atoms)) if ragged else max_atoms
        t, d, e, c = molecule(rng, na, V, elem_p, with_coord=True)
        out.append(({"src_tokens": t, "src_distance": d, "src_coord": c, "src_edge_type": e}, np.zeros(1, dtype=np.int64)))
    return out


def host_side(lines, B, atoms):
    from mmdti_hip.collate import collate_batch, device_payload
    for ragged in (False, True):
        smp = samples(B, atoms, ragged)
        for mode in ("planes", "coords"):
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                batch, _ = collate_batch(smp, PAD, None, pair_inputs=mode)
                pay = device_payload(batch, E, PAD, pair_inputs=mode)
                ts.append(time.perf_counter() - t0)
            nbytes = sum(v.numel() * v.element_size() for k, v in pay.items() if torch.is_tensor(v) and k not in ("atom_counts", "token_counts"))
            lines.append(f"host  {'mixed' if ragged else 'dense'} {B} x {pay['src_tokens'].shape[1]}  pair_inputs={mode:6s}  collate + payload {1e3 * statistics.median(ts):8.2f} ms/batch "
                         f"(median of 7, one process)   tower-1 H2D bytes {nbytes / 1e6:8.3f} MB")


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def device_side(lines, B, atoms, baseline):
    from mmdti_hip import ops, _abi
    from mmdti_hip.collate import collate_batch, device_payload
    from mmdti_hip.packing import PackedRows
    lib = ops.lib()
    libs = [("this build", lib._dll)]
    if baseline:
        libs.append(("parent build", ctypes.CDLL(baseline)))
    protos = _abi.parse_header()
    for _, dll in libs:
        for name in ("mmdti_gbf_bias_fwd", "mmdti_gbf_bias_bwd_full", "mmdti_gbf_bias_fwd_coords", "mmdti_gbf_bias_bwd_full_coords"):
            if hasattr(dll, name):
                getattr(dll, name).restype, getattr(dll, name).argtypes = protos[name][0], protos[name][1]
    gen = torch.Generator().manual_seed(5)
    K, Fh, H = 128, 128, 64
    mul, bias = (1 + 0.1 * torch.randn(E, generator=gen)).cuda(), (0.1 * torch.randn(E, generator=gen)).cuda()
    means, stds = (torch.rand(K, generator=gen) * 3).cuda(), (torch.rand(K, generator=gen) * 3 - 1.5).cuda()
    w1, b1 = (torch.randn(Fh, K, generator=gen) * 0.2).bfloat16().cuda(), (torch.randn(Fh, generator=gen) * 0.1).cuda()
    w2, b2 = (torch.randn(H, Fh, generator=gen) * 0.2).bfloat16().cuda(), (torch.randn(H, generator=gen) * 0.1).cuda()
    grads = [torch.zeros(s, device="cuda") for s in (Fh * K, Fh, H * Fh, H, E, E, K, K)]
    ws = torch.empty(lib._dll.mmdti_gbf_bias_bwd_full_workspace(E), device="cuda", dtype=torch.uint8)
    p = lambda t: 0 if t is None else t.data_ptr()
    st = 0
    for ragged in (False, True):
        batch, _ = collate_batch(samples(B, atoms, ragged), PAD, None)
        pay = device_payload(batch, E, PAD)
        N = pay["src_tokens"].shape[1]
        ld = ops.pair_ld(N)
        tok, coord = pay["src_tokens"].cuda(), batch["src_coord"].cuda()
        dist, et = pay["src_distance"].cuda(), pay["src_edge_type"].cuda()
        pf = pb = rf = rb = None
        if ragged:
            ac = pay["atom_counts"].to(torch.int64)
            pf, pb, rf, rb = ops.gbf_tile_prefixes((ac + 15) // 16, N, "cuda", PackedRows(ac, N).rows_host)
        rec = ops.pair_records(coord, tok)
        out = ops.pair_empty(B, H, N, "cuda", True, zero=True, dtype=torch.float16)
        g = (torch.randn(out.shape, generator=gen) * 0.01).bfloat16().cuda()
        tabs = [mul, bias, means, stds]
        tag = f"{'mixed, packed rows' if ragged else 'dense'} {B} x {N}"

        def fwd_planes(dll):
            rc = dll.mmdti_gbf_bias_fwd(st, p(dist), p(et), et.element_size(), *map(p, tabs), p(w1), p(b1), p(w2), p(b2), B, N, ld, K, Fh, H, E, p(out), 0, 0, 0, 5, p(pf), p(rf))
            assert rc == 0

        def fwd_coords(dll):
            rc = dll.mmdti_gbf_bias_fwd_coords(st, p(rec), V, PAD, *map(p, tabs), p(w1), p(b1), p(w2), p(b2), B, N, ld, K, Fh, H, E, p(out), 5, p(pf), p(rf))
            assert rc == 0

        def bwd_planes(dll):
            rc = dll.mmdti_gbf_bias_bwd_full(st, p(g), p(dist), p(et), et.element_size(), *map(p, tabs), p(w1), p(b1), p(w2), B, N, ld, K, Fh, H, E, 5, *map(p, grads), p(pb), p(rb),
                                             p(ws), ws.numel())
            assert rc == 0

        def bwd_coords(dll):
            rc = dll.mmdti_gbf_bias_bwd_full_coords(st, p(g), p(rec), V, PAD, *map(p, tabs), p(w1), p(b1), p(w2), B, N, ld, K, Fh, H, E, 5, *map(p, grads), p(pb), p(rb), p(ws),
                                                    ws.numel())
            assert rc == 0

        st = torch.cuda.current_stream().cuda_stream
        for rep in range(2):                                   # (twice: the second pass shows the run-to-run spread of each figure)
            for name, dll in libs:
                for what, fn in (("gbf_bias_fwd      planes", fwd_planes), ("gbf_bias_bwd_full planes", bwd_planes)):
                    med, lo, hi = timed(lambda: fn(dll))
                    lines.append(f"chip  {tag}  {what}  {name:12s}  pass {rep}  median {med:7.3f} ms  (min {lo:7.3f}, max {hi:7.3f}; 20 launches)")
            for what, fn in (("gbf_bias_fwd      coords", fwd_coords), ("gbf_bias_bwd_full coords", bwd_coords)):
                med, lo, hi = timed(lambda: fn(lib._dll))
                lines.append(f"chip  {tag}  {what}  {'this build':12s}  pass {rep}  median {med:7.3f} ms  (min {lo:7.3f}, max {hi:7.3f}; 20 launches)")
        med, lo, hi = timed(lambda: ops.pair_records(coord, tok))
        lines.append(f"chip  {tag}  pair_records (pack, once per forward; includes the allocation)  median {med:7.3f} ms")
        med, lo, hi = timed(lambda: ops.pair_inputs_from_records(rec, V, PAD))
        lines.append(f"chip  {tag}  pair_inputs_from_coords (the fallback's materialiser, int16 edge types)  median {med:7.3f} ms")
        torch.cuda.synchronize()


def step_side(lines, B, atoms, tokens):
    """The whole fine-tune step of bench.py's model on a resident batch, fed the planes or the coordinates (alternated, three rounds)."""
    sys.path.insert(0, ROOT)
    import bench
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.synth import synth_batch
    from mmdti_hip.collate import device_payload, to_device
    model, _ = bench.build_model()
    model = model.cuda().train()
    tuner = FineTuner(model, "classification", total_steps=100000)
    for ragged in (False, True):
        cpu, label = synth_batch(B, atoms, tokens, seed=4321, ragged=ragged, with_coord=True)
        feeds = {m: to_device(device_payload(cpu, E, PAD, pair_inputs=m), "cuda", non_blocking=False) for m in ("planes", "coords")}
        y = label.cuda()
        for rnd in range(3):
            for mode in ("planes", "coords"):
                for _ in range(3):
                    tuner.step(feeds[mode], y)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(15):
                    tuner.step(feeds[mode], y)
                torch.cuda.synchronize()
                lines.append(f"step  {'mixed' if ragged else 'dense'} {B} x {cpu['src_tokens'].shape[1]} x {tokens} tokens ({model.last_layout} rows)  pair_inputs={mode:6s}  round {rnd}  "
                             f"{1e3 * (time.perf_counter() - t0) / 15:7.3f} ms/step (15 steps, resident batch)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--atoms", type=int, default=128)
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--step", action="store_true", help="also time the whole fine-tune step in both modes")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []
    host_side(lines, a.batch, a.atoms)
    if not a.cpu_only:
        device_side(lines, a.batch, a.atoms, a.baseline_lib)
        if a.step:
            step_side(lines, a.batch, a.atoms, a.tokens)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
