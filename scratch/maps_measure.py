"""profiles/attention_maps.txt: what the attention-map read-out costs, on one MI355X.

    python scratch/maps_measure.py kernel     the two map kernels alone on the chip, each beside the forward kernel of the same shape
    python scratch/maps_measure.py model      model(**net_input) under no_grad against MM_Model.attention_maps, bench and ragged batch
    python scratch/maps_measure.py            both

Each launch is timed alone between two events, median of 20 after 3 warm-up launches (the method of scratch/ema_measure.py).  The
headline step of this commit against the parent commit's package runs beside it in the same job: `python bench.py --gpus 1 --steps 10
--warmup 3 --no-cpu-baseline --no-rooflines` from the two trees, alternating, three times (scratch/ab/run.sh alternates two LIBRARIES under
one header; the parent's library lacks the three new exports, so here the whole parent package runs from its own tree)."""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mm-dti_amd")]

import torch  # noqa: E402

from mmdti_hip import ops  # noqa: E402

DEV = "cuda"


def timed(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def line(name, us, nbytes=None, note=""):
    gbs = f"{nbytes / us / 1e3:9.1f} GB/s" if nbytes else " " * 14
    print(f"   {name:<58s}{us:9.1f} us   {gbs}   {note}", flush=True)


def kernels():
    print("1. The kernels alone on the chip (median of 20 launches after 3)\n")
    # ---- pair map: 256 molecules x 130 atom rows x 64 heads, compact fp16 planes (the bench batch's tower 1)
    B, N, H = 256, 130, 64
    ld, D = ops.pair_ld(N), H * 8
    g = torch.Generator(device=DEV).manual_seed(1)
    bias = ops.pair_tile(torch.randn(B, H, N, N, device=DEV, generator=g), N).half()
    qkv = (torch.randn(B * N, 3 * D, device=DEV, generator=g)).to(ops.act16())
    s, _ = ops.pair_attn_fwd(qkv, bias, None, B, N, H, ld, 8 ** -0.5)
    plane = float(B) * H * N * ld * 2
    t_fwd = timed(lambda: ops.pair_attn_fwd(qkv, bias, None, B, N, H, ld, 8 ** -0.5))
    line("mmdti_pair_attn_fwd (p = 0), 256 x 130 x 64 heads, layout 3", t_fwd, 2 * plane + B * N * 64.0 * H, "reads and writes the planes")
    t_map = timed(lambda: ops.pair_attn_map(s, B, N, H, ld))
    line("mmdti_pair_attn_map, head mean", t_map, plane + 4.0 * B * N * N, "reads the planes once, writes [B,N,N] fp32")
    t_one = timed(lambda: ops.pair_attn_map(s, B, N, H, ld, head=5))
    line("mmdti_pair_attn_map, one head", t_one, plane / H + 4.0 * B * N * N)
    print(f"\n   condition time(map) <= time(forward): {t_map:.1f} <= {t_fwd:.1f} us: {'met' if t_map <= t_fwd else 'NOT MET'}\n")
    # ---- fused map: tower 2 (8 heads x 64, 256 x 256 tokens) and the cross block (16 heads x 32, 130 atoms x 256 tokens, both directions)
    for what, heads, hd, Lq, Lk in (("tower 2: 8 heads x 64, 256 x 256 tokens", 8, 64, 256, 256), ("cross: 16 heads x 32, 130 atoms x 256 tokens", 16, 32, 130, 256),
                                    ("cross: 16 heads x 32, 256 tokens x 130 atoms", 16, 32, 256, 130)):
        Dm = heads * hd
        q = torch.randn(B * Lq, Dm, device=DEV, generator=g).bfloat16()
        k = torch.randn(B * Lk, Dm, device=DEV, generator=g).bfloat16()
        v = torch.randn(B * Lk, Dm, device=DEV, generator=g).bfloat16()
        key_add = torch.zeros(B, Lk, device=DEV)
        fwd = ops.attn_dispatch(Lq, Lk)[0]
        _, stats = fwd(q, k, v, key_add, B, heads, Lq, Lk, hd ** -0.5)
        t_f = timed(lambda: fwd(q, k, v, key_add, B, heads, Lq, Lk, hd ** -0.5))
        t_m = timed(lambda: ops.attn_map(q, k, key_add, stats, B, heads, Lq, Lk, hd ** -0.5))
        line(f"mmdti_attn_fwd, {what}", t_f)
        line("mmdti_attn_map, head mean, same shape", t_m, 4.0 * B * Lq * Lk, "(bytes: the map written)")
    print()


def model_level():
    import bench
    from mmdti_hip.collate import device_payload, HOST_FIELDS
    print("2. The whole model: model(**net_input) under no_grad against attention_maps (eval mode; median of 5 after 2 calls; peak = max memory allocated)\n")
    model, _ = bench.build_model()
    model = model.cuda().eval()
    for what, ragged in (("bench batch (256 x 128 atoms x 256 tokens)", False), ("ragged batch (256 molecules of mixed length)", True)):
        _, batch, _ = bench.synth(256, 128, 256, seed=3, ragged=ragged)
        full = device_payload(dict(batch), pad_idx=0)
        host = {k: full[k] for k in HOST_FIELDS if k in full}
        dev = {k: v.cuda() for k, v in batch.items()}
        kw = dict(dev, **host)

        def fwd():
            with torch.no_grad():
                return model(**kw)

        arms = (("model(**net_input), no_grad", fwd), ("attention_maps(which=('cross',))", lambda: model.attention_maps(**kw)),
                ("attention_maps(all three, layers='all')", lambda: model.attention_maps(**kw, which=("cross", "unimol", "bert"), layers="all")))
        print(f"   {what}", flush=True)
        for name, fn in arms:
            fn()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            us = timed(fn, n=5, warm=1)
            peak = torch.cuda.max_memory_allocated()
            print(f"      {name:<46s}{us / 1e3:9.2f} ms   peak {peak / 2 ** 20:9.1f} MiB (+{(peak - base) / 2 ** 20:8.1f} over the resident {base / 2 ** 20:.1f})   layout {model.last_layout}",
                  flush=True)
        print()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    assert torch.cuda.is_available()
    print("Attention maps (mmdti_attn_map, mmdti_pair_attn_map) -- one MI355X, scratch/maps_measure.py\n")
    if mode in ("kernel", "all"):
        kernels()
    if mode in ("model", "all"):
        model_level()
