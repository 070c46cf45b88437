"""Standalone timing of the fused BERT attention kernels against the materialised-scores chain at one shape.

    python scratch/attn_bench.py [p] [iters] [--L 512 | --Lq 258 --Lk 384] [--heads 8] [--hd 64] [--B 256]

Up to 256 x 256 the short kernels (ops.attn_fwd / attn_bwd) run, above them the long pair (ops.attn_long_*): ops.attn_dispatch, as
functional.py picks them.  The materialised chain is the one functional._bert_layer_fwd / _bwd launch with ops.FUSED_ATTN = False:
scores GEMM, softmax_fwd, context GEMM; dP, dV, softmax_bwd, dQ, dK."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "mm-dti_amd"))
import torch
from mmdti_hip import ops
ap = argparse.ArgumentParser()
ap.add_argument("p", nargs="?", type=float, default=0.1)
ap.add_argument("iters", nargs="?", type=int, default=20)
ap.add_argument("--L", type=int, default=256)
ap.add_argument("--Lq", type=int)
ap.add_argument("--Lk", type=int)
ap.add_argument("--B", type=int, default=256)
ap.add_argument("--heads", type=int, default=8)
ap.add_argument("--hd", type=int, default=64)
a = ap.parse_args()
B, heads, hd, p, iters = a.B, a.heads, a.hd, a.p, a.iters
Lq, Lk = a.Lq or a.L, a.Lk or a.L
D = heads * hd
ld = (Lk + 7) // 8 * 8
g = torch.Generator(device="cuda").manual_seed(0)
q, do = (torch.randn(B * Lq, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2))
k, v = (torch.randn(B * Lk, D, device="cuda", generator=g).to(torch.bfloat16) for _ in range(2))
add = torch.zeros(B, Lk, device="cuda")
scale = hd ** -0.5
F32, BF16 = torch.float32, torch.bfloat16
def t(fn, n=iters):
    for _ in range(3): fn()
    torch.cuda.synchronize(); s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize(); return s.elapsed_time(e) / n * 1e3
sA = (heads * Lq * ld, Lq * ld)
def mat_fwd():
    S = torch.empty(B, heads, Lq, ld, device="cuda", dtype=F32)
    ops.gemm(q, k, M=Lq, N=Lk, K=hd, lda=D, ldb=D, out=S, ldc=ld, batch=(B, heads), sA=(Lq * D, hd), sB=(Lk * D, hd), sC=sA, alpha=scale)
    P, Pd = ops.softmax_fwd(S, add, B, heads, Lq, Lk, ld, p, 1, 1)
    ctx = torch.empty(B * Lq, D, device="cuda", dtype=ops.act16())
    ops.gemm(Pd, v, M=Lq, N=hd, K=Lk, lda=ld, ldb=D, transB=True, out=ctx, ldc=D, batch=(B, heads), sA=sA, sB=(Lk * D, hd), sC=(Lq * D, hd))
    return P, Pd
def mat_bwd(P, Pd):
    dP = torch.empty(B, heads, Lq, ld, device="cuda", dtype=F32)
    ops.gemm(do, v, M=Lq, N=Lk, K=hd, lda=D, ldb=D, out=dP, ldc=ld, batch=(B, heads), sA=(Lq * D, hd), sB=(Lk * D, hd), sC=sA)
    dv = torch.empty(B * Lk, D, device="cuda", dtype=BF16)
    ops.gemm(Pd, do, M=Lk, N=hd, K=Lq, lda=ld, ldb=D, transA=True, transB=True, out=dv, ldc=D, batch=(B, heads), sA=sA, sB=(Lq * D, hd), sC=(Lk * D, hd))
    dS = ops.softmax_bwd(P, dP, B, heads, Lq, Lk, ld, scale, p, 1, 1)
    dq = torch.empty(B * Lq, D, device="cuda", dtype=BF16)
    ops.gemm(dS, k, M=Lq, N=hd, K=Lk, lda=ld, ldb=D, transB=True, out=dq, ldc=D, batch=(B, heads), sA=sA, sB=(Lk * D, hd), sC=(Lq * D, hd))
    dk = torch.empty(B * Lk, D, device="cuda", dtype=BF16)
    ops.gemm(dS, q, M=Lk, N=hd, K=Lq, lda=ld, ldb=D, transA=True, transB=True, out=dk, ldc=D, batch=(B, heads), sA=sA, sB=(Lq * D, hd), sC=(Lk * D, hd))
fl = 4.0 * Lq * Lk * hd * B * heads
line = f"B={B} heads={heads}x{hd} Lq={Lq} Lk={Lk} p={p}:"
if ops.attn_eligible(Lq, Lk, hd, D):
    fwd, bwd = ops.attn_dispatch(Lq, Lk)
    ctx, stats = fwd(q, k, v, add, B, heads, Lq, Lk, scale, p, 1, 1)
    tf = [t(lambda: fwd(q, k, v, add, B, heads, Lq, Lk, scale, p, 1, 1)) for _ in range(3)]
    tb = [t(lambda: bwd(q, k, v, add, do, stats, B, heads, Lq, Lk, scale, p, 1, 1)) for _ in range(3)]
    line += (f" fused[{fwd.__name__}] fwd {min(tf):.1f}-{max(tf):.1f} us ({fl / min(tf) / 1e6:.0f} TF/s) bwd {min(tb):.1f}-{max(tb):.1f} us"
             f" ({2.5 * fl / min(tb) / 1e6:.0f} TF/s);")
P, Pd = mat_fwd()
mf = [t(mat_fwd) for _ in range(3)]
mb = [t(lambda: mat_bwd(P, Pd)) for _ in range(3)]
print(line + f" materialised fwd {min(mf):.1f}-{max(mf):.1f} us bwd {min(mb):.1f}-{max(mb):.1f} us   (min-max of 3 x {iters} launches)")
