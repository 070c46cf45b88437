"""GPU parity tests, kernel level: every C-ABI entry point vs the CPU oracle / golden vectors.

Tolerances: integer outputs bit-exact; fp32-math kernels 1e-5..1e-4 relative; kernels that store bf16 are compared
against the oracle evaluated on the SAME bf16-rounded operands (accumulation-order tolerance), so a layout or
indexing bug cannot hide behind bf16 noise.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mmdti_hip import ops as _ops
    return _ops


def dev(t):
    return t.cuda()


def bf(t):
    return t.to(torch.bfloat16)


def rt(t):
    """bf16 round trip on the CPU."""
    return t.to(torch.bfloat16).to(torch.float32)


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().float().cpu(), b.detach().float().cpu(), rtol=rtol, atol=atol)


G = lambda s: torch.Generator().manual_seed(s)


# ------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (130, 50, 72), (300, 200, 512), (33, 1536, 512), (1000, 64, 128)])
def test_gemm_nt(ops, M, N, K):
    x, w, b = rt(torch.randn(M, K, generator=G(1))), rt(torch.randn(N, K, generator=G(2)) * 0.1), torch.randn(N, generator=G(3))
    y = ops.linear_fwd(dev(bf(x)), dev(bf(w)), dev(b), out_dtype=torch.float32)
    close(y, x @ w.T + b, 1e-4, 1e-4)
    yb = ops.linear_fwd(dev(bf(x)), dev(bf(w)), dev(b), out_dtype=torch.bfloat16)
    close(yb, rt(x @ w.T + b), 1e-2, 1e-2)


def test_gemm_epilogues(ops):
    M, N, K = 200, 192, 128
    x, w, b = rt(torch.randn(M, K, generator=G(1))), rt(torch.randn(N, K, generator=G(2)) * 0.1), torch.randn(N, generator=G(3))
    res = torch.randn(M, N, generator=G(4))
    u_ref = x @ w.T + b
    aux = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
    y = ops.linear_fwd(dev(bf(x)), dev(bf(w)), dev(b), act=ops.ACT_GELU, aux_out=aux, out_dtype=torch.float32)
    close(y, O.gelu(u_ref), 1e-4, 1e-4)
    close(aux, rt(u_ref), 1e-2, 1e-2)
    y = ops.linear_fwd(dev(bf(x)), dev(bf(w)), dev(b), residual=dev(res), out_dtype=torch.float32)
    close(y, u_ref + res, 1e-4, 1e-4)
    # gelu backward epilogue: dx = (dy . W) * gelu'(u)
    dy = rt(torch.randn(M, N, generator=G(5)))
    u = rt(torch.randn(M, K, generator=G(6)))
    dx = ops.linear_bwd_input(dev(bf(dy)), dev(bf(w)), act=ops.ACT_GELU_BWD, aux_in=dev(bf(u)), out_dtype=torch.float32)
    uu = u.clone().requires_grad_()
    (gr,) = torch.autograd.grad(O.gelu(uu).sum(), uu)
    close(dx, (dy @ w) * gr, 1e-4, 1e-4)


def test_gemm_transposed_and_splitk(ops):
    M, N, K = 777, 192, 160   # dW[N,K] = dy[M,N]^T x[M,K]
    dy, x = rt(torch.randn(M, N, generator=G(1))), rt(torch.randn(M, K, generator=G(2)))
    dw = torch.zeros(N, K, device="cuda")
    ops.linear_bwd_weight(dev(bf(dy)), dev(bf(x)), dw)
    close(dw, dy.T @ x, 1e-4, 2e-3)
    ops.linear_bwd_weight(dev(bf(dy)), dev(bf(x)), dw)          # accumulates
    close(dw, 2 * (dy.T @ x), 1e-4, 4e-3)
    w = rt(torch.randn(N, K, generator=G(3)))
    dx = ops.linear_bwd_input(dev(bf(dy)), dev(bf(w)), out_dtype=torch.float32)
    close(dx, dy @ w, 1e-4, 2e-3)


def test_gemm_batched_heads(ops):
    # S[b,h] = q[b,:,h,:] . k[b,:,h,:]^T from a packed [B,L,3D] buffer, K-tail (Lk=13 not a multiple of 8) on P.V
    B, L, H, hd = 3, 13, 4, 32
    D = H * hd
    qkv = rt(torch.randn(B, L, 3 * D, generator=G(1)))
    dq = dev(bf(qkv))
    ld = 16
    S = torch.zeros(B, H, L, ld, device="cuda")
    ops.gemm(dq, dq[:, :, D:], M=L, N=L, K=hd, lda=3 * D, ldb=3 * D, out=S, ldc=ld, batch=(B, H), sA=(L * 3 * D, hd),
             sB=(L * 3 * D, hd), sC=(H * L * ld, L * ld), alpha=0.5)
    q = qkv[..., :D].view(B, L, H, hd).transpose(1, 2)
    k = qkv[..., D:2 * D].view(B, L, H, hd).transpose(1, 2)
    v = qkv[..., 2 * D:].view(B, L, H, hd).transpose(1, 2)
    close(S[..., :L], 0.5 * q @ k.transpose(-1, -2), 1e-4, 1e-3)
    P = torch.zeros(B, H, L, ld)
    P[..., :L] = torch.softmax(torch.randn(B, H, L, L, generator=G(2)), -1)
    P = rt(P)
    ctx = torch.empty(B, L, D, device="cuda", dtype=torch.bfloat16)
    ops.gemm(dev(bf(P)), dq[:, :, 2 * D:], M=L, N=hd, K=L, lda=ld, ldb=3 * D, transB=True, out=ctx, ldc=D, batch=(B, H),
             sA=(H * L * ld, L * ld), sB=(L * 3 * D, hd), sC=(L * D, hd))
    ref = (P[..., :L] @ v).transpose(1, 2).reshape(B, L, D)
    close(ctx, ref, 1e-2, 1e-2)


def test_gemm_dropout_epilogue(ops):
    M, N, K = 256, 256, 64
    x, w = torch.ones(M, K), torch.ones(N, K) / K
    y1 = ops.linear_fwd(dev(bf(x)), dev(bf(w)), None, out_dtype=torch.float32, drop_p=0.25, seed=7, site=3)
    y2 = ops.linear_fwd(dev(bf(x)), dev(bf(w)), None, out_dtype=torch.float32, drop_p=0.25, seed=7, site=3)
    assert torch.equal(y1, y2)                                   # counter-based: reproducible
    keep = (y1 != 0).float().mean().item()
    assert abs(keep - 0.75) < 0.01
    close(y1[y1 != 0], torch.full_like(y1[y1 != 0], 1 / 0.75), 1e-5, 1e-5)
    y3 = ops.linear_fwd(dev(bf(x)), dev(bf(w)), None, out_dtype=torch.float32, drop_p=0.25, seed=8, site=3)
    assert not torch.equal(y1, y3)


def test_gemm_rejects_bad_arguments(ops):
    from mmdti_hip._abi import MMDTIError
    x = torch.zeros(16, 12, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(MMDTIError):
        ops.gemm(x, x, M=16, N=16, K=12, lda=12, ldb=12)          # lda not a multiple of 8


# ------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,D,eps", [(37, 512, 1e-5), (260, 64, 1e-12), (5, 2048, 1e-5)])
def test_layernorm(ops, rows, D, eps):
    x = torch.randn(rows, D, generator=G(1)) * 2 + 0.5
    g, b = 1 + 0.1 * torch.randn(D, generator=G(2)), 0.1 * torch.randn(D, generator=G(3))
    rz = torch.zeros(rows, dtype=torch.bool); rz[::5] = True
    y32, y16, mean, rstd = ops.layernorm_fwd(dev(x), dev(g), dev(b), eps, want_f32=True, want_bf16=True, row_zero=dev(rz))
    ref = O.layer_norm(x, g, b, eps) * (~rz).unsqueeze(-1)
    close(y32, ref, 1e-5, 1e-5)
    close(y16, rt(ref), 1e-2, 1e-2)
    # backward (fp32 dy and bf16 dy), with residual-gradient add
    xr = x.clone().requires_grad_(); gr = g.clone().requires_grad_(); br = b.clone().requires_grad_()
    dy = torch.randn(rows, D, generator=G(4)); dres = torch.randn(rows, D, generator=G(5))
    out = O.layer_norm(xr, gr, br, eps) * (~rz).unsqueeze(-1)
    (out * dy).sum().backward()
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    dx = ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, dg, db, dres=dev(dres), row_zero=dev(rz))
    close(dx, xr.grad + dres, 1e-4, 1e-4)
    close(dg, gr.grad, 1e-4, 1e-3)
    close(db, br.grad, 1e-4, 1e-3)
    dg.zero_(); db.zero_()
    dx = ops.layernorm_bwd(dev(bf(dy)), dev(x), dev(g), mean, rstd, dg, db, row_zero=dev(rz))
    xr.grad = None
    (O.layer_norm(xr, g, b, eps) * (~rz).unsqueeze(-1) * rt(dy)).sum().backward()
    close(dx, xr.grad, 1e-4, 1e-4)


def test_layernorm_dropout_consistency(ops):
    rows, D = 64, 512
    x = torch.randn(rows, D, generator=G(1)); g = torch.ones(D); b = torch.zeros(D)
    y32, _, mean, rstd = ops.layernorm_fwd(dev(x), dev(g), dev(b), 1e-5, want_f32=True, want_bf16=False, drop_p=0.1, seed=5, site=1)
    ref = O.layer_norm(x, g, b, 1e-5)
    mask = (y32 != 0).cpu()
    assert abs(mask.float().mean().item() - 0.9) < 0.01
    close(y32.cpu()[mask], (ref / 0.9)[mask], 1e-5, 1e-5)
    # backward regenerates the same mask: dx of a masked-out element's dy contribution is zero
    dy = torch.ones(rows, D)
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, dg, db, drop_p=0.1, seed=5, site=1)
    close(db, (mask.float() / 0.9).sum(0), 1e-5, 1e-4)


def test_layernorm_bwd_fused_bf16_copy(ops):
    """The optional second output equals the separate cast kernel applied to dx (same dropout site): bit-exact."""
    rows, D = 70, 512
    x = torch.randn(rows, D, generator=G(1)); g = torch.randn(D, generator=G(2)); dy = torch.randn(rows, D, generator=G(3))
    _, _, mean, rstd = ops.layernorm_fwd(dev(x), dev(g), dev(torch.zeros(D)), 1e-5, want_f32=True, want_bf16=False)
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    for p in (0.0, 0.1):
        dx, dx16 = ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, dg, db, bf16_copy=(p, 7), seed=11)
        ref = ops.cast_bf16(dx, p, 11, 7)
        assert torch.equal(dx16, ref)
        assert torch.equal(dx, ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, dg, db))
        # and its column sums (the next Linear's bias gradient) == the separate column-sum pass over the same bf16 tensor
        cs = torch.full((D,), 0.5, device="cuda")
        _, dx16b = ops.layernorm_bwd(dev(dy), dev(x), dev(g), mean, rstd, dg, db, bf16_copy=(p, 7, cs), seed=11)
        want = ops.colsum(dx16, torch.full((D,), 0.5, device="cuda"))
        assert torch.equal(dx16b, dx16)
        close(cs, want, 1e-5, 1e-4)


# ------------------------------------------------------------------------------------------- pair attention
def _pair_ref(qkv, bias, key_pad, H, scale, dO=None, g_in=None):
    """oracle core of unimol_layer's attention on given (bf16-rounded) qkv.  Returns S,O and grads."""
    B, N, D3 = qkv.shape
    D = D3 // 3
    hd = D // H
    qkv = qkv.clone().requires_grad_()
    bias = bias.clone().requires_grad_()
    q, k, v = qkv.chunk(3, -1)
    heads = lambda t: t.view(B, N, H, hd).transpose(1, 2)
    b = bias
    if key_pad is not None:
        b = b.masked_fill(key_pad.view(B, 1, 1, N), float("-inf"))
    S = (heads(q) * scale) @ heads(k).transpose(-1, -2) + b
    P = torch.softmax(S, -1)
    Oo = (P @ heads(v)).transpose(1, 2).reshape(B, N, D)
    if dO is None:
        return S, Oo
    loss = (Oo * dO).sum()
    if g_in is not None:
        fin = torch.isfinite(S)
        loss = loss + (torch.where(fin, S, torch.zeros_like(S)) * g_in).sum()
    loss.backward()
    return S, Oo, qkv.grad, bias.grad


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("B,N,H", [(2, 7, 8), (3, 70, 4), (2, 130, 64), (1, 200, 2), (1, 210, 64), (2, 240, 8), (1, 258, 64), (1, 272, 4)])
def test_pair_attn(ops, B, N, H, tiled):
    """Both pair layouts: row-major [B,H,N,ld] planes and the tiled [B,H,nt,nt,256] form the hot path streams.
    N in 209..258 is what the reference's crop at max_atoms=256 can produce (data/conformer.py:53,199-204): the NT=17
    instantiation of the MFMA kernels; 272 is its last supported size."""
    D = H * 8
    ld = ops.pair_ld(N)
    scale = 8 ** -0.5
    up = (lambda t, pad=float("-inf"): ops.pair_tile(dev(t), N, pad)) if tiled else (lambda t, pad=None: dev(t))   # host standard -> device layout
    down = (lambda t: ops.pair_untile(t, N).cpu()) if tiled else (lambda t: t.cpu()[..., :N])
    qkv = rt(torch.randn(B, N, 3 * D, generator=G(1)))
    bias = torch.randn(B, H, N, N, generator=G(2))
    key_pad = torch.zeros(B, N, dtype=torch.bool)
    key_pad[0, N - max(1, N // 3):] = True
    bias_ld = torch.zeros(B, H, N, ld); bias_ld[..., :N] = bias
    s_out, o = ops.pair_attn_fwd(dev(bf(qkv)).view(B * N, 3 * D), up(bias_ld), dev(key_pad), B, N, H, ld, scale)
    assert ops.pair_is_tiled(s_out) == tiled
    dO = rt(torch.randn(B, N, D, generator=G(3)))
    g_in = torch.randn(B, H, N, N, generator=G(4)).masked_fill(key_pad.view(B, 1, 1, N), 0.0)   # G is 0 at -inf entries
    S, Oref, dqkv_ref, dbias_ref = _pair_ref(qkv, bias, key_pad, H, scale, dO, g_in)
    s_cpu = down(s_out)
    assert torch.equal(torch.isinf(s_cpu), torch.isinf(S.detach()))        # masked columns are exactly -inf
    fin = torch.isfinite(S.detach())
    close(s_cpu[fin], S.detach()[fin], 1e-5, 1e-5)
    close(o.view(B, N, D), rt(Oref), 1e-2, 1e-2)
    g = torch.zeros(B, H, N, ld); g[..., :N] = g_in
    g = up(g, 0.0)
    dqkv = ops.pair_attn_bwd(dev(bf(qkv)).view(B * N, 3 * D), s_out, dev(bf(dO)).view(B * N, D), g, B, N, H, ld, scale, False)
    close(down(g)[fin], (dbias_ref + 0)[fin], 1e-4, 1e-4)
    close(dqkv.view(B, N, 3 * D), rt(dqkv_ref), 2e-2, 2e-2)
    # g_in_zero path == g_in of zeros
    g2 = up(torch.full((B, H, N, ld), 7.0), 0.0)
    dq2 = ops.pair_attn_bwd(dev(bf(qkv)).view(B * N, 3 * D), s_out, dev(bf(dO)).view(B * N, D), g2, B, N, H, ld, scale, True)
    _, _, dqkv0, dbias0 = _pair_ref(qkv, bias, key_pad, H, scale, dO, None)
    close(down(g2)[fin], dbias0[fin], 1e-4, 1e-4)
    close(dq2.view(B, N, 3 * D), rt(dqkv0), 2e-2, 2e-2)
    # no padding mask at all: the structural pads (keys / queries >= N) must take care of themselves in both layouts
    s_np, o_np = ops.pair_attn_fwd(dev(bf(qkv)).view(B * N, 3 * D), up(bias_ld), None, B, N, H, ld, scale)
    qkv_n = qkv.clone()
    S_np, O_np, dqkv_np, dbias_np = _pair_ref(qkv_n, bias.clone(), None, H, scale, dO, None)
    close(down(s_np), S_np.detach(), 1e-5, 1e-5)
    close(o_np.view(B, N, D), rt(O_np), 1e-2, 1e-2)
    g3 = up(torch.full((B, H, N, ld), 3.0), 0.0)
    dq3 = ops.pair_attn_bwd(dev(bf(qkv)).view(B * N, 3 * D), s_np, dev(bf(dO)).view(B * N, D), g3, B, N, H, ld, scale, True)
    close(down(g3), dbias_np, 1e-4, 1e-4)
    close(dq3.view(B, N, 3 * D), rt(dqkv_np), 2e-2, 2e-2)
    if tiled:   # pads of a tiled S stay -inf, pads of a tiled G stay 0 (what the next layer's unpredicated loads rely on):
        # the only pad slots of the blocked-row planes are the keys N .. N4-1 of a real query (+ the alignment tail of a plane)
        s_pads = s_np.reshape(B, H, -1).clone(); g_pads = g3.reshape(B, H, -1).clone()
        idx = ops._tile_index(N, s_np.device).reshape(-1)
        s_pads[:, :, idx] = float("-inf"); g_pads[:, :, idx] = 0.0
        used = N * ops.pair_ld(N)
        assert torch.isinf(s_pads[:, :, :used]).all() and (s_pads[:, :, :used] < 0).all()
        assert (g_pads[:, :, :used] == 0).all()
    if tiled:   # the two layouts run the same arithmetic: identical bits
        s_std, o_std = ops.pair_attn_fwd(dev(bf(qkv)).view(B * N, 3 * D), dev(bias_ld), dev(key_pad), B, N, H, ld, scale)
        assert torch.equal(o_std, o) and torch.equal(s_std.cpu()[..., :N], s_cpu)


def test_pair_tile_roundtrip(ops):
    N = 37
    x = torch.randn(2, 3, N, N, generator=G(1))
    t = ops.pair_tile(dev(x), N)
    assert t.shape == (2, 3, ops.pair_plane(N)) and ops.pair_plane(N) == 37 * 40 and torch.equal(ops.pair_untile(t, N).cpu(), x)
    # blocked rows: element (q, k) at 16 (q//16) N4 + vr (k - k%4) + 4 (q%16) + k%4, vr = rows of the query block (16, or N - 16 qb)
    assert t[1, 2, 16 * 40 + 16 * 32 + 4 * (20 % 16) + 35 % 4].item() == x[1, 2, 20, 35].item()
    assert t[1, 2, 32 * 40 + 5 * 32 + 4 * (36 % 16) + 35 % 4].item() == x[1, 2, 36, 35].item()       # (the last block holds 5 queries)
    # a complete 16x16 tile is 256 contiguous elements in MFMA accumulator order: ((k%16)//4*16 + q%16)*4 + k%4
    tile = t[0, 1, 16 * 40 + 256:16 * 40 + 512]
    assert tile[((22 % 16) // 4 * 16 + 27 % 16) * 4 + 22 % 4].item() == x[0, 1, 27, 22].item()


@pytest.mark.parametrize("B,N,H,p", [(2, 7, 8, 0.0), (3, 70, 4, 0.0), (2, 130, 64, 0.1), (1, 210, 64, 0.0), (2, 240, 8, 0.1), (1, 258, 64, 0.0), (1, 272, 4, 0.0)])
def test_pair_attn_compact_planes_are_the_fp32_kernels_plus_rounding(ops, B, N, H, p):
    """COMPACT tiled planes (layout 3: logits chain fp16, gradient chain fp32 -- the hot path; layout 7: gradient chain bf16,
    opt-in) against the fp32 tiled kernels, which the test above pins to autograd.  The relations are exact, bit for bit:
      forward   S16 = fp16_rne(S32) when both start from the same fp16 bias;  O16 = the fp32 kernel's O when that is handed
                the ROUNDED logits (q = 0, bias = S16): the layer's own softmax runs on what is stored;
      backward  (S16, G fp32) -> dqkv and G identical to the fp32 kernel on S16 widened to fp32;
                (S16, G bf16) -> dqkv identical too -- the products use the unrounded G of the layer -- and G_out = bf16_rne(G_out32)."""
    D, ld, scale = H * 8, ops.pair_ld(N), 8 ** -0.5
    kw = dict(drop_p=p, seed=11, site=2)
    qkv = dev(bf(torch.randn(B, N, 3 * D, generator=G(1)))).view(B * N, 3 * D)
    dO = dev(bf(torch.randn(B, N, D, generator=G(3)))).view(B * N, D)
    key_pad = torch.zeros(B, N, dtype=torch.bool)
    key_pad[0, N - max(1, N // 3):] = True
    bias = torch.zeros(B, H, N, ld); bias[..., :N] = 3.0 * torch.randn(B, H, N, N, generator=G(2))
    b16 = ops.pair_tile(dev(bias), N, float("-inf")).half()
    b32 = b16.float()
    s16, o16 = ops.pair_attn_fwd(qkv, b16, dev(key_pad), B, N, H, ld, scale, **kw)
    s32, o32 = ops.pair_attn_fwd(qkv, b32, dev(key_pad), B, N, H, ld, scale, **kw)
    assert s16.dtype == torch.float16 and ops.pair_is_tiled(s16) and s32.dtype == torch.float32
    un = lambda t: ops.pair_untile(t, N)                                           # (slots with q >= N or k >= N are never read)
    assert torch.equal(un(s16), un(s32).half())
    assert float((un(s16).float() - un(s32))[torch.isfinite(un(s32))].abs().max()) > 0       # ... and the rounding is really there
    q0 = qkv.clone(); q0[:, :D] = 0
    _, o_chk = ops.pair_attn_fwd(q0, s16.float(), None, B, N, H, ld, scale, **kw)
    assert torch.equal(o16, o_chk)
    close(o16.float().cpu(), o32.float().cpu(), 3e-2, 3e-2)                                   # (and close to the unrounded layer)
    # a second layer on top: reads fp16, writes fp16
    s16b, o16b = ops.pair_attn_fwd(qkv, s16, None, B, N, H, ld, scale, **kw)
    s32b, _ = ops.pair_attn_fwd(qkv, s16.float(), None, B, N, H, ld, scale, **kw)
    assert torch.equal(un(s16b), un(s32b).half())
    # backward
    g_in = torch.zeros(B, H, N, ld); g_in[..., :N] = torch.randn(B, H, N, N, generator=G(4)).masked_fill(key_pad.view(B, 1, 1, N), 0.0)
    g16 = ops.pair_tile(dev(g_in), N, 0.0).bfloat16()
    g32 = g16.float(); g32c = g32.clone()
    dq16 = ops.pair_attn_bwd(qkv, s16, dO, g16, B, N, H, ld, scale, False, **kw)
    dq32 = ops.pair_attn_bwd(qkv, s16.float(), dO, g32, B, N, H, ld, scale, False, **kw)
    dq32c = ops.pair_attn_bwd(qkv, s16, dO, g32c, B, N, H, ld, scale, False, **kw)            # the default pairing: fp16 logits, fp32 gradients
    assert torch.equal(dq32c, dq32) and torch.equal(un(g32c), un(g32))
    assert g16.dtype == torch.bfloat16 and torch.equal(dq16, dq32)
    assert torch.equal(un(g16), un(g32).bfloat16())
    gz16 = torch.full_like(g16, 7.0); gz32 = torch.full_like(g32, 7.0)
    dqz16 = ops.pair_attn_bwd(qkv, s16, dO, gz16, B, N, H, ld, scale, True, **kw)
    dqz32 = ops.pair_attn_bwd(qkv, s16.float(), dO, gz32, B, N, H, ld, scale, True, **kw)
    assert torch.equal(dqz16, dqz32) and torch.equal(un(gz16), un(gz32).bfloat16())
    # saturation instead of +inf: logits beyond the fp16 range stay finite
    big = b16.clone(); big[0, 0, :4] = 65504.0
    qbig = (qkv.float() * 16).bfloat16()
    sbig, obig = ops.pair_attn_fwd(qbig, big, None, B, N, H, ld, scale)
    assert not torch.isnan(obig.float()).any() and not torch.isposinf(un(sbig).float()).any()
    # mismatched element types are refused
    with pytest.raises(ops.MMDTIError):
        ops.pair_attn_bwd(qkv, s32, dO, g16, B, N, H, ld, scale, False)            # bf16 gradients only go with fp16 logits
    with pytest.raises(ops.MMDTIError):
        ops.pair_attn_fwd(qkv, dev(bias).half(), None, B, N, H, ld, scale)         # fp16 row-major planes do not exist


@pytest.mark.parametrize("B,N,H,lens,p", [(4, 130, 8, (130, 37, 64, 5), 0.0), (3, 100, 64, (100, 17, 81), 0.1), (2, 258, 8, (40, 258), 0.0), (2, 16, 8, (3, 16), 0.0),
                                          (5, 200, 4, (200, 33, 90, 150, 177), 0.1), (4, 240, 8, (10, 70, 130, 240), 0.0)])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_pair_attn_ragged_key_tile_skipping_equals_dense(ops, B, N, H, lens, p, gdt):
    """Ragged batches (compact tiled planes): with key_tiles = ceil(length / 16) per molecule the kernels neither load, compute
    nor store the all-padding key tiles.  Everything that is defined must equal the dense run bit for bit: O, dqkv, S and G on
    the kept tiles; rag_store writes -inf into the skipped S tiles (the dense run has -inf there too); skipped G tiles stay as
    handed in (zero).  Pad QUERY rows are computed in both."""
    D, ld, scale = H * 8, ops.pair_ld(N), 8 ** -0.5
    nt = ops.pair_tiles(N)
    qkv = dev(bf(torch.randn(B, N, 3 * D, generator=G(1)))).view(B * N, 3 * D)
    dO = dev(bf(torch.randn(B, N, D, generator=G(3)))).view(B * N, D)
    key_pad = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(lens):
        key_pad[b, n:] = True
    bias = torch.zeros(B, H, N, ld); bias[..., :N] = torch.randn(B, H, N, N, generator=G(2))
    bias_t = ops.pair_tile(dev(bias), N, float("-inf")).half()
    kt = torch.tensor([(n + 15) // 16 for n in lens], dtype=torch.int32, device="cuda")
    ke = [ops.pair_key_tiles_effective(int(k), nt) for k in kt]                # tiles the kernels cover (>= kt: see ops.pair_key_tiles_effective)
    assert all(int(a) <= b <= nt for a, b in zip(kt, ke))
    kw = dict(drop_p=p, seed=5, site=3)

    def rows(t):                                                                # -> [B,H,nt,N,16]: the N x N block by key tile (slots with q >= N or k >= N are never written or read)
        u = torch.zeros(B, H, N, nt * 16, device=t.device)
        u[..., :N] = ops.pair_untile(t, N).float()
        return u.view(B, H, N, nt, 16).transpose(2, 3)

    s_d, o_d = ops.pair_attn_fwd(qkv, bias_t, dev(key_pad), B, N, H, ld, scale, **kw)
    s_r, o_r = ops.pair_attn_fwd(qkv, bias_t, dev(key_pad), B, N, H, ld, scale, key_tiles=kt, rag_store=True, **kw)
    assert s_r.dtype == torch.float16
    assert torch.equal(o_r, o_d) and torch.equal(rows(s_r), rows(s_d))          # (skipped tiles: -inf in both)
    s_n, o_n = ops.pair_attn_fwd(qkv, bias_t, dev(key_pad), B, N, H, ld, scale, key_tiles=kt, rag_store=False, **kw)
    assert torch.equal(o_n, o_d)
    for b in range(B):
        k = ke[b]
        assert torch.equal(rows(s_n)[b, :, :k], rows(s_d)[b, :, :k])
    # second layer on top of the not-stored S: the skipped tiles are never read
    s2_d, o2_d = ops.pair_attn_fwd(qkv, s_d, None, B, N, H, ld, scale, **kw)
    s_poison = s_n.clone()
    for b in range(B):
        s_poison[b][:, ops.pair_slots(N, "cuda", k_lo=16 * ke[b])] = float("nan")
    s2_r, o2_r = ops.pair_attn_fwd(qkv, s_poison, None, B, N, H, ld, scale, key_tiles=kt, rag_store=True, **kw)
    assert torch.equal(o2_r, o2_d) and torch.equal(rows(s2_r), rows(s2_d))
    # backward
    g_in = torch.zeros(B, H, N, ld); g_in[..., :N] = torch.randn(B, H, N, N, generator=G(4)).masked_fill(key_pad.view(B, 1, 1, N), 0.0)
    g_0 = ops.pair_tile(dev(g_in), N, 0.0).to(gdt)      # the gradient chain in fp32 (layout 3) or bf16 (layout 7): both have the ragged form
    g_d = g_0.clone(); g_r = g_0.clone()
    dq_d = ops.pair_attn_bwd(qkv, s_d, dO, g_d, B, N, H, ld, scale, False, **kw)
    dq_r = ops.pair_attn_bwd(qkv, s_poison, dO, g_r, B, N, H, ld, scale, False, key_tiles=kt, **kw)
    assert torch.equal(dq_r, dq_d)
    for b in range(B):
        k = ke[b]
        assert torch.equal(rows(g_r)[b, :, :k], rows(g_d)[b, :, :k])
        if k < nt:
            assert float(rows(g_d)[b, :, k:].abs().max()) == 0.0                # (what the dense run computes there is exactly 0 ...)
            assert torch.equal(rows(g_r)[b, :, k:], rows(g_0)[b, :, k:])        # (... and the ragged run leaves them untouched)
    gz = torch.zeros_like(g_d)
    dq_z = ops.pair_attn_bwd(qkv, s_poison, dO, gz, B, N, H, ld, scale, True, key_tiles=kt, **kw)
    gz_d = torch.full_like(g_d, 7.0)
    dq_zd = ops.pair_attn_bwd(qkv, s_d, dO, gz_d, B, N, H, ld, scale, True, **kw)
    assert torch.equal(dq_z, dq_zd)
    for b in range(B):
        assert torch.equal(rows(gz)[b, :, :ke[b]], rows(gz_d)[b, :, :ke[b]])
    with pytest.raises(ops.MMDTIError):                                         # the fp32 planes have no ragged form
        ops.pair_attn_fwd(qkv, bias_t.float(), dev(key_pad), B, N, H, ld, scale, key_tiles=kt)


def test_pair_attn_dropout(ops):
    B, N, H = 2, 64, 8
    D, ld, scale = H * 8, 64, 8 ** -0.5
    qkv = rt(torch.randn(B, N, 3 * D, generator=G(1)))
    qkv[..., 2 * D:] = 1.0                                   # v = 1  ->  O = sum_j dropout(P)_j
    bias = torch.zeros(B, H, N, ld)
    _, o = ops.pair_attn_fwd(dev(bf(qkv)).view(B * N, 3 * D), dev(bias), None, B, N, H, ld, scale, drop_p=0.5, seed=3, site=9)
    o = o.float().cpu()
    assert abs(o.mean().item() - 1.0) < 0.05 and o.std().item() > 0.05      # unbiased, actually random
    _, o2 = ops.pair_attn_fwd(dev(bf(qkv)).view(B * N, 3 * D), dev(bias), None, B, N, H, ld, scale, drop_p=0.5, seed=3, site=9)
    assert torch.equal(o2.float().cpu(), o)


def test_pair_attn_dropout_mask_statistics(ops):
    """The same generator in the pair-attention kernels (a key per (molecule, head) plane, counters from (query, key / 4)):
    masks recovered through indicator V columns (head_dim 8: eight keys per pass), 64 planes x 128 x 128 = 1 M decisions,
    judged by the battery of test_attn_dropout_mask_statistics (defined below)."""
    B, N, H, p_drop = 2, 128, 32, 0.1
    D, ld, scale = H * 8, 128, 8 ** -0.5
    bias = dev(torch.zeros(B, H, N, ld))
    pd = torch.zeros(B, H, N, N)
    for c0 in range(0, N, 8):
        qkv = torch.zeros(B, N, 3, H, 8)
        for d in range(8):
            qkv[:, c0 + d, 2, :, d] = 1.0
        _, o = ops.pair_attn_fwd(dev(bf(qkv.view(B * N, 3 * D))), bias, None, B, N, H, ld, scale, drop_p=p_drop, seed=77, site=5)
        pd[..., c0:c0 + 8] = o.view(B, N, H, 8).float().cpu().permute(0, 2, 1, 3)
    drop = (pd == 0).view(B * H, N, N)
    kept = pd[pd != 0]
    close(kept, torch.full_like(kept, 1.0 / N / (1 - p_drop)), 1e-2, 0)
    z = _mask_battery(drop, p_drop)
    assert abs(z["mean"]) < 3.0, z
    worst = max(z, key=lambda k: abs(z[k]))
    assert abs(z[worst]) < 4.5, (worst, z)


# ------------------------------------------------------------------------------------------- Gaussian basis, permutes
def _gbf_params(E, K, seed=0):
    g = G(seed)
    return {"gbf.means.weight": torch.rand(1, K, generator=g) * 3, "gbf.stds.weight": torch.rand(1, K, generator=g) * 3 - 0.3,
            "gbf.mul.weight": 1 + 0.1 * torch.randn(E, 1, generator=g), "gbf.bias.weight": 0.1 * torch.randn(E, 1, generator=g)}


@pytest.mark.parametrize("B,N,K,V", [(2, 9, 16, 7), (2, 33, 128, 31)])
def test_gbf_features(ops, B, N, K, V):
    E = V * V
    P = {k: v.requires_grad_() for k, v in _gbf_params(E, K).items()}
    dist = torch.rand(B, N, N, generator=G(1)) * 6
    et = torch.randint(0, E, (B, N, N), generator=G(2))
    ref = O.gaussian_layer(dist, et, P)
    args = [dev(P[k].detach().reshape(-1)) for k in ("gbf.mul.weight", "gbf.bias.weight", "gbf.means.weight", "gbf.stds.weight")]
    feat = ops.gbf_features_fwd(dev(dist), dev(et), *args)
    close(feat.view(B, N, N, K), rt(ref), 1e-2, 1e-3)
    df = rt(torch.randn(B, N, N, K, generator=G(3)))
    (ref * df).sum().backward()
    grads = [torch.zeros_like(a) for a in args]
    ops.gbf_features_bwd(dev(dist), dev(et), *args, dev(bf(df)).view(-1, K), *grads)
    for gr, k in zip(grads, ("gbf.mul.weight", "gbf.bias.weight", "gbf.means.weight", "gbf.stds.weight")):
        close(gr, P[k].grad.reshape(-1), 2e-3, 2e-3)


def test_pair_permute(ops):
    B, N, H = 2, 13, 8
    ld = ops.pair_ld(N)
    x = torch.randn(B, N, N, H, generator=G(1))
    out = ops.pair_permute_fwd(dev(x), B, N, H, ld)
    assert torch.equal(out.cpu()[..., :N], x.permute(0, 3, 1, 2).contiguous())       # pure data movement: bit-exact
    g = torch.randn(B, H, N, ld, generator=G(2))
    back = ops.pair_permute_bwd(dev(g), B, N, H, ld)
    assert torch.equal(back.float().cpu().view(B, N, N, H), rt(g[..., :N].permute(0, 2, 3, 1)))
    back_t = ops.pair_permute_bwd(ops.pair_tile(dev(g), N, 0.0), B, N, H, ld)                 # same gradient from the tiled layout
    assert torch.equal(back_t, back)


# ------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("B,h,Lq,Lk", [(2, 3, 5, 13), (2, 2, 70, 130), (1, 2, 9, 256)])
def test_softmax(ops, B, h, Lq, Lk):
    ld = (Lk + 7) // 8 * 8
    s = torch.randn(B, h, Lq, ld, generator=G(1)) * 3
    mask = torch.ones(B, Lk); mask[0, Lk // 2:] = 0
    add = (1 - mask) * -10000.0
    p, pd = ops.softmax_fwd(dev(s), dev(add), B, h, Lq, Lk, ld)
    ref = torch.softmax(s[..., :Lk] + add.view(B, 1, 1, Lk), -1)
    close(p.cpu()[..., :Lk], rt(ref), 1e-2, 1e-3)
    assert (p.cpu()[..., Lk:] == 0).all()
    dp = torch.randn(B, h, Lq, ld, generator=G(2))
    pr = p.float().cpu()[..., :Lk]
    ds_ref = 0.25 * pr * (dp[..., :Lk] - (dp[..., :Lk] * pr).sum(-1, keepdim=True))
    ds = ops.softmax_bwd(p, dev(dp), B, h, Lq, Lk, ld, 0.25)
    close(ds.cpu()[..., :Lk], rt(ds_ref), 1e-2, 1e-3)
    assert (ds.cpu()[..., Lk:] == 0).all()
    # roberta-style mask (dtype minimum) gives exact zeros too
    p2, _ = ops.softmax_fwd(dev(s), dev((1 - mask) * torch.finfo(torch.float32).min), B, h, Lq, Lk, ld)
    assert (p2.cpu()[0, :, :, Lk // 2:Lk] == 0).all()


# ------------------------------------------------------------------------------------------- embeddings / position ids
def test_embedding_and_position_ids(ops, golden):
    g = golden("g6_roberta_eager")
    ids = torch.from_numpy(g["input_ids"])
    pos = ops.roberta_position_ids(dev(ids), 1)
    assert torch.equal(pos.cpu(), torch.from_numpy(g["position_ids"]))          # int64, bit-exact
    big = torch.randint(0, 5, (7, 300), generator=G(1))
    assert torch.equal(ops.roberta_position_ids(dev(big), 1).cpu(), O.roberta_position_ids(big, 1))
    table = torch.randn(40, 32, generator=G(2))
    out = ops.embedding_fwd(dev(ids), dev(table))
    assert torch.equal(out.cpu(), table[ids])
    ops.embedding_fwd(dev(pos), dev(table), out=out, accumulate=True)
    close(out, table[ids] + table[pos.cpu()], 1e-6, 1e-6)
    dout = torch.randn(*ids.shape, 32, generator=G(3))
    dt = torch.zeros(40, 32, device="cuda")
    ops.embedding_bwd(dev(ids), dev(dout), dt, padding_idx=1)
    tr = table.clone().requires_grad_()
    (torch.nn.functional.embedding(ids, tr, padding_idx=1) * dout).sum().backward()
    close(dt, tr.grad, 1e-5, 1e-5)
    # same gradient as ONE one-hot MFMA GEMM (the path the modules use); dout passes through bf16 there
    dt2 = torch.zeros(40, 32, device="cuda")
    ops.embedding_bwd_gemm(dev(ids), dev(bf(dout)).view(-1, 32), dt2, padding_idx=1)
    tr.grad = None
    (torch.nn.functional.embedding(ids, tr, padding_idx=1) * rt(dout)).sum().backward()
    close(dt2, tr.grad, 1e-4, 1e-4)
    assert dt2[1].abs().max().item() == 0.0                                   # padding row receives nothing
    one = torch.zeros(1, 32, device="cuda")
    ops.embedding_bwd_gemm(dev(torch.zeros_like(ids)), dev(bf(dout)).view(-1, 32), one, padding_idx=-1)
    close(one, rt(dout).view(-1, 32).sum(0, keepdim=True), 1e-4, 1e-3)


def test_roberta_embedding_sum_in_one_pass(ops):
    """word + position + token-type embeddings (HF RobertaEmbeddings.forward) as ONE gather-add kernel == three nn.Embedding
    lookups summed in the reference's order; out-of-range ids clamp like the single-table kernel."""
    gen = G(3)
    Vw, Vp, D, B, L = 600, 258, 512, 5, 37
    word, pos_t, typ = torch.randn(Vw, D, generator=gen), torch.randn(Vp, D, generator=gen), torch.randn(1, D, generator=gen)
    ids, pos = torch.randint(0, Vw, (B, L), generator=gen), torch.randint(0, Vp, (B, L), generator=gen)
    out = ops.embedding_fwd3(dev(ids), dev(word), dev(pos), dev(pos_t), dev(typ))
    ref = (word[ids] + pos_t[pos]) + typ[0]
    assert torch.equal(out.cpu(), ref)
    one = ops.embedding_fwd(dev(ids), dev(word)); ops.embedding_fwd(dev(pos), dev(pos_t), out=one, accumulate=True)
    ops.embedding_fwd(dev(torch.zeros_like(ids)), dev(typ), out=one, accumulate=True)
    assert torch.equal(out, one)


# ------------------------------------------------------------------------------------------- InfoNCE (golden G1)
@pytest.mark.parametrize("B", [2, 16])
def test_infonce_golden(ops, golden, B):
    g = golden(f"g1_info_nce_B{B}")
    q, k = dev(torch.from_numpy(g["q"])), dev(torch.from_numpy(g["k"]))
    qh, qi = ops.l2norm_fwd(q)
    kh, ki = ops.l2norm_fwd(k)
    loss = torch.zeros(1, device="cuda")
    dqh, dkh = torch.zeros_like(qh), torch.zeros_like(kh)
    ops.infonce_dir(qh, kh, 0, B, 0.1, loss, dqh, dkh)
    ops.infonce_dir(kh, qh, 0, B, 0.1, loss, dkh, dqh)
    close(loss / (2 * B), torch.from_numpy(g["loss"]).reshape(1), 1e-5, 1e-6)
    close(ops.l2norm_bwd(dqh, qh, qi), torch.from_numpy(g["dq"]), 1e-4, 1e-6)
    close(ops.l2norm_bwd(dkh, kh, ki), torch.from_numpy(g["dk"]), 1e-4, 1e-6)


def test_infonce_sharded_rows_equal_full(ops):
    """global negatives: two 'ranks' each owning half of the anchors reproduce the single-process loss + grads."""
    B, D = 24, 50
    q, k = torch.randn(B, D, generator=G(1)), torch.randn(B, D, generator=G(2))
    qh, _ = ops.l2norm_fwd(dev(q)); kh, _ = ops.l2norm_fwd(dev(k))
    full = [torch.zeros(1, device="cuda"), torch.zeros_like(qh), torch.zeros_like(kh)]
    ops.infonce_dir(qh, kh, 0, B, 0.1, *full); ops.infonce_dir(kh, qh, 0, B, 0.1, full[0], full[2], full[1])
    part = [torch.zeros(1, device="cuda"), torch.zeros_like(qh), torch.zeros_like(kh)]
    for r0 in (0, 12):
        ops.infonce_dir(qh, kh, r0, 12, 0.1, *part); ops.infonce_dir(kh, qh, r0, 12, 0.1, part[0], part[2], part[1])
    for a, b in zip(full, part):
        close(a, b, 1e-5, 1e-6)
    qr, kr = q.clone().requires_grad_(), k.clone().requires_grad_()
    ref = O.info_nce(qr, kr)
    close(full[0] / (2 * B), ref.reshape(1), 1e-5, 1e-6)


@pytest.mark.parametrize("Bg,Bl,row0,D", [(300, 300, 0, 50), (2048, 256, 512, 50), (77, 30, 40, 64), (40, 40, 0, 96)])
def test_infonce_matrix_pipe_kernels_vs_autograd(ops, Bg, Bl, row0, D):
    """The similarity matrix and both gradient products on fp32 MFMAs (feature width <= 64; 96 takes the scalar kernels): one
    direction of the symmetric CE for the anchors [row0, row0 + Bl) of a (global) batch of Bg -- ragged tile counts, the 8-GPU
    global batch -- against fp32 autograd of the same expression."""
    q = torch.nn.functional.normalize(torch.randn(Bg, D, generator=G(5)), dim=-1)
    k = torch.nn.functional.normalize(torch.randn(Bg, D, generator=G(6)), dim=-1)
    qr, kr = q.clone().requires_grad_(), k.clone().requires_grad_()
    logits = qr[row0:row0 + Bl] @ kr.t() / 0.1
    ce = torch.nn.functional.cross_entropy(logits, torch.arange(row0, row0 + Bl), reduction="sum")
    (ce / (2 * Bg)).backward()
    loss = torch.zeros(1, device="cuda")
    dq, dk = torch.zeros(Bg, D, device="cuda"), torch.zeros(Bg, D, device="cuda")
    ops.infonce_dir(dev(q), dev(k), row0, Bl, 0.1, loss, dq, dk)
    close(loss, ce.detach().reshape(1), 2e-5, 1e-4)
    close(dq, qr.grad, 1e-4, 1e-7)
    close(dk, kr.grad, 1e-4, 1e-7)
    assert float(dq[:row0].abs().max() if row0 else 0.0) == 0.0 and float(dq[row0 + Bl:].abs().max() if row0 + Bl < Bg else 0.0) == 0.0


def test_seq_mean(ops):
    B, S, D, ld = 3, 11, 50, 64
    x = torch.zeros(B, S, ld); x[..., :D] = torch.randn(B, S, D, generator=G(1))
    x = rt(x)
    m = ops.seq_mean_fwd(dev(bf(x)), B, S, D, ld)
    close(m, x[..., :D].mean(1), 1e-5, 1e-6)
    d = torch.randn(B, D, generator=G(2))
    dx = ops.seq_mean_bwd(dev(d), B, S, D, ld).float().cpu().view(B, S, ld)
    close(dx[..., :D], rt((d / S).unsqueeze(1).expand(B, S, D)), 1e-2, 1e-6)
    assert (dx[..., D:] == 0).all()


@pytest.mark.parametrize("B,S,D", [(3, 130, 512), (5, 37, 64), (2, 256, 512)])
def test_seq_mean_wide_rows_and_gelu_factor(ops, B, S, D):
    """The pooled-first InfoNCE head (mean_t(W2 h_t + b2) = W2 mean_t(h_t) + b2): 16-byte pooling over [B*S, D] bf16 rows and
    its backward  dx[b*S+s] = dout[b] / S * f(aux[b*S+s])  with f = identity on a saved gelu' (mode 1) or gelu' itself (mode 2)."""
    x = rt(torch.randn(B, S, D, generator=G(1)))
    m = ops.seq_mean_fwd(dev(bf(x)).view(B * S, D), B, S, D, D)
    close(m, x.mean(1), 1e-5, 1e-6)
    d = torch.randn(B, D, generator=G(2))
    u = rt(torch.randn(B * S, D, generator=G(3)))
    want0 = (d / S).unsqueeze(1).expand(B, S, D).reshape(B * S, D)
    close(ops.seq_mean_bwd(dev(d), B, S, D, D).float().cpu(), rt(want0), 1e-2, 1e-6)
    close(ops.seq_mean_bwd(dev(d), B, S, D, D, aux=dev(bf(u)), aux_mode=1).float().cpu(), want0 * u, 1e-2, 1e-5)
    t = u.double()
    gp = (0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * torch.pi) ** 0.5).float()
    close(ops.seq_mean_bwd(dev(d), B, S, D, D, aux=dev(bf(u)), aux_mode=2).float().cpu(), want0 * gp, 1e-2, 1e-5)


# ------------------------------------------------------------------------------------------- ConR / SupCon (golden G3)
def test_ct_losses_golden(ops, golden):
    g = golden("g3_contrastive")
    names = sorted({k.split("__")[0] for k in g})
    assert len(names) >= 20
    for name in names:
        c = {k.split("__")[1]: v for k, v in g.items() if k.startswith(name + "__")}
        f = torch.from_numpy(c["f"])
        use_w = bool(c.get("use_w", False))
        wts = dev(torch.from_numpy(c["wts"]).float()) if use_w else None
        fh, inv = ops.l2norm_fwd(dev(f))
        if name.startswith("regress"):
            loss, Gm = ops.ct_loss_fwd(ops.CT_REGRESS, fh, labels_f=dev(torch.from_numpy(c["y"]).float().mean(1).contiguous()),
                                       pred=dev(torch.from_numpy(c["yhat"]).float().mean(1).contiguous()), weights=wts,
                                       w=float(c["w"]), e=0.01)
        elif name.startswith("single"):
            loss, Gm = ops.ct_loss_fwd(ops.CT_SINGLE, fh, labels_f=dev(torch.from_numpy(c["y"]).float().reshape(-1).contiguous()), weights=wts, e=0.2)
        else:
            loss, Gm = ops.ct_loss_fwd(ops.CT_MULTI, fh, labels_i=dev(torch.from_numpy(c["y"]).long().contiguous()), weights=wts, e=0.2)
        df = ops.l2norm_bwd(ops.ct_loss_bwd(fh, Gm), fh, inv)
        close(loss, torch.from_numpy(c["loss"]).reshape(1), 2e-4, 1e-6)
        close(df, torch.from_numpy(c["df"]), 2e-3, 2e-6)


# ------------------------------------------------------------------------------------------- FDS (golden G4)
@pytest.mark.parametrize("tag", ["gauss51", "gauss52_bs2", "triang", "laplace"])
def test_fds_golden(ops, golden, tag):
    g = golden(f"g4_fds_{tag}")
    bn, bs = int(g["cfg_bucket_num"]), int(g["cfg_bucket_start"])
    mn, bw = float(g["min_value"]), float(g["bin_width"])
    lab = torch.from_numpy(g["labels"])[:, 0].contiguous()
    bins, flags = ops.fds_bins(dev(lab), mn, bw, bs, bn)
    assert torch.equal(bins.cpu().long(), torch.from_numpy(g["label_bin"]).long())        # integer part: bit-exact
    nb, D = bn - bs, 16
    rm, rv, tr = torch.zeros(nb, D, device="cuda"), torch.ones(nb, D, device="cuda"), torch.zeros(nb, device="cuda")
    feats0 = torch.from_numpy(g["feats0"])
    ops.fds_update_stats(dev(feats0), bins, flags, bs, bn, 0.0, rm, rv, tr)              # epoch == start_update -> factor 0
    close(rm, torch.from_numpy(g["s0_running_mean"]), 1e-4, 1e-5)
    close(rv, torch.from_numpy(g["s0_running_var"]), 1e-4, 1e-5)
    close(tr, torch.from_numpy(g["s0_num_samples_tracked"]), 0, 0)
    win = dev(torch.from_numpy(g["window"]))
    sm, sv = ops.fds_smooth_stats(rm, win), ops.fds_smooth_stats(rv, win)
    close(sm, torch.from_numpy(g["s1_smoothed_mean_last_epoch"]), 1e-4, 1e-5)
    close(sv, torch.from_numpy(g["s1_smoothed_var_last_epoch"]), 1e-4, 1e-5)
    xb = torch.from_numpy(g["xb"])
    b40, f40 = ops.fds_bins(dev(lab[:40].contiguous()), mn, bw, bs, bn)
    y, sc = ops.fds_smooth(dev(xb), b40, f40, bs, bn, rm, rv, sm, sv)
    close(y, torch.from_numpy(g["smooth1"]), 1e-4, 1e-4)
    # second epoch: momentum 0.9
    ops.fds_update_stats(dev(feats0 * 0.7 + 0.1), bins, flags, bs, bn, 0.9, rm, rv, tr)
    close(rm, torch.from_numpy(g["s2_running_mean"]), 1e-4, 1e-5)
    close(rv, torch.from_numpy(g["s2_running_var"]), 1e-4, 1e-5)
    sm, sv = ops.fds_smooth_stats(rm, win), ops.fds_smooth_stats(rv, win)
    y, sc = ops.fds_smooth(dev(xb), b40, f40, bs, bn, rm, rv, sm, sv)
    close(y, torch.from_numpy(g["smooth2"]), 1e-4, 1e-4)
    # d y / d x is the per-element scale
    xr = xb.clone().requires_grad_()
    fo = O.FDSOracle(D, mn, bw, bucket_num=bn, bucket_start=bs, kernel=str(g["cfg_kernel"]), ks=5, sigma=float(g["cfg_sigma"]))
    fo.running_mean_last_epoch, fo.running_var_last_epoch = rm.cpu(), rv.cpu()
    fo.smoothed_mean_last_epoch, fo.smoothed_var_last_epoch = sm.cpu(), sv.cpu()
    fo.smooth(xr, torch.from_numpy(g["labels"])[:40], 5).sum().backward()
    close(sc, xr.grad, 1e-4, 1e-5)


def test_calibrate_branches_golden(ops, golden):
    g = golden("g4_calibrate")
    x = dev(torch.from_numpy(g["x"]))
    bins = torch.zeros(6, device="cuda", dtype=torch.int32); flags = torch.ones(2, device="cuda", dtype=torch.int32)
    st = lambda k: dev(torch.from_numpy(g[k]).reshape(1, 8))
    for v1k, outk in (("v1", "out_full"), ("v1z", "out_part")):
        y, _ = ops.fds_smooth(x, bins, flags, 0, 1, st("m1"), st(v1k), st("m2"), st("v2"))
        close(y, torch.from_numpy(g[outk]), 1e-5, 1e-6)
    y, _ = ops.fds_smooth(x, bins, flags, 0, 1, st("m1"), dev(torch.zeros(1, 8)), st("m2"), st("v2"))
    close(y, torch.from_numpy(g["out_tiny"]), 0, 0)


# ------------------------------------------------------------------------------------------- pooling / head / losses / adam
def test_masked_pool(ops):
    B, Na, Nt, D = 3, 7, 11, 64
    a, t = torch.randn(B, Na, D, generator=G(1)), torch.randn(B, Nt, D, generator=G(2))
    ma = torch.ones(B, Na, dtype=torch.bool); ma[0, 4:] = False
    mt = torch.ones(B, Nt, dtype=torch.bool); mt[1, 6:] = False
    ar, tr_ = a.clone().requires_grad_(), t.clone().requires_grad_()
    ref = (torch.cat((ar * ma.unsqueeze(-1), tr_ * mt.unsqueeze(-1)), 1)).sum(1) / (ma.sum(1) + mt.sum(1)).view(-1, 1)
    out = ops.masked_pool_fwd(dev(a), dev(t), dev(ma).view(torch.uint8), dev(mt).view(torch.uint8))
    close(out, ref, 1e-5, 1e-6)
    dp = torch.randn(B, D, generator=G(3))
    (ref * dp).sum().backward()
    da, dt = ops.masked_pool_bwd(dev(dp), dev(ma).view(torch.uint8), dev(mt).view(torch.uint8), Na, Nt)
    close(da, ar.grad, 1e-5, 1e-6); close(dt, tr_.grad, 1e-5, 1e-6)


@pytest.mark.parametrize("B,D", [(37, 64), (301, 512), (32, 512)])
def test_head_and_losses(ops, B, D):
    # (301 x 512: several 128-deep k slices in every mode of the fp32 MFMA linear, ragged last slices and edge tiles)
    x = torch.randn(B, D, generator=G(1))
    P = {"classification_head.dense.weight": torch.randn(D, D, generator=G(2)) * 0.1, "classification_head.dense.bias": torch.randn(D, generator=G(3)) * 0.1,
         "classification_head.out_proj.weight": torch.randn(2, D, generator=G(4)) * 0.1, "classification_head.out_proj.bias": torch.randn(2, generator=G(5)) * 0.1}
    P = {k: v.requires_grad_() for k, v in P.items()}
    xr = x.clone().requires_grad_()
    logits = O.classification_head(xr, P)
    tgt = torch.randint(0, 2, (B, 1), generator=G(6))
    loss = O.task_loss(logits, tgt, "classification")
    loss.backward()
    w1, b1, w2, b2 = (dev(P[k].detach()) for k in P)
    h = ops.linear_f32_fwd(dev(x), w1, b1, act=ops.ACT_TANH)
    lg = ops.linear_f32_fwd(h, w2, b2)
    s = (D / 64) ** 0.5                                       # (fp32 sums of D terms in another order than torch's: the absolute floor grows with sqrt(D))
    close(lg, logits, 1e-5, 1e-6 * s * 2)
    l, dl = ops.ce_loss(lg, dev(tgt.flatten()))
    close(l, loss.reshape(1), 1e-5, 1e-6)
    dw2, db2, dw1, db1 = (torch.zeros_like(t) for t in (w2, b2, w1, b1))
    dh = ops.linear_f32_bwd(h, w2, lg, dl, dw2, db2)
    dx = ops.linear_f32_bwd(dev(x), w1, h, dh, dw1, db1, act=ops.ACT_TANH)
    close(dx, xr.grad, 1e-4, 1e-7 * s)
    for got, k in ((dw1, "dense.weight"), (db1, "dense.bias"), (dw2, "out_proj.weight"), (db2, "out_proj.bias")):
        close(got, P["classification_head." + k].grad, 1e-4, 1e-7 * s)
    pred, tg = torch.randn(B, 1, generator=G(7)), torch.randn(B, 1, generator=G(8))
    l, d = ops.mse_loss(dev(pred), dev(tg))
    close(l, torch.nn.functional.mse_loss(pred, tg).reshape(1), 1e-5, 1e-6)
    close(d, 2 * (pred - tg) / B, 1e-5, 1e-7)


def test_adam_matches_torch(ops):
    n = 1000
    p0, g = torch.randn(n, generator=G(1)), torch.randn(n, generator=G(2))
    pr = p0.clone().requires_grad_()
    opt = torch.optim.Adam([pr], lr=1e-3, eps=1e-6)
    p, m, v = dev(p0.clone()), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pb = torch.empty(n, device="cuda", dtype=torch.bfloat16)
    for step in (1, 2, 3):
        pr.grad = g * step
        opt.step()
        ops.adam_step(p, dev(g * step), m, v, pb, 1e-3, 0.9, 0.999, 1e-6, 0.0, step)
    close(p, pr.detach(), 1e-5, 1e-6)
    close(pb, rt(p.cpu()), 0, 0)
    ss = torch.zeros(1, device="cuda")
    ops.sumsq(dev(g), ss)
    close(ss, (g * g).sum().reshape(1), 1e-5, 1e-5)
    # the reproducible form (what ParamArena.adam_step calls): per-workgroup partials folded in a fixed order -- same bits every time
    for nn in (1000, 1003, 5_000_003):
        gg = torch.randn(nn, generator=G(7))
        outs = []
        for _ in range(3):
            buf = torch.zeros(1 + 2048, device="cuda")
            ops.sumsq(dev(gg), buf[:1], buf[1:])
            outs.append(buf[:1].clone())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        close(outs[0], (gg.double() * gg.double()).sum().float().reshape(1), 2e-6, 0)


def test_colsum_and_casts(ops):
    x = rt(torch.randn(333, 200, generator=G(1)))
    out = torch.zeros(200, device="cuda")
    ops.colsum(dev(bf(x)), out)
    close(out, x.sum(0), 1e-4, 1e-3)
    y = torch.randn(1027, generator=G(2))
    close(ops.cast_bf16(dev(y)), rt(y), 0, 0)
    close(ops.cast_f32(dev(bf(y))), rt(y), 0, 0)
    d = ops.dropout_f32(dev(torch.ones(100000)), 0.3, 11, 2).cpu()
    assert abs((d != 0).float().mean().item() - 0.7) < 0.01


def test_probe_tr_read_semantics(ops):
    """ds_read_b64_tr_b16: lane i of a 16-lane group receives column i of a 4x16 block (rows q=0..3 in elements 0..3)."""
    stride = 64
    out = ops.probe_tr_read(stride).cpu().view(64, 4).long()
    for lane in range(64):
        g, i = lane // 16, lane % 16
        exp = [(4 * g + q) * stride + i for q in range(4)]
        assert out[lane].tolist() == exp, (lane, out[lane].tolist(), exp)


@pytest.mark.parametrize("B,N", [(3, 13), (2, 130), (1, 1), (2, 37)])
def test_gbf_bias_fused_matches_unfused_chain(ops, B, N):
    """gbf -> Linear+GELU -> Linear -> permute in one kernel vs the four-kernel chain it replaces (same bf16 rounding
    points, so the saved intermediates agree to an ulp of bf16 and the bias to fp32 accumulation order)."""
    K, Fh, H, E = 128, 128, 64, 31 * 31
    ld = ops.pair_ld(N)
    gen = G(7)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(0, E, (B, N, N), generator=gen)
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, b1 = torch.randn(Fh, K, generator=gen) * 0.2, torch.randn(Fh, generator=gen) * 0.1
    w2, b2 = torch.randn(H, Fh, generator=gen) * 0.2, torch.randn(H, generator=gen) * 0.1
    d = [dev(t) for t in (dist, et, mul, bias, means, stds)]
    feat = ops.gbf_features_fwd(*d)
    u = torch.empty(B * N * N, Fh, device="cuda", dtype=torch.bfloat16)
    h = ops.linear_fwd(feat, dev(bf(w1)), dev(b1), act=ops.ACT_GELU, aux_out=u)
    o = ops.linear_fwd(h, dev(bf(w2)), dev(b2), out_dtype=torch.float32)
    ref = ops.pair_permute_fwd(o, B, N, H, ld)
    out, (f2, u2, h2) = ops.gbf_bias_fwd(*d, dev(bf(w1)), dev(b1), dev(bf(w2)), dev(b2), ld, save=True)
    close(f2, feat, 1e-2, 1e-6)
    close(u2, u, 1e-2, 2e-2)
    close(h2, h, 1e-2, 2e-2)
    close(out[..., :N], ref[..., :N], 2e-2, 3e-2)
    assert float((out[..., :N] - ref[..., :N]).abs().mean()) < 2e-3 * float(ref[..., :N].abs().mean()) + 1e-5
    assert (out[..., N:] == 0).all()
    out2, none = ops.gbf_bias_fwd(*d, dev(bf(w1)), dev(b1), dev(bf(w2)), dev(b2), ld, save=False)
    assert none is None and torch.equal(out2, out)
    # tiled output: same numbers in the tile layout, every pad slot -inf
    out_t, _ = ops.gbf_bias_fwd(*d, dev(bf(w1)), dev(b1), dev(bf(w2)), dev(b2), ld, save=False, tiled=True)
    assert torch.equal(ops.pair_untile(out_t, N), out[..., :N])
    used = N * ops.pair_ld(N)             # (every slot of the blocked-row planes: N real keys + the pad keys up to N4 of each query)
    assert int(torch.isinf(out_t.reshape(B, H, -1)[:, :, :used]).sum()) == B * H * (used - N * N)
    # and against the fp32 oracle of the same chain
    P = {"gbf.means.weight": means.view(1, K), "gbf.stds.weight": stds.view(1, K), "gbf.mul.weight": mul.view(E, 1), "gbf.bias.weight": bias.view(E, 1)}
    g = O.gaussian_layer(dist, et, P) if hasattr(O, "gaussian_layer") else None
    if g is not None:
        hid = torch.nn.functional.gelu(rt(g) @ rt(w1).T + b1)
        want = (rt(hid) @ rt(w2).T + b2).permute(0, 3, 1, 2)
        close(out[..., :N], want, 3e-2, 5e-2)


@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("B,N", [(2, 13), (2, 37), (1, 130)])
def test_gbf_bias_bwd_fused_matches_unfused_chain(ops, B, N, tiled):
    """One pass over G vs (re-layout, dX GEMM with GELU', dX GEMM, Gaussian backward): same bf16 rounding points."""
    K, Fh, H, E = 128, 128, 64, 31 * 31
    ld = ops.pair_ld(N)
    gen = G(11)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(0, E, (B, N, N), generator=gen)
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, w2 = dev(bf(torch.randn(Fh, K, generator=gen) * 0.2)), dev(bf(torch.randn(H, Fh, generator=gen) * 0.2))
    b1, b2 = dev(torch.randn(Fh, generator=gen) * 0.1), dev(torch.randn(H, generator=gen) * 0.1)
    d = [dev(t) for t in (dist, et, mul, bias, means, stds)]
    _, (feat, u, h) = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=True, tiled=tiled)
    g_std = torch.zeros(B, H, N, ld); g_std[..., :N] = torch.randn(B, H, N, N, generator=gen)
    g = ops.pair_tile(dev(g_std), N, 0.0) if tiled else dev(g_std)
    # unfused chain
    do_r = ops.pair_permute_bwd(g, B, N, H, ld)
    du_r = ops.linear_bwd_input(do_r, w2, act=ops.ACT_GELU_BWD, aux_in=u)
    df_r = ops.linear_bwd_input(du_r, w1)
    gr_r = [torch.zeros_like(t) for t in d[2:]]
    ops.gbf_features_bwd(*d, df_r, *gr_r)
    # fused
    gr = [torch.zeros_like(t) for t in d[2:]]
    do, du = ops.gbf_bias_bwd(g, *d, w1, w2, u, ld, *gr)
    assert torch.equal(do, do_r)
    close(du, du_r, 1e-2, 1e-3)
    assert float((du.float() - du_r.float()).abs().mean()) < 2e-3 * float(du_r.float().abs().mean()) + 1e-6
    for a, b_, name in zip(gr, gr_r, ("dmul", "dbias", "dmeans", "dstds")):
        r = float((a - b_).norm() / (b_.norm() + 1e-12))
        assert r < 2e-2, (name, r)
    # flag bit 1: the forward saves gelu'(u) (same erf / exponential as its GELU), the backward multiplies
    _, (feat2, ug, h2) = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=True, tiled=tiled, save_grad=True)
    assert torch.equal(feat2, feat) and torch.equal(h2, h)
    t = u.double()
    close(ug.double(), 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * torch.pi) ** 0.5, 2e-2, 8e-3)   # (u itself is bf16-rounded)
    gr2 = [torch.zeros_like(t_) for t_ in d[2:]]
    do2, du2 = ops.gbf_bias_bwd(g, *d, w1, w2, ug, ld, *gr2, u_is_grad=True)
    assert torch.equal(do2, do)
    assert float((du2.float() - du_r.float()).abs().mean()) < 6e-3 * float(du_r.float().abs().mean()) + 1e-6
    for a, b_, name in zip(gr2, gr_r, ("dmul", "dbias", "dmeans", "dstds")):
        r = float((a - b_).norm() / (b_.norm() + 1e-12))
        assert r < 2e-2, (name, r)


@pytest.mark.parametrize("edge_dtype", [torch.int64, torch.int32, torch.int16])
@pytest.mark.parametrize("tiled", [False, True])
@pytest.mark.parametrize("B,N", [(2, 13), (3, 37), (1, 130), (9, 21), (1, 1)])
def test_gbf_bias_complete_backward_matches_chain_and_autograd(ops, B, N, tiled, edge_dtype):
    """ONE kernel (nothing saved by the forward: basis / hidden recomputed, every parameter gradient accumulated on chip)
    vs the round-1 chain (fused per-pair half + two weight-gradient GEMMs) and vs fp32 autograd of the bf16-rounded chain.
    Edge types as int64 (the reference's collate), int32 or int16 must give the same gradients."""
    K, Fh, H, E = 128, 128, 64, 31 * 31
    ld = ops.pair_ld(N)
    gen = G(23)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(0, E, (B, N, N), generator=gen)
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1f, w2f = rt(torch.randn(Fh, K, generator=gen) * 0.2), rt(torch.randn(H, Fh, generator=gen) * 0.2)
    b1f, b2f = torch.randn(Fh, generator=gen) * 0.1, torch.randn(H, generator=gen) * 0.1
    w1, w2, b1, b2 = dev(bf(w1f)), dev(bf(w2f)), dev(b1f), dev(b2f)
    d = [dev(t) for t in (dist, et, mul, bias, means, stds)]
    dn = list(d); dn[1] = d[1].to(edge_dtype)
    g_std = torch.zeros(B, H, N, ld); g_std[..., :N] = torch.randn(B, H, N, N, generator=gen)
    g = ops.pair_tile(dev(g_std), N, 0.0) if tiled else dev(g_std)
    # the forward with narrowed edge types is the same forward
    out64, _ = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=False, tiled=tiled)
    outn, _ = ops.gbf_bias_fwd(*dn, w1, b1, w2, b2, ld, save=False, tiled=tiled)
    assert torch.equal(out64, outn)
    # round-1 chain
    _, (feat, u, h) = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=True, tiled=tiled)
    gr_r = [torch.zeros_like(t) for t in d[2:]]
    do, du = ops.gbf_bias_bwd(g, *d, w1, w2, u, ld, *gr_r)
    ref = {"dw2": do.float().T @ h.float(), "db2": do.float().sum(0), "dw1": du.float().T @ feat.float(), "db1": du.float().sum(0),
           "dmul": gr_r[0], "dbias": gr_r[1], "dmeans": gr_r[2], "dstds": gr_r[3]}
    # complete kernel; buffers start non-zero: the kernel accumulates
    names = ("dw1", "db1", "dw2", "db2", "dmul", "dbias", "dmeans", "dstds")
    shapes = ((Fh, K), (Fh,), (H, Fh), (H,), (E,), (E,), (K,), (K,))
    got = {n: torch.full(sh, 0.5, device="cuda") for n, sh in zip(names, shapes)}
    ops.gbf_bias_bwd_full(g, *dn, w1, b1, w2, ld, *[got[n].view(-1) for n in names])
    for n in names:
        a, b_ = got[n] - 0.5, ref[n]
        r = float((a - b_).norm() / (b_.norm() + 1e-12))
        assert r < (2e-2 if n in ("dmul", "dbias", "dmeans", "dstds") else 6e-3), (n, r)
    # fp32 autograd of the same chain with the same operand rounding
    P = {k: v.clone().requires_grad_(True) for k, v in (("mul", mul), ("bias", bias), ("means", means), ("stds", stds), ("w1", w1f), ("b1", b1f),
                                                         ("w2", w2f), ("b2", b2f))}
    y = P["mul"][et] * dist + P["bias"][et]
    sg = P["stds"].abs() + 1e-5
    basis = torch.exp(-0.5 * ((y[..., None] - P["means"]) / sg) ** 2) / ((2 * 3.14159) ** 0.5 * sg)
    hid = torch.nn.functional.gelu(basis @ P["w1"].T + P["b1"])
    o = (hid @ P["w2"].T + P["b2"]).permute(0, 3, 1, 2)
    (o * rt(g_std[..., :N])).sum().backward()
    want = {"dw1": P["w1"].grad, "db1": P["b1"].grad, "dw2": P["w2"].grad, "db2": P["b2"].grad, "dmul": P["mul"].grad, "dbias": P["bias"].grad,
            "dmeans": P["means"].grad, "dstds": P["stds"].grad}
    for n in names:
        a, b_ = (got[n] - 0.5).cpu(), want[n]
        r = float((a - b_).norm() / (b_.norm() + 1e-12))
        assert r < 3e-2, (n, "vs autograd", r)


@pytest.mark.parametrize("B,N", [(2, 13), (3, 37), (1, 130), (1, 1)])
def test_gbf_bias_compact_planes(ops, B, N):
    """Compact tiled planes at the two ends of the pair chain: the fused pair-bias forward writes fp16 = fp16_rne(its fp32
    output) with -inf in every pad slot, and both backward forms read the gradient as bf16 exactly as they read the same values
    in fp32."""
    K, Fh, H, E = 128, 128, 64, 31 * 31
    ld = ops.pair_ld(N)
    gen = G(29)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(0, E, (B, N, N), generator=gen)
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, b1 = dev(bf(torch.randn(Fh, K, generator=gen) * 0.2)), dev(torch.randn(Fh, generator=gen) * 0.1)
    w2, b2 = dev(bf(torch.randn(H, Fh, generator=gen) * 0.2)), dev(torch.randn(H, generator=gen) * 0.1)
    d = [dev(t) for t in (dist, et.to(torch.int16), mul, bias, means, stds)]
    o32, _ = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=False, tiled=True)
    o16, saved = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=True, tiled=True, compact=True)
    assert o16.dtype == torch.float16 and o16.shape == o32.shape
    assert torch.equal(o16, o32.half())                                # every slot, pads (-inf) included
    idx = ops._tile_index(N, o16.device).reshape(-1)
    pads = torch.ones(o16[0, 0].numel(), dtype=torch.bool, device=o16.device); pads[idx] = False
    pads[N * ld:] = False                                              # (the alignment tail of a plane is no slot)
    assert torch.isneginf(o16.reshape(B, H, -1)[:, :, pads]).all()
    with pytest.raises(ops.MMDTIError):
        ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=False, tiled=False, compact=True)
    g32 = ops.pair_tile(dev(torch.randn(B, H, N, N, generator=gen)), N, 0.0).bfloat16().float()
    g16 = g32.bfloat16()
    # round-1 chain: per-pair half
    feat, u, h = saved
    gr_a = [torch.zeros_like(t) for t in d[2:]]; gr_b = [torch.zeros_like(t) for t in d[2:]]
    do_a, du_a = ops.gbf_bias_bwd(g32, *d, w1, w2, u, ld, *gr_a)
    do_b, du_b = ops.gbf_bias_bwd(g16, *d, w1, w2, u, ld, *gr_b)
    assert torch.equal(do_a, do_b) and torch.equal(du_a, du_b)
    # complete kernel (fp32 atomics at the flush: equal up to summation order)
    names = ("dw1", "db1", "dw2", "db2", "dmul", "dbias", "dmeans", "dstds")
    shapes = ((Fh, K), (Fh,), (H, Fh), (H,), (E,), (E,), (K,), (K,))
    got = {}
    for tag, g in (("f32", g32), ("bf16", g16)):
        got[tag] = {n: torch.zeros(sh, device="cuda") for n, sh in zip(names, shapes)}
        ops.gbf_bias_bwd_full(g, *d, w1, b1, w2, ld, *[got[tag][n].view(-1) for n in names])
    for n in names:
        a, b_ = got["bf16"][n], got["f32"][n]
        assert float((a - b_).norm() / (b_.norm() + 1e-12)) < 1e-5, n


@pytest.mark.parametrize("B,N,lens", [(4, 130, (130, 37, 64, 5)), (3, 37, (37, 16, 17)), (2, 200, (33, 200)), (3, 21, (21, 21, 21))])
def test_gbf_bias_ragged_tile_prefixes(ops, B, N, lens):
    """Ragged batches at the two ends of the pair chain: with the per-molecule tile prefixes the fused pair-bias forward writes only
    the blocks of each molecule's first key tiles (the ones the ragged pair-attention kernels read; bit-identical there, everything
    behind them left untouched), and the complete backward visits only those blocks -- the gradient is zero behind them, so all
    eight parameter gradients agree with the dense run up to the summation order of the fp32 atomics."""
    K, Fh, H, E = 128, 128, 64, 31 * 31
    ld, nt = ops.pair_ld(N), ops.pair_tiles(N)
    gen = G(31)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(1, E, (B, N, N), generator=gen)
    for b, n in enumerate(lens):                                   # padded as the reference collates: distance 0, edge type 0
        dist[b, n:, :] = 0; dist[b, :, n:] = 0; et[b, n:, :] = 0; et[b, :, n:] = 0
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, b1 = dev(bf(torch.randn(Fh, K, generator=gen) * 0.2)), dev(torch.randn(Fh, generator=gen) * 0.1)
    w2, b2 = dev(bf(torch.randn(H, Fh, generator=gen) * 0.2)), dev(torch.randn(H, generator=gen) * 0.1)
    d = [dev(t) for t in (dist, et.to(torch.int16), mul, bias, means, stds)]
    kt = torch.tensor([(n + 15) // 16 for n in lens])
    ke = [ops.pair_key_tiles_effective(int(k), nt) for k in kt]
    pre_f, pre_b = ops.gbf_tile_prefixes(kt, N, "cuda")
    nb4 = (N + 3) // 4
    assert pre_f.dtype == torch.int32 and pre_f.shape == (B + 1,) and int(pre_f[-1]) == sum(min(4 * k, nb4) * nb4 for k in ke)
    dense, _ = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=False, tiled=True, compact=True)
    canary = 123.0
    import mmdti_hip.ops as O_
    orig_empty = O_.pair_empty
    O_.pair_empty = lambda *a, **k: torch.full_like(orig_empty(*a, **k), canary)       # so that "not written" is observable
    try:
        rag, _ = ops.gbf_bias_fwd(*d, w1, b1, w2, b2, ld, save=False, tiled=True, compact=True, tile_prefix=pre_f)
    finally:
        O_.pair_empty = orig_empty
    for b in range(B):
        kept, behind = ops.pair_slots(N, "cuda", k_hi=16 * ke[b]), ops.pair_slots(N, "cuda", k_lo=16 * ke[b])
        assert torch.equal(rag[b][:, kept], dense[b][:, kept])             # key tiles < ke, every query, pad keys included
        if ke[b] < nt:
            assert bool((rag[b][:, behind] == canary).all())           # (the bias of padded keys: the ragged attention kernels never read it)
    # backward: g is zero behind the kept tiles (as the ragged attention backward leaves it)
    g = ops.pair_tile(dev(torch.randn(B, H, N, N, generator=gen)), N, 0.0)
    for b in range(B):
        g[b][:, ops.pair_slots(N, "cuda", k_lo=16 * ke[b])] = 0.0
    names = ("dw1", "db1", "dw2", "db2", "dmul", "dbias", "dmeans", "dstds")
    shapes = ((Fh, K), (Fh,), (H, Fh), (H,), (E,), (E,), (K,), (K,))
    got = {}
    for tag, pre in (("dense", None), ("ragged", pre_b)):
        got[tag] = {n: torch.zeros(sh, device="cuda") for n, sh in zip(names, shapes)}
        gg = g.clone()
        if pre is not None:
            for b in range(B):
                gg[b][:, ops.pair_slots(N, "cuda", k_lo=16 * ke[b])] = float("nan")          # never read
        ops.gbf_bias_bwd_full(gg, *d, w1, b1, w2, ld, *[got[tag][n].view(-1) for n in names], tile_prefix=pre)
    for n in names:
        a, b_ = got["ragged"][n], got["dense"][n]
        assert torch.isfinite(a).all(), n
        assert float((a - b_).norm() / (b_.norm() + 1e-12)) < 1e-5, n


@pytest.mark.parametrize("E", [1600, 5000])
def test_gbf_bias_forward_with_large_edge_type_tables(ops, E):
    """E = 1600 (a 40-token dictionary): tables in LDS, but more than the complete backward kernel keeps (1536), so the model
    falls back to the round-1 backward chain; E = 5000: beyond the forward's LDS tables too (global gathers).  Same numbers as
    the unfused chain in both."""
    K, Fh, H, B, N = 128, 128, 64, 2, 21
    ld = ops.pair_ld(N)
    gen = G(41)
    dist = torch.rand(B, N, N, generator=gen) * 8
    et = torch.randint(0, E, (B, N, N), generator=gen)
    et[0, 0, :4] = torch.tensor([0, E - 1, E + 7, -3])            # out-of-range indices clamp, as in the unfused kernel
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, b1 = dev(bf(torch.randn(Fh, K, generator=gen) * 0.2)), dev(torch.randn(Fh, generator=gen) * 0.1)
    w2, b2 = dev(bf(torch.randn(H, Fh, generator=gen) * 0.2)), dev(torch.randn(H, generator=gen) * 0.1)
    d = [dev(t) for t in (dist, et, mul, bias, means, stds)]
    feat = ops.gbf_features_fwd(*d)
    h = ops.linear_fwd(feat, w1, b1, act=ops.ACT_GELU)
    o = ops.linear_fwd(h, w2, b2, out_dtype=torch.float32)
    ref = ops.pair_permute_fwd(o, B, N, H, ld)
    for dt in (torch.int64, torch.int32):
        dn = list(d); dn[1] = d[1].to(dt)
        out, _ = ops.gbf_bias_fwd(*dn, w1, b1, w2, b2, ld, save=False)
        close(out[..., :N], ref[..., :N], 2e-2, 3e-2)
        assert float((out[..., :N] - ref[..., :N]).abs().mean()) < 2e-3 * float(ref[..., :N].abs().mean()) + 1e-5


def test_gbf_bias_complete_backward_rejects_bad_arguments(ops):
    from mmdti_hip._abi import MMDTIError
    K, Fh, H, E, B, N = 128, 128, 64, 2000, 1, 8
    ld = ops.pair_ld(N)
    z = lambda *s: torch.zeros(*s, device="cuda")
    args = [z(B, H, N, ld), z(B, N, N), torch.zeros(B, N, N, device="cuda", dtype=torch.int64), z(E), z(E), z(K), z(K) + 1,
            z(Fh, K).bfloat16(), z(Fh), z(H, Fh).bfloat16(), ld, z(Fh * K), z(Fh), z(H * Fh), z(H), z(E), z(E), z(K), z(K)]
    with pytest.raises(MMDTIError):            # E beyond the tables the kernel keeps in LDS
        ops.gbf_bias_bwd_full(*args)
    with pytest.raises(TypeError):
        args[2] = args[2].to(torch.int8)
        ops.gbf_bias_bwd_full(*args)


@pytest.mark.parametrize("M,N,K,out_dtype", [(300, 128, 64, torch.bfloat16), (1000, 256, 192, torch.float32), (129, 64, 128, torch.bfloat16)])
def test_gemm_epilogue_column_sums(ops, M, N, K, out_dtype):
    """colsum_out: the bias gradient of the producing Linear, accumulated (+=) by the epilogue from the STORED values."""
    x, w = dev(bf(torch.randn(M, K, generator=G(1)))), dev(bf(torch.randn(N, K, generator=G(2))))
    cs = torch.full((N,), 0.25, device="cuda")
    y = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, out_dtype=out_dtype, colsum=cs)
    ref = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, out_dtype=out_dtype)
    assert torch.equal(y, ref)
    close(cs, 0.25 + y.float().sum(0), 1e-5, 1e-3)
    from mmdti_hip._abi import MMDTIError
    with pytest.raises(MMDTIError):                                            # split-K partial sums have no column sums
        ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, out=torch.zeros(M, N, device="cuda"), atomic=True, splitk=2, colsum=cs)


@pytest.mark.parametrize("M,N,K", [(300, 256, 64), (1000, 2048, 512), (77, 40, 96)])
def test_gemm_gelu_saving_its_gradient(ops, M, N, K):
    """ACT_GELU_G: y = gelu(x.w^T + b) and aux = bf16(gelu'(pre-activation)) from the same erf / exponential;
    ACT_MUL_AUX: dX-GEMM output times that saved factor == the ACT_GELU / ACT_GELU_BWD pair up to the bf16 rounding of the
    saved tensor (gelu' of the rounded u there, rounded gelu' of the exact u here).  Last shape: scalar epilogue (N % 8 != 0)."""
    x, w, b = dev(bf(torch.randn(M, K, generator=G(1)))), dev(bf(torch.randn(N, K, generator=G(2)) * 0.2)), dev(torch.randn(N, generator=G(3)))
    ldx = (N + 7) // 8 * 8
    u = torch.zeros(M, ldx, device="cuda", dtype=torch.bfloat16)
    gsv = torch.zeros(M, ldx, device="cuda", dtype=torch.bfloat16)
    y0 = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, bias=b, act=ops.ACT_GELU, aux_out=u)
    y1 = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, bias=b, act=ops.ACT_GELU_G, aux_out=gsv)
    assert torch.equal(y0, y1)
    pre = x.float() @ w.float().t() + b
    t = pre.double()
    want = 0.5 * (1 + torch.erf(t / 2 ** 0.5)) + t * torch.exp(-0.5 * t * t) / (2 * torch.pi) ** 0.5
    close(gsv[:, :N].double(), want, 6e-3, 4e-3)                       # bf16 rounding of a value in [-0.13, 1.13]
    dy = dev(bf(torch.randn(M, ldx, generator=G(4))))[:, :N]
    wt = dev(bf(torch.randn(K, N, generator=G(5)) * 0.2))              # dX = dy . W  with W [N_out=K? no: weight layout [N, K]]
    d0 = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, act=ops.ACT_GELU_BWD, aux_in=u)
    d1 = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, act=ops.ACT_MUL_AUX, aux_in=gsv)
    close(d1, d0, 2e-2, 2e-2 * float(d0.float().abs().mean()))
    raw = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=K, out_dtype=torch.float32)
    close(d1.float(), raw * gsv[:, :N].float(), 1e-2, 1e-2 * float(raw.abs().mean()))


@pytest.mark.parametrize("rows,N,K", [(33280, 1536, 512), (4096, 1536, 512), (2050, 512, 512), (3000, 104, 64), (4096, 520, 2048)])
def test_weight_gradient_carries_the_bias_gradient(ops, rows, N, K):
    """linear_bwd_weight(db=...): dW += dy^T x and db += column sums of dy in ONE pass over dy (an extra MFMA per dy
    fragment against a ones operand in the double-buffered split-K kernel; the column-sum kernel on the other paths).
    Both accumulate (+=).  Shapes: the in_proj gradient of the bench, a smaller one, ragged rows, small / unaligned outputs."""
    from mmdti_hip import _abi
    from gemm_plan_helpers import dw_case, plan_of
    # bare-load shapes (rows % 64 == 0): the double-buffered kernel sums dy itself; the others: register-staged kernel + column-sum pass
    with_db, without = plan_of(_abi.lib(), dw_case(ops, N, K, rows, db=True)), plan_of(_abi.lib(), dw_case(ops, N, K, rows, db=False))
    if rows % 64 == 0:
        assert with_db[0] == "gemm_glds_kernel<true, true, 1, false, false>" and with_db[9] == 1, with_db
    else:
        assert with_db[0] == "gemm_bf16_kernel<true, true, false, false, false>" and with_db[9] == 2, with_db
    assert without[9] == 0 and with_db[5] > 1
    dy = dev(bf(torch.randn(rows, N, generator=G(1))))
    x = dev(bf(torch.randn(rows, K, generator=G(2))))
    dw, db = torch.full((N, K), 0.5, device="cuda"), torch.full((N,), -0.25, device="cuda")
    ops.linear_bwd_weight(dy, x, dw, db=db)
    dw0 = torch.full((N, K), 0.5, device="cuda")
    ops.linear_bwd_weight(dy, x, dw0)
    close(dw, dw0, 1e-4, 1e-2)                                    # (atomic accumulation order differs run to run)
    close(dw, 0.5 + dy.float().t() @ x.float(), 2e-3, 2e-2 * (rows ** 0.5))
    want = -0.25 + dy.double().sum(0)
    close(db.double(), want, 1e-4, 1e-3 * (rows ** 0.5))
    # a row-strided dy (a [rows, 3N] buffer's middle third), as the fused q|k|v layout hands it over
    big = dev(bf(torch.randn(rows, 3 * N, generator=G(3))))
    if N % 8 == 0:
        db2 = torch.zeros(N, device="cuda")
        ops.linear_bwd_weight(big[:, N:2 * N], x, torch.zeros(N, K, device="cuda"), db=db2)
        close(db2.double(), big[:, N:2 * N].double().sum(0), 1e-4, 1e-3 * (rows ** 0.5))


@pytest.mark.parametrize("transB", [False, True])
def test_gemm_tall_tiles_match_square_tiles(ops, transB, monkeypatch):
    """M = 256 x 130 rows, N = 512: the shape that switches to 144-row tiles advancing by 130 rows (one round of resident
    workgroups instead of two).  Same numbers as the 128-row tiling, including the fused epilogue and the column sums."""
    import os
    from mmdti_hip import _abi
    from gemm_plan_helpers import case as plan_case, plan_of
    M, N, K = 256 * 130, 512, 192
    for pc in (plan_case(M, N, K, tB=int(transB), bias=1, residual=1, out="f32", colsum=1), plan_case(M, N, K, tB=int(transB), bias=1)):
        name, gx, gz, block, lds, sk, mstep = plan_of(_abi.lib(), pc)[:7]
        assert name == "gemm_glds_tall_kernel<%s, false>" % str(transB).lower() and mstep == 130 and gx == 256 * 4, (name, mstep, gx)
    x = dev(bf(torch.randn(M, K, generator=G(1))))
    w = dev(bf(torch.randn(K, N, generator=G(2)))) if transB else dev(bf(torch.randn(N, K, generator=G(2))))
    bias, res = dev(torch.randn(N, generator=G(3))), dev(torch.randn(M, N, generator=G(4)))
    kw = dict(M=M, N=N, K=K, lda=K, ldb=(N if transB else K), transB=transB, bias=bias, residual=res, out_dtype=torch.float32, drop_p=0.1, seed=5, site=2)
    cs = torch.zeros(N, device="cuda")
    y = ops.gemm(x, w, colsum=cs, **kw)
    wf = w.float() if transB else w.float().t()
    ref_nodrop = x.float() @ wf + bias
    keep = (y - res) != 0
    close((y - res)[keep], (ref_nodrop / 0.9)[keep], 2e-3, 2e-2)
    assert abs(float(keep.float().mean()) - 0.9) < 0.01
    close(cs, y.sum(0), 1e-4, 2e-2)
    yb = ops.gemm(x, w, M=M, N=N, K=K, lda=K, ldb=(N if transB else K), transB=transB, bias=bias)   # bf16 output path
    close(yb, ref_nodrop, 1e-2, 5e-2)
    # row 129 of every 130-row step is the last row a tall tile stores; row 130 belongs to the next tile
    assert torch.isfinite(yb.float()).all()


SMALL_LAUNCH_SHAPES = [(1695, 512, 2048), (1311, 2048, 512), (8, 64, 64), (77, 520, 128), (3000, 1536, 512), (640, 512, 192)]


def _small_launch_variant(M, N, K, transB, small, deep):
    """the kernel a bare-load forward shape is meant to take under (gemm_small, gemm_deep): 64 x 64 tiles up to 128 tiles of 128 x 128,
    the four-stage ring up to 256 of them when K has four K-tiles, else the single-buffered kernel"""
    tiles = -(-M // 128) * -(-N // 128)
    return ("gemm_small_kernel" if small and tiles <= 128 else
            "gemm_glds_kernel<false, %s, 2," % str(transB).lower() if deep and tiles <= 256 and K >= 256 else
            "gemm_glds_kernel<false, %s, 0," % str(transB).lower())


def test_gemm_small_launch_shapes_reach_all_three_variants():
    """(3000, 1536, 512) has 288 tiles and runs the single-buffered kernel under every setting: it is the past-both-limits case.  The
    next largest, (1311, 2048, 512) with 176 tiles, takes the four-stage ring even under gemm_small.  The other four take the 64 x 64 kernel under gemm_small, and some of them the four-stage ring / the plain kernel with it off."""
    for transB in (False, True):
        variants = lambda small, deep: [_small_launch_variant(M, N, K, transB, small, deep) for M, N, K in SMALL_LAUNCH_SHAPES]
        assert sum(v == "gemm_small_kernel" for v in variants(1, 1)) == 4 and sum(v.endswith(", 2,") for v in variants(1, 1)) == 1
        assert sum(v.endswith(", 2,") for v in variants(0, 1)) >= 2 and sum(v.endswith(", 0,") for v in variants(0, 1)) >= 2
        assert all(v.endswith(", 0,") for v in variants(0, 0))


@pytest.mark.parametrize("M,N,K", SMALL_LAUNCH_SHAPES)
@pytest.mark.parametrize("transB", [False, True])
def test_gemm_small_launch_paths_are_bitwise_the_128_tile_kernel(ops, M, N, K, transB):
    """Small launches (the reference's default batch of 16-32 molecules) take 64 x 64 tiles behind a four-stage LDS-DMA ring
    (gemm_small_kernel) or, past its tile limit, the four-stage ring on 128 x 128 tiles: both sum the same products in the
    same order as the single-buffered 128 x 128 kernel, so every fused epilogue gives the SAME BITS on all three paths."""
    from mmdti_hip import _abi
    lib = _abi.lib()
    from gemm_plan_helpers import case as plan_case, plan_of
    x = dev(bf(torch.randn(M, K, generator=G(1))))
    w = dev(bf(torch.randn(K, N, generator=G(2)))) if transB else dev(bf(torch.randn(N, K, generator=G(2))))
    bias, res = dev(torch.randn(N, generator=G(3))), dev(torch.randn(M, N, generator=G(4)))
    u = dev(bf(torch.randn(M, N, generator=G(5))))
    base = dict(M=M, N=N, K=K, lda=K, ldb=(N if transB else K), transB=transB)
    cases = [dict(bias=bias), dict(bias=bias, residual=res, out_dtype=torch.float32, drop_p=0.1, seed=5, site=2),
             dict(bias=bias, act=ops.ACT_GELU, aux_out=torch.empty(M, N, device="cuda", dtype=torch.bfloat16)),
             dict(act=ops.ACT_GELU_BWD, aux_in=u), dict(out_dtype=torch.float32)]
    outs = {}
    try:
        for name, (small, deep) in {"small": (1, 1), "deep": (0, 1), "plain": (0, 0)}.items():
            lib.mmdti_set_option(b"gemm_small", small); lib.mmdti_set_option(b"gemm_deep", deep)
            # the variant this setting is meant to reach (all shapes here are bare-load shapes: K % 64 == 0)
            want = _small_launch_variant(M, N, K, transB, small, deep)
            for pc in (plan_case(M, N, K, tB=int(transB), bias=1), plan_case(M, N, K, tB=int(transB), out="f32")):
                assert plan_of(lib, pc)[0].startswith(want), (name, plan_of(lib, pc))
            outs[name] = []
            for kw in cases:
                kw = dict(kw)
                if "aux_out" in kw:
                    kw["aux_out"] = torch.empty_like(kw["aux_out"])
                y = ops.gemm(x, w, **base, **kw)
                outs[name].append((y.clone(), kw["aux_out"].clone() if "aux_out" in kw else None))
    finally:
        lib.mmdti_set_option(b"gemm_small", 1); lib.mmdti_set_option(b"gemm_deep", 1)
    for name in ("small", "deep"):
        for (y, aux), (y0, aux0) in zip(outs[name], outs["plain"]):
            assert torch.equal(y, y0), name
            assert aux is None or torch.equal(aux, aux0), name
    wf = w.float() if transB else w.float().t()
    close(outs["small"][4][0], x.float() @ wf, 2e-3, 2e-2 * (K ** 0.5))


@pytest.mark.parametrize("M,K,R", [(1, 512, 0), (63, 512, 0), (64, 64, 0), (130, 2048, 0), (1000, 512, 80), (3333, 2048, 64), (33280, 512, 0), (12713, 2048, 0)])
def test_gemm_ln_fused_matches_gemm_then_layernorm(ops, M, K, R, monkeypatch):
    """mmdti_gemm_ln_bf16: the Linear that closes a residual branch and the LayerNorm behind it in one kernel (N = 512) against the
    two kernels it replaces.  x = residual + dropout(A.W^T + b): bit-equal (same k order, same dropout counters); mean / rstd / h:
    the row sums are taken in another order -- 1e-6 relative, bf16 outputs within one rounding step."""
    if R:
        monkeypatch.setenv("MMDTI_GEMM_LN_ROWS", str(R))       # (read once per process: the first parametrisation that sets it wins)
    monkeypatch.setattr(ops, "GEMM_LN_MAX_K", 4096)            # (the product only sends K <= 1024 to the fused kernel: measured)
    from mmdti_hip import _abi
    rows_per_tile = _abi.lib()._dll.mmdti_gemm_ln_rows(M)
    auto = 80 if -(-(-(-M // 80)) // 512) * 5 < -(-(-(-M // 64)) // 512) * 4 else 64
    # R is forced only if its parametrisation makes the first fused call of the process: MMDTI_GEMM_LN_ROWS is read once, and in file
    # order (1, 512, 0) reads it unset (so does tests/test_gemm_plan_cpu.py, whose options() writes gemm_ln_rows back to 0) -- then
    # both forced cases run the automatic choice, as they always have.  The forced values are pinned in test_gemm_plan_cpu.py.
    assert rows_per_tile in {auto, R or auto}
    if not R:
        assert rows_per_tile == (80 if M == 33280 else 64)       # R = 5 at the bench's tower-1 row count, R = 4 on the others
    N = 512
    g = G(M + K)
    x = dev(bf(torch.randn(M, K, generator=g)))
    w = dev(bf(torch.randn(N, K, generator=g) * 0.05))
    b = dev(torch.randn(N, generator=g))
    res = dev(torch.randn(M, N, generator=g) * 2.0 + 0.5)
    gam, bet = dev(torch.randn(N, generator=g) * 0.2 + 1.0), dev(torch.randn(N, generator=g) * 0.1)
    for kw in (dict(residual=res, drop_p=0.1, seed=7, site=3), dict(residual=None, drop_p=0.0), dict(residual=res, drop_p=0.0)):
        for f32, b16 in ((False, True), (True, True), (True, False)):
            y, h32, h16, mean, rstd = ops.linear_ln_fwd(x, w, b, gam, bet, 1e-5, want_f32=f32, want_bf16=b16, **kw)
            y_ref = ops.linear_fwd(x, w, b, out_dtype=torch.float32, **kw)
            r32, r16, rm, rr = ops.layernorm_fwd(y_ref, gam, bet, 1e-5, want_f32=True, want_bf16=True)
            assert torch.equal(y, y_ref)
            close(mean, rm, 1e-5, 1e-6); close(rstd, rr, 1e-5, 1e-6)
            assert (h32 is None) == (not f32) and (h16 is None) == (not b16)
            if f32:
                close(h32, r32, 1e-5, 2e-6)
            if b16:
                d = (h16.float() - r16.float()).abs()
                assert float(d.max()) <= 2.0 ** -7 * float(r16.float().abs().max()) and float((d > 0).float().mean()) < 0.01
    assert ops.linear_ln_eligible(x, w, res)
    # other widths take the two kernels (same results through the same wrapper)
    w2 = dev(bf(torch.randn(256, K, generator=g) * 0.05))
    assert not ops.linear_ln_eligible(x, w2)
    y, _, h16, mean, rstd = ops.linear_ln_fwd(x, w2, None, gam[:256].contiguous(), bet[:256].contiguous(), 1e-5)
    assert y.shape == (M, 256) and h16.shape == (M, 256)


# ------------------------------------------------------------------------------------------- fused attention
def _attn_ref(q, k, v, add, heads, scale, keep=None, p_drop=0.0):
    """fp32 torch restatement on bf16-rounded operands (oracle mha, mmdti_oracle.py:320-338, minus the Linears)."""
    B, Lq, D = q.shape
    Lk = k.shape[1]
    hd = D // heads
    qh, kh, vh = (t.view(B, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-1, -2)) * scale
    if add is not None:
        s = s + add.view(B, 1, 1, Lk)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep / (1.0 - p_drop)
    pr = p + (rt(p) - p).detach()                       # bf16 operand rounding, straight-through
    return torch.matmul(pr, vh).transpose(1, 2).reshape(B, Lq, D), p


@pytest.mark.parametrize("B,heads,Lq,Lk,hd", [(2, 8, 256, 256, 64), (2, 3, 37, 50, 64), (3, 16, 130, 256, 32), (2, 16, 256, 130, 32),
                                              (1, 2, 1, 1, 32), (2, 4, 161, 161, 64), (1, 2, 16, 160, 32), (2, 4, 37, 50, 16), (1, 4, 200, 256, 16)])
def test_attn_fused_matches_reference(ops, B, heads, Lq, Lk, hd):
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (rt(torch.randn(B, L, D, generator=G(s)) * 1.5) for L, s in ((Lq, 1), (Lk, 2), (Lk, 3), (Lq, 4)))
    mask = torch.ones(B, Lk)
    if Lk > 2:
        mask[0, Lk - Lk // 3:] = 0
    add = (1 - mask) * torch.finfo(torch.float32).min
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    ref, _ = _attn_ref(qg, kg, vg, add, heads, scale)
    ref.backward(do)
    flat = lambda t, L: dev(bf(t.reshape(B * L, D)))
    ctx, stats = ops.attn_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), dev(add), B, heads, Lq, Lk, scale)
    close(ctx.view(B, Lq, D), ref, 2e-2, 2e-2)
    assert float((ctx.view(B, Lq, D).float().cpu() - ref.detach()).abs().mean()) < 3e-3
    dq, dk, dv = ops.attn_bwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), dev(add), flat(do, Lq), stats, B, heads, Lq, Lk, scale)
    for got, want, L in ((dq, qg.grad, Lq), (dk, kg.grad, Lk), (dv, vg.grad, Lk)):
        w = want.reshape(B * L, D)
        tol = 2e-2 * float(w.abs().max()) + 1e-3
        assert float((got.float().cpu() - w).abs().max()) < tol, float((got.float().cpu() - w).abs().max())
        assert float((got.float().cpu() - w).abs().mean()) < 0.01 * float(w.abs().mean()) + 1e-4
    # masked keys receive exactly zero gradient
    if Lk > 2:
        assert (dk.view(B, Lk, D)[0, Lk - Lk // 3:] == 0).all() and (dv.view(B, Lk, D)[0, Lk - Lk // 3:] == 0).all()


@pytest.mark.parametrize("Lq,Lk,hd", [(70, 96, 64), (130, 256, 32), (40, 48, 16)])
def test_attn_fused_dropout_mask_consistent(ops, Lq, Lk, hd):
    """The keep mask is recovered from the forward itself (indicator V columns); with that mask plugged into the torch
    reference, forward and all three gradients must agree -- i.e. the three kernels regenerate the SAME mask."""
    B, heads, p_drop = 2, 4, 0.1
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (rt(torch.randn(B, L, D, generator=G(s))) for L, s in ((Lq, 11), (Lk, 12), (Lk, 13), (Lq, 14)))
    flat = lambda t, L: dev(bf(t.reshape(B * L, D)))
    seed, site = 987654321, 3
    pd = torch.zeros(B, heads, Lq, Lk)
    for c0 in range(0, Lk, hd):                                # V = indicator of keys [c0, c0+hd): ctx column c = pd[.., c0+c]
        vi = torch.zeros(B, Lk, heads, hd)
        for c in range(min(hd, Lk - c0)):
            vi[:, c0 + c, :, c] = 1.0
        ctx, _ = ops.attn_fwd(flat(q, Lq), flat(k, Lk), flat(vi.view(B, Lk, D), Lk), None, B, heads, Lq, Lk, scale, p_drop, seed, site)
        got = ctx.view(B, Lq, heads, hd).float().cpu().permute(0, 2, 1, 3)
        n = min(hd, Lk - c0)
        pd[..., c0:c0 + n] = got[..., :n]
    keep = (pd != 0).float()
    rate = float(keep.mean())
    assert abs(rate - (1 - p_drop)) < 0.01, rate
    # rows and columns are not systematically correlated
    assert float(keep.mean(-1).std()) < 0.06 and float(keep.mean(-2).std()) < 0.06
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    ref, p = _attn_ref(qg, kg, vg, None, heads, scale, keep, p_drop)
    close(pd, rt(p.detach()), 1e-2, 1e-4)
    ref.backward(do)
    ctx, stats = ops.attn_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, B, heads, Lq, Lk, scale, p_drop, seed, site)
    close(ctx.view(B, Lq, D), ref, 2e-2, 2e-2)
    dq, dk, dv = ops.attn_bwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, flat(do, Lq), stats, B, heads, Lq, Lk, scale, p_drop, seed, site)
    for got, want, L in ((dq, qg.grad, Lq), (dk, kg.grad, Lk), (dv, vg.grad, Lk)):
        w = want.reshape(B * L, D)
        assert float((got.float().cpu() - w).abs().max()) < 2e-2 * float(w.abs().max()) + 1e-3
        assert float((got.float().cpu() - w).abs().mean()) < 0.01 * float(w.abs().mean()) + 1e-4
    # a different site gives a different mask
    ctx2, _ = ops.attn_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, B, heads, Lq, Lk, scale, p_drop, seed, site + 1)
    assert not torch.equal(ctx, ctx2)


def _mask_battery(drop, p):
    """z-scores of a dropout mask tensor [planes, Q, K] (True = dropped) against independent Bernoulli(p) decisions: keep rate,
    serial correlations along keys / queries / planes (incl. the quad and word strides of the generator), the two diagonals, and
    the spread of per-row / per-column / per-plane drop rates.  (scratch/rng_study.py runs the same battery, plus byte-level
    chi-squares, on the CPU restatement of the generator and on numpy's PCG64.)"""
    d = drop.double() - p
    v = p * (1 - p)
    z = {"mean": float(d.mean()) / (v / d.numel()) ** 0.5}
    for l in (1, 2, 3, 4, 5, 8, 16, 64):
        if d.shape[2] > l:
            z[f"key+{l}"] = float((d[:, :, :-l] * d[:, :, l:]).mean()) / v * d[:, :, l:].numel() ** 0.5
    for l in (1, 2, 4, 16):
        if d.shape[1] > l:
            z[f"query+{l}"] = float((d[:, :-l] * d[:, l:]).mean()) / v * d[:, l:].numel() ** 0.5
    for l in (1, 2, 8):
        z[f"plane+{l}"] = float((d[:-l] * d[l:]).mean()) / v * d[l:].numel() ** 0.5
    z["diag"] = float((d[:, :-1, :-1] * d[:, 1:, 1:]).mean()) / v * d[:, 1:, 1:].numel() ** 0.5
    z["antidiag"] = float((d[:, :-1, 1:] * d[:, 1:, :-1]).mean()) / v * d[:, 1:, 1:].numel() ** 0.5
    for name, dims in (("rows", (2,)), ("cols", (1,)), ("planes", (1, 2))):
        m = drop.double().mean(dim=dims)
        n = drop.numel() // m.numel()
        z[name] = (float(m.var(unbiased=False)) / (v / n) - 1) * (m.numel() / 2) ** 0.5
    return z


@pytest.mark.parametrize("p_drop", [0.1, 0.35])
def test_attn_dropout_mask_statistics(ops, p_drop):
    """The attention-probability dropout generator (common.h Rng24: two full-rate 24-bit multiplies per four keys, a drop
    threshold per query row so that P(drop) = p and not p rounded to 1/256), judged on masks RECOVERED from the fused attention
    forward (uniform probabilities, indicator V columns): 2 x 16 planes x 256 x 256 = 2.1 M decisions per site, two sites (layers).
    Every statistic within 4.5 sigma (25 statistics x 2 sites: 3 sigma would fail one run in eight by chance); the keep rate
    itself within 3 sigma -- which also tells p = 0.1 from 26/256 = 0.1016 (15 sigma apart at this sample size)."""
    B, heads, L, hd = 2, 16, 256, 32
    D = heads * hd
    q = torch.zeros(B * L, D, device="cuda", dtype=torch.bfloat16)            # all logits 0: every probability 1 / L
    planes = []
    for site in (3, 4):
        pd = torch.zeros(B, heads, L, L)
        for c0 in range(0, L, hd):
            vi = torch.zeros(B, L, heads, hd)
            for c in range(hd):
                vi[:, c0 + c, :, c] = 1.0
            ctx, _ = ops.attn_fwd(q, q, dev(bf(vi.view(B * L, D))), None, B, heads, L, L, 1.0, p_drop, 20240607, site)
            pd[..., c0:c0 + hd] = ctx.view(B, L, heads, hd).float().cpu().permute(0, 2, 1, 3)
        drop = (pd == 0).view(B * heads, L, L)
        kept = pd[pd != 0]
        close(kept, torch.full_like(kept, 1.0 / L / (1 - p_drop)), 1e-2, 0)      # the survivors carry 1 / (1 - p), not 1 / (1 - t8 / 256)
        z = _mask_battery(drop, p_drop)
        assert abs(z["mean"]) < 3.0, (site, z)
        worst = max(z, key=lambda k: abs(z[k]))
        assert abs(z[worst]) < 4.5, (site, worst, z)
        planes.append(drop)
    # two sites (layers) draw unrelated masks
    a, b = planes[0].double() - p_drop, planes[1].double() - p_drop
    assert abs(float((a * b).mean()) / (p_drop * (1 - p_drop)) * a.numel() ** 0.5) < 4.0


def test_attn_fused_rejects_unsupported_shapes(ops):
    from mmdti_hip._abi import MMDTIError
    q = torch.zeros(300, 128, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(MMDTIError):
        ops.attn_fwd(q, q, q, None, 1, 2, 300, 300, 0.125)                # more than 256 keys
    q2 = torch.zeros(16, 96, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(MMDTIError):
        ops.attn_fwd(q2, q2, q2, None, 1, 2, 16, 16, 0.1)                  # head_dim 48


@pytest.mark.parametrize("rows", [4096 + 64 * 3, 3616, 1031, 1024 + 63, 8192 + 1])
def test_grouped_weight_gradients(ops, rows):
    """mmdti_linear_dw_grouped: the weight + bias gradients of several Linears over the same token rows in one launch (slab
    split-K, no atomics) == dy^T.x / column sums of dy in fp32, accumulated INTO the buffers; ineligible items fall back.
    Token counts that are not a multiple of the 64-deep K tile (small / ragged batches): the kernel zero-fills the tail of the
    last tile from a zero page -- 1 to 63 valid rows, in the last split only, rows past the end never read (the operands below
    are exact-size allocations followed by NaN-poisoned neighbours would not matter: they are never addressed)."""
    g = G(11)
    shapes = [(512, 2048), (2048, 512), (1536, 512), (512, 512), (256, 768)]
    from mmdti_hip import _abi
    from gemm_plan_helpers import grouped_plan
    (name, gx, gz, block, lds, sk, atomic, second_pass), _ = grouped_plan(_abi.lib(), shapes, rows)
    # 64 x 64 tiles up to 4096 rows; above, 256 x 256 tiles with K splits through slabs (K-tail instance for ragged row counts)
    if rows <= 4096:
        assert (name, gx, sk) == ("gemm_small_dw_grouped_kernel<3, false>", sum(a * b for a, b in shapes) // 4096, 1)
    else:
        assert (name, gx) == ("gemm_big_grouped_kernel<false, %s>" % str(rows % 64 != 0).lower(), sum(a * b for a, b in shapes) // 65536)
        assert sk > 1 and gz == sk and not atomic and second_pass
    items, refs = [], []
    for i, (no, ni) in enumerate(shapes):
        big = torch.randn(rows, no + 64, generator=g)          # dy as a column slice of a wider buffer (row stride != N_out)
        dy = bf(big).cuda()[:, :no] if i == 2 else bf(torch.randn(rows, no, generator=g)).cuda()
        x = bf(torch.randn(rows, ni, generator=g)).cuda()
        dw = torch.randn(no, ni, generator=g).cuda()
        db = torch.randn(no, generator=g).cuda() if i != 1 else None
        refs.append((dw.clone() + dy.float().t() @ x.float(), None if db is None else db.clone() + dy.float().sum(0)))
        items.append((dy, x, dw, db, None))
    # one item that the grouped kernel cannot take (N_in not a multiple of 256): must still be computed
    dy_s, x_s = bf(torch.randn(rows, 512, generator=g)).cuda(), bf(torch.randn(rows, 136, generator=g)).cuda()
    dw_s, db_s = torch.zeros(512, 136).cuda(), torch.zeros(512).cuda()
    items.append((dy_s, x_s, dw_s, db_s, None))
    refs.append((dy_s.float().t() @ x_s.float(), dy_s.float().sum(0)))
    ops.linear_bwd_weight_grouped(items)
    for (dy, x, dw, db, _), (rw, rb) in zip(items, refs):
        close(dw, rw, 2e-3, 2e-2)
        if db is not None:
            close(db, rb, 2e-3, 2e-2)


@pytest.mark.parametrize("rows", [1695, 1311, 513, 4096, 577, 130])
def test_grouped_weight_gradients_small_token_counts_are_reproducible(ops, rows):
    """Batches of 16-32 molecules (<= 4096 rows): the grouped weight gradients run on 64 x 64 tiles without a K split and add into
    dW by read-modify-write (gemm_small_dw_grouped_kernel) -- against fp32 torch, against the 256 x 256 split-K launch they
    replace, and bit-identical from run to run (one workgroup owns a tile; the split-K launch adds with fp32 atomics)."""
    from mmdti_hip import _abi
    lib = _abi.lib()
    g = G(12)
    shapes = [(1536, 512), (512, 512), (2048, 512), (512, 2048)]
    base = []
    for i, (no, ni) in enumerate(shapes):
        big = bf(torch.randn(rows, no + 64, generator=g)).cuda()
        dy = big[:, :no] if i == 0 else bf(torch.randn(rows, no, generator=g)).cuda()
        base.append((dy, bf(torch.randn(rows, ni, generator=g)).cuda(), torch.randn(no, ni, generator=g).cuda(),
                     torch.randn(no, generator=g).cuda() if i != 2 else None))

    def run():
        items = [(dy, x, dw.clone(), None if db is None else db.clone(), None) for dy, x, dw, db in base]
        ops.linear_bwd_weight_grouped(items)
        return [(it[2], it[3]) for it in items]

    from gemm_plan_helpers import grouped_plan
    assert grouped_plan(lib, shapes, rows)[0][0] == "gemm_small_dw_grouped_kernel<3, false>"      # the 64 x 64 kernel ...
    a, b = run(), run()
    for (dwa, dba), (dwb, dbb) in zip(a, b):
        assert torch.equal(dwa, dwb) and (dba is None or torch.equal(dba, dbb))
    try:
        lib.mmdti_set_option(b"gemm_small", 0)
        (name, gx, gz, block, lds, sk, atomic, second_pass), _ = grouped_plan(lib, shapes, rows)
        # ... against the 256 x 256 split-K launch with atomics
        assert (name, gx, atomic, second_pass) == ("gemm_big_grouped_kernel<false, %s>" % str(rows % 64 != 0).lower(), 48, 1, 0)
        c = run()
    finally:
        lib.mmdti_set_option(b"gemm_small", 1)
    for (dy, x, dw, db), (dwa, dba), (dwc, dbc) in zip(base, a, c):
        close(dwa, dw + dy.float().t() @ x.float(), 2e-3, 2e-2)
        close(dwa, dwc, 1e-4, 1e-2)                                 # (split-K order + atomics on the other side)
        if db is not None:
            close(dba, db + dy.float().sum(0), 2e-3, 2e-2)
            close(dba, dbc, 1e-4, 1e-2)


@pytest.mark.parametrize("rows", [3616, 200, 1000])
def test_weight_gradient_with_ragged_token_count(ops, rows):
    """Weight gradients over a token count that is not a multiple of the 64-deep K tile (small batches take the predicated
    kernel; a split into a bare-load main part + predicated tail was measured no faster in the step and dropped)."""
    g = G(rows)
    dy, x = bf(torch.randn(rows, 512, generator=g)).cuda(), bf(torch.randn(rows, 264, generator=g)).cuda()
    dw, db = torch.ones(512, 264).cuda(), torch.ones(512).cuda()
    ops.linear_bwd_weight(dy, x, dw, db=db)
    close(dw, 1.0 + dy.float().t() @ x.float(), 2e-3, 2e-2)
    close(db, 1.0 + dy.float().sum(0), 2e-3, 2e-2)
