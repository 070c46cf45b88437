"""Fused attention for 1 <= Lq, Lk <= 512 (mmdti_attn_long_fwd / _bwd) on the GPU.  The bounds are the ones the short kernels are held to
(tests/test_kernels_gpu.py, tests/test_packed_gpu.py, tests/test_modules_gpu.py): the rounding points are the same, and the only
length-dependent term -- fp32 accumulation over twice as many keys -- is orders below bf16's 2^-9 on the output.

The long kernels are the whole-row form (the short kernels' templates with 24 / 32 score tiles), so without dropout they are held
BIT-IDENTICAL to the short kernels on shapes both take."""
import math
from types import SimpleNamespace

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


def _attn_ref(q, k, v, add, heads, scale, keep=None, p_drop=0.0):
    """fp32 torch restatement on bf16-rounded operands (the oracle's mha minus the Linears)."""
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


def _grad_bounds(got, want):
    err = (got.float().cpu() - want).abs()
    assert float(err.max()) < 2e-2 * float(want.abs().max()) + 1e-3, float(err.max())
    assert float(err.mean()) < 0.01 * float(want.abs().mean()) + 1e-4, float(err.mean())


# ------------------------------------------------------------------------------------------- 1. kernel vs fp32 autograd
@pytest.mark.parametrize("B,heads,Lq,Lk,hd", [(2, 8, 512, 512, 64), (2, 4, 257, 257, 64), (2, 16, 258, 384, 32), (2, 16, 384, 258, 32),
                                              (1, 2, 1, 512, 32), (1, 2, 512, 1, 32), (2, 4, 300, 130, 16), (1, 4, 130, 300, 16),
                                              (2, 4, 161, 161, 64), (1, 4, 40, 500, 16)])
def test_attn_long_matches_reference(ops, B, heads, Lq, Lk, hd):
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
    ctx, stats = ops.attn_long_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), dev(add), B, heads, Lq, Lk, scale)
    close(ctx.view(B, Lq, D), ref, 2e-2, 2e-2)
    assert float((ctx.view(B, Lq, D).float().cpu() - ref.detach()).abs().mean()) < 3e-3
    dq, dk, dv = ops.attn_long_bwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), dev(add), flat(do, Lq), stats, B, heads, Lq, Lk, scale)
    for got, want, L in ((dq, qg.grad, Lq), (dk, kg.grad, Lk), (dv, vg.grad, Lk)):
        _grad_bounds(got, want.reshape(B * L, D))
    if Lk > 2:                                           # masked keys receive exactly zero gradient
        assert (dk.view(B, Lk, D)[0, Lk - Lk // 3:] == 0).all() and (dv.view(B, Lk, D)[0, Lk - Lk // 3:] == 0).all()


# ------------------------------------------------------------------------------------------- 2. one mask in all three kernels
def _recover_mask(ops, q, k, B, heads, Lq, Lk, hd, scale, p_drop, seed, site):
    """dropout(p) of the forward, read through indicator V columns: [B, heads, Lq, Lk]."""
    D = heads * hd
    pd = torch.zeros(B, heads, Lq, Lk)
    for c0 in range(0, Lk, hd):
        vi = torch.zeros(B, Lk, heads, hd)
        n = min(hd, Lk - c0)
        for c in range(n):
            vi[:, c0 + c, :, c] = 1.0
        ctx, _ = ops.attn_long_fwd(q, k, dev(bf(vi.view(B * Lk, D))), None, B, heads, Lq, Lk, scale, p_drop, seed, site)
        pd[..., c0:c0 + n] = ctx.view(B, Lq, heads, hd).float().cpu().permute(0, 2, 1, 3)[..., :n]
    return pd


@pytest.mark.parametrize("Lq,Lk,hd", [(300, 512, 64), (258, 384, 32), (512, 300, 16)])
def test_attn_long_dropout_mask_consistent(ops, Lq, Lk, hd):
    B, heads, p_drop = 2, 4, 0.1
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (rt(torch.randn(B, L, D, generator=G(s))) for L, s in ((Lq, 11), (Lk, 12), (Lk, 13), (Lq, 14)))
    flat = lambda t, L: dev(bf(t.reshape(B * L, D)))
    seed, site = 987654321, 3
    pd = _recover_mask(ops, flat(q, Lq), flat(k, Lk), B, heads, Lq, Lk, hd, scale, p_drop, seed, site)
    keep = (pd != 0).float()
    rate = float(keep.mean())
    assert abs(rate - (1 - p_drop)) < 0.01, rate
    assert float(keep.mean(-1).std()) < 0.06 and float(keep.mean(-2).std()) < 0.06
    qg, kg, vg = (t.clone().requires_grad_() for t in (q, k, v))
    ref, p = _attn_ref(qg, kg, vg, None, heads, scale, keep, p_drop)
    close(pd, rt(p.detach()), 1e-2, 1e-4)
    ref.backward(do)
    ctx, stats = ops.attn_long_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, B, heads, Lq, Lk, scale, p_drop, seed, site)
    close(ctx.view(B, Lq, D), ref, 2e-2, 2e-2)
    dq, dk, dv = ops.attn_long_bwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, flat(do, Lq), stats, B, heads, Lq, Lk, scale, p_drop, seed, site)
    for got, want, L in ((dq, qg.grad, Lq), (dk, kg.grad, Lk), (dv, vg.grad, Lk)):
        _grad_bounds(got, want.reshape(B * L, D))
    ctx2, _ = ops.attn_long_fwd(flat(q, Lq), flat(k, Lk), flat(v, Lk), None, B, heads, Lq, Lk, scale, p_drop, seed, site + 1)
    assert not torch.equal(ctx, ctx2)


def _mask_battery(drop, p):
    """z-scores of a dropout mask tensor [planes, Q, K] (True = dropped) against independent Bernoulli(p) decisions."""
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


def test_attn_long_dropout_mask_statistics(ops):
    """2 x 16 planes x 512 x 512 decisions at p = 0.1: keep rate within 3 sigma, every statistic within 4.5 sigma (the bounds, and
    their reason, of test_attn_dropout_mask_statistics: some 25 statistics, 3 sigma would fail by chance too often)."""
    B, heads, L, hd, p_drop = 2, 16, 512, 32, 0.1
    D = heads * hd
    q = torch.zeros(B * L, D, device="cuda", dtype=torch.bfloat16)            # all logits 0: every probability 1 / L
    pd = _recover_mask(ops, q, q, B, heads, L, L, hd, 1.0, p_drop, 20240607, 3)
    drop = (pd == 0).view(B * heads, L, L)
    kept = pd[pd != 0]
    close(kept, torch.full_like(kept, 1.0 / L / (1 - p_drop)), 1e-2, 0)
    z = _mask_battery(drop, p_drop)
    assert abs(z["mean"]) < 3.0, z
    worst = max(z, key=lambda k: abs(z[k]))
    assert abs(z[worst]) < 4.5, (worst, z)


# ------------------------------------------------------------------------------------------- 3. packed == masked dense
def _pack(lens, S):
    from mmdti_hip.packing import PackedRows
    return PackedRows(torch.tensor(lens), S, device="cuda")


@pytest.mark.parametrize("B,heads,hd,qlens,klens,Sq,Sk", [(3, 4, 64, (5, 258, 130), (512, 40, 300), 258, 512),
                                                          (3, 8, 32, (300, 512, 17), (300, 512, 17), 512, 512),
                                                          (2, 4, 16, (384, 100), (258, 257), 384, 258)])
def test_attn_long_packed_sequences_equal_masked_dense(ops, B, heads, hd, qlens, klens, Sq, Sk):
    """Packed sequences against the dense long kernels with an additive finfo.min mask on the padded keys, p = 0: every packed row's
    context, dq and the real rows' dk / dv equal bit for bit; the representative pad row of the key side receives dk = dv = 0."""
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    pq, pkk = _pack(qlens, Sq), _pack(klens, Sk)
    q = rt(torch.randn(B, Sq, D, generator=G(1)) * 1.5)
    k = rt(torch.randn(B, Sk, D, generator=G(2)) * 1.5)
    v = rt(torch.randn(B, Sk, D, generator=G(3)) * 1.5)
    do = rt(torch.randn(B, Sq, D, generator=G(4)))
    for b, n in enumerate(qlens):          # surplus padded query rows get no upstream gradient (the dense run then matches one pad row)
        do[b, n + 1:] = 0
    mask = torch.zeros(B, Sk)
    for b, n in enumerate(klens):
        mask[b, :n] = 1
    add = (1 - mask) * torch.finfo(torch.float32).min
    flat = lambda t, L: dev(bf(t.reshape(B * L, D)))
    qd, kd, vd, dod = flat(q, Sq), flat(k, Sk), flat(v, Sk), flat(do, Sq)
    vl = ops.AttnVarlen(pq, pkk)
    assert vl.Lq <= 512 and vl.Lk <= 512 and max(vl.Lq, vl.Lk) > 256
    ctx_d, st_d = ops.attn_long_fwd(qd, kd, vd, dev(add), B, heads, Sq, Sk, scale)
    ctx_p, st_p = ops.attn_long_fwd(qd[pq.gather].contiguous(), kd[pkk.gather].contiguous(), vd[pkk.gather].contiguous(), None, B, heads,
                                    vl.Lq, vl.Lk, scale, vl=vl)
    assert torch.equal(ctx_p, ctx_d[pq.gather])
    dq_d, dk_d, dv_d = ops.attn_long_bwd(qd, kd, vd, dev(add), dod, st_d, B, heads, Sq, Sk, scale)
    dq_p, dk_p, dv_p = ops.attn_long_bwd(qd[pq.gather].contiguous(), kd[pkk.gather].contiguous(), vd[pkk.gather].contiguous(), None,
                                         dod[pq.gather].contiguous(), st_p, B, heads, vl.Lq, vl.Lk, scale, vl=vl)
    assert bool(torch.isfinite(dk_p.float()).all()) and bool(torch.isfinite(dv_p.float()).all())
    assert torch.equal(dq_p, dq_d[pq.gather])
    assert torch.equal(dk_p, dk_d[pkk.gather]) and torch.equal(dv_p, dv_d[pkk.gather])
    for b, n in enumerate(klens):
        if n < Sk:
            row = int(pkk.off[b]) + n
            assert float(dk_p[row].float().abs().max()) == 0.0 and float(dv_p[row].float().abs().max()) == 0.0
    # against the fp32 reference on the packed data (per sequence)
    off_q, off_k = pq.off.cpu().tolist(), pkk.off.cpu().tolist()
    for b in range(B):
        nq, nk = min(qlens[b] + 1, Sq), klens[b]
        qg, kg, vg = (t[b:b + 1, :n].clone().requires_grad_() for t, n in ((q, nq), (k, nk), (v, nk)))
        ref, _ = _attn_ref(qg, kg, vg, None, heads, scale)
        ref.backward(do[b:b + 1, :nq])
        close(ctx_p[off_q[b]:off_q[b] + nq], ref[0], 2e-2, 2e-2)
        _grad_bounds(dq_p[off_q[b]:off_q[b] + nq], qg.grad[0])
        _grad_bounds(dk_p[off_k[b]:off_k[b] + nk], kg.grad[0])
        _grad_bounds(dv_p[off_k[b]:off_k[b] + nk], vg.grad[0])


# ------------------------------------------------------------------------------------------- 4. agreement with the short kernels
@pytest.mark.parametrize("B,heads,Lq,Lk,hd", [(2, 8, 256, 256, 64), (3, 16, 130, 256, 32), (2, 4, 37, 50, 16)])
def test_attn_long_equals_short_kernels_on_shared_shapes(ops, B, heads, Lq, Lk, hd):
    """Whole-row form: up to 256 keys the long entry points launch the short kernels' instantiations -- bit-identical, dropout
    included."""
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    q, k, v, do = (dev(bf(torch.randn(B * L, D, generator=G(s)) * 1.5)) for L, s in ((Lq, 1), (Lk, 2), (Lk, 3), (Lq, 4)))
    add = torch.zeros(B, Lk)
    add[0, Lk - Lk // 3:] = torch.finfo(torch.float32).min
    for p in (0.0, 0.1):
        c0, s0 = ops.attn_fwd(q, k, v, dev(add), B, heads, Lq, Lk, scale, p, 5, 2)
        c1, s1 = ops.attn_long_fwd(q, k, v, dev(add), B, heads, Lq, Lk, scale, p, 5, 2)
        assert torch.equal(c0, c1) and torch.equal(s0, s1)
        g0 = ops.attn_bwd(q, k, v, dev(add), do, s0, B, heads, Lq, Lk, scale, p, 5, 2)
        g1 = ops.attn_long_bwd(q, k, v, dev(add), do, s1, B, heads, Lq, Lk, scale, p, 5, 2)
        for a, b in zip(g0, g1):
            assert torch.equal(a, b)


@pytest.mark.parametrize("heads,hd,Lq,Lk_real,Lk_pad", [(8, 64, 256, 256, 512), (16, 32, 130, 200, 384), (4, 16, 64, 256, 300)])
def test_attn_long_tiles_past_the_keys_add_exact_zeros(ops, heads, hd, Lq, Lk_real, Lk_pad):
    """The 24- / 32-tile instantiations against the short kernels: the same keys followed by masked padding up to Lk_pad (dense,
    key_add = finfo.min) give, at p = 0, the short kernels' context, statistics, dq, dk and dv bit for bit."""
    B = 2
    D = heads * hd
    scale = 1.0 / math.sqrt(hd)
    q, do = (dev(bf(torch.randn(B * Lq, D, generator=G(s)) * 1.5)) for s in (1, 4))
    kp, vp = (bf(torch.randn(B, Lk_pad, D, generator=G(s)) * 1.5) for s in (2, 3))
    k, v = (dev(t[:, :Lk_real].reshape(B * Lk_real, D).contiguous()) for t in (kp, vp))
    add = torch.zeros(B, Lk_pad)
    add[:, Lk_real:] = torch.finfo(torch.float32).min
    c0, s0 = ops.attn_fwd(q, k, v, None, B, heads, Lq, Lk_real, scale)
    c1, s1 = ops.attn_long_fwd(q, dev(kp.view(-1, D)), dev(vp.view(-1, D)), dev(add), B, heads, Lq, Lk_pad, scale)
    assert torch.equal(c0, c1) and torch.equal(s0, s1)
    dq0, dk0, dv0 = ops.attn_bwd(q, k, v, None, do, s0, B, heads, Lq, Lk_real, scale)
    dq1, dk1, dv1 = ops.attn_long_bwd(q, dev(kp.view(-1, D)), dev(vp.view(-1, D)), dev(add), do, s1, B, heads, Lq, Lk_pad, scale)
    assert torch.equal(dq0, dq1)
    assert torch.equal(dk0.view(B, Lk_real, D), dk1.view(B, Lk_pad, D)[:, :Lk_real])
    assert torch.equal(dv0.view(B, Lk_real, D), dv1.view(B, Lk_pad, D)[:, :Lk_real])
    assert float(dk1.view(B, Lk_pad, D)[:, Lk_real:].float().abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- 5. rejections
def test_attn_long_rejects_unsupported_shapes(ops):
    from mmdti_hip._abi import MMDTIError
    z = lambda r, D: torch.zeros(r, D, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(MMDTIError, match="512"):
        ops.attn_long_fwd(z(16, 128), z(513, 128), z(513, 128), None, 1, 2, 16, 513, 0.125)          # 513 keys
    with pytest.raises(MMDTIError, match="512"):
        ops.attn_long_fwd(z(513, 128), z(16, 128), z(16, 128), None, 1, 2, 513, 16, 0.125)           # 513 queries
    with pytest.raises(MMDTIError):
        ops.attn_long_fwd(z(16, 96), z(16, 96), z(16, 96), None, 1, 2, 16, 16, 0.1)                  # head_dim 48
    st = torch.zeros(1, 2, 16, 2, device="cuda")
    with pytest.raises(MMDTIError, match="512"):
        ops.attn_long_bwd(z(16, 128), z(513, 128), z(513, 128), None, z(16, 128), st, 1, 2, 16, 513, 0.125)
    vl = ops.AttnVarlen(_pack((300, 20), 300), _pack((300, 20), 300))
    with pytest.raises(MMDTIError):                                                                  # key_add with packed offsets
        ops.attn_long_fwd(z(vl.q_rows, 128), z(vl.k_rows, 128), z(vl.k_rows, 128), torch.zeros(2, 300, device="cuda"), 2, 2, vl.Lq, vl.Lk,
                          0.125, vl=vl)
    with pytest.raises(MMDTIError):
        ops.attn_fwd(z(300, 128), z(300, 128), z(300, 128), None, 1, 2, 300, 300, 0.125)             # the short op keeps its limit


# ------------------------------------------------------------------------------------------- 6. tower 2 at 300 and 512 tokens
def rel_l2(a, b):
    a, b = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _tower(cfg, seed=5):
    import mmdti_hip.models.bert_layers as bl
    torch.manual_seed(seed)
    return bl.RobertaTower(cfg).cuda().eval()


def _spy_layers(monkeypatch):
    from mmdti_hip import functional as Fn
    seen = []
    inner = Fn._bert_layer_fwd

    def spy(*a, **kw):
        r = inner(*a, **kw)
        seen.append(r[0])
        return r
    monkeypatch.setattr(Fn, "_bert_layer_fwd", spy)
    return seen


@pytest.mark.parametrize("L", [300, 512])
@pytest.mark.parametrize("heads,fused", [(2, True), (4, True), (2, False)])
def test_roberta_tower_long_sequences_vs_oracle(monkeypatch, L, heads, fused):
    """Tower 2 above 256 tokens: fused kernels (head_dim 64 / 32) and, with FUSED_ATTN off, the materialised-scores path, against the
    oracle's bf16 mode at the bounds of test_roberta_tower_fused_attention_vs_oracle; the path that ran is asserted."""
    from mmdti_hip import ops
    cfg = SimpleNamespace(layers=2, dim=128, heads=heads, ffn=256, vocab=60, max_pos=514, type_vocab=1, pad_idx=1, ln_eps=1e-12,
                          hidden_dropout=0.1, attn_dropout=0.1)
    tower = _tower(cfg)
    P = {"bert." + k: v.detach().cpu().clone().requires_grad_() for k, v in tower.state_dict().items()}
    gen = torch.Generator().manual_seed(3)
    ids = torch.randint(4, 60, (2, L), generator=gen)
    am = torch.ones(2, L, dtype=torch.long)
    ids[1, L - 37:], am[1, L - 37:] = 1, 0
    seen = _spy_layers(monkeypatch)
    monkeypatch.setattr(ops, "FUSED_ATTN", fused)
    out = tower(ids.cuda(), am.cuda(), return_dict=True)[0]
    assert len(seen) == 2 and all(bool(l.fused) == fused for l in seen), [l.fused for l in seen]
    ocfg = O.RobertaCfg(layers=2, dim=128, heads=heads, ffn=256, vocab=60, max_pos=514, pad_idx=1)
    ob = O.roberta_encoder(ids, am, P, ocfg, bf16=True)
    assert rel_l2(out, ob) <= 2e-3, rel_l2(out, ob)
    gout = torch.randn(out.shape, generator=gen)
    (out * gout.cuda()).sum().backward()
    (ob * gout).sum().backward()
    for n, p in tower.named_parameters():
        ref = P["bert." + n].grad
        if p.grad is None or ref is None or "pooler" in n or "key.bias" in n:
            continue
        if ref.abs().max() == 0:
            assert p.grad.abs().max().item() < 1e-6, n
            continue
        assert rel_l2(p.grad, ref) <= 5e-2, (n, rel_l2(p.grad, ref))


# ------------------------------------------------------------------------------------------- 10. memory
def test_long_fused_attention_keeps_less_memory_than_materialised(monkeypatch):
    """Tower 2 forward + backward at B = 32, L = 512: the fused run's peak allocated bytes are strictly below the materialised run's
    (which keeps two bf16 [B, heads, L, ld] tensors per layer for the backward)."""
    from mmdti_hip import ops
    cfg = SimpleNamespace(layers=2, dim=128, heads=2, ffn=256, vocab=60, max_pos=514, type_vocab=1, pad_idx=1, ln_eps=1e-12,
                          hidden_dropout=0.1, attn_dropout=0.1)
    tower = _tower(cfg)
    ids = torch.randint(4, 60, (32, 512), generator=G(3)).cuda()
    am = torch.ones(32, 512, dtype=torch.long, device="cuda")
    peak = {}
    for fused in (True, False, True):                  # (first pass warms caches up; the last two are compared)
        monkeypatch.setattr(ops, "FUSED_ATTN", fused)
        tower.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = tower(ids, am, return_dict=True)[0]
        out.float().square().mean().backward()
        torch.cuda.synchronize()
        peak[fused] = torch.cuda.max_memory_allocated()
        del out
    print(f"peak allocated bytes: fused {peak[True]}, materialised {peak[False]}")
    assert peak[True] < peak[False], peak


# ------------------------------------------------------------------------------------------- 7. cross block, 258 atoms x 384 tokens
def _lens_mask(lens, L):
    m = torch.zeros(len(lens), L)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("Lq,Lk,ql,kl", [(258, 384, (258, 40, 131), (384, 77, 300)), (384, 258, (384, 300, 19), (258, 131, 40))])
def test_cross_block_long_vs_oracle(Lq, Lk, ql, kl, packed):
    """The cross-modal layer at the reference's largest molecule (258 rows with BOS / EOS) against 384 tokens, both directions,
    dim 512 / 16 heads, against the oracle's co-attention layer in bf16 mode at the bounds test_cross_encoder_golden holds the
    layer to (output 2e-3, input gradients 4e-2, parameter gradients 5e-2 without key.bias, whose gradient is analytically zero)."""
    import mmdti_hip.models.bert_layers as bl
    from mmdti_hip.packing import PackedRows
    D, heads, ffn, B = 512, 16, 256, 3
    ccfg = SimpleNamespace(hidden_size=D, num_attention_heads=heads, intermediate_size=ffn, attention_probs_dropout_prob=0.2,
                           hidden_dropout_prob=0.3, hidden_act="gelu", layer_norm_eps=1e-12)
    torch.manual_seed(9)
    enc = bl.BertCrossEncoder(ccfg, 1).cuda().eval()
    P = {k: v.detach().cpu().clone().requires_grad_() for k, v in enc.state_dict().items() if v.is_floating_point()}
    g = G(11)
    s1, s2 = torch.randn(B, Lq, D, generator=g), torch.randn(B, Lk, D, generator=g)
    mask2 = _lens_mask(kl, Lk)
    gout = torch.randn(B, Lq, D, generator=g)
    s1o, s2o = s1.clone().requires_grad_(), s2.clone().requires_grad_()
    ob = O.cross_layer(s1o, s2o, (1.0 - mask2) * -10000.0, P, "layer.0.", O.CrossCfg(dim=D, heads=heads, ffn=ffn), bf16=True)
    if packed:
        pq, pk = PackedRows(torch.tensor(ql), Lq, "cuda"), PackedRows(torch.tensor(kl), Lk, "cuda")
        a = s1.cuda().reshape(B * Lq, D)[pq.gather].clone().requires_grad_()
        b_ = s2.cuda().reshape(B * Lk, D)[pk.gather].clone().requires_grad_()
        out = enc(a, b_, None, packs=(pq, pk))[-1]
        gq, gk = pq.gather_host, pk.gather_host
        w = gout.reshape(B * Lq, D)[gq]
        dense_w = torch.zeros(B * Lq, D)
        dense_w[gq] = w                                    # the padded rows a packed batch does not hold get no upstream gradient
        assert rel_l2(out, ob.reshape(B * Lq, D)[gq]) <= 2e-3
        (out * w.cuda()).sum().backward()
        (ob * dense_w.view(B, Lq, D)).sum().backward()
        assert rel_l2(a.grad, s1o.grad.reshape(B * Lq, D)[gq]) <= 4e-2
        assert rel_l2(b_.grad, s2o.grad.reshape(B * Lk, D)[gk]) <= 4e-2
    else:
        a, b_ = s1.cuda().requires_grad_(), s2.cuda().requires_grad_()
        ext = ((1.0 - mask2) * -10000.0).view(B, 1, 1, Lk).cuda()
        out = enc(a, b_, ext)[-1]
        assert rel_l2(out, ob) <= 2e-3
        (out * gout.cuda()).sum().backward()
        (ob * gout).sum().backward()
        assert rel_l2(a.grad, s1o.grad) <= 4e-2 and rel_l2(b_.grad, s2o.grad) <= 4e-2
    for n, p in enc.named_parameters():
        ref = P[n].grad
        if p.grad is None or ref is None or "key.bias" in n:
            continue
        assert rel_l2(p.grad, ref) <= 5e-2, (n, rel_l2(p.grad, ref))


# ------------------------------------------------------------------------------------------- 8. sequencers at L = 384
LENS_384 = [384, 300, 257, 120, 350, 290]


def _tower_inputs(lens, L, vocab=40):
    ids = torch.randint(4, vocab, (len(lens), L), generator=G(3))
    am = _lens_mask(lens, L).long()
    ids[am == 0] = 1
    return ids, am


def _same_grads(g0, g1):
    """Parameter gradients of two runs: equal bit for bit where no atomic is involved; the grouped / split-K weight-gradient and
    one-hot embedding GEMMs accumulate with atomics, whose order is not fixed from run to run -- there the mirrored tests
    (tests/test_modules_gpu.py) hold 2e-4 relative, and so does this one."""
    assert set(g0) == set(g1)
    worst = ("", 0.0)
    for n in g0:
        d = float((g0[n].double() - g1[n].double()).norm()) / (float(g0[n].double().norm()) + 1e-30)
        worst = max(worst, (n, d), key=lambda t: t[1])
        assert d < 2e-4, (n, d)
    print("worst parameter-gradient difference between the two paths:", worst)


@pytest.mark.parametrize("packed", [False, True])
def test_bert_layer_sequenced_in_the_library_at_384_tokens(packed, monkeypatch):
    """test_bert_layer_sequenced_in_the_library_equals_the_op_by_op_path with only the lengths raised: L = 384, dropout on."""
    import mmdti_hip.models.bert_layers as bl
    from mmdti_hip import functional as Fn, paths
    from mmdti_hip.runtime import dropout_state, ParamArena
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.trainer import _qkv_groups
    cfg = SimpleNamespace(layers=2, dim=512, heads=8, ffn=256, vocab=40, max_pos=514, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1, attn_dropout=0.1)
    tower = bl.RobertaTower(cfg).cuda().train()
    arena = ParamArena(tower.parameters(), adjacent=_qkv_groups(tower))
    L = 384
    ids, am = _tower_inputs(LENS_384, L)
    pk = PackedRows(torch.tensor(LENS_384), L, "cuda") if packed else None
    calls, layer_paths = [], []
    monkeypatch.setattr(Fn, "STACK_SEQ", False)
    real_f, real_b, real_l = Fn._bert_layer_fwd_seq, Fn._bert_layer_bwd_seq, Fn._bert_layer_fwd
    monkeypatch.setattr(Fn, "_bert_layer_fwd_seq", lambda *a, **k: (calls.append("f"), real_f(*a, **k))[1])
    monkeypatch.setattr(Fn, "_bert_layer_bwd_seq", lambda *a, **k: (calls.append("b"), real_b(*a, **k))[1])

    def spy(*a, **k):
        r = real_l(*a, **k)
        layer_paths.append(r[0].path)
        return r
    monkeypatch.setattr(Fn, "_bert_layer_fwd", spy)

    def run(seq):
        monkeypatch.setattr(Fn, "LAYER_SEQ", seq)
        arena.zero_grad()
        dropout_state.reseed(777)
        out = tower(ids.cuda(), am.cuda(), return_dict=True, pack=pk)[0]
        w = torch.randn(out.shape, generator=G(5)).cuda()
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.clone() for n, p in tower.named_parameters() if p.grad is not None}

    o1, g1 = run(True)
    assert layer_paths == [paths.LAYER] * 2 and calls.count("f") == 2 and calls.count("b") == 2, (layer_paths, calls)
    del calls[:], layer_paths[:]
    o0, g0 = run(False)
    assert layer_paths == [paths.OPS] * 2 and not calls
    assert torch.equal(o0, o1)
    _same_grads(g0, g1)


@pytest.mark.parametrize("packed", [False, True])
def test_bert_stack_sequenced_in_the_library_at_384_tokens(packed, monkeypatch):
    """test_bert_stack_sequenced_in_the_library_equals_the_per_layer_calls with only the lengths raised (2304 rows < STACK_MAX_ROWS)."""
    import mmdti_hip.models.bert_layers as bl
    from mmdti_hip import functional as Fn
    from mmdti_hip.runtime import dropout_state, ParamArena
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.trainer import _qkv_groups
    cfg = SimpleNamespace(layers=3, dim=512, heads=8, ffn=256, vocab=40, max_pos=514, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1, attn_dropout=0.1)
    tower = bl.RobertaTower(cfg).cuda().train()
    arena = ParamArena(tower.parameters(), adjacent=_qkv_groups(tower))
    L = 384
    ids, am = _tower_inputs(LENS_384, L)
    assert len(LENS_384) * L < Fn.STACK_MAX_ROWS
    pk = PackedRows(torch.tensor(LENS_384), L, "cuda") if packed else None
    calls = []
    real_f, real_b, real_lf = Fn._bert_stack_fwd, Fn._bert_stack_bwd, Fn._bert_layer_fwd_seq
    monkeypatch.setattr(Fn, "_bert_stack_fwd", lambda *a, **k: (calls.append("F"), real_f(*a, **k))[1])
    monkeypatch.setattr(Fn, "_bert_stack_bwd", lambda *a, **k: (calls.append("B"), real_b(*a, **k))[1])
    monkeypatch.setattr(Fn, "_bert_layer_fwd_seq", lambda *a, **k: (calls.append("l"), real_lf(*a, **k))[1])

    def run(stack, layer=True):
        monkeypatch.setattr(Fn, "STACK_SEQ", stack)
        monkeypatch.setattr(Fn, "LAYER_SEQ", layer)
        arena.zero_grad()
        dropout_state.reseed(777)
        out = tower(ids.cuda(), am.cuda(), return_dict=True, pack=pk)[0]
        w = torch.randn(out.shape, generator=G(5)).cuda()
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), {n: p.grad.clone() for n, p in tower.named_parameters() if p.grad is not None}

    o1, g1 = run(True)
    assert calls == ["F", "B"], calls                      # the path that ran: STACK
    del calls[:]
    o0, g0 = run(False)
    assert calls == ["l"] * 3
    del calls[:]
    o2, g2 = run(False, layer=False)                       # ... and op by op
    assert not calls
    assert torch.equal(o0, o1) and torch.equal(o2, o1)
    _same_grads(g0, g1)
    _same_grads(g2, g1)


@pytest.mark.parametrize("packed", [False, True])
def test_cross_layer_sequenced_in_the_library_at_258_x_384(packed, monkeypatch):
    """test_cross_layer_sequenced_in_the_library_equals_the_op_by_op_path with only the lengths raised: 258 queries x 384 keys."""
    import mmdti_hip.models.bert_layers as bl
    from mmdti_hip import functional as Fn
    from mmdti_hip.runtime import dropout_state, ParamArena
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.trainer import _qkv_groups
    D, heads, ffn = 512, 16, 256
    ccfg = SimpleNamespace(hidden_size=D, num_attention_heads=heads, intermediate_size=ffn, attention_probs_dropout_prob=0.1, hidden_dropout_prob=0.1,
                           hidden_act="gelu", layer_norm_eps=1e-12)
    torch.manual_seed(4)
    enc = bl.BertCrossEncoder(ccfg, 1).cuda().train()
    arena = ParamArena(enc.parameters(), adjacent=_qkv_groups(enc))
    B, Lq, Lk = 5, 258, 384
    ql, kl = [258, 17, 133, 8, 257], [384, 300, 41, 5, 384]
    g = G(11)
    s1, s2 = torch.randn(B, Lq, D, generator=g), torch.randn(B, Lk, D, generator=g)
    ext = ((1.0 - _lens_mask(kl, Lk)) * -10000.0).view(B, 1, 1, Lk).cuda()
    pq, pk = (PackedRows(torch.tensor(ql), Lq, "cuda"), PackedRows(torch.tensor(kl), Lk, "cuda")) if packed else (None, None)
    calls = []
    rf, rb = Fn._bert_cross_layer_fwd_seq, Fn._bert_cross_layer_bwd_seq
    monkeypatch.setattr(Fn, "_bert_cross_layer_fwd_seq", lambda *a, **k: (calls.append("f"), rf(*a, **k))[1])
    monkeypatch.setattr(Fn, "_bert_cross_layer_bwd_seq", lambda *a, **k: (calls.append("b"), rb(*a, **k))[1])

    def run(seq):
        monkeypatch.setattr(Fn, "LAYER_SEQ", seq)
        arena.zero_grad()
        dropout_state.reseed(31)
        if packed:
            a = s1.cuda().reshape(B * Lq, D)[pq.gather].clone().requires_grad_()
            b_ = s2.cuda().reshape(B * Lk, D)[pk.gather].clone().requires_grad_()
            out = enc(a, b_, None, packs=(pq, pk))[-1]
        else:
            a, b_ = s1.cuda().clone().requires_grad_(), s2.cuda().clone().requires_grad_()
            out = enc(a, b_, ext)[-1]
        w = torch.randn(out.shape, generator=G(5)).cuda()
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach().clone(), a.grad.clone(), b_.grad.clone(), {n: prm.grad.clone() for n, prm in enc.named_parameters() if prm.grad is not None}

    o1, da1, db1, g1 = run(True)
    assert calls == ["f", "b"], calls                      # the path that ran: LAYER
    del calls[:]
    o0, da0, db0, g0 = run(False)
    assert not calls
    assert torch.equal(o0, o1) and torch.equal(da0, da1) and torch.equal(db0, db1)
    _same_grads(g0, g1)


# ------------------------------------------------------------------------------------------- 9. whole model
def _long_batch(ocfg, sizes, seed=21):
    """A right-padded batch whose members have the given (atoms, tokens): one synth_batch member each, padded as the reference's
    collater pads (token / edge pad index, distance 0, RoBERTa pad id)."""
    u, r = ocfg.unimol, ocfg.roberta
    parts = [O.synth_batch(1, na, nt, ocfg, seed=seed + i, ragged=False) for i, (na, nt) in enumerate(sizes)]
    N = max(p[0]["src_tokens"].shape[1] for p in parts)
    L = max(p[0]["input_ids"].shape[1] for p in parts)
    B = len(parts)
    batch = {"src_tokens": torch.full((B, N), u.pad_idx, dtype=parts[0][0]["src_tokens"].dtype),
             "src_distance": torch.zeros(B, N, N, dtype=parts[0][0]["src_distance"].dtype),
             "src_edge_type": torch.full((B, N, N), u.pad_idx, dtype=parts[0][0]["src_edge_type"].dtype),
             "input_ids": torch.full((B, L), r.pad_idx, dtype=torch.int64)}
    for b, (p, _) in enumerate(parts):
        n, l = p["src_tokens"].shape[1], p["input_ids"].shape[1]
        batch["src_tokens"][b, :n] = p["src_tokens"][0]
        batch["src_distance"][b, :n, :n] = p["src_distance"][0]
        batch["src_edge_type"][b, :n, :n] = p["src_edge_type"][0]
        batch["input_ids"][b, :l] = p["input_ids"][0]
    batch["attention_mask"] = batch["input_ids"].ne(r.pad_idx).long()
    return batch, torch.cat([p[1] for p in parts])


LONG_SIZES = [(256, 512), (40, 300), (100, 60), (256, 400), (17, 257)]      # 258 rows with BOS / EOS; 300-512 tokens among shorter ones


def _small_refarch(task):
    from g9util import refarch_cfg, product_model, load_fixture_weights
    ocfg = refarch_cfg(task, 600)
    ocfg.unimol.layers, ocfg.roberta.layers = 2, 2
    model = product_model(ocfg).cuda()
    P = O.init_params(ocfg, seed=5, std=0.05)
    load_fixture_weights(model, P)
    return ocfg, model, P


def _host_fields(batch):
    from mmdti_hip.collate import device_payload
    full = device_payload(batch)
    return {k: full[k] for k in ("atom_counts", "token_counts", "token_pad_id", "packable")}


def test_whole_model_runs_packed_with_258_atoms_and_512_tokens():
    """The reference's widths at reduced depth (tests/test_packed_gpu.py's architecture), a mixed-length batch with 258-row and 300-512-token
    members: eval picks the packed layout; at dropout 0 the packed step equals the strict_reference (padded) step at the bounds of
    test_packed_step_equals_padded_step_at_dropout_zero; the losses are within 1e-3 of the oracle's (tests/test_configs_gpu.py)."""
    from mmdti_hip.functional import CELossFn
    task = "classification"
    ocfg, model, P = _small_refarch(task)
    batch, label = _long_batch(ocfg, LONG_SIZES)
    assert batch["src_tokens"].shape[1] == 258 and batch["input_ids"].shape[1] == 512
    host = _host_fields(batch)
    assert host["packable"]
    d = {k: v.cuda() for k, v in batch.items()}
    tgt = label.cuda().long()
    model.eval()
    with torch.no_grad():
        model(**d, **host)
    assert model.last_layout == "packed"
    model.train()                                           # every dropout probability is 0
    res = {}
    for layout in ("padded", "packed"):
        model.zero_grad(set_to_none=True)
        model.strict_reference = layout == "padded"
        logits, infonce, ct = model(**d, **host, return_infonce_loss=True, return_ct_loss=True, net_target=tgt)
        assert model.last_layout == layout
        loss = CELossFn.apply(logits, tgt) + 0.1 * infonce + 0.1 * ct
        loss.backward()
        torch.cuda.synchronize()
        res[layout] = dict(logits=logits.detach().clone(), infonce=float(infonce), ct=float(ct), loss=float(loss),
                           grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    a, b = res["padded"], res["packed"]
    for k in ("infonce", "ct", "loss"):
        rel = 3e-5 if k == "ct" else 1e-6
        print(k, a[k], b[k])
        assert abs(a[k] - b[k]) <= rel * abs(a[k]) + 1e-7, (k, a[k], b[k])
    assert rel_l2(b["logits"], a["logits"]) < 1e-6
    assert set(a["grads"]) == set(b["grads"])
    for n in a["grads"]:
        if float(a["grads"][n].abs().max()) < 1e-9 or any(z in n for z in ("pooler", "key.bias", "gbf_proj.linear2.bias")):
            continue
        r = rel_l2(b["grads"][n], a["grads"][n])
        assert r < (4e-2 if n.startswith(("gbf.", "gbf_proj.")) else 6e-3), (n, r)
    with torch.no_grad():
        out = O.mm_forward(batch, P, ocfg, net_target=label, bf16=True)
        ref, _ = O.step_loss(out, label, task)
    print("loss packed", b["loss"], "oracle", float(ref), "infonce", b["infonce"], float(out["infonce"]))
    assert abs(b["loss"] - float(ref)) <= 1e-3 * abs(float(ref)), (b["loss"], float(ref))
    assert abs(b["infonce"] - float(out["infonce"])) <= 1e-3 * abs(float(out["infonce"]))


def test_long_packed_step_has_no_host_synchronisation():
    """test_step_has_no_host_synchronisation's sync-debug region around one packed training step of the same long batch."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.collate import device_payload, to_device
    task = "classification"
    ocfg, model, _ = _small_refarch(task)
    batch, label = _long_batch(ocfg, LONG_SIZES)
    lab = label.cuda()
    tuner = FineTuner(model.train(), task)
    tuner.model.strict_reference = False
    resident = lambda: to_device(device_payload(batch), "cuda")
    for _ in range(2):
        tuner.step(resident(), lab)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = tuner.step(resident(), lab)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(out.loss).item()
    assert tuner.model.last_layout == "packed"
