"""The deterministic mode on the device: every fixed-order site, through ops.*, with the mode on.

"Bit-identical" always means FIVE launches on the same inputs, each torch.equal to the first (one lucky pair proves little; the shapes
make hundreds of partial sums meet per element).

Float64 reference bound.  A fixed-order fp32 sum of n terms may sit (n + c) * 2^-24 * sum|term_i| from the float64 sum, c = the roundings
per term inside the kernel (1 for a plain add).  Each test states its n and c; a destination that is accumulated into (`+=`) is one term
more.  Nothing here is tuned to what a kernel gives."""
import numpy as np
import pytest
import torch

from mmdti_hip import ops
from mmdti_hip._abi import MMDTIError

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
RUNS = 5


@pytest.fixture(autouse=True)
def det_mode():
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


def f64(t):
    return t.detach().float().cpu().double().numpy()


def assert_within(got, ref, abs_terms, n, c, what):
    """|got - ref| <= (n + c) * 2^-24 * sum|terms|, element by element"""
    bound = (n + c) * U * abs_terms
    err = np.abs(f64(got) - ref)
    worst = float((err - bound).max())
    assert worst <= 0, f"{what}: error exceeds the bound by {worst:.3e} (max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e})"


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_case(rows, D, dy_bf16, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, D, device="cuda", generator=g) * 1.5 + 0.3
    gamma = torch.randn(D, device="cuda", generator=g) * 0.5 + 1.0
    beta = torch.randn(D, device="cuda", generator=g) * 0.1
    dy = torch.randn(rows, D, device="cuda", generator=g)
    if dy_bf16:
        dy = dy.bfloat16()
    _, _, mean, rstd = ops.layernorm_fwd(x, gamma, beta, 1e-5, want_f32=False, want_bf16=True)
    pre = [torch.randn(D, device="cuda", generator=g) for _ in range(3)]          # non-zero dgamma / dbeta / colsum to accumulate into
    return x, gamma, dy, mean, rstd, pre


def _ln_run(x, gamma, dy, mean, rstd, pre, copy):
    dg, db, cs = (p.clone() for p in pre)
    out = ops.layernorm_bwd(dy, x, gamma, mean, rstd, dg, db, bf16_copy=(0.0, 0, cs) if copy else None)
    dx, dx16 = out if copy else (out, None)
    torch.cuda.synchronize()
    return dx, dx16, dg, db, cs


@pytest.mark.parametrize("copy", [False, True], ids=["plain", "bf16copy+colsum"])
@pytest.mark.parametrize("dy_bf16", [True, False], ids=["dy_bf16", "dy_f32"])
@pytest.mark.parametrize("rows", [37, 12805])           # 3 workgroups (the last partial) / 641 (D = 512), 458 (D = 1024)
@pytest.mark.parametrize("D", [512, 1024])              # the 3- and the 2-workgroups-per-CU variants
def test_layernorm_bwd_fixed_order(D, rows, dy_bf16, copy):
    case = _ln_case(rows, D, dy_bf16, seed=rows + D)
    x, gamma, dy, mean, rstd, pre = case
    ops.set_deterministic(False)
    dx_default = _ln_run(*case, copy)[0]
    ops.set_deterministic(True)
    first = _ln_run(*case, copy)
    for _ in range(RUNS - 1):
        again = _ln_run(*case, copy)
        for a, b in zip(first, again):
            assert (a is None and b is None) or torch.equal(a, b)
    dx, dx16, dg, db, cs = first
    assert torch.equal(dx, dx_default)                   # that part of the kernel does not change with the mode
    # float64 reference from the SAME fp32 mean / rstd the kernel reads
    xh = (f64(x) - f64(mean)[:, None]) * f64(rstd)[:, None]
    d = f64(dy)
    # dgamma: n = rows + 1 terms (the accumulated-into value is one); c = 4: x - mean, * rstd, dy * xhat, the add
    assert_within(dg, f64(pre[0]) + (d * xh).sum(0), np.abs(f64(pre[0])) + np.abs(d * xh).sum(0), rows + 1, 4, "dgamma")
    # dbeta: n = rows + 1, c = 1 (bf16 -> fp32 is exact)
    assert_within(db, f64(pre[1]) + d.sum(0), np.abs(f64(pre[1])) + np.abs(d).sum(0), rows + 1, 1, "dbeta")
    if copy:
        # the column sums are those of the ROUNDED bf16 copy: n = rows + 1, c = 1
        v = f64(dx16)
        assert_within(cs, f64(pre[2]) + v.sum(0), np.abs(f64(pre[2])) + np.abs(v).sum(0), rows + 1, 1, "dx_colsum")
    else:
        assert torch.equal(cs, pre[2])


@pytest.mark.parametrize("rows,D", [(37, 512), (12805, 1024)])
def test_layernorm_bwd_keeps_plus_equals_exactly_for_a_zero_dy(rows, D):
    x, gamma, dy, mean, rstd, pre = _ln_case(rows, D, True, seed=5)
    dx, dx16, dg, db, cs = _ln_run(x, gamma, torch.zeros_like(dy), mean, rstd, pre, True)
    assert torch.equal(dg, pre[0]) and torch.equal(db, pre[1]) and torch.equal(cs, pre[2])
    assert not dx.any()


# ------------------------------------------------------------------------------------------------ weight and bias gradients
def _dw_case(shapes, rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    items = []
    for n_out, n_in in shapes:
        # (row stride a multiple of 8 elements, as every activation of the model has: a 50-wide dy is a view of 56-wide rows)
        dy = (torch.randn(rows, (n_out + 7) // 8 * 8, device="cuda", generator=g) * 0.5).bfloat16()[:, :n_out]
        x = torch.randn(rows, n_in, device="cuda", generator=g).bfloat16()
        dw0 = torch.randn(n_out, n_in, device="cuda", generator=g)
        db0 = torch.randn(n_out, device="cuda", generator=g)
        items.append((dy, x, dw0, db0))
    return items


def _dw_check(items, rows, outs):
    for (dy, x, dw0, db0), (dw, db) in zip(items, outs):
        a, b = f64(dy), f64(x)                            # bf16 operands: every product is exact in fp32
        # dw: n = rows + 1 terms (dw0 is one), c = 1 (the accumulate); db: the same over the column of dy
        assert_within(dw, f64(dw0) + a.T @ b, np.abs(f64(dw0)) + np.abs(a).T @ np.abs(b), rows + 1, 1, "dw")
        assert_within(db, f64(db0) + a.sum(0), np.abs(f64(db0)) + np.abs(a).sum(0), rows + 1, 1, "db")


@pytest.mark.parametrize("n_out,n_in,rows", [(256, 256, 4160), (50, 512, 333)], ids=["256x256-4160rows", "50x512-333rows-Ktail"])
def test_linear_bwd_weight_fixed_order(n_out, n_in, rows):
    items = _dw_case([(n_out, n_in)], rows, seed=rows)
    dy, x, dw0, db0 = items[0]

    def run():
        dw, db = dw0.clone(), db0.clone()
        ops.linear_bwd_weight(dy, x, dw, db=db)
        torch.cuda.synchronize()
        return dw, db

    first = run()
    for _ in range(RUNS - 1):
        again = run()
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    _dw_check(items, rows, [first])


@pytest.mark.parametrize("rows", [4160, 192], ids=["4160rows-big-slabs", "192rows-small"])
def test_linear_bwd_weight_grouped_fixed_order(rows):
    items = _dw_case([(256, 256), (512, 256)], rows, seed=rows + 1)

    def run():
        outs = [(dw0.clone(), db0.clone()) for _, _, dw0, db0 in items]
        ops.linear_bwd_weight_grouped([(dy, x, dw, db, None) for (dy, x, _, _), (dw, db) in zip(items, outs)])
        torch.cuda.synchronize()
        return outs

    first = run()
    for _ in range(RUNS - 1):
        for (a, b), (c, d) in zip(first, run()):
            assert torch.equal(a, c) and torch.equal(b, d)
    _dw_check(items, rows, first)


# ------------------------------------------------------------------------------------------------ embedding gradients / column sums
def _emb_case(V, D=512, n=318, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    vals = torch.tensor([0, 2, 5, 11, 17, 23, 30][: max(2, min(7, V))], device="cuda") % V      # padding (0) + 6 values
    ids = vals[torch.randint(0, len(vals), (n,), device="cuda", generator=g)]
    dout = torch.randn(n, D, device="cuda", generator=g)
    return ids, dout, torch.randn(V, D, device="cuda", generator=g)


@pytest.mark.parametrize("V", [31, 1])
def test_embedding_bwd_gemm_fixed_order(V):
    ids, dout, t0 = _emb_case(V)
    d16 = dout.bfloat16()

    def run():
        t = t0.clone()
        ops.embedding_bwd_gemm(ids, d16, t, padding_idx=0 if V > 1 else -1)
        torch.cuda.synchronize()
        return t

    first = run()
    for _ in range(RUNS - 1):
        assert torch.equal(first, run())
    ref = f64(t0).copy()
    terms = np.abs(f64(t0))
    idc, d = ids.cpu().numpy(), f64(d16)
    for i in range(len(idc)):
        if V > 1 and idc[i] == 0:
            continue
        ref[idc[i]] += d[i]
        terms[idc[i]] += np.abs(d[i])
    assert_within(first, ref, terms, len(idc) + 1, 1, "dtable")


def test_colsum_fixed_order():
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(1000, 512, device="cuda", generator=g).bfloat16()
    o0 = torch.randn(512, device="cuda", generator=g)

    def run():
        o = o0.clone()
        ops.colsum(x, o)
        torch.cuda.synchronize()
        return o

    first = run()
    for _ in range(RUNS - 1):
        assert torch.equal(first, run())
    assert_within(first, f64(o0) + f64(x).sum(0), np.abs(f64(o0)) + np.abs(f64(x)).sum(0), 1001, 1, "colsum")


# ------------------------------------------------------------------------------------------------ strictness
def test_a_stream_without_a_workspace_is_refused_before_anything_is_launched():
    x, gamma, dy, mean, rstd, pre = _ln_case(37, 512, True, seed=1)
    dg, db = pre[0].clone(), pre[1].clone()
    dx_probe = torch.full_like(x, 7.0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    lib = ops.lib()
    with pytest.raises(MMDTIError, match="layernorm_bwd"):
        # straight through the C ABI on a fresh stream: ops._stream() would register a workspace at first use
        lib.mmdti_layernorm_bwd(side.cuda_stream, dy.data_ptr(), ops.DT_BF16, 0, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                37, 512, 0, dx_probe.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, 0.0, 0, 0, 0, 0.0, 0, 0)
    # ... and one that is too small
    small = torch.empty(1024, device="cuda", dtype=torch.uint8)
    lib.mmdti_det_workspace(side.cuda_stream, small.data_ptr(), small.numel())
    with pytest.raises(MMDTIError, match="layernorm_bwd.*1024 bytes"):
        lib.mmdti_layernorm_bwd(side.cuda_stream, dy.data_ptr(), ops.DT_BF16, 0, x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                37, 512, 0, dx_probe.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, 0.0, 0, 0, 0, 0.0, 0, 0)
    lib.mmdti_det_workspace(side.cuda_stream, 0, 0)
    torch.cuda.synchronize()
    assert torch.equal(dg, pre[0]) and torch.equal(db, pre[1]) and bool((dx_probe == 7.0).all())


def test_embedding_bwd_ordered_form():
    ids, dout, t0 = _emb_case(31)

    def run():
        t = t0.clone()
        ops.embedding_bwd(ids, dout, t, padding_idx=0)
        torch.cuda.synchronize()
        return t

    first = run()
    for _ in range(RUNS - 1):
        assert torch.equal(first, run())
    ref, terms = f64(t0).copy(), np.abs(f64(t0))
    idc, d = ids.cpu().numpy(), f64(dout)
    for i in range(len(idc)):
        if idc[i] != 0:
            ref[idc[i]] += d[i]
            terms[idc[i]] += np.abs(d[i])
    assert_within(first, ref, terms, len(idc) + 1, 1, "dtable")


# ------------------------------------------------------------------------------------------------ pair-bias backward
def test_pair_bias_backward_fixed_order(monkeypatch):
    """B = 3, N = 40, atom vocabulary 4 -> 16 edge types: every histogram bin of mul / bias collects over a thousand terms from all eight
    waves of a workgroup, over several workgroups (300 tiles of 16 pairs, 8 per workgroup iteration)."""
    B, N, K, F, H, E = 3, 40, 128, 128, 64, 16
    g = torch.Generator(device="cuda").manual_seed(21)
    atoms = torch.randint(0, 4, (B, N), device="cuda", generator=g)
    et = (atoms[:, :, None] * 4 + atoms[:, None, :]).contiguous()
    dist = (torch.rand(B, N, N, device="cuda", generator=g) * 6.0).contiguous()
    mul = torch.randn(E, device="cuda", generator=g) * 0.3 + 1.0
    bias = torch.randn(E, device="cuda", generator=g) * 0.3
    means = torch.rand(K, device="cuda", generator=g) * 3.0
    stds = torch.rand(K, device="cuda", generator=g) * 3.0 + 0.1
    w1 = (torch.randn(F, K, device="cuda", generator=g) * 0.1).bfloat16()
    b1 = torch.randn(F, device="cuda", generator=g) * 0.1
    w2 = (torch.randn(H, F, device="cuda", generator=g) * 0.1).bfloat16()
    gin = torch.randn(B, H, N, N, device="cuda", generator=g).contiguous()
    names = ("dw1", "db1", "dw2", "db2", "dmul", "dbias", "dmeans", "dstds")
    shapes = ((F, K), (F,), (H, F), (H,), (E,), (E,), (K,), (K,))

    def run():
        outs = [torch.zeros(s, device="cuda") for s in shapes]
        ops.gbf_bias_bwd_full(gin, dist, et, mul, bias, means, stds, w1, b1, w2, N, *outs)       # (ops sizes and hands in the slab workspace)
        torch.cuda.synchronize()
        return outs

    first = run()
    for n, o in zip(names, first):
        assert torch.isfinite(o).all() and float(o.abs().max()) > 0, n
    for _ in range(RUNS - 1):
        for n, a, b in zip(names, first, run()):
            assert torch.equal(a, b), n
    # the mode's sums sit inside the default mode's own band around them (fp32 sums in another order)
    ops.set_deterministic(False)
    for n, a, b in zip(names, first, run()):
        assert float((a - b).norm() / b.norm()) < 2e-5, n
    ops.set_deterministic(True)
    # without the slabs (MMDTI_GBF_SLABS=0) the mode refuses instead of taking atomics
    monkeypatch.setattr(ops, "GBF_SLABS", False)
    with pytest.raises(MMDTIError, match="gbf_bias_bwd_full: deterministic mode needs the workspace"):
        run()


def test_unfused_pair_bias_feature_backward_fixed_order():
    """ops.gbf_features_bwd (the pair-bias backward of head / basis counts the fused kernel is not built for -- every small fixture):
    the same B = 3, N = 40, 16 edge types; 4800 pairs on 256 workgroups, K = 136 basis functions (a second, partial block of 128)."""
    P, K, E = 3 * 40 * 40, 136, 16
    g = torch.Generator(device="cuda").manual_seed(22)
    et = torch.randint(0, E, (P,), device="cuda", generator=g)
    dist = torch.rand(P, device="cuda", generator=g) * 6.0
    mul = torch.randn(E, device="cuda", generator=g) * 0.3 + 1.0
    bias = torch.randn(E, device="cuda", generator=g) * 0.3
    means = torch.rand(K, device="cuda", generator=g) * 3.0
    stds = torch.rand(K, device="cuda", generator=g) * 3.0 + 0.1
    dfeat = torch.randn(P, K, device="cuda", generator=g).bfloat16()
    pre = [torch.randn(n, device="cuda", generator=g) for n in (E, E, K, K)]

    def run():
        outs = [t.clone() for t in pre]
        ops.gbf_features_bwd(dist, et, mul, bias, means, stds, dfeat, *outs)
        torch.cuda.synchronize()
        return outs

    first = run()
    for _ in range(RUNS - 1):
        for a, b in zip(first, run()):
            assert torch.equal(a, b)
    ops.set_deterministic(False)
    for n, a, b, p0 in zip(("dmul", "dbias", "dmeans", "dstds"), first, run(), pre):
        assert float(((a - p0) - (b - p0)).norm() / (b - p0).norm()) < 2e-5, n       # same sums, another order
    ops.set_deterministic(True)


def test_general_pair_attention_backward_adds_its_waves_in_order():
    """row-major pair tensors with ld % 4 != 0 take the per-element pair_attn_bwd_kernel, whose four waves meet in LDS: N = 70 keys, so every
    dK / dV element collects four partial sums"""
    B, N, H, ld = 2, 70, 8, 71
    D = H * 8
    g = torch.Generator(device="cuda").manual_seed(33)
    qkv = torch.randn(B * N, 3 * D, device="cuda", generator=g).bfloat16()
    dO = torch.randn(B * N, D, device="cuda", generator=g).bfloat16()
    s = torch.randn(B, H, N, ld, device="cuda", generator=g)

    def run():
        gbuf = torch.zeros(B, H, N, ld, device="cuda")
        out = ops.pair_attn_bwd(qkv, s, dO, gbuf, B, N, H, ld, 0.35, True)
        torch.cuda.synchronize()
        return out, gbuf

    first = run()
    for _ in range(RUNS - 1):
        again = run()
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    ops.set_deterministic(False)
    ref = run()
    ops.set_deterministic(True)
    assert torch.equal(first[1], ref[1])                       # the pair gradient has one writer per element either way
    # dq | dk | dv are bf16: four fp32 partial sums in another order move the sum by <= 4 * 2^-24 * sum|terms| (far below 1e-5 of the
    # tensor's largest element), which can flip one bf16 rounding: 2^-7 relative
    a, b = first[0].float(), ref[0].float()
    assert bool(((a - b).abs() <= 2.0 ** -7 * b.abs() + 1e-5 * float(b.abs().max())).all())


# ------------------------------------------------------------------------------------------------ model level
from oracle import mmdti_oracle as O                                      # noqa: E402
from g9util import load_fixture_weights, product_model, rel_l2, tiny_cfg  # noqa: E402


def _wide_cfg():
    """the 2-layer configuration of test_step_gradients_are_reproducible_on_the_batch_that_used_to_scatter_by_21_percent"""
    ocfg = tiny_cfg("classification", 40)
    ocfg.unimol = O.UniMolCfg(layers=2, dim=512, ffn=256, heads=64, K=128, vocab=31)
    ocfg.cross, ocfg.roberta = O.CrossCfg(dim=512, heads=16, ffn=128), O.RobertaCfg(layers=1, dim=512, heads=8, ffn=128, vocab=40, max_pos=40)
    return ocfg


def _scatter_batch(ocfg):
    import random
    rng = random.Random(11)
    for trial in range(62):
        B = rng.choice([2, 3, 5, 8])
        nmax = rng.choice([6, 14, 30, 46, 62, 78, 94, 110, 126, 142, 158, 190, 222, 256])
    return O.synth_batch(B, nmax, 20, ocfg, seed=1000 + trial, ragged=True), 77 + trial


def _three_steps_are_identical(model, batch, label, seed, counts=None, band=2e-5):
    """three steps with one dropout seed: loss and every parameter gradient torch.equal (identically zero gradients aside); and the
    mode's gradients within `band` relative L2 of the default mode's"""
    from mmdti_hip.functional import CELossFn
    from mmdti_hip.runtime import dropout_state
    dev = {k: v.cuda() for k, v in batch.items()}
    extra = {} if counts is None else {"atom_counts": counts}

    def step():
        dropout_state.reseed(seed)
        model.zero_grad(set_to_none=True)
        logits, infonce, ct = model(**dev, **extra, return_infonce_loss=True, return_ct_loss=True, net_target=label.cuda())
        loss = CELossFn.apply(logits, label.cuda()) + 0.1 * infonce + 0.1 * ct
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    l1, g1 = step()
    for _ in range(2):
        l2, g2 = step()
        assert torch.equal(l1, l2)
        assert g1.keys() == g2.keys()
        for n in g1:
            assert torch.equal(g1[n], g2[n]), (n, rel_l2(g2[n], g1[n]))
    ops.set_deterministic(False)
    l0, g0 = step()
    ops.set_deterministic(True)
    names = [n for n in g1 if float(g0[n].abs().max()) > 0 and not any(z in n for z in ("pooler", "key.bias", "gbf_proj.linear2.bias"))]
    assert len(names) > 20
    worst = max(((rel_l2(g1[n], g0[n]), n) for n in names))
    assert worst[0] < band, worst
    return g1


def test_model_step_is_bit_identical_on_the_batch_that_used_to_scatter():
    from mmdti_hip import collate
    ocfg = _wide_cfg()
    model = product_model(ocfg).cuda().train()
    load_fixture_weights(model, O.init_params(ocfg, seed=12, std=0.05))
    (batch, label), seed = _scatter_batch(ocfg)
    counts = collate.atom_counts(batch["src_tokens"], 0)
    assert counts.tolist() == [159, 88, 130, 110, 107]
    _three_steps_are_identical(model, batch, label, seed)
    _three_steps_are_identical(model, batch, label, seed, counts=counts)          # the ragged kernels, ragged against ragged


def test_model_step_is_bit_identical_on_the_large_row_path():
    """36 molecules at N = 128 atoms (130 with BOS / EOS), L = 128 tokens: more than 4096 token rows in both towers -- the 256 x 256
    split-K grouped weight gradients with their slab pass, and the bias gradients' column-sum pass"""
    ocfg = _wide_cfg()
    ocfg.roberta = O.RobertaCfg(layers=1, dim=512, heads=8, ffn=128, vocab=40, max_pos=140)
    model = product_model(ocfg).cuda().train()
    load_fixture_weights(model, O.init_params(ocfg, seed=12, std=0.05))
    batch, label = O.synth_batch(36, 128, 128, ocfg, seed=4, ragged=False)
    assert batch["src_tokens"].shape[0] * batch["src_tokens"].shape[1] > 4096
    _three_steps_are_identical(model, batch, label, 5)


SEQUENCERS = {"_unimol_stack_fwd": "F", "_unimol_stack_bwd": "B", "_unimol_layer_bwd_seq": "l",
              "_bert_stack_fwd": "bF", "_bert_stack_bwd": "bB", "_bert_layer_bwd_seq": "bl"}


def _train3(flags, monkeypatch, calls, seed=31):
    """three optimizer steps of the 2-layer 512 / 256 configuration (the widths the library's sequencers take) under FineTuner -- the
    parameters sit in an arena, 8 molecules x 31 atoms and 8 x 20 tokens: rows between the grouped launch's 128 and the stack's 8192"""
    import mmdti_hip.functional as Fn
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    monkeypatch.setattr(Fn, "STACK_SEQ", flags[0])
    monkeypatch.setattr(Fn, "LAYER_SEQ", flags[1])
    monkeypatch.setattr(Fn, "STACK_SIDE_WGRAD", flags[2])
    ocfg = _wide_cfg()
    ocfg.roberta = O.RobertaCfg(layers=1, dim=512, heads=8, ffn=256, vocab=40, max_pos=40)
    torch.manual_seed(0)
    model = product_model(ocfg, dropout=True).cuda().train()
    load_fixture_weights(model, O.init_params(ocfg, seed=3, std=0.05))
    dropout_state.reseed(seed)
    tuner = FineTuner(model, "classification", learning_rate=1e-3, warmup_ratio=0.25, total_steps=8, max_norm=5.0, deterministic=True)
    assert tuner.deterministic and ops.is_deterministic()
    batches = [O.synth_batch(8, 30, 20, ocfg, seed=20 + i, ragged=False) for i in range(3)]
    del calls[:]
    for b, y in batches:
        dev = {k: v.cuda() for k, v in b.items()}
        tuner.step(dev, y.cuda())
    torch.cuda.synchronize()
    a = tuner.arena
    return a.data.clone(), a.adam_m.clone(), a.adam_v.clone()


# (STACK_SEQ, LAYER_SEQ, STACK_SIDE_WGRAD)
PATHS = {"stack": (True, True, False), "stack+side-wgrad": (True, True, True), "per-layer": (False, True, False), "op-by-op": (False, False, False)}


def test_three_optimizer_steps_end_in_the_same_bits(monkeypatch):
    """parameters and both Adam moments after three steps, twice from identical weights and seeds: torch.equal, on each execution path
    of paths.py -- and each path is seen to be taken (spies on the sequencer calls of functional.py, as the *_sequenced_in_the_library_*
    tests have them).  Across paths only the default band.  Through step(): graphed_step is not offered in the mode (next test)."""
    import mmdti_hip.functional as Fn
    calls = []
    for fn, tag in SEQUENCERS.items():
        real = getattr(Fn, fn)
        monkeypatch.setattr(Fn, fn, lambda *a, _r=real, _t=tag, **k: (calls.append(_t), _r(*a, **k))[1])
    per_path = {}
    for name, flags in PATHS.items():
        r1 = _train3(flags, monkeypatch, calls)
        r2 = _train3(flags, monkeypatch, calls)
        seen = {t: calls.count(t) for t in SEQUENCERS.values()}
        print(name, seen)
        # tower 1 (2 layers, 3 steps): one stack call per direction and step / one library call per layer and step / neither
        if name.startswith("stack"):
            assert (seen["F"], seen["B"], seen["l"]) == (3, 3, 0), (name, seen)
        elif name == "per-layer":
            assert (seen["F"], seen["B"], seen["l"]) == (0, 0, 6), (name, seen)
            assert seen["bF"] == 0 and seen["bB"] == 0, (name, seen)
        else:
            assert not any(seen.values()), (name, seen)
        if name == "stack+side-wgrad":
            # the weight-gradient stream handed to mmdti_unimol_stack_bwd by value has its own registered workspace
            sides = [ent[0].cuda_stream for ent in Fn._stack_sides.values()]
            assert sides and all(h in ops._det_ws for h in sides)
        for what, a, b in zip(("parameters", "adam_m", "adam_v"), r1, r2):
            assert torch.equal(a, b), (name, what, rel_l2(a, b))
        per_path[name] = r1[0]
    for name in ("stack+side-wgrad", "per-layer", "op-by-op"):
        assert rel_l2(per_path[name], per_path["stack"]) < 1e-3, name


def test_graphed_step_is_refused_in_the_mode_before_anything_is_captured():
    from mmdti_hip.trainer import FineTuner
    ocfg = tiny_cfg("classification", 40)
    model = product_model(ocfg).cuda().train()
    b, y = O.synth_batch(8, 10, 14, ocfg, seed=20, ragged=False)
    dev = {k: v.cuda() for k, v in b.items()}
    tuner = FineTuner(model, "classification", total_steps=8, deterministic=True)
    with pytest.raises(RuntimeError, match="graphed_step: not supported in the deterministic mode"):
        tuner.graphed_step(dev, y.cuda())
    assert not tuner._graphs and tuner._state is None
    # the mode is process-wide: an engine built without the keyword is refused as well while it is on
    plain = FineTuner(product_model(ocfg).cuda().train(), "classification", total_steps=8)
    with pytest.raises(RuntimeError, match="graphed_step: not supported in the deterministic mode"):
        plain.graphed_step(dev, y.cuda())


_CHILD = r"""
import hashlib, sys
sys.path[:0] = [%r, %r, %r]
import torch
from oracle import mmdti_oracle as O
from g9util import load_fixture_weights, product_model, tiny_cfg
from mmdti_hip.runtime import dropout_state
from mmdti_hip.trainer import FineTuner
ocfg = tiny_cfg("classification", 40)
model = product_model(ocfg, dropout=True).cuda().train()
load_fixture_weights(model, O.init_params(ocfg, seed=3, std=0.08))
dropout_state.reseed(31)
tuner = FineTuner(model, "classification", learning_rate=1e-3, warmup_ratio=0.25, total_steps=8, max_norm=5.0, deterministic=True)
for i in range(3):
    b, y = O.synth_batch(8, 10, 14, ocfg, seed=20 + i, ragged=True)
    tuner.step({k: v.cuda() for k, v in b.items()}, y.cuda())
torch.cuda.synchronize()
print("digest", hashlib.sha256(tuner.arena.data.cpu().numpy().tobytes()).hexdigest())
"""


def test_two_fresh_processes_end_in_the_same_parameters():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = _CHILD % (root, os.path.join(root, "mm-dti_amd"), os.path.join(root, "tests"))
    digests = []
    for _ in range(2):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-800:]                 # (the second child is not started if the first failed)
        digests.append([l for l in r.stdout.splitlines() if l.startswith("digest ")][-1])
    assert digests[0] == digests[1]


def test_default_mode_step_never_touches_the_switch_or_the_table():
    from mmdti_hip.functional import CELossFn
    ops.set_deterministic(False)
    lib = ops.lib()
    calls = []
    real = {n: getattr(lib, n) for n in ("mmdti_set_deterministic", "mmdti_det_workspace")}
    try:
        for n in real:
            lib.__dict__[n] = lambda *a, _n=n: calls.append(_n)
        ocfg = tiny_cfg("classification", 40)
        model = product_model(ocfg).cuda().train()
        batch, label = O.synth_batch(8, 10, 14, ocfg, seed=20, ragged=True)
        from mmdti_hip.trainer import FineTuner
        tuner = FineTuner(model, "classification", total_steps=10)
        assert tuner.deterministic is False
        tuner.step({k: v.cuda() for k, v in batch.items()}, label.cuda())
        torch.cuda.synchronize()
        assert calls == [] and not ops._det_ws and ops._stream is ops._stream_fast
    finally:
        lib.__dict__.update(real)
