"""The case table of tests/attn_cases.py, checked without a GPU: that it reaches all 27 kernel instances of csrc/attn.hip by the rule of
attn_nt (still verbatim in the source), through both entry points, at the edges the issue lists; that the float64 reference agrees
with float64 autograd; that the exact modes are exact by construction; and that an fp32 emulation of the kernels' rounding points
(P' and dS to bf16, the outputs to bf16 / fp16) stays inside the bounds the device results are held to -- while the same emulation
with a softmax denominator wrong by 1 / 256 does not."""
import os

import pytest
import torch

import attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attn_nt_is_the_rule_the_table_declares():
    src = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "attn.hip")).read()
    assert A.ATTN_NT_LINE in src
    for Lk, nt in ((1, 10), (160, 10), (161, 16), (256, 16), (257, 24), (384, 24), (385, 32), (512, 32)):
        assert A.attn_nt(Lk) == nt
    for c in A.CASES:
        assert c["nt"] == A.attn_nt(c["Lk"]) and c["lqp"] == ((c["Lq"] + 31) // 32) * 32
        assert 1 <= c["Lq"] <= 512 and 1 <= c["Lk"] <= 512 and (c["entry"] == "long" or max(c["Lq"], c["Lk"]) <= 256), A.case_id(c)
    assert len({A.case_id(c) for c in A.CASES}) == len(A.CASES)
    assert len({A.run_id(r) for r in A.runs(A.PLAIN + ("dropout",))}) == len(A.runs(A.PLAIN + ("dropout",)))


def test_the_table_reaches_all_27_instances_and_the_edges():
    fwd, bq, bkv = (set(x) for x in zip(*(A.instances(c) for c in A.CASES)))
    pairs = [(hd, nt) for hd in (16, 32, 64) for nt in (10, 16, 24, 32)]
    assert fwd == {f"attn_fwd_kernel<{hd}, {nt}>" for hd, nt in pairs} and bq == {f"attn_bwd_q_kernel<{hd}, {nt}>" for hd, nt in pairs}
    assert bkv == {f"attn_bwd_kv_kernel<{hd}>" for hd in (16, 32, 64)} and len(fwd) + len(bq) + len(bkv) == 27
    for hd in (16, 32, 64):
        cs = [c for c in A.CASES if c["hd"] == hd]
        dense = [c for c in cs if c["packed"] is None]
        for nt in (10, 16):                                              # through both entry points
            assert {c["entry"] for c in cs if c["nt"] == nt} == {"short", "long"}, (hd, nt)
        assert any(c["lqp"] < 256 for c in cs) and any(c["lqp"] > 256 for c in cs)
        assert {c["Lk"] for c in dense} >= {1, 15, 17, 33, 160, 161, 256, 257, 384, 385, 511, 512}
        assert {c["Lq"] for c in dense} >= {1, 16, 17, 31, 33, 129, 257, 512}
        assert {c["layout"] for c in cs} == {"tight", "padded", "fused", "cross"} and any(c["ldo4"] for c in cs)
        for nt in (10, 16, 24, 32):                                      # every instance: both context types, every plain mode, dropout
            of = [c for c in cs if c["nt"] == nt]
            assert {c["ctx_f16"] for c in of} == {0, 1}, (hd, nt)
            assert {m for c in of for m in c["modes"]} == set(A.PLAIN + ("dropout",)), (hd, nt)
            assert any(c["bias"] for c in of) and any(not c["bias"] for c in of) and any(c["allmask"] for c in of), (hd, nt)
        assert {p for c in cs for p in c["drop"] if "dropout" in c["modes"]} == {0.1, 0.35}
        packed = {(c["packed"][0], c["packed"][1], c["entry"]) for c in cs if c["packed"]}
        assert ((1, 17, 33), (16, 1, 40), "short") in packed and ((5, 258, 130), (512, 40, 300), "long") in packed
    assert A.B == 2 and A.HEADS == 3


def _keep(t, p, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(A.HEADS, lq, lk, generator=g) >= p for (_, lq, _, lk, _) in t["seqs"]]


@pytest.mark.parametrize("r", [r for r in A.runs(("random", "dropout")) if r[0]["Lq"] * r[0]["Lk"] <= 33 * 160 and r[0]["hd"] == 32], ids=A.run_id)
def test_the_reference_agrees_with_float64_autograd(r):
    c, mode, p = r
    t = A.make_inputs(c, mode)
    keep = _keep(t, p) if p else None
    ref = A.reference(c, t, p, keep, bounds=False)
    hd = c["hd"]
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        Q, K, V = (A._heads(t[n], r0, n_, hd, A.F64).clone().requires_grad_() for n, r0, n_ in (("q", q0, lq), ("k", k0, lk), ("v", k0, lk)))
        s = t["scale"] * (Q @ K.transpose(1, 2))
        if t["add"] is not None:
            s = s + t["add"][b, :lk].to(A.F64)
        pr = torch.softmax(s, -1)
        if keep is not None:
            pr = pr * keep[b].to(A.F64) / (1.0 - p)
        ctx = pr @ V
        ctx.backward(A._heads(t["do"], q0, lq, hd, A.F64))
        for name, mine, want in (("ctx", ref["ctx"][q0:q0 + lq], ctx.detach()), ("dq", ref["dq"][q0:q0 + lq], Q.grad),
                                 ("dk", ref["dk"][k0:k0 + lk], K.grad), ("dv", ref["dv"][k0:k0 + lk], V.grad)):
            d = float((mine - A._rows(want)).abs().max())
            assert d <= 1e-12 * max(1.0, float(want.abs().max())), (A.run_id(r), b, name, d)


def _same(got, ref, c):
    for k in ("ctx", "dq", "dk", "dv"):
        want = A.round16(ref[k], A.ctx_dtype(c) if k == "ctx" else A.BF16)
        assert torch.equal(got[k].to(A.F64), want.to(A.F64)), k


@pytest.mark.parametrize("r", A.runs(("uniform",)), ids=A.run_id)
def test_uniform_cases_are_exact_by_construction(r):
    """every term of every final sum a multiple of one quantum, sum |term| < 2^24 quanta; and the fp32 emulation EQUALS the reference"""
    c = r[0]
    t = A.make_inputs(c, "uniform")
    assert A.exactness(c, t) < 2 ** 24
    ref, got = A.reference(c, t, exact=True, bounds=False), A.emulate(c, t)
    _same(got, ref, c)
    for b, n in enumerate(t["n_real"]):
        assert bool((got["m2"][b] == 0).all()) and bool((got["inv"][b] == 1.0 / n).all())
        assert torch.equal(got["r"][b].to(A.F64), ref["r"][b])


@pytest.mark.parametrize("r", A.runs(("selector",)), ids=A.run_id)
def test_selector_cases_are_one_hot_in_fp32(r):
    c = r[0]
    t = A.make_inputs(c, "selector")
    for (q0, lq, k0, lk, krows), s in zip(t["seqs"], t["sel"]):
        assert int(s.max()) == lk - 1 and (lq < 4 or lk < 4 or len(set(s.tolist())) < min(lq, lk))
        for h in range(A.HEADS):
            k = t["k"][k0:k0 + krows, h * c["hd"]:(h + 1) * c["hd"]].float()
            ham = (c["hd"] - k @ k.T) / 2
            assert krows == 1 or float((ham + 1e9 * torch.eye(krows)).min()) >= 1                      # distinct codes
    got = A.emulate(c, t)
    ctx, dv, m = A.selector_expectation(c, t)
    assert torch.equal(got["ctx"].to(A.F64), ctx) and torch.equal(got["dv"].to(A.F64), dv)
    assert float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0
    for b in range(len(t["seqs"])):
        assert bool((got["m2"][b] == m).all()) and bool((got["inv"][b] == 1.0).all())


@pytest.mark.parametrize("r", A.runs(("random", "large", "dropout")), ids=A.run_id)
def test_the_fp32_emulation_stays_inside_the_bounds(r):
    c, mode, p = r
    t = A.make_inputs(c, mode)
    keep = _keep(t, p) if p else None
    ref = A.reference(c, t, p, keep)
    if mode == "large":
        smax = max(float(m[m > -1e30].max()) for m in ref["m2"] if bool((m > -1e30).any())) / A.LOG2E    # (the largest row max, natural units)
        assert 60.0 <= smax <= 160.0, smax
    res = A.evaluate(c, ref, A.emulate(c, t, p, keep))
    for k, (ratio, z) in res.items():
        assert ratio < 1.0 and abs(z) < 3.0, (A.run_id(r), k, ratio, z)
    for k in ("ctx", "dq", "dk", "dv"):
        assert not torch.isnan(ref[k]).any() and not torch.isinf(A.out_bound(c, ref, k)).any()


@pytest.mark.parametrize("hd,Lq,Lk", [(64, 257, 256), (32, 33, 160), (16, 129, 161)])
def test_a_denominator_wrong_by_1_in_256_leaves_the_bounds(hd, Lq, Lk):
    """the systematic error the older bounds let through: every probability 0.4 % high.  The elementwise bound is grazed, the gain is not."""
    c = next(c for c in A.CASES if (c["hd"], c["Lq"], c["Lk"]) == (hd, Lq, Lk) and "random" in c["modes"])
    t = A.make_inputs(c, "random")
    ref = A.reference(c, t)
    good = A.emulate(c, t)
    bad = dict(good, ctx=(good["ctx"].double() * (1 + 1 / 256)).to(good["ctx"].dtype))
    zg, zb = A.evaluate(c, ref, good)["ctx"][1], A.evaluate(c, ref, bad)["ctx"][1]
    print(f"gain of the context: correct {zg:.2f}, denominator off by 1/256 {zb:.2f}")
    assert abs(zg) < 3.0 and abs(zb) > A.Z_MAX


def test_placement_cuts_every_operand_from_guarded_arenas():
    for c in (c for c in A.CASES if c["hd"] == 16 and c["Lq"] <= 33 and c["Lk"] <= 40):
        t = A.make_inputs(c, c["modes"][-1] if c["modes"][-1] != "dropout" else "random")
        pl = A.place(c, t, "cpu")
        for n in ("q", "k", "v", "do"):
            assert torch.equal(pl["views"][n], t[n]) and pl["ptr"][n] % 16 == 0 and pl["ld"][n] % 8 == 0
        for n, a in pl["arenas"].items():
            if n in pl["outs"]:
                assert a.outside_untouched() == 0 and bool(torch.isnan(a.view.float()).all())
            else:
                inside = sum(pl["views"][m].numel() for m in ("q", "k", "v", "do") if pl["views"][m].untyped_storage().data_ptr() == a.buf.untyped_storage().data_ptr())
                inside = inside or a.view.numel()
                assert int(torch.isnan(a.buf.float()).sum()) == a.buf.numel() - inside, (A.case_id(c), n)
