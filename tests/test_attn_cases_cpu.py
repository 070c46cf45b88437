"""The case table of tests/attn_cases.py, checked without a GPU: that it reaches all 27 kernel instances of csrc/attn.hip by the rule of
attn_nt, through both entry points, at the edges the issue lists -- and that the library, asked through the launch-free query
mmdti_attn_plan, plans for every case and for a sweep of every length what the table declares; that the float64 reference agrees
with float64 autograd; that the exact modes are exact by construction; and that an fp32 emulation of the kernels' rounding points
(P' and dS to bf16, the outputs to bf16 / fp16) stays inside the bounds the device results are held to -- while the same emulation
with a softmax denominator wrong by 1 / 256 does not."""
import ctypes
import os

import pytest
import torch

from mmdti_hip import _abi

import attn_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table_names():
    lib = _abi.lib()
    n = ctypes.c_int()
    lib.mmdti_plan_table_size(0, ctypes.byref(n))
    names = [lib.mmdti_plan_kernel_name(0, i).decode() for i in range(n.value)]
    assert lib.mmdti_plan_kernel_name(0, n.value) is None and lib.mmdti_plan_kernel_name(0, -1) is None
    return names


def test_the_library_plans_what_every_case_declares():
    """instance names, grid, workgroup size, LDS, LDS opt-in, nt and lqp of every case, through its own entry point -- and, up to 256
    queries and keys, through the other one"""
    lib = _abi.lib()
    for c in A.CASES:
        nb = len(c["packed"][0]) if c["packed"] else A.B
        A.assert_declared_plan(lib, c, nb)
        if max(c["Lq"], c["Lk"]) <= 256:
            A.assert_declared_plan(lib, c, nb, entry="long" if c["entry"] == "short" else "short")
    names = _table_names()
    assert len(names) == len(set(names)) == 27 and set(names) == {i for c in A.CASES for i in A.instances(c)}


EDGES = (1, 31, 32, 33, 160, 161, 256, 257, 384, 385, 480, 481, 512)


def test_a_sweep_of_every_length_plans_the_declared_launches_or_refuses_as_the_launcher_does():
    """Lq = 1..512 at the edges of Lk and Lk = 1..512 at the edges of Lq, three head sizes, both entry points, forward and backward; every
    table row is reached, and nothing outside the table is named"""
    lib = _abi.lib()
    seen = set()
    pairs = sorted({(lq, lk) for lq in range(1, 513) for lk in EDGES} | {(lq, lk) for lq in EDGES for lk in range(1, 513)})
    for hd in (16, 32, 64):
        for long_entry in (0, 1):
            cap = 512 if long_entry else 256
            for backward in (0, 1):
                who = ("attn_long_" if long_entry else "attn_") + ("bwd" if backward else "fwd")
                for lq, lk in pairs:
                    if max(lq, lk) > cap:
                        with pytest.raises(_abi.MMDTIError, match=rf"{who}: at most {cap} queries / keys per head \(got {lq} / {lk}\)"):
                            A.library_plan(lib, backward, long_entry, hd, lq, lk, 2)
                        continue
                    got = A.library_plan(lib, backward, long_entry, hd, lq, lk, 2)
                    assert got == A.declared_plan(hd, lq, lk, 2, backward), (hd, long_entry, backward, lq, lk, got)
                    seen |= {k[0] for k in got[2]}
    assert seen == set(_table_names())


def test_the_plan_query_validates_like_the_launch():
    lib = _abi.lib()
    ok = {n: A.PTR for n in ("q", "k", "v", "ctx", "do", "dq", "dk", "dv", "stats", "drow")}
    for backward, bad, msg in ((0, dict(q=0), "attn_fwd: bad arguments"), (0, dict(k=A.PTR + 8), "attn_fwd: 16-byte alignment required"),
                               (0, dict(ctx=A.PTR + 4), "attn_fwd: bad output arguments"), (1, dict(drow=0), "attn_bwd: null argument"),
                               (1, dict(do=A.PTR + 8), "attn_bwd: dctx stride/alignment"), (1, dict(dv=A.PTR + 4), "attn_bwd: output stride/alignment")):
        with pytest.raises(_abi.MMDTIError, match=msg):
            A.library_plan(lib, backward, 0, 32, 16, 16, 2, ptr=dict(ok, **bad))
    with pytest.raises(_abi.MMDTIError, match="head_dim must be 16, 32 or 64"):
        A.library_plan(lib, 0, 0, 48, 16, 16, 2)
    with pytest.raises(_abi.MMDTIError, match="come together"):
        A.library_plan(lib, 0, 0, 32, 16, 16, 2, vargs=(A.PTR, 0, 0, 32))
    with pytest.raises(_abi.MMDTIError, match="dropout p out of range"):
        A.library_plan(lib, 1, 1, 32, 16, 16, 2, p_drop=1.0)


def test_attn_nt_is_the_rule_the_table_declares():
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
