"""The case table of tests/pair_cases.py, checked without a GPU: that the device-side rules it mirrors are verbatim in the sources; that
the library, asked through the launch-free query mmdti_pair_attn_plan, plans for every case and for a sweep of every size what the
table declares, and refuses what the launchers refuse with their message; that the table reaches all 85 forward and 98 backward
kernel instances (enumerated independently from the template parameter ranges, and equal to the library's kernel tables) and all 86
ragged bodies in each direction, every instance in every mode that applies to it, with and without a padding mask and with dropout at both rates; that the float64 reference agrees with float64
autograd; that the exact modes are exact by construction; and that an fp32 emulation of the kernels' rounding points stays inside
the bounds the device results are held to -- while the same emulation without the low parts of the hi + lo splits, or with a
softmax denominator wrong by 1 / 256, does not."""
import ctypes
import os

import pytest
import torch

from mmdti_hip import _abi

import pair_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mm-dti_amd", "csrc")


def test_the_mirrored_lines_are_verbatim_in_the_sources():
    for name, lines in P.SOURCE_LINES.items():
        src = open(os.path.join(CSRC, name)).read()
        for line in lines:
            assert line in src, (name, line)
    assert [P.pa_kt_effective(k, 17) for k in (0, 1, 4, 5, 16, 17, 20)] == [4, 4, 4, 8, 16, 17, 17]
    assert [P.pa_kt_effective(k, 12) for k in (1, 2, 3, 10, 11, 12)] == [2, 2, 4, 10, 12, 12] and P.pa_kt_effective(3, 9) == 3
    assert [P.fwd_block(n) for n in (1, 2, 3, 4, 5, 6, 16, 17)] == [64, 128, 192, 256, 256, 192, 256, 256]
    assert [P.bwd_block(n) for n in (1, 2, 3, 4, 5, 6, 16, 17)] == [64, 128, 192, 256, 192, 192, 192, 192]
    from mmdti_hip import ops
    for N in (1, 5, 16, 17, 37, 130, 258, 272):
        assert P.pair_ld(N) == ops.pair_ld(N) and P.pair_plane(N) == ops.pair_plane(N) and P.tiles(N) == ops.pair_tiles(N)
        c = dict(N=N, layout=3, B=1, H=1, ld=P.pair_ld(N), lens=None, packed=False, f16=False, det=False, shift=False)
        assert torch.equal(P.geometry(c)["idx"], ops._tile_index(N, "cpu", ops.pair_ld(N)))
        for k in range(0, 19):
            assert P.pa_kt_effective(k, P.tiles(N)) == ops.pair_key_tiles_effective(k, P.tiles(N))


def _table(families):
    """the names of the library's kernel tables (mmdti_plan_kernel_name), the defaulted DET = false written out"""
    lib, names = _abi.lib(), []
    for fam in families:
        n = ctypes.c_int()
        lib.mmdti_plan_table_size(fam, ctypes.byref(n))
        assert lib.mmdti_plan_kernel_name(fam, n.value) is None and lib.mmdti_plan_kernel_name(fam, -1) is None
        names += [lib.mmdti_plan_kernel_name(fam, i).decode() for i in range(n.value)]
    return [n[:-1] + ", false>" if n.startswith("pair_attn_bwd_kernel<") and "," not in n else n for n in names]


def test_the_library_plans_what_every_case_declares():
    """instance, grid, workgroup size, nqb and NW of both launches of every case; the library's tables hold the 85 + 98 instances"""
    lib = _abi.lib()
    for c in P.CASES:
        for backward in (False, True):
            P.assert_declared_plan(lib, c, backward)
    fwd, bwd = P.all_instances()
    tf, tb = _table((2, 4)), _table((3, 5))
    assert len(tf) == len(set(tf)) == 85 and len(tb) == len(set(tb)) == 98 and set(tf) == fwd and set(tb) == bwd


def _refusal(c, backward):
    """the launcher's message for a combination it refuses, in the order of its checks; None: it launches"""
    lay = c["layout"] if backward else c["layout"] & 3
    tiled, compact = lay & 1, lay & 2
    if c["lens"] is not None and not compact:
        return "key_tiles .ragged batches. needs the compact"
    if not backward and c["f16"] and not compact:
        return "fp16 q . k . v .the fp16 forward-operand mode. is built for the compact tiled pair layout"
    if tiled and (c["ld"] % 4 or c["N"] > 16 * P.PA_MAX_NT):
        return "the tiled pair layout needs ld % 4 == 0 and N <= 272"
    if tiled and c["shift"]:
        return "tiled pair tensors must be 16-byte aligned"
    if backward and c["f16"] and not P.mfma(c):
        return "fp16 q . k . v are read by the MFMA kernels only"
    return None


def test_a_sweep_of_every_size_plans_the_declared_launches_or_refuses_as_the_launcher_does():
    """N = 1..320 x layouts 0 / 1 / 3 / 7 x ragged x fp16 operands x aligned / unaligned planes x ld % 4 x deterministic, both directions:
    every table row is reached, nothing outside the tables is named"""
    lib = _abi.lib()
    seen, refused = [set(), set()], set()
    for N in range(1, 321):
        for lay in (0, 1, 3, 7):
            for rag in (False, True):
                for f16 in (False, True):
                    for shift in (False, True):
                        for ld in (P.pair_ld(N), P.pair_ld(N) + 1):
                            for det in (False, True):
                                c = dict(N=N, layout=lay, B=3, H=3, ld=ld, lens=(N,) if rag else None, packed=False, f16=f16, det=det, shift=shift)
                                for backward in (False, True):
                                    msg = _refusal(c, backward)
                                    if msg:
                                        refused.add(msg)
                                        with pytest.raises(_abi.MMDTIError, match=("pair_attn_bwd: " if backward else "pair_attn_fwd: ") + msg):
                                            P.library_plan(lib, c, backward)
                                        continue
                                    got = P.library_plan(lib, c, backward)
                                    # (the backward reads fp16 q | k | v on every MFMA instance; its instance does not depend on them)
                                    assert got == P.declared_plan(dict(c, f16=False) if backward else c, backward), (c, backward, got)
                                    seen[backward].add(got[0])
    assert seen[0] == set(_table((2, 4))) and seen[1] == set(_table((3, 5))) and len(refused) == 5
    with pytest.raises(_abi.MMDTIError, match="exceeds the supported 320 atoms"):
        P.library_plan(lib, dict(N=321, layout=0, B=3, H=3, ld=324, lens=None, packed=False, f16=False, det=False, shift=False), False)
    with pytest.raises(_abi.MMDTIError, match="pair_attn_bwd: alignment"):
        P.library_plan(lib, P.CASES[0], True, ptr=dict(qkv=P.PTR, s=P.PTR, g=P.PTR, o=P.PTR + 8, dqkv=P.PTR))


def test_the_table_reaches_every_instance_and_every_ragged_body():
    fwd, bwd = P.all_instances()
    assert len(fwd) == 85 and len(bwd) == 98 and len(P.all_bodies()) == 86
    got = [P.instances(c) for c in P.CASES]
    assert {f for f, _, _ in got} == fwd and {b for _, b, _ in got} == bwd
    for rag_f, rag_b in (("true, _Float16>", "float>"), ("true, _Float16, true>", "__bf16>")):    # every body of both directions, in both operand / gradient types
        assert set().union(*(bd for f, _, bd in got if f.endswith(rag_f))) == P.all_bodies()
        assert set().union(*(bd for _, b, bd in got if b.endswith(rag_b) and bd)) == P.all_bodies()
    assert len({P.case_id(c) for c in P.CASES}) == len(P.CASES) and len({P.run_id(r) for r in P.runs()}) == len(P.runs())
    for c in P.CASES:
        assert 1 <= c["N"] <= 320 and c["ld"] >= c["N"] and (c["lens"] is None or (len(c["lens"]) <= 9 and max(c["lens"]) == c["N"] and min(c["lens"]) >= 1))
        assert P.blocks(c)[0] in (64, 128, 192, 256) and P.blocks(c)[1] in (64, 128, 192, 256)


def test_every_instance_runs_every_mode_masked_and_unmasked_at_both_dropout_rates():
    by = {}
    for c, mode, p, mask in P.runs():
        f, b, _ = P.instances(c)
        masked = mask is not None or c["lens"] is not None or mode in ("uq", "uk")
        unmasked = mask is None and mode not in ("uq", "uk")      # (ragged cases: their second layer and their backward take no key_pad)
        for inst in (f, b):
            row = by.setdefault(inst, dict(modes=set(), masked=set(), drop=set()))
            row["modes"].add(mode)
            row["masked"] |= ({True} if masked else set()) | ({False} if unmasked else set())
            if p:
                row["drop"].add(p)
    for inst, row in by.items():
        compact = "_Float16" in inst
        assert row["modes"] == set(P.MODES16 if compact else P.MODES32), inst
        assert row["masked"] == {True, False} and row["drop"] == {0.1, 0.35}, inst


def test_the_table_holds_the_edges():
    dense = [c for c in P.CASES if c["layout"] & 2 and c["lens"] is None]
    rag = [c for c in P.CASES if c["lens"] is not None]
    assert {c["N"] for c in P.CASES if c["layout"] & 2} >= {1, 4, 5, 12, 13, 16, 17}
    for k in range(1, 18):
        Ns = {c["N"] for c in P.CASES if c["layout"] & 2 and P.tiles(c["N"]) == k}
        assert 16 * (k - 1) + 1 in Ns and 16 * k in Ns and any(n % 4 for n in Ns), k
        assert any(c["f16"] for c in dense if P.tiles(c["N"]) == k) and any(c["f16"] for c in rag if P.tiles(c["N"]) == k)
        of = [c for c in rag if P.tiles(c["N"]) == k]
        assert any(c["packed"] for c in of) and {c["layout"] for c in of} == {3, 7}
        for c in of:                                              # one launch covers every body of its kernel; one length rounds up
            assert P.instances(c)[2] == {(k, n) for n in P.supported_counts(k)}
            assert k < 10 or any(P.tiles(n) not in P.supported_counts(k) for n in c["lens"])
    by = {}                                                       # every compact instance at the three edge sizes, the exact modes at each
    for c in (c for c in P.CASES if c["layout"] & 2 and (c["B"], c["H"]) == (3 if c["lens"] is None else c["B"], 3)):
        f, b, _ = P.instances(c)
        assert {"selector", "uq", "uk", "random"} <= set(c["modes"])
        for inst in (f, b):
            by.setdefault(inst, set()).add(c["N"])
    fwd, bwd = P.all_instances()
    for inst in (i for i in fwd | bwd if "_Float16" in i):
        k = int(inst.split("<")[1].split(",")[0])
        want = {1, 16} if k == 1 else {16 * (k - 1) + 1, 16 * (k - 1) + 6, 16 * k}
        assert by[inst] >= want and (k > 1 or any(n % 4 for n in by[inst])), (inst, by[inst])
    assert any(c["H"] == 64 for c in P.CASES) and any(c["B"] * c["H"] == 16 for c in P.CASES) and any(c["B"] * c["H"] % 8 for c in P.CASES)
    assert any(c["layout"] == 0 and P.mfma(c) and c["ld"] == P.pair_ld(c["N"]) + 4 for c in P.CASES)
    pe = [c for c in P.CASES if not P.mfma(c)]
    for det in (False, True):
        assert {(c["N"], c["ld"]) for c in pe if c["det"] == det and not c["shift"]} == {(9, 10), (70, 71), (130, 131), (200, 201), (258, 259), (273, 276), (300, 300), (320, 320)}
        assert any(c["shift"] and c["ld"] % 4 == 0 for c in pe if c["det"] == det)
    assert any(r[3] == "one" for r in P.runs()) and any(1 in (c["lens"] or ()) for c in P.CASES)


def _small(r):
    c = r[0]
    return c["N"] <= 40 and c["B"] * c["H"] <= 27


@pytest.mark.parametrize("r", [r for r in P.runs(("random", "dropout")) if _small(r)], ids=P.run_id)
def test_the_reference_agrees_with_float64_autograd(r):
    c, mode, p, mask = r
    t, geo = P.make_inputs(c, mode, mask), P.geometry(c)
    keep = P.random_keep(c, p) if p else None
    B, N = c["B"], c["N"]
    S_st, _ = P.logits(c, t, geo)
    ref = P.reference(c, t, geo, S_st, p, keep, bounds=False)
    ql, kl = P._live(c, geo)
    rb = (lambda x: x.to(P.BF16)) if c["f16"] else (lambda x: x)
    Q, K, V = (P._bh(rb(t[n])).clone().requires_grad_() for n in ("q", "k", "v"))
    Sin = torch.where(ql & kl, S_st, torch.full_like(S_st, float("-inf"))).clone()
    Sin = torch.where(ql, Sin, torch.zeros_like(Sin)).requires_grad_()
    pr = torch.softmax(Sin, -1)
    if keep is not None:
        pr = pr * keep.to(P.F64) / (1.0 - p)
    O = (pr @ V) * ql.to(P.F64)
    O.backward(P._bh(t["do"]))
    # (the chain: G_out = dL/dS of this layer + G_in; dq, dk are G_out pushed through S = bias + scale q.k^T)
    G = (Sin.grad + t["gin"].to(P.F64)) * ql.to(P.F64) * kl.to(P.F64)
    O_fwd = (pr.detach() @ P._bh(t["v"])) * ql.to(P.F64)          # (fp16 q | k | v: the forward multiplies them as stored, the backward their bf16 roundings)
    want = dict(O=O_fwd, dv=V.grad, dq=t["scale"] * (G @ K.detach()), dk=t["scale"] * (G.transpose(2, 3) @ Q.detach()))
    assert float((ref["G"] - G).abs().max()) <= 1e-12 * max(1.0, float(G.abs().max()))
    for k, w in want.items():
        d = float((ref[k] - w.permute(0, 2, 1, 3)).abs().max())
        assert d <= 1e-12 * max(1.0, float(w.abs().max())), (P.run_id(r), k, d)


@pytest.mark.parametrize("r", P.runs(("selector",)), ids=P.run_id)
def test_selector_cases_are_one_hot_in_fp32(r):
    c, mode, _, mask = r
    t, geo = P.make_inputs(c, mode, mask), P.geometry(c)
    assert P.selector_is_one_hot(c, t)
    for gz in (False, True):
        want, got = P.selector_expectation(c, t, geo, gz), P.emulate(c, t, geo, gz=gz)
        ql, kl = P._live(c, geo)
        live = (ql & kl).expand_as(want["S"])
        assert torch.equal(got["S"].to(P.F64)[live], want["S"][live]) and torch.equal(got["G"].to(P.F64), want["G"])
        for k in ("O", "dq", "dk", "dv"):
            assert torch.equal(got[k].to(P.F64), P.token_rows(c, geo, want[k])), (P.run_id(r), k)


@pytest.mark.parametrize("r", P.runs(("uq", "uk")), ids=P.run_id)
def test_uniform_cases_are_exact_by_construction(r):
    c, mode, _, mask = r
    t, geo = P.make_inputs(c, mode, mask), P.geometry(c)
    S_st, E = P.logits(c, t, geo)
    assert float(S_st[torch.isfinite(S_st)].abs().max()) == 0.0 and float(E.max()) <= 2.0 ** -25
    for gz in (False, True):
        ref = P.reference(c, t, geo, S_st, bounds=False, gz=gz)
        assert P.exactness(c, t, geo, ref) < 2 ** 24
        got = P.emulate(c, t, geo, gz=gz)
        assert torch.equal(got["G"].to(P.F64), ref["G"].to(P.g_dtype(c)).to(P.F64))          # (layout 7 stores bf16(G); the products used G itself)
        for k in ("O", "dq", "dk", "dv"):
            want = P.round16(P.token_rows(c, geo, ref[k]), P.o_dtype(c) if k == "O" else P.BF16)
            assert torch.equal(got[k], want), (P.run_id(r), k)
        live = "dq" if mode == "uq" else "dk"
        assert float(got["dk" if mode == "uq" else "dq"].float().abs().max()) == 0.0 and (c["N"] < 4 or float(got[live].float().abs().max()) > 0.0)


def _held(r, **wrong):
    c, mode, p, mask = r
    t, geo = P.make_inputs(c, mode, mask), P.geometry(c)
    keep = P.random_keep(c, p) if p else None
    got = P.emulate(c, t, geo, p, keep, **wrong)
    S_ref, E_S = P.logits(c, t, geo)
    ref = P.reference(c, t, geo, got["S"].to(P.F64), p, keep)
    return P.evaluate(c, geo, ref, got, S_ref, E_S), ref


RANDOM = P.runs(("random", "saturate", "dropout"))


@pytest.mark.parametrize("r", RANDOM, ids=P.run_id)
def test_the_fp32_emulation_stays_inside_the_bounds(r):
    res, ref = _held(r)
    for k, (ratio, z) in res.items():
        assert ratio < 1.0 and abs(z) < 3.0, (P.run_id(r), k, ratio, z)
    for k in ("O", "dq", "dk", "dv"):
        assert not torch.isnan(ref[k]).any() and not torch.isinf(P.out_bound(r[0], ref, k)).any()
    if r[1] == "saturate":
        S = P.logits(r[0], P.make_inputs(r[0], r[1], r[3]), P.geometry(r[0]))[0]
        assert float(S.max()) == 65504.0 or r[0]["N"] < 8


WRONG = [r for r in RANDOM if P.mfma(r[0]) and r[0]["N"] >= 16 and r[1] != "saturate"]


@pytest.mark.parametrize("r", WRONG, ids=P.run_id)
def test_the_emulation_without_the_low_parts_leaves_the_bounds(r):
    """a build that drops the low product of a hi + lo pair (relative error 2^-9 per factor)"""
    res, _ = _held(r, drop_lo=True)
    for k in ("O", "dq", "dk", "dv"):                              # each product on its own: O without pl, dK without aGl, ...
        assert res[k][0] > 1.0 or abs(res[k][1]) > P.Z_MAX, (k, res[k])


@pytest.mark.parametrize("r", [r for r in RANDOM if r[0]["N"] >= 16 and r[1] != "saturate"], ids=P.run_id)
def test_a_denominator_wrong_by_1_in_256_leaves_the_bounds(r):
    res, _ = _held(r, denom=1.0 + 1.0 / 256)
    assert res["O"][0] > 1.0 or abs(res["O"][1]) > P.Z_MAX, res["O"]
    assert res["dv"][0] > 1.0 or abs(res["dv"][1]) > P.Z_MAX, res["dv"]
