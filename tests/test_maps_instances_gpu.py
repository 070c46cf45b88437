"""The twelve kernel instances of csrc/attn_maps.hip against the float64 references of tests/maps_cases.py, through the C entry points
mmdti_attn_map and mmdti_pair_attn_map.  tests/test_maps_cases_cpu.py proves on the CPU that the tables reach every instance and
that the bounds hold for an fp32 emulation of the kernels' rounding points.

q, k and the pair logits are cut from NaN-filled arenas, `out` from a sentinel-filled one.  After every launch every element of
`out` is written and finite, no sentinel outside it has changed, and a second call gives the same bits.  The fused map's row
statistics come from the matching forward entry point (mmdti_attn_fwd, or mmdti_attn_long_fwd past 256) on the same operands, in
the layout that forward writes (dense [B,heads,Lq,2], packed [heads,q_rows,2]).  In the ragged pair cases every skipped key tile and
every row from n_real on of `s` holds NaN bit patterns: the output is finite, and exactly 0 there.
  selector, uniform   the map EQUALS what the mode requires, bit for bit
  random              elementwise within the derived bound"""
import pytest
import torch

from mmdti_hip import _abi, ops

import maps_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _arena(rows, cols, ld, dtype, out=False):
    return M.Arena((rows, cols, ld, 0, 0, rows * ld), (1, 1), dtype, DEV, out=out)


def _finish(rid, out_arena, launch):
    """launch twice into the sentinel-filled arena -> the output on the CPU, after the write / bounds / repeat checks"""
    launch()
    torch.cuda.synchronize()
    assert out_arena.outside_untouched() == 0, (rid, "a store outside the output")
    first = out_arena.view[0, 0].clone()
    assert int((out_arena.iview[0, 0] == out_arena.sent).sum()) == 0, (rid, "an element of out was never written")
    assert bool(torch.isfinite(first).all()), (rid, "a non-finite value: a read outside an operand")
    out_arena.iview[0, 0].fill_(out_arena.sent)
    launch()
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), out_arena.view[0, 0].view(torch.int32)), (rid, "two calls differ")
    return first.cpu()


def _attn_map(c, t, head):
    lib = _abi.lib()
    hd, H, B = c["hd"], c["heads"], c["B"]
    D = H * hd
    rq, rk = t["rows_q"], t["rows_k"]
    pad = 8 if c["vec"] else 0
    Aq, Ak = _arena(rq, D, D + pad, M.BF16), _arena(rk, D, D + pad, M.BF16)
    Aq.view[0, 0].copy_(t["q"].to(DEV))
    Ak.view[0, 0].copy_(t["k"].to(DEV))
    add = t["add"].to(DEV).contiguous() if t["add"] is not None else None
    vl, vargs = None, (0, 0, 0, 0)
    if c["packed"] is not None:
        from mmdti_hip.packing import PackedRows
        ql, kl, Sq, Sk = c["packed"]
        vl = ops.AttnVarlen(PackedRows(torch.tensor(ql), Sq, device=DEV), PackedRows(torch.tensor(kl), Sk, device=DEV))
        assert (vl.Lq, vl.Lk, vl.q_rows, vl.k_rows) == (c["Lq"], c["Lk"], rq, rk)
        vargs = vl.args()
    # the forward of this attention: its stats, in its layout
    v = torch.zeros(rk, D + pad, device=DEV, dtype=M.BF16)
    ctx = torch.empty(rq, D, device=DEV, dtype=M.BF16)
    nstat = 2 * H * (rq if vl is not None else B * c["Lq"])
    stats = torch.full((nstat,), float("nan"), device=DEV, dtype=M.F32)
    fwd = lib.mmdti_attn_long_fwd if max(c["Lq"], c["Lk"]) > 256 else lib.mmdti_attn_fwd
    fwd(ops._stream(), Aq.ptr(), Ak.ptr(), v.data_ptr(), ops._p(add), ctx.data_ptr(), stats.data_ptr(), B, H, c["Lq"], c["Lk"], hd, D + pad, D + pad, D,
        t["scale"], 0.0, 1, 1, *vargs, 0)
    q_cnt = torch.tensor(c["qcnt"], dtype=torch.int32, device=DEV) if c["qcnt"] is not None else None
    out = _arena(B * c["Lq_out"], c["ld_out"], c["ld_out"], M.F32, out=True)
    got_plan = M.library_attn_plan(lib, B, H, c["Lq"], c["Lk"], hd, c["Lq_out"], c["ld_out"], head, Aq.ptr(), Ak.ptr(), ops._p(add), stats.data_ptr(),
                                   out.ptr(), D + pad, D + pad, vargs, ops._p(q_cnt))
    assert got_plan == M.declared_attn_plan(B, c["Lq_out"], c["ld_out"], hd)

    def launch():
        lib.mmdti_attn_map(ops._stream(), Aq.ptr(), Ak.ptr(), ops._p(add), stats.data_ptr(), out.ptr(), B, H, c["Lq"], c["Lk"], hd, D + pad, D + pad,
                           c["Lq_out"], c["ld_out"], t["scale"], head, *vargs, ops._p(q_cnt))

    got = _finish(M.attn_case_id(c), out, launch)
    return got.view(B, c["Lq_out"], c["ld_out"])


@pytest.mark.parametrize("r", M.attn_runs(("selector", "uniform")), ids=M.run_id)
def test_attn_map_exact(r):
    c, mode = r
    t = M.attn_inputs(c, mode)
    for head in (-1, c["heads"] - 1):
        want = (M.attn_selector_expectation if mode == "selector" else M.attn_uniform_expectation)(c, t, head)
        got = _attn_map(c, t, head)
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), (M.run_id(r), head, int(bad.sum()), "first at", bad.nonzero()[0].tolist())


@pytest.mark.parametrize("r", M.attn_runs(("random",)), ids=M.run_id)
def test_attn_map_random(r):
    c, mode = r
    t = M.attn_inputs(c, mode)
    for head in (-1, 1):
        ref, bnd = M.attn_reference(c, t, head)
        got = _attn_map(c, t, head)
        ratio = M.worst_ratio(got, ref, bnd)
        print(M.run_id(r), head, round(ratio, 4))
        assert ratio <= 1.0, (M.run_id(r), head, ratio)
        assert float(got[ref == 0].abs().max() if bool((ref == 0).any()) else 0.0) == 0.0, (M.run_id(r), head, "a masked position is not zero")


def _pair_map(c, t, head):
    lib = _abi.lib()
    B, H, N = c["B"], c["H"], c["N"]
    flat, kts, nrl = M.pair_store(c, t)
    As = _arena(1, flat.numel(), flat.numel(), M.pair_dtype(c))
    As.view[0, 0, 0].copy_(flat.to(DEV))
    kt = torch.tensor(kts, dtype=torch.int32, device=DEV) if kts is not None else None
    nr = torch.tensor(nrl, dtype=torch.int32, device=DEV) if nrl is not None else None
    out = _arena(B * N, c["ld_out"], c["ld_out"], M.F32, out=True)
    assert M.library_pair_plan(lib, B, N, H, c["ld"], c["ld_out"], c["layout"], head, As.ptr(), out.ptr(), ops._p(kt), ops._p(nr)) == \
        M.declared_pair_plan(B, N, c["layout"])

    def launch():
        lib.mmdti_pair_attn_map(ops._stream(), As.ptr(), out.ptr(), B, N, H, c["ld"], c["ld_out"], head, c["layout"], ops._p(kt), ops._p(nr))

    return _finish(M.pair_case_id(c), out, launch).view(B, N, c["ld_out"])


def _ragged_zeros(c, t, got):
    """a ragged case: exactly 0 in every skipped tile and in every row from n_real on"""
    if c["lens"] is None:
        return
    nt = M.cdiv(c["N"], 16)
    for b, n in enumerate(t["lens"]):
        k0 = 16 * M.pa_kt_effective(M.cdiv(n, 16), nt)
        assert float(got[b, n:].abs().max() if n < c["N"] else 0.0) == 0.0 and float(got[b, :, k0:].abs().max() if k0 < c["ld_out"] else 0.0) == 0.0


@pytest.mark.parametrize("r", M.pair_runs(("selector", "uniform")), ids=M.run_id)
def test_pair_attn_map_exact(r):
    c, mode = r
    t = M.pair_inputs(c, mode)
    for head in (-1, c["H"] - 1):
        want = (M.pair_selector_expectation if mode == "selector" else M.pair_uniform_expectation)(c, t, head)
        got = _pair_map(c, t, head)
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), (M.run_id(r), head, int(bad.sum()), "first at", bad.nonzero()[0].tolist())
        _ragged_zeros(c, t, got)


@pytest.mark.parametrize("r", M.pair_runs(("random",)), ids=M.run_id)
def test_pair_attn_map_random(r):
    c, mode = r
    t = M.pair_inputs(c, mode)
    for head in (-1, 1):
        ref, bnd = M.pair_reference(c, t, head)
        got = _pair_map(c, t, head)
        ratio = M.worst_ratio(got, ref, bnd)
        print(M.run_id(r), head, round(ratio, 4))
        assert ratio <= 1.0, (M.run_id(r), head, ratio)
        _ragged_zeros(c, t, got)


def test_ops_wrappers():
    """ops.attn_map / ops.pair_attn_map: the tensors' own shapes and strides reach the library"""
    c = next(x for x in M.ATTN_CASES if x["hd"] == 32 and (x["Lq"], x["Lk"]) == (17, 33) and x["packed"] is None)
    t = M.attn_inputs(c, "random")
    q, k = t["q"].to(DEV), t["k"].to(DEV)
    add = t["add"].to(DEV)
    _, stats = ops.attn_fwd(q, k, torch.zeros_like(k), add, c["B"], c["heads"], c["Lq"], c["Lk"], t["scale"])
    got = ops.attn_map(q, k, add, stats, c["B"], c["heads"], c["Lq"], c["Lk"], t["scale"]).cpu()
    c2 = dict(c, ld_out=c["Lk"])
    ref, bnd = M.attn_reference(c2, t)
    assert M.worst_ratio(got, ref, bnd) <= 1.0
    pc = next(x for x in M.PAIR_CASES if x["N"] == 22 and x["layout"] == 3)
    pt = M.pair_inputs(pc, "random")
    s = ops.pair_tile(pt["S"].to(DEV), pc["N"]).to(M.F16)
    gotp = ops.pair_attn_map(s, pc["B"], pc["N"], pc["H"], pc["ld"]).cpu()
    refp, bndp = M.pair_reference(dict(pc, ld_out=pc["N"]), pt)
    assert M.worst_ratio(gotp, refp, bndp) <= 1.0
    with pytest.raises(_abi.MMDTIError, match="key_tiles needs n_real"):
        ops.pair_attn_map(s, pc["B"], pc["N"], pc["H"], pc["ld"], key_tiles=torch.ones(pc["B"], dtype=torch.int32, device=DEV))
