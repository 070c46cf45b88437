"""The 27 kernel instances of csrc/attn.hip (forward and dQ at head_dim 16 / 32 / 64 x 10 / 16 / 24 / 32 score tiles, dK/dV at three head
sizes) against the float64 reference of tests/attn_cases.py, through the C entry points mmdti_attn_fwd / _bwd and
mmdti_attn_long_fwd / _bwd.  tests/test_attn_cases_cpu.py proves on the CPU that the table reaches every instance and that the
bounds hold for an fp32 emulation of the kernels' rounding points.

q, k, v and dctx are cut from NaN-filled arenas (masked keys are real rows with finite values; only memory outside the operands
is NaN), ctx, stats, drow, dq, dk and dv from sentinel-filled ones, in the case's row layout (tight, padded, q|k|v slices of one
[rows, 3D] buffer, k|v slices of [rows, 2D], ctx at D + 4).  After every launch no output holds a NaN (a read outside an
operand, or an element never stored) and no sentinel outside an output view has changed (a store outside the output).
  selector, uniform   the outputs EQUAL what the mode requires, bit for bit
  random, large, dropout   elementwise within the derived bounds, |gain| <= 6, stats and drow within their fp32 bounds

With MMDTI_ATTN_PROFILE=<path> the largest |got - ref| / bound and |z| of every instance and output are written there as JSON
(profiles/attn_instances.json is such a run: on MI355X the largest ratio is 0.90 -- dv of attn_bwd_kv_kernel<64> --, the largest
|z| 2.8, stats and drow below 0.04 of their fp32 bounds; the 216 tests take 4.5 s)."""
import json
import os

import pytest
import torch

from mmdti_hip import _abi, ops
from mmdti_hip._abi import MMDTIError

import attn_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MMDTI_ATTN_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(c, res):
    fwd, bq, bkv = A.instances(c)
    for inst, keys in ((fwd, ("ctx", "stats_m", "stats_lse")), (bq, ("dq", "drow")), (bkv, ("dk", "dv"))):
        row = REPORT.setdefault(inst, {})
        for k in keys:
            old = row.get(k, {"ratio": 0.0, "z": 0.0})
            row[k] = {"ratio": max(old["ratio"], res[k][0]), "z": max(old["z"], abs(res[k][1]))}


def _varlen(c, t):
    if t["packed"] is None:
        return None, (0, 0, 0, 0)
    from mmdti_hip.packing import PackedRows
    ql, kl, Sq, Sk = c["packed"]
    vl = ops.AttnVarlen(PackedRows(torch.tensor(ql), Sq, device=DEV), PackedRows(torch.tensor(kl), Sk, device=DEV))
    assert (vl.Lq, vl.Lk, vl.q_rows, vl.k_rows) == (c["Lq"], c["Lk"], t["rows_q"], t["rows_k"])
    assert vl.q_off.tolist() == t["packed"]["q_off"] and vl.k_off.tolist() == t["packed"]["k_off"] and vl.k_cnt.tolist() == t["packed"]["k_cnt"]
    return vl, vl.args()


def _launch(c, t, p_drop=0.0, entry=None):
    """forward and backward of a case on arenas -> (placement, got) with got on the CPU in the layout of attn_cases.evaluate"""
    lib = _abi.lib()
    pl = A.place(c, t, DEV)
    P, ld, arenas = pl["ptr"], pl["ld"], pl["arenas"]
    vl, vargs = _varlen(c, t)
    nb = len(t["seqs"])
    name = {"short": "mmdti_attn", "long": "mmdti_attn_long"}[entry or c["entry"]]
    add = arenas["add"].ptr() if "add" in arenas else 0
    A.assert_declared_plan(lib, c, nb, dict(P, stats=arenas["stats"].ptr(), drow=arenas["drow"].ptr()), ld, add, vargs, p_drop, entry or c["entry"])
    getattr(lib, name + "_fwd")(ops._stream(), P["q"], P["k"], P["v"], add, P["ctx"], arenas["stats"].ptr(), nb, A.HEADS, c["Lq"], c["Lk"], c["hd"],
                                ld["q"], ld["k"], ld["ctx"], t["scale"], p_drop, A.SEED, A.SITE, *vargs, c["ctx_f16"])
    getattr(lib, name + "_bwd")(ops._stream(), P["q"], P["k"], P["v"], add, P["do"], arenas["stats"].ptr(), arenas["drow"].ptr(), P["dq"], P["dk"],
                                P["dv"], nb, A.HEADS, c["Lq"], c["Lk"], c["hd"], ld["q"], ld["k"], ld["do"], ld["dq"], ld["dk"], t["scale"], p_drop,
                                A.SEED, A.SITE, *vargs)
    torch.cuda.synchronize()
    rid = A.case_id(c)
    for n in pl["outs"]:
        assert arenas[n].outside_untouched() == 0, (rid, n, "a store outside the output")
    got = {n: pl["views"][n].cpu() for n in ("ctx", "dq", "dk", "dv")}
    stats, drow = arenas["stats"].view.flatten().cpu(), arenas["drow"].view.flatten().cpu()
    for n, x in list(got.items()) + [("stats", stats), ("drow", drow)]:
        assert not bool(torch.isnan(x.float()).any()), (rid, n, "NaN: a read outside an operand, or an element never stored")
    st = A.split_stats(c, t, stats, 2)
    got.update(m2=[s[..., 0] for s in st], inv=[s[..., 1] for s in st], r=[x[..., 0] for x in A.split_stats(c, t, drow, 1)])
    return pl, got


def _pad_rows_are_zero(c, t, got):
    """packed rows: the representative pad row of the key side receives dk = dv = 0 exactly"""
    for (q0, lq, k0, lk, krows) in t["seqs"]:
        if krows > lk:
            assert float(got["dk"][k0 + lk:k0 + krows].float().abs().max()) == 0.0 and float(got["dv"][k0 + lk:k0 + krows].float().abs().max()) == 0.0


@pytest.mark.parametrize("r", A.runs(("selector",)), ids=A.run_id)
def test_selector(r):
    c = r[0]
    t = A.make_inputs(c, "selector")
    _, got = _launch(c, t)
    ctx, dv, m = A.selector_expectation(c, t)
    for name, g, want in (("ctx", got["ctx"], ctx), ("dv", got["dv"], dv)):
        bad = g.to(A.F64) != want
        assert not bool(bad.any()), (A.run_id(r), name, int(bad.sum()), "first at", bad.nonzero()[0].tolist())
    assert float(got["dq"].float().abs().max()) == 0.0 and float(got["dk"].float().abs().max()) == 0.0, A.run_id(r)
    for b in range(len(t["seqs"])):
        assert bool((got["m2"][b] == m).all()) and bool((got["inv"][b] == 1.0).all()), (A.run_id(r), b)
    _pad_rows_are_zero(c, t, got)


@pytest.mark.parametrize("r", A.runs(("uniform",)), ids=A.run_id)
def test_uniform(r):
    c = r[0]
    t = A.make_inputs(c, "uniform")
    _, got = _launch(c, t)
    ref = A.reference(c, t, exact=True, bounds=False)
    for k in ("ctx", "dq", "dk", "dv"):
        want = A.round16(ref[k], A.ctx_dtype(c) if k == "ctx" else A.BF16).to(A.F64)
        bad = got[k].to(A.F64) != want
        assert not bool(bad.any()), (A.run_id(r), k, int(bad.sum()), "first at", bad.nonzero()[0].tolist(), float(got[k][bad][0]), float(want[bad][0]))
    for b, n in enumerate(t["n_real"]):
        assert bool((got["m2"][b] == 0).all()) and bool((got["inv"][b] == 1.0 / n).all()), (A.run_id(r), b)
        assert torch.equal(got["r"][b].to(A.F64), ref["r"][b]), (A.run_id(r), b)
    _pad_rows_are_zero(c, t, got)


def _held(r, t, got, p=0.0, keep=None):
    c = r[0]
    ref = A.reference(c, t, p, keep)
    res = A.evaluate(c, ref, got)
    print(A.run_id(r), {k: (round(v[0], 4), round(v[1], 2)) for k, v in res.items()})
    _record(c, res)
    for k, (ratio, z) in res.items():
        assert ratio <= 1.0 and abs(z) <= A.Z_MAX, (A.run_id(r), k, ratio, z)
    _pad_rows_are_zero(c, t, got)


@pytest.mark.parametrize("r", A.runs(("random", "large")), ids=A.run_id)
def test_random_and_large(r):
    c, mode, _ = r
    t = A.make_inputs(c, mode)
    _, got = _launch(c, t)
    _held(r, t, got)
    if c["allmask"]:                                   # every key masked: the uniform row
        b = len(t["seqs"]) - 1
        assert bool(((got["inv"][b].double() * c["Lk"] - 1.0).abs() <= 2.0 ** -22).all()) and bool((got["m2"][b] == -A.FLT_MAX).all())


def _recover_keep(c, t, p, entry):
    """the forward's keep mask through indicator V columns, at q = 0 (every probability 1 / Lk): [B, heads, Lq, Lk] bool"""
    hd, Lq, Lk, nb = c["hd"], c["Lq"], c["Lk"], len(t["seqs"])
    D = A.HEADS * hd
    fwd = ops.attn_fwd if entry == "short" else ops.attn_long_fwd
    z = torch.zeros(nb * Lq, D, dtype=A.BF16, device=DEV)
    kz = torch.zeros(nb * Lk, D, dtype=A.BF16, device=DEV)
    keep = torch.zeros(nb, A.HEADS, Lq, Lk, dtype=torch.bool)
    for c0 in range(0, Lk, hd):
        n = min(hd, Lk - c0)
        vi = torch.zeros(nb, Lk, A.HEADS, hd)
        for j in range(n):
            vi[:, c0 + j, :, j] = 1.0
        ctx, _ = fwd(z, kz, vi.view(nb * Lk, D).to(A.BF16).to(DEV), None, nb, A.HEADS, Lq, Lk, 1.0, p, A.SEED, A.SITE)
        keep[..., c0:c0 + n] = (ctx.view(nb, Lq, A.HEADS, hd).permute(0, 2, 1, 3)[..., :n] != 0).cpu()
    return keep


@pytest.mark.parametrize("r", A.runs(("dropout",)), ids=A.run_id)
def test_dropout(r):
    c, _, p = r
    t = A.make_inputs(c, "dropout")
    keep = _recover_keep(c, t, p, c["entry"])
    n = keep.numel()
    rate, sd = float(keep.sum()) / n, (p * (1 - p) / n) ** 0.5
    assert abs(rate - (1 - p)) <= 4 * sd, (A.run_id(r), rate)
    if max(c["Lq"], c["Lk"]) <= 256:                   # both entry points launch one instance there: one mask
        other = "long" if c["entry"] == "short" else "short"
        assert torch.equal(keep, _recover_keep(c, t, p, other)), A.run_id(r)
    _, got = _launch(c, t, p)
    _held(r, t, got, p, [keep[b] for b in range(keep.shape[0])])


@pytest.mark.parametrize("hd,nt", [(16, 10), (32, 16), (64, 10), (64, 16)])
def test_both_entry_points_launch_one_instance_up_to_256_keys(hd, nt):
    c = next(c for c in A.CASES if c["hd"] == hd and c["nt"] == nt and c["entry"] == "short" and c["packed"] is None and "dropout" in c["modes"])
    t = A.make_inputs(c, "random")
    (_, a), (_, b) = _launch(c, t, 0.1, "short"), _launch(c, t, 0.1, "long")
    for k in ("ctx", "dq", "dk", "dv"):
        assert torch.equal(a[k], b[k]), k
    for k in ("m2", "inv", "r"):
        assert all(torch.equal(x, y) for x, y in zip(a[k], b[k])), k


def _plain(hd=32):
    D = A.HEADS * hd
    z = lambda rows, w=D: torch.zeros(rows, w, dtype=A.BF16, device=DEV)
    return D, z


def test_the_wrappers_refuse_a_v_whose_row_stride_is_not_k_s():
    """ops._attn_fwd / _attn_bwd hand the library ONE key-side row stride: a v with another must not reach a launch"""
    D, z = _plain()
    q, k, v = z(16), z(16), z(16, D + 8)[:, :D]
    with pytest.raises(MMDTIError, match="row stride"):
        ops.attn_fwd(q, k, v, None, 1, A.HEADS, 16, 16, 0.25)
    st = torch.zeros(1, A.HEADS, 16, 2, device=DEV)
    for bwd in (ops.attn_bwd, ops.attn_long_bwd):
        with pytest.raises(MMDTIError, match="row stride"):
            bwd(q, k, v, None, z(16), st, 1, A.HEADS, 16, 16, 0.25)


def test_the_backward_wrapper_refuses_operands_of_another_stride_or_type():
    D, z = _plain()
    st = torch.zeros(1, A.HEADS, 16, 2, device=DEV)
    good = dict(q=z(16), k=z(16), v=z(16), dctx=z(16))
    for name in good:
        for bad in (z(16, 2 * D)[:, ::2], z(16).to(torch.float16)):           # column stride 2; fp16
            a = dict(good, **{name: bad})
            with pytest.raises(MMDTIError):
                ops.attn_bwd(a["q"], a["k"], a["v"], None, a["dctx"], st, 1, A.HEADS, 16, 16, 0.25)
    dq, dk, dv = ops.attn_bwd(good["q"], good["k"], good["v"], None, good["dctx"], ops.attn_fwd(good["q"], good["k"], good["v"], None, 1, A.HEADS, 16, 16, 0.25)[1],
                              1, A.HEADS, 16, 16, 0.25)
    assert float(dq.float().abs().max()) == 0.0
