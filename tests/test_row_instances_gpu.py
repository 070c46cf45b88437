"""The 26 LayerNorm and row-softmax kernel instances (csrc/layernorm.hip; softmax_fwd / softmax_bwd of csrc/elementwise.hip) against the
float64 reference of tests/row_cases.py, through the C entry points mmdti_layernorm_fwd / _bwd and mmdti_softmax_fwd / _bwd with explicit
pointers.  tests/test_row_cases_cpu.py proves on the CPU that the table reaches every instance and option and that the bounds hold for
an fp32 emulation and not for nine wrong ones.  Every dropout mask is the host rule of tests/dropout_rule.py (a dropped element's bound
is 0: it must be exactly 0, a kept one must not be), which test_dropout_f32_is_the_host_rule first holds, bit for bit, to the simplest
kernel, and test_the_salt_reaches_every_mask with a non-zero per-step salt.

Inputs are cut from NaN-filled arenas (the score and dp columns [Lk, ld) of the softmax are NaN), outputs from sentinel-filled ones with
guards on both sides; the gradient buffers start at row_cases.FILL.  After every launch: no NaN or sentinel where the contract gives a
value, no sentinel outside a view has moved, the pad columns [Lk, ld) of p, pd and ds are exactly 0.  Each output: worst |got - ref| /
bound <= 1 and |gain| <= 6.  const: y32 EQUALS beta; sat: the fp16 copy holds exactly +-65504 where the reference passes it, the bf16 copy
goes beyond; finfo.min keys: probabilities exactly 0, a row of them uniform at bf16(1 / Lk).

With MMDTI_ROW_PROFILE=<path> the largest ratio and |z| per instance and output are merged into that JSON file under "device"
(profiles/row_instances.json is such a run, next to the CPU emulation's own ratios under "emulation".  On MI355X the largest ratio of an
fp32 output is 0.34 (dx; mean 0.18, y32 0.17, rstd 0.14, dgamma 0.14, dbeta 0.11, colsum and colsum_own below 0.05); the 16-bit outputs
(y16, dx16, p, pd, ds), where the reference rounds too and one flipped rounding is one ulp against a bound of one ulp + L, reach 0.9999;
the largest |z| is 0.71 (y32).  The 222 tests take 7 s on the MI355X host, the slowest -- the 8197 x 516 backward -- 1.3 s.)"""
import json
import os

import pytest
import torch

from mmdti_hip import _abi, ops

import dropout_rule as DR
import row_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
F64, F32, BF16, F16 = R.F64, R.F32, R.BF16, R.F16


@pytest.fixture(scope="module", autouse=True)
def _salt_and_profile():
    ops.seed_salt_reset()                 # the salt is a device global: an earlier trainer test of this process may have left one
    yield
    path = os.environ.get("MMDTI_ROW_PROFILE")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("device", {}).update(REPORT)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(c, res):
    row = REPORT.setdefault(R.instance(c), {})
    for k, v in res.items():
        old = row.get(k, {"ratio": 0.0, "z": 0.0})
        row[k] = {"ratio": max(old["ratio"], v[0]), "z": max(old["z"], abs(v[1]))}


Bufs = lambda: R.Bufs(DEV)


def _launch_ln_fwd(c, t):
    lib, b, what = _abi.lib(), Bufs(), R.case_id(c)
    rows, D = c["rows"], c["D"]
    y32 = b.out("y32", rows, D, F32, on=c["outs"] != "y16")
    y16 = b.out("y16", rows, D, F16 if c["f16"] else BF16, on=c["outs"] != "y32")
    rz = t["rz"].to(torch.uint8).to(DEV) if t["rz"] is not None else None
    lib.mmdti_layernorm_fwd(ops._stream(), b.put(t["x"]), b.put(t["gamma"]), b.put(t["beta"]), c["eps"], rows, D, y32, y16,
                            b.out("mean", 1, rows, F32), b.out("rstd", 1, rows, F32), ops._p(rz), c["p"], R.SEED, R.SITE_LN, int(c["f16"]))
    torch.cuda.synchronize()
    return {k: b.read(k, what).view(-1) if k in ("mean", "rstd") else b.read(k, what) for k in b.outs if k != "_in"}


def _launch_ln_bwd(c, t):
    lib, b, what = _abi.lib(), Bufs(), R.case_id(c)
    rows, D = c["rows"], c["D"]
    copy = c["copy"]
    rz = t["rz"].to(torch.uint8).to(DEV) if t["rz"] is not None else None
    if c["det"]:
        assert ops.det_workspace_bytes("layernorm_bwd", rows, D) <= ops.det_workspace_mb() << 20
        ops.set_deterministic(True)
    try:
        lib.mmdti_layernorm_bwd(ops._stream(), b.put(t["dy"]), ops.DT_BF16 if c["dybf"] else ops.DT_F32, b.put(t["dy_add"]), b.put(t["x"]), b.put(t["gamma"]),
                                b.put(t["mean32"]), b.put(t["rstd32"]), rows, D, b.put(t["dres"]), b.out("dx", rows, D, F32),
                                b.out("dgamma", 1, D, F32, R.FILL, on=not c["nullg"]), b.out("dbeta", 1, D, F32, R.FILL, on=not c["nullg"]), ops._p(rz),
                                c["p"], R.SEED, R.SITE_LN, b.out("dx16", rows, D, BF16, on=copy is not None), copy[0] if copy else 0.0, R.SITE_LN2,
                                b.out("colsum", 1, D, F32, R.FILL, on=bool(copy and copy[1])))
        torch.cuda.synchronize()
    finally:
        if c["det"]:
            ops.set_deterministic(False)
    got = {k: b.read(k, what) for k in b.outs if k != "_in"}
    for k in ("dgamma", "dbeta", "colsum"):
        if k in got:
            got[k] = got[k].view(-1).to(F64) - R.FILL
    return got


def _pads_are_zero(x, Lk, what):
    assert x.shape[1] == Lk or float(x[:, Lk:].float().abs().max()) == 0.0, (what, "a pad column [Lk, ld) is not exactly 0")
    return x[:, :Lk]


def _launch_sm_fwd(c, t):
    lib, b, what = _abi.lib(), Bufs(), R.case_id(c)
    rows, Lk, ld = R.sm_rows(c), c["Lk"], c["ld"]
    p = b.out("p", rows, ld, BF16)
    pd = b.out("pd", rows, ld, BF16) if c["p"] > 0 else p                      # without dropout pd is p: aliased
    lib.mmdti_softmax_fwd(ops._stream(), b.put(t["s"], ld), b.put(t["key_add"].reshape(-1) if t["key_add"] is not None else None), p, pd,
                          c["B"], c["heads"], c["Lq"], Lk, ld, c["p"], R.SEED, R.SITE_SM)
    torch.cuda.synchronize()
    got = {k: _pads_are_zero(b.read(k, what), Lk, what) for k in b.outs if k != "_in"}
    got.setdefault("pd", got["p"])
    return got


def _launch_sm_bwd(c, t):
    lib, b, what = _abi.lib(), Bufs(), R.case_id(c)
    rows, Lk, ld = R.sm_rows(c), c["Lk"], c["ld"]
    lib.mmdti_softmax_bwd(ops._stream(), b.put(t["p16"], ld), b.put(t["dp"], ld), b.out("ds", rows, ld, BF16), c["B"], c["heads"], c["Lq"], Lk, ld,
                          c["scale"], c["p"], R.SEED, R.SITE_SM)
    torch.cuda.synchronize()
    return dict(ds=_pads_are_zero(b.read("ds", what), Lk, what))


LAUNCH = {"ln_fwd": _launch_ln_fwd, "ln_bwd": _launch_ln_bwd, "sm_fwd": _launch_sm_fwd, "sm_bwd": _launch_sm_bwd}


def _check(c, t, ref, got, record=True):
    res = R.evaluate(c, ref, got)
    if record:
        _record(c, res)
    for k, (ratio, z) in res.items():
        print(f"{R.case_id(c)} {R.instance(c)} {k}: ratio {ratio:.4g} z {z:.3g}")
    for k, (ratio, z) in res.items():
        assert ratio <= 1.0 and abs(z) <= R.Z_MAX, f"{R.instance(c)} {R.case_id(c)} {k}: worst ratio {ratio:.4g}, gain {z:.3g}"
    return res


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_instance(c):
    t, ref = R.prepared(c["i"])
    R.assert_declared_plan(_abi.lib(), c)          # (host only: the launch below is the one the case declares)
    got = LAUNCH[c["kind"]](c, t)
    res = _check(c, t, ref, got)
    k = c["kind"]
    if k == "ln_fwd":
        assert set(res) == {"mean", "rstd"} | ({"y32"} if c["outs"] != "y16" else set()) | ({"y16"} if c["outs"] != "y32" else set())
        if c["mode"] == "const":
            want = t["beta"].expand(c["rows"], -1).clone()
            if t["rz"] is not None:
                want[t["rz"]] = 0.0
            assert torch.equal(got["y32"], want), "const: y32 is not beta, bit for bit"
        if c["mode"] == "sat":
            m, want = R.saturated(c, ref)
            assert int(m.sum()) > 0
            if c["f16"]:
                assert torch.equal(got["y16"][m].to(F64), want[m]), "sat: an fp16 output past 65504 is not exactly +-65504"
                assert bool(torch.isfinite(got["y16"].float()).all())
            else:
                assert float(got["y16"].float().abs().max()) > 65504.0, "sat: the bf16 copy must not saturate"
    elif k == "ln_bwd":
        assert set(res) == {"dx"} | (set() if c["nullg"] else {"dgamma", "dbeta"}) | ({"dx16"} if c["copy"] else set()) | ({"colsum", "colsum_own"} if c["copy"] and c["copy"][1] else set())
    elif k == "sm_fwd":
        per = c["heads"] * c["Lq"]
        if c["p"] == 0:
            assert torch.equal(got["pd"], got["p"])
        if c["key_add"] == "min_all":
            assert bool((got["p"][(c["B"] - 1) * per:] == torch.tensor(1.0 / c["Lk"], dtype=F32).to(BF16)).all()), "a row of finfo.min keys is not uniform at 1 / Lk"
        if c["key_add"] == "min_half" and c["Lk"] > 1:
            assert float(got["p"][:per, c["Lk"] // 2:].float().abs().max()) == 0.0, "a finfo.min key has a non-zero probability"


# ------------------------------------------------------------------------------------------------ the keep rule on the device
def _dropout_ones(n, p, salt=0):
    lib = _abi.lib()
    b = Bufs()
    lib.mmdti_dropout_f32(ops._stream(), b.put(torch.ones(n)), b.out("y", 1, n, F32), n, p, R.SEED, 3)
    torch.cuda.synchronize()
    got = b.read("y", f"dropout_f32 n={n} p={p}").view(-1)
    want = torch.from_numpy(DR.keep_flat(R.SEED, 3, n, p, salt)).to(F32) * torch.tensor(DR.dscale(p), dtype=F32)
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f"dropout_f32(ones) p={p}: {bad.numel()} of {n} elements differ from the host rule, the first at {int(bad[0])}"


@pytest.mark.parametrize("p", (0.1, 0.35, 0.999))
def test_dropout_f32_is_the_host_rule(p):
    _dropout_ones(1048576 + 1027, p)          # past the 4096-workgroup cap: the grid-stride second round, and a ragged tail


def _cast_ones(n, p, salt):
    lib, b = _abi.lib(), Bufs()
    lib.mmdti_cast_f32_bf16(ops._stream(), b.put(torch.ones(n)), b.out("y", 1, n, BF16), n, p, R.SEED, 5)
    torch.cuda.synchronize()
    got = b.read("y", "cast_f32_bf16").view(-1)
    want = (torch.from_numpy(DR.keep_flat(R.SEED, 5, n, p, salt)).to(F32) * torch.tensor(DR.dscale(p), dtype=F32)).to(BF16)
    assert torch.equal(got, want), "cast_f32_bf16: the mask is not the host rule's"


def test_the_salt_reaches_every_mask():
    """a non-zero per-step salt: the LayerNorm forward, cast, dropout_f32 and softmax masks are keep(..., salt=S)"""
    lib = _abi.lib()
    S = 0x9E3779B97F4A7C15 ^ 0x0123456789ABCDEF
    word = torch.tensor([S - (1 << 64) if S >= 1 << 63 else S], dtype=torch.int64, device=DEV)
    ln = next(c for c in R.CASES if c["kind"] == "ln_fwd" and c["p"] > 0 and c["rows"] == 37 and c["mode"] == "random" and c["outs"] != "y16")
    sm = next(c for c in R.CASES if c["kind"] == "sm_fwd" and c["p"] > 0 and R.sm_rows(c) == 42 and c["ld"] > c["Lk"] > 100)
    try:
        lib.mmdti_seed_salt_pull(ops._stream(), word.data_ptr())
        torch.cuda.synchronize()
        _dropout_ones(4099, 0.35, S)
        _cast_ones(4099, 0.35, S)
        for c in (ln, sm):
            t = R.make_inputs(c, salt=S)
            assert not torch.equal(t["keep"], R.prepared(c["i"])[0]["keep"])
            _check(c, t, R.chain(c, t), LAUNCH[c["kind"]](c, t), record=False)
    finally:
        ops.seed_salt_reset()
    _dropout_ones(4099, 0.35, 0)
