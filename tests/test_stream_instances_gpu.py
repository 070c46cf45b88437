"""The stream kernels of csrc/elementwise.hip -- the four casts, dropout_f32, axpy, GELU, the column sums in both modes, the three forms of
the sum of squares with its non-finite count and guard, the four adam_kernel<GUARD, MASK> instantiations over three steps and the step
state -- against the references of tests/stream_cases.py, through the C entry points with explicit pointers, at n = 1, 3, 1027 and at
the sizes that pass each launcher's grid cap once with a ragged tail.  tests/test_stream_cases_cpu.py proves on the CPU that the table
reaches every kernel and instantiation, that the fp32 emulation stays inside the bounds and that six wrong emulations do not.

Inputs are cut from NaN-filled arenas (the bf16 elements behind column `cols` of a column-sum operand are NaN), outputs from
sentinel-filled ones with guards on both sides; column sums start at stream_cases.FILL.  After every launch no sentinel outside a view
has moved and no NaN stands where the contract gives a value.  Casts, dropout and the exact modes must EQUAL the reference (16-bit
values as bit patterns); the rest: worst |got - ref| / bound <= 1 and |gain| <= 6.  Adam: masked groups keep their bits in all five
buffers (the shadows: the sentinel), a flagged step leaves every buffer untouched, the shadows EQUAL the rounding of the device's own p.

With MMDTI_ROW_PROFILE=<path> the largest ratio and |z| per kernel and output are merged into that JSON file under "device"
(profiles/row_instances.json: on MI355X the casts, dropout and every exact mode EQUAL the reference; Adam's p reaches 0.98 of its bound
-- three roundings of p against 3 U |p| where the step is small --, m 0.30, v 0.33; GELU 0.89, axpy 0.50, the sums of squares 0.04, the
column sums 0.006, the step state's bias corrections 0.32; the largest |z| is 1.2.  The 144 tests take 3.5 s on the MI355X host, the
slowest -- the 4 195 335-element cast with dropout -- 0.2 s.)"""
import json
import os

import pytest
import torch

from mmdti_hip import _abi, ops

import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
F64, F32, BF16, F16 = S.F64, S.F32, S.BF16, S.F16
B1, B2, EPS = 0.9, 0.999, 1e-8
Bufs = lambda: S.Bufs(DEV)


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
    for name in S.instance(c):
        row = REPORT.setdefault(name, {})
        for k, v in res.items():
            old = row.get(k, {"ratio": 0.0, "z": 0.0})
            row[k] = {"ratio": max(old["ratio"], v[0]), "z": max(old["z"], abs(v[1]))}


def _inout(b, name, x):
    """an operand the kernel updates in place: a sentinel arena holding x"""
    ptr = b.out(name, 1, x.numel(), x.dtype)
    b.outs[name].view[0, 0, 0].copy_(x.to(DEV))
    return ptr


def _launch_cast(c, t):
    lib, b, n = _abi.lib(), Bufs(), c["n"]
    fn = lib.mmdti_cast_f32_f16 if c["f16"] else lib.mmdti_cast_f32_bf16
    y = b.out("y", 1, n, F16 if c["f16"] else BF16)
    fn(ops._stream(), b.put(t["x"]), y, n, c["p"], S.SEED, S.SITE)
    torch.cuda.synchronize()
    a = b.outs["y"]
    assert a.outside_untouched() == 0, "a store outside the output"
    return dict(y=S.bits16(a.view[0, 0, 0].cpu()))              # (inf and the saturated values are data here: compared as bits)


def _launch_dropout(c, t):
    lib, b, n = _abi.lib(), Bufs(), c["n"]
    lib.mmdti_dropout_f32(ops._stream(), b.put(t["x"]), b.out("y", 1, n, F32), n, c["p"], S.SEED, S.SITE)
    torch.cuda.synchronize()
    a = b.outs["y"]
    assert a.outside_untouched() == 0, "a store outside the output"
    return dict(y=a.view[0, 0, 0].cpu())


def _launch_cast_hb(c, t):
    lib, b = _abi.lib(), Bufs()
    lib.mmdti_cast_f16_bf16(ops._stream(), b.put(t["x"], c["ldx"]), c["rows"], c["cols"], c["ldx"], b.out("y", c["rows"], c["cols"], BF16))
    torch.cuda.synchronize()
    return dict(y=S.bits16(b.read("y", S.case_id(c))))


def _launch_cast_b32(c, t):
    lib, b = _abi.lib(), Bufs()
    lib.mmdti_cast_bf16_f32(ops._stream(), b.put(t["x"]), b.out("y", 1, c["n"], F32), c["n"])
    torch.cuda.synchronize()
    return dict(y=b.read("y", S.case_id(c)).view(-1))


def _launch_axpy(c, t):
    lib, b = _abi.lib(), Bufs()
    lib.mmdti_axpy_f32(ops._stream(), b.put(t["x"]), _inout(b, "y", t["y"]), c["n"], c["a"])
    torch.cuda.synchronize()
    return dict(y=b.read("y", S.case_id(c)).view(-1))


def _launch_gelu(c, t):
    lib, b = _abi.lib(), Bufs()
    lib.mmdti_gelu_fwd_bf16(ops._stream(), b.put(t["u"]), b.out("y", 1, c["n"], BF16), c["n"])
    torch.cuda.synchronize()
    return dict(y=b.read("y", S.case_id(c)).view(-1))


def _launch_colsum(c, t):
    lib, b = _abi.lib(), Bufs()
    if c["det"]:
        assert ops.det_workspace_bytes("colsum", c["rows"], c["cols"]) <= ops.det_workspace_mb() << 20
        ops.set_deterministic(True)
    try:
        lib.mmdti_colsum_bf16(ops._stream(), b.put(t["x"], c["ld"]), c["rows"], c["cols"], c["ld"], b.out("out", 1, c["cols"], F32, S.FILL))
        torch.cuda.synchronize()
    finally:
        if c["det"]:
            ops.set_deterministic(False)
    return dict(out=b.read("out", S.case_id(c)).view(-1).to(F64) - S.FILL)


GUARD0 = (1.0, 2.0, 0.0, 0.5, 0.25)          # the guard before a table case: one step taken, two skipped
TABLE = ((0.625, 0.0625), (0.875, 0.4375), (0.9375, 0.71875))


def _launch_sumsq(c, t):
    lib, b, n, form = _abi.lib(), Bufs(), c["n"], c["form"]
    g = b.put(t["x"])
    out = b.out("out", 1, 3, F32, 0.0)
    ws = b.out("ws", 1, c["ws"], F32) if form != "atomic" else 0
    guard = table = None
    if form == "atomic":
        lib.mmdti_sumsq_f32(ops._stream(), g, n, out, 0, 0)
    elif form == "part":
        lib.mmdti_sumsq_f32(ops._stream(), g, n, out, ws, c["ws"])
    else:
        if form != "check":
            guard = torch.tensor(GUARD0 if form == "guard_table" else (0.0,) * 5, dtype=F32, device=DEV)
        if form == "guard_table":
            table = torch.tensor(TABLE, dtype=F32, device=DEV)
        lib.mmdti_sumsq_check_f32(ops._stream(), g, n, out, ws, c["ws"], ops._p(guard), ops._p(table), 0 if table is None else len(TABLE), B1, B2)
    torch.cuda.synchronize()
    assert b.outs["out"].outside_untouched() == 0 and (form == "atomic" or b.outs["ws"].outside_untouched() == 0), "a store outside out or the workspace"
    o = b.outs["out"].view[0, 0, 0].cpu()
    got = dict(sum=float(o[0]), count=int(o[1]))
    if form in ("atomic", "part"):
        got["count"] = int((~torch.isfinite(t["x"])).sum())            # (these forms do not count)
        assert float(o[1]) == 0.0 and float(o[2]) == 0.0
    if guard is not None:
        skip = got["count"] != 0
        gw = guard.cpu()
        assert float(o[2]) == float(skip), "out[2] is not the skip flag"
        if form == "guard_table":
            want = (1.0, 3.0, 1.0, 0.5, 0.25) if skip else (2.0, 2.0, 0.0) + TABLE[1]
            assert gw.tolist() == list(want), f"the guard's five words {gw.tolist()} are not {want}"
        elif skip:
            assert gw.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]
        else:
            (bc1, e1), (bc2, e2) = S.step_bias(1)
            assert gw[:3].tolist() == [1.0, 0.0, 0.0] and abs(float(gw[3]) - bc1) <= e1 and abs(float(gw[4]) - bc2) <= e2
    elif form == "check":
        assert float(o[2]) == 0.0
    return got


def _launch_adam(c, t):
    lib, b, n = _abi.lib(), Bufs(), c["n"]
    ptr = {k: _inout(b, k, t[k]) for k in ("p", "m", "v")}
    pb = b.out("pb", 1, n, BF16, on="bf16" in c["shadows"])
    ph = b.out("ph", 1, n, F16, on="f16" in c["shadows"])
    skip = t["skip"].to(DEV) if c["mask"] else None
    gs = torch.tensor([c["gs"]], dtype=F32, device=DEV) if c["gs"] is not None else None
    names = [k for k in ("p", "m", "v", "pb", "ph") if k in b.outs]
    snap = lambda: {k: b.outs[k].buf.view(b.outs[k].ibits).clone() for k in names}
    for st, g in zip(t["steps"], t["g"]):
        by_ptr = c["state"] or c["guard"]
        state = torch.tensor([st["step"], st["lr"], st["bc1"], st["bc2"]], dtype=F32, device=DEV) if c["state"] else None
        guard = torch.tensor([st["step"], 0.0, float(st["flag"]), st["bc1"], st["bc2"]], dtype=F32, device=DEV) if c["guard"] else None
        lr = 123.0 if c["state"] else st["lr"]                          # (with a step state the by-value rate must not be read)
        step = st["step"] if not by_ptr else 7
        before = snap() if st["flag"] else None
        head = (ops._stream(), ptr["p"], b.put(g), ptr["m"], ptr["v"], pb, n, lr, B1, B2, EPS, c["wd"])
        if c["mask"]:
            lib.mmdti_adam_step_masked(*head, step, ops._p(gs), ops._p(state), ph, ops._p(guard), skip.data_ptr())
        elif c["guard"]:
            lib.mmdti_adam_step_guarded(*head, ops._p(gs), ops._p(state), ph, guard.data_ptr())
        else:
            lib.mmdti_adam_step(*head, step, ops._p(gs), ops._p(state), ph)
        torch.cuda.synchronize()
        if before is not None:
            after = snap()
            assert all(torch.equal(before[k], after[k]) for k in names), "a step under a set guard flag wrote to a buffer"
    for k in names:
        assert b.outs[k].outside_untouched() == 0, (k, "a store outside the buffer")
    got = {k: b.outs[k].view[0, 0, 0].cpu() for k in names}
    assert not any(bool(torch.isnan(got[k]).any()) for k in ("p", "m", "v"))
    live = torch.ones(n, dtype=torch.bool) if not c["mask"] else ~t["skip"].bool().repeat_interleave(8)[:n]
    for k in ("p", "m", "v"):
        assert torch.equal(got[k][~live].view(torch.int32), t[k][~live].view(torch.int32)), f"{k}: a masked element changed"
    for k, dt in (("pb", BF16), ("ph", F16)):
        if k in got:
            bits = S.bits16(got[k])
            assert bool((bits[~live] == S.SENT16).all()), f"{k}: a masked element of the shadow was written"
            assert torch.equal(bits[live], S.bits16(S.round16(got["p"].to(F64), dt))[live]), f"{k}: not the rounding of the device's own fp32 p"
    if c["zero"] and c["wd"] == 0:
        for k in ("p", "m", "v"):
            assert torch.equal(got[k].view(torch.int32), t[k].view(torch.int32)), f"{k} moved with g = 0, m = v = 0 and no weight decay"
    return {k: got[k] for k in ("p", "m", "v")}


LAUNCH = {"cast": _launch_cast, "dropout": _launch_dropout, "cast_hb": _launch_cast_hb, "cast_b32": _launch_cast_b32, "axpy": _launch_axpy, "gelu": _launch_gelu,
          "colsum": _launch_colsum, "sumsq": _launch_sumsq, "adam": _launch_adam}


@pytest.mark.parametrize("c", [c for c in S.CASES if c["kind"] != "step"], ids=S.case_id)
def test_instance(c):
    t, ref = S.prepared(c["i"])
    S.assert_declared_plan(_abi.lib(), c)          # (host only: the launches below are the ones the case declares)
    got = LAUNCH[c["kind"]](c, t)
    res = S.evaluate(c, ref, got)
    _record(c, res)
    assert set(res) == set(ref)
    for k, (ratio, z) in res.items():
        print(f"{S.case_id(c)} {k}: ratio {ratio:.4g} z {z:.3g}")
    for k, (ratio, z) in res.items():
        what = "differs from the reference, which admits only itself" if ref[k][1] is None else f"worst ratio {ratio:.4g}, gain {z:.3g}"
        if ratio > 1.0 and ref[k][1] is None and torch.is_tensor(ref[k][0]):
            bad = (got[k].reshape(-1).to(ref[k][0].dtype) != ref[k][0].reshape(-1)).nonzero().flatten()
            what += f": {bad.numel()} elements, the first at {int(bad[0]) if bad.numel() else -1}"
        assert ratio <= 1.0 and abs(z) <= S.Z_MAX, f"{S.instance(c)} {S.case_id(c)} {k}: {what}"


def test_the_guard_follows_the_table_past_its_end():
    """three clean steps and a skipped one against a table of two steps: the third clean step takes the table's last row"""
    lib, b = _abi.lib(), Bufs()
    clean, bad = torch.ones(1003), torch.ones(1003)
    bad[1001] = float("inf")
    guard = torch.zeros(5, dtype=F32, device=DEV)
    table = torch.tensor(TABLE[:2], dtype=F32, device=DEV)
    want = [(1.0, 0.0, 0.0) + TABLE[0], (2.0, 0.0, 0.0) + TABLE[1], (2.0, 1.0, 1.0) + TABLE[1], (3.0, 1.0, 0.0) + TABLE[1]]
    for x, w in zip((clean, clean, bad, clean), want):
        out, ws = torch.zeros(3, dtype=F32, device=DEV), torch.empty(64, dtype=F32, device=DEV)
        lib.mmdti_sumsq_check_f32(ops._stream(), b.put(x), 1003, out.data_ptr(), ws.data_ptr(), 64, guard.data_ptr(), table.data_ptr(), 2, B1, B2)
        torch.cuda.synchronize()
        assert guard.cpu().tolist() == list(w) and float(out[2]) == w[2]


def test_step_state_advance():
    """12 steps from zero, warm-up 3, 10 in all -- past the end of the schedule: counter and salt pair EQUAL the host splitmix64, the rate
    EQUALS the two fp32 operations, the bias corrections stay within the bound 2 ulp of powf carry through 1 - x and the root (measured
    on MI355X: the largest |got - ref| / bound is 0.32, below 0.5)"""
    c = next(c for c in S.CASES if c["kind"] == "step")
    lib = _abi.lib()
    S.assert_declared_plan(lib, c)
    state = torch.zeros(4, dtype=F32, device=DEV)
    salt = torch.zeros(2, dtype=torch.int64, device=DEV)
    x, worst = 0, 0.0
    for k in range(c["steps"]):
        lib.mmdti_step_state_advance(ops._stream(), state.data_ptr(), salt.data_ptr(), c["base_lr"], c["warmup"], c["total"], B1, B2)
        torch.cuda.synchronize()
        st, sl = state.cpu(), [int(v) & S.M64 for v in salt.cpu().tolist()]
        x, z = S.splitmix64(x)
        assert sl == [x, z], f"step {k}: the salt pair is not splitmix64's"
        assert float(st[0]) == k + 1
        assert st[1].view(torch.int32).item() == torch.tensor(float(S.step_lr(k, c["base_lr"], c["warmup"], c["total"])), dtype=F32).view(torch.int32).item(), f"step {k}: rate {float(st[1])!r}"
        (bc1, e1), (bc2, e2) = S.step_bias(k + 1)
        worst = max(worst, abs(float(st[2]) - bc1) / e1, abs(float(st[3]) - bc2) / e2)
    print(f"step_state_advance: worst bias-correction ratio {worst:.3g}")
    REPORT.setdefault("step_state_advance_kernel", {})["bias"] = {"ratio": worst, "z": 0.0}
    assert worst <= 1.0
