"""Every kernel instance of csrc/gemm.hip against a float64 reference of the same operation (tests/gemm_cases.py): the 39 instances
of mmdti_gemm_bf16's launch table, splitk_reduce_kernel, the column-sum pass behind arowsum, and the four gemm_ln_kernel instances.

Each case runs the plan query first and asserts the instance it declares (tests/test_gemm_cases_cpu.py proves on the CPU that the
declarations cover the table), then launches on operands cut from NaN-filled arenas into outputs cut from sentinel-filled arenas:
  exact    integer inputs whose every partial sum fp32 holds exactly -- the output must EQUAL the reference, bit for bit;
  random   randn inputs -- elementwise within (K + 8) * 2^-23 * T + R, the worst case of fp32 summation in any order.
A NaN in the output is a read outside the operand (or an element never stored); a changed sentinel is a store outside the output.

With MMDTI_GEMM_PROFILE=<path> the largest |got - ref| / bound of every instance, the measured GELU error G and the gemm_ln bands are
written there as JSON (profiles/gemm_instances.json is such a run)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from mmdti_hip import _abi, ops

import gemm_cases as G
from head_refs import nerr
from test_gemm_plan_cpu import DEFAULTS

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {"instances": {}, "gelu_G": {}, "gemm_ln": {}}
MASKS = {}            # dropout masks by element count: a function of row * N + col at equal (seed, site), whatever the instance


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MMDTI_GEMM_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(kernel, out, ratio):
    """per instance and output type (a 16-bit output sits near 1 by construction: R is the half-ulp of its rounding)"""
    row = REPORT["instances"].setdefault(kernel, {})
    row[out] = max(row.get(out, 0.0), ratio)


def _launch(c, t):
    lib = _abi.lib()
    ptr = G.pointers(t)
    with G.options(lib, c["opts"], DEFAULTS):
        p = G.assert_declared_plan(lib, c, ptr)
        lib.mmdti_gemm_bf16(ops._stream(), *G.call_args(c, ptr))
    torch.cuda.synchronize()
    return p


def _check_case(c, mode):
    t = G.make_inputs(c, mode, DEV)
    p = _launch(c, t)
    name = G.case_id(c)
    for k in ("C", "aux_out", "colsum", "arowsum", "ws"):
        if k in t:
            assert t[k].outside_untouched() == 0, (name, k, "a store outside the output")
    got = t["C"].view
    keep = None
    if c["drop"]:
        keep = got != 0
        n = keep.numel()
        rate, sd = float(keep.sum()) / n, (c["drop"] * (1 - c["drop"]) / n) ** 0.5
        assert abs(rate - (1 - c["drop"])) <= 4 * sd, (name, rate)
        base = MASKS.setdefault(n, (name, keep.flatten().clone()))
        assert torch.equal(base[1], keep.flatten()), (name, "mask differs from", base[0])
    ref = G.reference(c, t, keep)
    sides = [k for k in ("aux_out", "colsum", "arowsum") if k in ref]
    if mode == "exact":
        _, gran = G.exact_r(c)
        assert float(ref["T"].max()) / gran < 2 ** 24, (name, "the case is not exact by construction")
        bad = got.to(G.F64) != ref["C_out"].to(G.F64)
        assert not bool(bad.any()), (name, p["kernel"], int(bad.sum()), "first at", bad.nonzero()[0].tolist(),
                                     float(got[bad][0]), float(ref["C_out"][bad][0]))
        for k in sides:
            assert float(ref[k + "_T"].max()) < 2 ** 24, (name, k)
            assert torch.equal(t[k].view.to(G.F64), ref[k]), (name, k, float((t[k].view.to(G.F64) - ref[k]).abs().max()))
    else:
        ratio = G.worst_ratio(got, ref["C"], G.bound(c, ref))
        print(f"{name}: {p['kernel']} |got - ref| / bound = {ratio:.4f}")
        _record(p["kernel"], "f32" if c["out"] == "atomic" else c["out"], ratio)
        assert ratio <= 1.0, (name, p["kernel"], ratio)
        for k in sides:
            rk = G.worst_ratio(t[k].view, ref[k], G.side_bound(c, ref, k))
            print(f"   {k}: {rk:.4f}")
            assert rk <= 1.0, (name, k, rk)


@pytest.mark.parametrize("c", [c for c in G.PLAIN_CASES if "exact" in c["modes"]], ids=G.case_id)
def test_exact(c):
    _check_case(c, "exact")


@pytest.mark.parametrize("c", [c for c in G.PLAIN_CASES if "random" in c["modes"]], ids=G.case_id)
def test_random(c):
    _check_case(c, "random")


@pytest.mark.parametrize("c", G.BIG_LD_CASES, ids=G.case_id)
def test_operand_offsets_round_2_to_the_31(c):
    """A of 8184 rows at lda = 131072 (M * lda * 2 just under 2^31: bare loads with 32-bit offsets) and of 8200 rows at 131080 (over:
    the plan must name a predicated instance, 64-bit addressing); every row is compared, the last 128 among them"""
    try:
        _check_case(c, "exact")
    finally:
        torch.cuda.empty_cache()


def test_gelu_error_G():
    """G: the absolute error of the device's gelu_erf / gelu_erf_grad (scalar and paired forms) against float64 over [-8, 8].  A K = 64
    GEMM against an identity weight hands the epilogue pre-activations that are known exactly: A[m][n] = -8 + m / 16 (bf16 holds
    it), plus an fp32 bias[n] in [0, 1/16) -- one fp32 addition, the same in torch.  N = 64 takes the vector epilogue, N = 60 the
    scalar one.  The bands of the GELU cases carry four times the values recorded in gemm_cases.GELU_G_MEASURED."""
    lib = _abi.lib()
    M, K = 257, 64
    worst = {"gelu": 0.0, "gelu_grad": 0.0}
    for N in (64, 60):
        A = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV)
        A[:, :N] = (-8.0 + torch.arange(M, device=DEV) / 16.0)[:, None].to(torch.bfloat16)
        B = torch.eye(K, dtype=torch.bfloat16, device=DEV)[:N].contiguous()
        bias = ((torch.arange(N, device=DEV) + 0.37) / 1024.0).float()
        pre = A[:, :N].float() + bias
        u = torch.linspace(-8.0, 8.0, M * N, device=DEV).to(torch.bfloat16).reshape(M, N).contiguous()
        one = torch.ones(N, device=DEV)
        for act, key in ((G.ACT_GELU, "gelu"), (G.ACT_GELU_G, "gelu"), (G.ACT_GELU_BWD, "gelu_grad")):
            y = torch.full((M, N), float("nan"), device=DEV)
            aux = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
            bwd = act == G.ACT_GELU_BWD
            Az = torch.zeros_like(A) if bwd else A
            lib.mmdti_gemm_bf16(ops._stream(), Az.data_ptr(), B.data_ptr(), y.data_ptr(), M, N, K, K, K, N, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1.0, 0.0,
                                (one if bwd else bias).data_ptr(), 0, N, act, u.data_ptr() if bwd else 0, aux.data_ptr() if act == G.ACT_GELU_G else 0,
                                N, 0, 0.0, 0, 0, 0, 0, 0, 0)
            torch.cuda.synchronize()
            ref = G.gelu_grad64(u.to(G.F64)) if bwd else G.gelu64(pre.to(G.F64))
            worst[key] = max(worst[key], float((y.to(G.F64) - ref).abs().max()))
    print("gelu error G:", worst)
    REPORT["gelu_G"] = worst
    for k, v in worst.items():
        assert v <= G.GELU_G_CAP and v <= 2 * G.GELU_G_MEASURED[k], (k, v, G.GELU_G_MEASURED[k])


@pytest.mark.parametrize("lc", G.LN_CASES, ids=lambda lc: f"rows{lc['rows']}-{'f16' if lc['f16'] else 'bf16'}-M{lc['M']}-K{lc['K']}-res{lc['residual']}")
@pytest.mark.parametrize("mode", ["exact", "random"])
def test_gemm_ln(lc, mode):
    """x_out as the plain GEMMs (exact on the integer inputs); mean, rstd, ln_f32 and the 16-bit copy as nerr against float64
    LayerNorm of the float64 x, within 16 times the nerr of an fp32 torch LayerNorm of the same rows (plus the 16-bit rounding)"""
    lib = _abi.lib()
    t = G.ln_inputs(lc, mode, DEV)
    M, K = lc["M"], lc["K"]
    res = t.get("residual")
    with G.options(lib, {"gemm_ln_rows": lc["rows"]}, DEFAULTS):
        assert lib._dll.mmdti_gemm_ln_rows(M) == lc["rows"]
        lib.mmdti_gemm_ln_bf16(ops._stream(), t["A"].ptr(), t["W"].ptr(), t["bias"].ptr(), res.ptr() if res else 0, M, G.LN_N, K, K + 8, K + 16,
                               G.LN_N + 4, 0.0, G.SEED, G.SITE, t["x_out"].ptr(), t["gamma"].data_ptr(), t["beta"].data_ptr(), G.LN_EPS,
                               t["ln_f32"].ptr(), t["ln_16"].ptr(), t["mean"].ptr(), t["rstd"].ptr(), 3 if lc["f16"] else 0)
    torch.cuda.synchronize()
    outs = ("x_out", "ln_f32", "ln_16", "mean", "rstd")
    for k in outs:
        assert t[k].outside_untouched() == 0, (k, "a store outside the output")
    ref = G.ln_reference(t)
    x = t["x_out"].view[0, 0]
    if mode == "exact":
        assert float(ref["T"].max()) < 2 ** 24
        assert torch.equal(x.to(G.F64), ref["x"]), float((x.to(G.F64) - ref["x"]).abs().max())
    else:
        ratio = G.worst_ratio(x, ref["x"], (K + 8) * 2.0 ** -23 * ref["T"])
        _record(f"gemm_ln_kernel<{lc['rows'] // 16}, {'true' if lc['f16'] else 'false'}>", "f32", ratio)
        assert ratio <= 1.0, ratio
    # the yardstick: torch's fp32 LayerNorm of the same rows
    x32 = ref["x"].float()
    y32 = G.ln_of(x32, t, torch.float32)
    y32["ln"] = F.layer_norm(x32, (G.LN_N,), t["gamma"], t["beta"], G.LN_EPS)
    got = {"mean": t["mean"].view[0, 0, 0], "rstd": t["rstd"].view[0, 0, 0], "ln": t["ln_f32"].view[0, 0], "ln_16": t["ln_16"].view[0, 0]}
    row = {}
    for k, g in got.items():
        rk = "ln" if k == "ln_16" else k
        mine, yard = nerr(g, ref[rk]), nerr(y32[rk], ref[rk])
        band = 16 * yard + ((2.0 ** -11 if lc["f16"] else 2.0 ** -8) if k == "ln_16" else 0.0)
        row[k] = dict(nerr=mine, fp32_torch_nerr=yard, band=band)
        print(k, row[k])
    REPORT["gemm_ln"][f"rows{lc['rows']}-f16_{lc['f16']}-M{M}-K{K}-res{lc['residual']}-{mode}"] = row
    for k, v in row.items():
        assert v["nerr"] <= v["band"], (k, v)
