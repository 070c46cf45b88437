"""The case table of tests/gemm_cases.py, checked without a GPU: plan queries (mmdti_gemm_plan, fake aligned pointers) prove that
the table reaches all 39 instances of the launch table and that every case reaches the instance it declares -- the GPU file
asserts the same plan before each launch --, and the float64 reference of every case is pinned against an fp32 evaluation of the
same formula on the CPU (the bound is the one the device results are held to)."""
import pytest
import torch

from mmdti_hip import _abi

import gemm_cases as G
from test_gemm_plan_cpu import DEFAULTS, GEMM_KERNELS


def test_the_table_reaches_all_39_instances_and_every_case_its_declared_one():
    lib = _abi.lib()
    named = set()
    for c in G.CASES:
        with G.options(lib, c["opts"], DEFAULTS):
            named.add(G.assert_declared_plan(lib, c)["kernel"])
    want = {k[0] for k in GEMM_KERNELS}
    assert len(want) == 39 and named == want, (sorted(want - named), sorted(named - want))
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)               # ids are unique: a parametrised test per case


def test_every_family_carries_the_edges_its_tile_loop_can_get_wrong():
    by = lambda fam, f: [c for c in G.CASES if c["fam"] == fam and f(c)]
    for fam in ("reg", "glds0", "dbuf", "deep", "small", "tall", "big"):
        assert by(fam, lambda c: c["alpha"] == 0.5 and c["bias"] and c["residual"] and c["beta"] == 1.0 and c["out"] == "f32"), fam
        assert by(fam, lambda c: c["out"] == "f16" and c["residual"]) and by(fam, lambda c: c["out"] == "bf16" and c["residual"]), fam
        assert by(fam, lambda c: c["ldr"] and c["ldr"] != c["ldc"] and c["lda"] and c["ldb"]) and by(fam, lambda c: c["ld_aux"]), fam
        assert by(fam, lambda c: c["act"] == G.ACT_MUL_AUX) and by(fam, lambda c: c["drop"] == 0.5), fam
        assert by(fam, lambda c: c["act"] == G.ACT_GELU) and by(fam, lambda c: c["act"] == G.ACT_GELU_G) and by(fam, lambda c: c["act"] == G.ACT_GELU_BWD), fam
        assert by(fam, lambda c: c["expect"].get("stream_c") == 1 and c["out"] == "f32") and by(fam, lambda c: c["expect"].get("stream_c") == 1 and c["out"] == "bf16"), fam
        assert by(fam, lambda c: c["opts"].get("gemm_stream_mb") == 0 and c["beta"] == 1.0 and c["expect"]["stream_c"] == 0), fam
        if fam not in ("small", "big"):
            assert by(fam, lambda c: c["colsum"]), fam
        if fam in ("reg", "dbuf", "big"):
            assert by(fam, lambda c: c["sk"] > 1 and c["bias"] and c["alpha"] == 2.0), fam
        if fam in ("reg", "glds0", "deep", "dbuf"):
            assert by(fam, lambda c: c["batch"] == (2, 3)), fam
        ktiles = {c["K"] // 64 for c in by(fam, lambda c: c["K"] % 64 == 0)}
        assert ktiles >= ({1, 3} if fam == "tall" else {4, 5, 16} if fam == "deep" else {1, 3, 5}), (fam, ktiles)
    assert by("reg", lambda c: c["batch"] == (2, 3) and c["sk"] == 2) and by("dbuf", lambda c: c["batch"] == (2, 3) and c["sk"] == 2)
    assert {c["K"] % 64 for c in by("reg", lambda c: True)} >= {8, 56} and by("reg", lambda c: c["K"] < 64)
    assert by("reg", lambda c: c["M"] == 4) and by("reg", lambda c: c["N"] == 4) and by("reg", lambda c: c["M"] == 8 and c["N"] == 8)
    assert by("reg", lambda c: c["tA"] and c["M"] % 8) and by("reg", lambda c: c["tB"] and c["N"] % 8)
    assert by("reg", lambda c: c["N"] % 8 == 0 and c["ldc"] and c["ldc"] % 4)
    assert by("small", lambda c: c["M"] == 65) and by("big", lambda c: c["expect"].get("slabs") == 1) and len(G.BIG_LD_CASES) == 2
    assert max(c["M"] * c["N"] for c in G.CASES) == 4500 * 4096 and max(c["K"] for c in G.CASES) <= 1024


def test_the_gemm_ln_instances():
    lib = _abi.lib()
    for lc in G.LN_CASES:
        with G.options(lib, {"gemm_ln_rows": lc["rows"]}, DEFAULTS):
            assert lib._dll.mmdti_gemm_ln_rows(lc["M"]) == lc["rows"]
    assert {(lc["rows"], lc["f16"]) for lc in G.LN_CASES} == {(64, 0), (64, 1), (80, 0), (80, 1)}
    assert {lc["M"] for lc in G.LN_CASES} == {1, 63, 64, 81, 161} and {lc["K"] for lc in G.LN_CASES} == {64, 320}


def _shapes():
    """one case per distinct (shape, epilogue) of the table: the reference does not depend on the option setting or the family"""
    seen, out = set(), []
    for c in G.PLAIN_CASES:
        key = tuple((k, v) for k, v in sorted(c.items(), key=lambda kv: kv[0]) if k not in ("label", "fam", "opts", "kernel", "expect", "modes", "ws"))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("mode", ["exact", "random"])
def test_the_reference_is_pinned_by_an_fp32_evaluation(mode):
    """The float64 reference against the same formula in fp32 (torch on the CPU: its own matmul, its own erf): equal on the exact
    inputs -- which also proves them exact: T, the sum of magnitudes, stays below 2^24 granules --, within the summation bound on
    the random ones.  (GELU bands carry the device's measured error G; torch's fp32 erf is held to the same.)"""
    worst = 0.0
    for c in _shapes():
        if mode not in c["modes"]:
            continue
        t = G.make_inputs(c, mode, "cpu")
        keep = None
        if c["drop"]:
            keep = torch.rand(t["C"].view.shape, generator=torch.Generator().manual_seed(5)) >= c["drop"]
        r64, r32 = G.reference(c, t, keep), G.reference(c, t, keep, dtype=torch.float32)
        for k in ("C", "colsum", "arowsum", "aux_out"):
            if k not in r64:
                continue
            if mode == "exact":
                _, gran = G.exact_r(c)
                Tk = r64["T" if k == "C" else k + "_T"]
                assert float(Tk.max()) / gran < 2 ** 24, (G.case_id(c), k, float(Tk.max()))
                assert torch.equal(r32[k].to(G.F64), r64[k]), (G.case_id(c), k)
            else:
                # (the fp32 evaluation is compared before the rounding of a 16-bit output: no R)
                b = G.bound(c, r64) - G.rounding_term(r64["C"], G.out_dtype(c)) if k == "C" else G.side_bound(c, r64, k)
                if k == "aux_out":
                    b = b - G.rounding_term(r64["aux_out"], torch.bfloat16)
                ratio = G.worst_ratio(r32[k], r64[k], b)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (G.case_id(c), k, ratio)
        if mode == "exact" and c["out"] in ("bf16", "f16"):
            assert torch.equal(r32["C_out"], r64["C_out"]), G.case_id(c)
    print(f"fp32 torch against float64, worst |diff| / bound: {worst:.4f}")


def test_the_gemm_ln_reference_is_pinned():
    for lc in G.LN_CASES:
        if lc["rows"] != 64:
            continue
        for mode in ("exact", "random"):
            t = G.ln_inputs(lc, mode, "cpu")
            r64, r32 = G.ln_reference(t), G.ln_reference(t, dtype=torch.float32)
            if mode == "exact":
                assert float(r64["T"].max()) < 2 ** 24 and torch.equal(r32["x"].to(G.F64), r64["x"]), lc
            else:
                assert bool(((r32["x"].to(G.F64) - r64["x"]).abs() <= (lc["K"] + 8) * 2.0 ** -23 * r64["T"]).all()), lc
            for k in ("mean", "rstd", "ln"):
                d, den = float((r32[k].to(G.F64) - r64[k]).abs().max()), float(r64[k].abs().max())
                assert d <= 1e-5 * max(den, 1e-30) or (mode == "exact" and k != "mean"), (lc, k, d, den)


def test_sentinels_and_guards_of_an_arena():
    c = next(c for c in G.CASES if c["batch"] == (2, 3) and c["out"] == "bf16")
    t = G.make_inputs(c, "random", "cpu")
    A, C = t["A"], t["C"]
    assert torch.isnan(A.buf[:A.guard].float()).all() and torch.isnan(A.buf[-A.guard:].float()).all() and not torch.isnan(A.view.float()).any()
    assert int(torch.isnan(A.buf.float()).sum()) == A.buf.numel() - A.view.numel()       # padding columns and batch gaps too
    assert torch.isnan(C.view.float()).all() and C.outside_untouched() == 0
    C.buf[C.guard - 1] = 0.0
    assert C.outside_untouched() == 1
    C.buf[C.guard - 1] = float("nan")                                                   # (another NaN than the sentinel)
    assert C.outside_untouched() == 1
