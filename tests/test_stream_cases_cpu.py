"""The case table of tests/stream_cases.py, checked without a GPU: the launch lines and update statements the references depend on are
verbatim in csrc/elementwise.hip; the table reaches every stream kernel and every Adam and sumsq instantiation; the sizes cross each
launcher's grid cap once, with a ragged tail (and the column sums pass the 1024-row-group cap, whose count is the library's:
ops.det_workspace_bytes("colsum", ...)); the exact modes are exact in the fp32 emulation; the emulation stays inside every bound with
|gain| <= 6; and six wrong emulations (Adam with eps inside the root, with bc2 applied to v, with decoupled weight decay; column sums
over ld; a truncating cast; a non-finite test that is `x != x`) leave the bounds or the equalities."""
import json
import os

import numpy as np
import pytest
import torch

from mmdti_hip import ops

import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32, BF16, F16 = S.F64, S.F32, S.BF16, S.F16
SMALL = [c for c in S.CASES if c["kind"] != "step"]
EMU = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MMDTI_ROW_PROFILE")
    if path and EMU:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc.setdefault("emulation", {}).update(EMU)
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def test_the_mirrored_lines_are_verbatim_in_the_source():
    src = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "elementwise.hip")).read()
    for line in S.SOURCE_LINES:
        assert line in src, line
    det = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "det.h")).read()
    for line in S.DET_LINES:
        assert line in det, line


def test_the_table_reaches_every_kernel_and_instantiation():
    got = {k for c in S.CASES for k in S.instance(c)}
    assert got == set(S.ALL_KERNELS) and len(S.ALL_KERNELS) == 19, got ^ set(S.ALL_KERNELS)
    ids = [S.case_id(c) for c in S.CASES]
    assert len(set(ids)) == len(ids)
    adam = {}
    for c in S.CASES:
        if c["kind"] == "adam":
            adam.setdefault(S.instance(c), []).append(c)
    assert len(adam) == 4
    for name, cs in adam.items():
        seen = lambda f: {f(c) for c in cs}
        assert seen(lambda c: c["wd"]) == {0.0, 0.01} and seen(lambda c: c["gs"]) == {None, 0.37} and seen(lambda c: c["state"]) == {True, False}, name
        assert {("bf16",), ("f16",), ("bf16", "f16")} <= seen(lambda c: c["shadows"]) and seen(lambda c: c["zero"]) == {True, False}, name
        assert all(c["n"] % 8 != 0 for c in cs) and any(c["n"] == S.BIGA for c in cs), name         # the mask's last group is partial
    forms = {c["form"] for c in S.CASES if c["kind"] == "sumsq"}
    assert forms == set(S.SUMSQ_FORMS)
    for form in ("check", "guard", "guard_table"):
        assert {c["special"] for c in S.CASES if c["kind"] == "sumsq" and c["form"] == form} == {None, "body", "tail", "last_wg", "denormal", "overflow"}


def test_the_sizes_cross_each_grid_cap_once():
    for c in S.CASES:
        k = c["kind"]
        if k in ("cast", "cast_b32", "dropout", "axpy", "gelu", "cast_hb"):
            g, per, items = S.launch(c)
            big = c.get("n", 0) > 5000 or c.get("rows", 0) > 100
            assert (g == S.CAP and S.rounds(c) == 2 and items % (g * per) not in (0,) and items - g * per < 4096) if big else (g <= 5 and S.rounds(c) <= 1), S.case_id(c)
        if k == "cast" and c["n"] > 5000:
            assert c["n"] % 4 == 3                                         # the scalar tail of the vector casts
        if k == "adam" and c["n"] == S.BIGA:
            assert S.launch(c)[0] < S.CAP and S.rounds(c) == 4 and c["n"] % 8 == 5
        if k == "sumsq" and c["ws"] < 4096:
            assert S.sumsq_wgs(c) == 3 and S.rounds(c) == 3                # many rounds of three workgroups
    assert {S.rounds(c) for c in S.CASES if c["kind"] == "sumsq" and c["form"] == "atomic"} == {1, 4, 8}        # (at most 8 terms a thread and round)
    assert S.sumsq_wgs(dict(form="check", ws=4096, n=1048576 + 7)) == 1026
    for rows, cols, ld in S.COLSUM_SHAPES + ((64, 8, 8), (65, 8, 8), (65536, 8, 8), (65537, 8, 8)):
        assert ops.det_workspace_bytes("colsum", rows, cols) == S.colsum_gy(rows) * cols * 4
    assert S.colsum_gy(65536 + 197) == 1024 and -(-(65536 + 197) // 64) > 1024       # the last shape passes the row-group cap
    assert any(c["cols"] % 8 and c["cols"] < c["ld"] for c in S.CASES if c["kind"] == "colsum")


def _emulate(c, mut=None):
    t, ref = S.prepared(c["i"])
    return t, ref, S.evaluate(c, ref, S.emulate(c, t, mut))


@pytest.mark.parametrize("c", SMALL, ids=S.case_id)
def test_the_emulation_stays_inside_the_bounds(c):
    """... and where the reference admits only itself (the casts, the exact modes, the counts) the emulation EQUALS it"""
    t, ref, res = _emulate(c)
    assert set(res) == set(ref)
    for k, (ratio, z) in res.items():
        for name in S.instance(c):
            old = EMU.setdefault(name, {}).get(k, {"ratio": 0.0, "z": 0.0})
            EMU[name][k] = {"ratio": max(old["ratio"], ratio), "z": max(old["z"], abs(z))}
        assert ratio <= 1.0 and abs(z) <= S.Z_MAX, (S.case_id(c), k, ratio, z)
    if c["kind"] in ("cast", "cast_hb", "cast_b32", "dropout") or c.get("mode") == "exact":
        assert all(b is None for k, (r, b) in ref.items() if k != "count")


def test_the_roundings_restated_agree_with_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(100000, generator=g) * torch.exp2(torch.randint(-30, 30, (100000,), generator=g).float()), torch.tensor(S.F16_SPECIALS)])
    assert torch.equal(S.bf16_bits_rne(x), S.bits16(x.to(BF16)))
    assert torch.equal(S.f16_bits_sat(x), S.bits16(x.clamp(-65504.0, 65504.0).to(F16)))
    sat = S.f16_bits_sat(torch.tensor([65520.0, 1e6, float("inf"), -65520.0, float("-inf"), 65519.99, 2.0 ** -25, 3 * 2.0 ** -25, -0.0]))
    assert sat.tolist() == [0x7BFF, 0x7BFF, 0x7BFF, 0xFBFF, 0xFBFF, 0x7BFF, 0x0000, 0x0002, 0x8000]


def _leaves(pred, mut):
    tried = 0
    for c in S.CASES:
        if c["kind"] == "step" or not pred(c) or c.get("n", 0) > 5000 or c.get("rows", 0) > 1000:
            continue
        tried += 1
        if any(r > 1.0 for r, _ in _emulate(c, mut)[2].values()):
            return S.case_id(c)
    raise AssertionError(f"the wrong emulation {mut} stays inside the bounds on {tried} cases")


def test_the_wrong_emulations_leave_the_bounds():
    adam = lambda c: c["kind"] == "adam" and not c["zero"] and c["n"] == 1003
    print(_leaves(adam, "eps_inside"))
    print(_leaves(adam, "bc2_on_v"))
    print(_leaves(lambda c: adam(c) and c["wd"] > 0, "adamw"))
    print(_leaves(lambda c: c["kind"] == "colsum" and c["ld"] > c["cols"], "over_ld"))
    print(_leaves(lambda c: c["kind"] == "cast" and not c["f16"] and c["n"] == 1027, "truncate"))
    print(_leaves(lambda c: c["kind"] == "cast" and c["f16"] and c["n"] == 1027, "truncate"))
    print(_leaves(lambda c: c["kind"] == "sumsq" and c["special"] in ("body", "tail"), "nan_only"))


def test_the_step_state_statement():
    """splitmix64 against its published first outputs; the schedule against transformers' linear warm-up formula in float64"""
    x, z = S.splitmix64(0)
    assert (x, z) == (0x9E3779B97F4A7C15, 0xE220A8397B1DCDAF)
    x, z = S.splitmix64(x)
    assert z == 0x6E789E6AA1B965F4
    c = next(c for c in S.CASES if c["kind"] == "step")
    for k in range(c["steps"]):
        lam = k / max(1, c["warmup"]) if k < c["warmup"] else max(0.0, (c["total"] - k) / max(1, c["total"] - c["warmup"]))
        lr = float(S.step_lr(k, c["base_lr"], c["warmup"], c["total"]))
        assert abs(lr - c["base_lr"] * lam) <= 3 * S.U * c["base_lr"] * lam and (k < c["total"] or lr == 0.0)
        (bc1, e1), (bc2, e2) = S.step_bias(k + 1)
        f = np.float32
        assert abs(float(f(1) - np.power(f(0.9), f(k + 1))) - bc1) <= e1 and abs(float(np.sqrt(f(1) - np.power(f(0.999), f(k + 1)))) - bc2) <= e2
