"""The case table of tests/stream_cases.py, checked without a GPU: the update statements the references depend on are verbatim in
csrc/elementwise.hip; the table reaches every stream kernel and every Adam and sumsq instantiation, and with the grouped Adam pass and
the EMA pair these are exactly the 29 rows of the library's MMDTI_PLAN_STREAM table; the declared dispatch and geometry are the
library's (mmdti_stream_plan) for every case and over sweeps across every grid cap, and the query refuses what the launchers refuse, in
their words; the sizes cross each launcher's grid cap once, with a ragged tail (and the column sums pass the 1024-row-group cap, whose
count is also the one the workspace size follows: ops.det_workspace_bytes("colsum", ...)); the exact modes are exact in the fp32 emulation; the emulation stays inside every bound with
|gain| <= 6; and six wrong emulations (Adam with eps inside the root, with bc2 applied to v, with decoupled weight decay; column sums
over ld; a truncating cast; a non-finite test that is `x != x`) leave the bounds or the equalities."""
import json
import os

import numpy as np
import pytest
import torch

from mmdti_hip import _abi, ops

import adam_group_cases as G
import ema_cases as E
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
    plan = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "stream_plan.h")).read()
    for line in S.PLAN_LINES:
        assert line in plan, line


def test_the_plan_table_is_the_three_instance_lists():
    """19 + 8 + 2 = 29 rows in the suites' own order, and every row is reached by a case through the library's own plan"""
    import ctypes
    lib = _abi.lib()
    n = ctypes.c_int()
    lib.mmdti_plan_table_size(S.PLAN_FAMILY, ctypes.byref(n))
    names = tuple(lib.mmdti_plan_kernel_name(S.PLAN_FAMILY, i).decode() for i in range(n.value))
    assert names == S.ALL_KERNELS + G.ALL_KERNELS + E.ALL_KERNELS and n.value == 29 and lib.mmdti_plan_kernel_name(S.PLAN_FAMILY, 29) is None
    reached = {l[0] for c in S.CASES for l in S.library_plan(lib, c)["launches"]} | {l[0] for c in G.CASES for l in G.library_plan(lib, c)["launches"]}
    reached |= {l[0] for swap in (False, True) for n_ in E.SIZES for l in E.library_plan(lib, swap, n_)["launches"]}
    assert reached == set(names) | {"det_fold_kernel"}, reached ^ set(names)


def test_the_declared_plan_is_the_librarys_for_every_case():
    lib = _abi.lib()
    for c in S.CASES:
        got = S.assert_declared_plan(lib, c)
        assert [l[0] for l in got["launches"] if l[0] != "det_fold_kernel"] == list(S.instance(c))


def _flat(lib, entry, ptrs, name, items_of, per, ns, **kw):
    for n in ns:
        got = S.stream_plan(lib, entry, ptrs, n, **kw)
        assert got == dict(launches=S.flat(name, S.grid_for(items_of(n), per)), wgs=0), (entry, n, got)


def test_the_declared_plan_is_the_librarys_on_both_sides_of_every_cap():
    """grid_for caps at 4096 workgroups: n from a few below to a few above the size that fills them, for 1, 4 and 8 elements per thread and
    for the 1024 and 2048 elements a workgroup of the Adam and EMA kernels takes; the sum of squares with every count of partials; the
    column sums round 64 rows x 1024 row groups; every (entry, guard, skip, decoupled) combination the four Adam entry points admit"""
    lib, P = _abi.lib(), S.PTR
    around = lambda x: [n for n in (1, 2, 3, 255, 256, 257, x - 257, x - 1, x, x + 1, x + 255, x + 256, x + 257, 3 * x + 5) if n > 0]
    cap1 = S.CAP * 256
    for entry, name in (("cast_bf16_f32", "cast_bf16_f32_kernel"), ("dropout_f32", "dropout_f32_kernel"), ("axpy_f32", "axpy_kernel"), ("gelu_fwd_bf16", "gelu_bf16_kernel")):
        _flat(lib, entry, [P, P], name, lambda n: n, 256, around(cap1))
    for entry, name in (("cast_f32_bf16", "cast_f32_bf16_kernel<false>"), ("cast_f32_f16", "cast_f32_bf16_kernel<true>")):
        _flat(lib, entry, [P, P], name, lambda n: n // 4 + 1, 256, around(4 * cap1) + list(range(4 * cap1 - 12, 4 * cap1 + 5)), f=0.1)
    for rows, cols in ((1, 8), (3, 2048), (511, 2048), (512, 2048), (513, 2048), (2049, 4096), (4097, 2048 * 8)):
        got = S.stream_plan(lib, "cast_f16_bf16", [P, P], a=rows, b=cols, c=cols + 8)
        assert got == dict(launches=S.flat("cast_f16_bf16_kernel", S.grid_for(rows * (cols // 8), 256)), wgs=0), (rows, cols)
    _flat(lib, "sumsq_f32", [P, P, 0], "sumsq_kernel", lambda n: n, 2048, around(S.CAP * 2048))
    _flat(lib, "ema_update", [P, P + 64, 0, 0], "ema_update_kernel", lambda n: n, 1024, around(S.CAP * 1024), a=1, f=0.9)
    _flat(lib, "ema_swap", [P, P + 64, P, 0], "ema_swap_kernel", lambda n: n, 2048, around(S.CAP * 2048))
    b = lambda x: "true" if x else "false"
    calls = []                                                         # (entry, guard, skip, decoupled, step state given)
    for state in (False, True):
        for guard in (False, True):
            for skip in (False, True):
                g, k, st = (P if guard else 0), (P if skip else 0), (P if state else 0)
                if skip:
                    entry, ptrs = "adam_step_masked", [P] * 4 + [st, g, k]
                elif guard:
                    entry, ptrs = "adam_step_guarded", [P] * 5               # (its step state is not part of the validation)
                else:
                    entry, ptrs = "adam_step", [P] * 4 + [st]
                if not (state and entry == "adam_step_guarded"):
                    _flat(lib, entry, ptrs, f"adam_kernel<{b(guard)}, {b(skip)}>", lambda n: n, 1024, around(S.CAP * 1024), a=0 if state or guard else 1)
                    calls.append((entry, guard, skip, None, state))
                for dec in (False, True):
                    _flat(lib, "adam_step_grouped", [P] * 4 + [0, 0, st, g, k, P, P], f"adam_group_kernel<{b(guard)}, {b(skip)}, {b(dec)}>", lambda n: n, 2048,
                          around(S.CAP * 2048), a=0 if state or guard else 1, b=4, c=int(dec))
                    calls.append(("adam_step_grouped", guard, skip, dec, state))
    # twelve (entry, guard, skip, decoupled) combinations are admitted -- 1 + 1 + 2 of the three adam_kernel entries, 8 of the grouped one --
    # each with its bias corrections by value and, where the entry has the argument, through the step state
    assert len({c[:4] for c in calls}) == 12 and len(calls) == 23
    for ws in (1, 2, 3, 6, 2048, 4096, 8192):
        for n in (1, 3, 4, 1003, 1023, 1024, 1025, 256 * 4 * 3, 1048576 + 7, 4 * 256 * 2047 - 1, 4 * 256 * 2047, 4 * 256 * 2048 + 9, 1 << 26):
            for form in ("part", "check"):
                c = dict(kind="sumsq", form=form, n=n, ws=ws)
                if form == "check" and ws < 2:
                    continue
                assert S.library_plan(lib, c) == S.declared_plan(c), (form, ws, n)
                assert S.library_plan(lib, c)["wgs"] == min(ws if form == "part" else ws // 2, 2048, (n // 4 + 255) // 256 + 1)
    for rows in (1, 63, 64, 65, 64 * 1024 - 1, 64 * 1024, 64 * 1024 + 1, 64 * 1024 + 64, 1 << 22):
        for cols in (1, 8, 255, 256, 257, 4096):
            for det in (False, True):
                c = dict(kind="colsum", rows=rows, cols=cols, ld=(cols + 7) // 8 * 8, det=det)
                got = S.library_plan(lib, c)
                assert got == S.declared_plan(c) and len(got["launches"]) == 1 + det, (rows, cols, det)
    assert S.stream_plan(lib, "adam_step_grouped", [P] * 4 + [0, 0, 0, 0, 0, P, P], 0, a=1, b=1) == dict(launches=[], wgs=0)       # an empty arena: no launch
    assert S.stream_plan(lib, "ema_update", [P, P + 64, 0, 0], 0, a=1, f=0.9) == dict(launches=[], wgs=0)


def test_the_query_refuses_in_the_launchers_words():
    lib, P = _abi.lib(), S.PTR
    cases = (("cast_f32_bf16: bad arguments", "cast_f32_bf16", [P, P], dict(n=0)),
             ("cast_f32_bf16: alignment", "cast_f32_bf16", [P + 8, P], dict(n=5)),
             ("cast_f32_f16: alignment", "cast_f32_f16", [P, P + 4], dict(n=5)),
             ("cast_f32_f16: dropout p out of range", "cast_f32_f16", [P, P], dict(n=5, f=1.0)),
             ("cast_f16_bf16: bad arguments \\(cols % 8, ldx % 8\\)", "cast_f16_bf16", [P, P], dict(a=3, b=12, c=16)),
             ("cast_f16_bf16: 16-byte alignment required", "cast_f16_bf16", [P, P + 8], dict(a=3, b=8, c=16)),
             ("cast_bf16_f32: bad arguments", "cast_bf16_f32", [0, P], dict(n=5)),
             ("dropout_f32: bad arguments", "dropout_f32", [P, 0], dict(n=5)),
             ("dropout_f32: dropout p out of range", "dropout_f32", [P, P], dict(n=5, f=-0.1)),
             ("axpy_f32: bad arguments", "axpy_f32", [P, P], dict(n=-1)),
             ("gelu_fwd_bf16: bad arguments", "gelu_fwd_bf16", [P, 0], dict(n=5)),
             ("colsum_bf16: bad arguments", "colsum_bf16", [P, P], dict(a=3, b=16, c=8)),
             ("colsum_bf16: ld%8 and 16-byte alignment required", "colsum_bf16", [P, P], dict(a=3, b=8, c=12)),
             ("sumsq_f32: bad arguments", "sumsq_f32", [P, 0, 0], dict(n=5)),
             ("sumsq_f32: deterministic mode needs the ws form", "sumsq_f32", [P, P, 0], dict(n=5, det=True)),
             ("sumsq_f32: deterministic mode needs the ws form", "sumsq_f32", [P + 4, P, P], dict(n=5, a=64, det=True)),
             ("sumsq_check_f32: bad arguments", "sumsq_check_f32", [P, P, P, 0], dict(n=5, a=1)),
             ("sumsq_check_f32: 16-byte alignment required", "sumsq_check_f32", [P + 4, P, P, 0], dict(n=5, a=64)),
             ("sumsq_check_f32: empty bias-correction table", "sumsq_check_f32", [P, P, P, P], dict(n=5, a=64, b=0)),
             ("adam_step: bad arguments", "adam_step", [P, P, P, P, 0], dict(n=5, a=0)),
             ("adam_step: bad arguments", "adam_step", [P, P, P, P, P], dict(n=0, a=1)),
             ("adam_step_guarded: bad arguments", "adam_step_guarded", [P, P, P, P, 0], dict(n=5)),
             ("adam_step_masked: bad arguments", "adam_step_masked", [P, P, P, P, 0, 0, 0], dict(n=5, a=1)),
             ("adam_step_masked: bad arguments", "adam_step_masked", [P, P, P, P, 0, 0, P], dict(n=5, a=0)),
             ("adam_step_grouped: null pointer", "adam_step_grouped", [P] * 9 + [0, P], dict(n=5, a=1, b=1)),
             ("adam_step_grouped: ngroups must be 1 .. 256", "adam_step_grouped", [P] * 11, dict(n=5, a=1, b=257)),
             ("adam_step_grouped: negative n", "adam_step_grouped", [P] * 11, dict(n=-1, a=1, b=1)),
             ("adam_step_grouped: no source of bias corrections", "adam_step_grouped", [P] * 6 + [0, 0, 0, P, P], dict(n=5, a=0, b=1)),
             ("adam_step_grouped: 16-byte alignment required", "adam_step_grouped", [P] * 4 + [P + 8] + [P] * 6, dict(n=5, a=1, b=1)),
             ("ema_update: p and ema are two non-null buffers", "ema_update", [P, P, 0, 0], dict(n=5, a=1, f=0.9)),
             ("ema_update: negative n", "ema_update", [P, P + 64, 0, 0], dict(n=-1, a=1, f=0.9)),
             ("ema_update: decay must lie in \\(0, 1\\)", "ema_update", [P, P + 64, 0, 0], dict(n=5, a=1, f=1.0)),
             ("ema_update: no source of t", "ema_update", [P, P + 64, 0, 0], dict(n=5, a=0, f=0.9)),
             ("ema_update: 16-byte alignment required", "ema_update", [P, P + 68, 0, 0], dict(n=5, a=1, f=0.9)),
             ("ema_swap: p, ema \\(two buffers\\) and p_bf16 must be given", "ema_swap", [P, P + 64, 0, 0], dict(n=5)),
             ("ema_swap: negative n", "ema_swap", [P, P + 64, P, 0], dict(n=-1)),
             ("ema_swap: 16-byte alignment required", "ema_swap", [P, P + 64, P, P + 2], dict(n=5)),
             ("step_state_advance: null pointer", "step_state_advance", [P, 0], dict(a=3, b=10)),
             ("step_state_advance: bad schedule", "step_state_advance", [P, P], dict(a=3, b=0)))
    for msg, entry, ptrs, kw in cases:
        with pytest.raises(_abi.MMDTIError, match=msg):
            S.stream_plan(lib, entry, ptrs, **kw)
    import ctypes
    with pytest.raises(_abi.MMDTIError, match="stream_plan: unknown entry 17"):
        lib.mmdti_stream_plan(17, 0, (ctypes.c_void_p * 2)(P, P), 5, 0, 0, 0, 0.0, (ctypes.c_longlong * 12)())


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
