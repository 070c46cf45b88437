"""The case table of tests/row_cases.py and the keep rule of tests/dropout_rule.py, checked without a GPU: the rounding points the
reference depends on are verbatim in the sources; the table reaches all 26 LayerNorm / softmax instances, which are exactly the rows of
the library's MMDTI_PLAN_ROW table, and every instance sees every option; the declared dispatch and geometry are the library's
(mmdti_row_plan) for every case and over sweeps of every D and ld, and the query refuses what the launchers refuse, in their words; the
grid statement of the LayerNorm backward is also the one the workspace size follows (ops.det_workspace_bytes); the exact modes are exact in the fp32 emulation; the emulation stays inside every bound with |gain| <= 6; and nine wrong
emulations (one-pass variance, eps outside the root, unbiased variance, row_zero before the statistics, dgamma from the un-dropped dy,
column sums before rounding, softmax over ld, dl before the dropout of dp, the mask indexed by row x Lk + key) leave them.

With MMDTI_ROW_PROFILE=<path> the worst emulation ratio and |gain| per instance and output are merged into that JSON file under
"emulation" (profiles/row_instances.json holds such a run next to the device's)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from mmdti_hip import _abi, ops

import dropout_rule as DR
import row_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = {}
F64, F32, BF16 = R.F64, R.F32, R.BF16


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


# ------------------------------------------------------------------------------------------------ the keep rule
def _keep_scalar(seed, site, idx, p, salt=0):
    """the rule once more, one element at a time in Python integers"""
    M = 0xFFFFFFFF

    def mix(x):
        x ^= x >> 16
        x = x * 0x7FEB352D & M
        x ^= x >> 15
        x = x * 0x846CA68B & M
        return x ^ (x >> 16)

    s = seed ^ salt
    k = mix((s & M) ^ (site * 0x9E3779B9 & M)) ^ (s >> 32)
    ctr = idx >> 2
    a = mix(((ctr & M) ^ k) + (ctr >> 32) * 0x85EBCA6B & M)
    b = mix(a ^ 0xB5297A4D)
    w = (a << 16 & M, a & 0xFFFF0000, b << 16 & M, b & 0xFFFF0000)[idx & 3]
    return w >= int(float(np.float32(p)) * 4294967296.0)


def test_keep_rule_vectorised_equals_scalar():
    idx = list(range(0, 67)) + [2 ** 32 - 1, 2 ** 32, 2 ** 34 + 5, 2 ** 40 + 3]
    for seed, site, salt, p in ((R.SEED, 11, 0, 0.1), (3, 0, 0, 0.35), (R.SEED, 29, 0x9E3779B97F4A7C15, 0.999), (2 ** 63 + 9, 2 ** 31 + 1, 12345, 0.5)):
        got = DR.keep(seed, site, np.array(idx, dtype=np.uint64), p, salt)
        assert got.tolist() == [_keep_scalar(seed, site, i, p, salt) for i in idx]
    assert DR.thresh(0.0) == 0 and DR.thresh(0.5) == 2 ** 31 and DR.thresh(0.1) == int(float(np.float32(0.1)) * 2 ** 32)
    assert DR.dscale(0.0) == 1.0 and DR.dscale(0.5) == 2.0 and DR.dscale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1)))
    assert bool(DR.keep(1, 2, np.arange(9, dtype=np.uint64), 0.0).all())


def test_keep_rule_statistics_and_streams():
    n = 1 << 20
    for p in (0.1, 0.35, 0.999):
        k = DR.keep_flat(R.SEED, 5, n, p)
        assert abs(k.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / n) + 2.0 ** -16          # (p is quantised to 1 / 65536)
    a, b, c = DR.keep_flat(R.SEED, 5, n, 0.5), DR.keep_flat(R.SEED, 6, n, 0.5), DR.keep_flat(R.SEED, 5, n, 0.5, salt=77)
    for u, v in ((a, b), (a, c)):
        assert abs((u == v).mean() - 0.5) < 0.01
    # row x ld + key and row x Lk + key are different masks wherever ld != Lk (wrong emulation 9: on the mask, exactly)
    for c in R.CASES:
        if c["kind"] == "sm_fwd" and c["p"] > 0 and c["ld"] != c["Lk"] and R.sm_rows(c) > 1:
            right = DR.keep_rows(R.SEED, R.SITE_SM, R.sm_rows(c), c["Lk"], c["p"], ld=c["ld"])
            wrong = DR.keep_rows(R.SEED, R.SITE_SM, R.sm_rows(c), c["Lk"], c["p"])
            assert np.array_equal(right[0], wrong[0]) and not np.array_equal(right[1:], wrong[1:]), R.case_id(c)
            assert np.array_equal(right, R.make_inputs(c)["keep"].numpy())


# ------------------------------------------------------------------------------------------------ the table
def test_the_mirrored_lines_are_verbatim_in_the_sources():
    for name, lines in R.SOURCE_LINES.items():
        src = open(os.path.join(ROOT, "mm-dti_amd", "csrc", name)).read()
        for line in lines:
            assert line in src, (name, line)


def test_the_table_reaches_every_instance():
    got = {R.instance(c) for c in R.CASES}
    assert len(R.ALL_INSTANCES) == len(set(R.ALL_INSTANCES)) == 26
    assert got == set(R.ALL_INSTANCES), got ^ set(R.ALL_INSTANCES)
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids)
    assert [R.ln_nv(D) for D in (4, 256, 260, 512, 516, 768, 772, 1024, 1028, 1536, 1792, 2048)] == [1, 1, 2, 2, 4, 4, 4, 4, 8, 8, 8, 8]
    assert [R.sm_nv(ld) for ld in (8, 256, 264, 512, 520, 768, 776, 1024)] == [1, 1, 2, 2, 4, 4, 4, 4]


def test_every_instance_sees_every_option():
    by = {}
    for c in R.CASES:
        by.setdefault(R.instance(c), []).append(c)
    for name, cs in by.items():
        seen = lambda f: {f(c) for c in cs}
        if name.startswith("ln_"):
            assert len([c for c in cs if c["rows"] in (17, 37)]) >= 2 and len({c["D"] for c in cs if c["rows"] in (17, 37)}) >= 2, name
            assert seen(lambda c: c["rz"]) == {True, False} and seen(lambda c: c["eps"]) == {1e-5, 1e-12}, name
        if name.startswith("ln_fwd"):
            assert seen(lambda c: c["p"]) == {0.0, 0.1, 0.35} and seen(lambda c: c["outs"]) == {"both", "y16", "y32"}, name
            assert seen(lambda c: c["f16"]) == {True, False} and seen(lambda c: c["mode"]) == {"random", "offset", "const", "sat"}, name
            assert any(c["mode"] == "sat" and c["f16"] for c in cs) and any(c["mode"] == "sat" and not c["f16"] for c in cs), name
        elif name.startswith("ln_bwd"):
            assert seen(lambda c: c["dy_add"]) == seen(lambda c: c["dres"]) == seen(lambda c: c["nullg"]) == {True, False}, name
            assert seen(lambda c: c["p"] > 0) == {True, False} and seen(lambda c: c["mode"]) == {"random", "offset", "const"}, name
            assert {None, (0.1, True), (0.0, True), (0.35, False)} <= seen(lambda c: c["copy"]), name
        else:
            assert seen(lambda c: c["p"]) == {0.0, 0.1} and len(seen(lambda c: R.sm_rows(c))) == 3, name
            assert seen(lambda c: c["key_add"]) == set(R.KEY_ADDS), name
    rpw = {R.ln_nv(c["D"]) <= 2: R.ln_rpw(c["rows"], c["D"]) for c in R.CASES if c["kind"] == "ln_bwd" and c["rows"] > 8000}
    assert rpw == {True: 5, False: 5}                      # rows_per_wave > 4, once per register class
    assert {(c["Lk"], c["ld"]) for c in R.CASES if c["kind"] == "sm_fwd"} == set(R.SM_SHAPES)


def test_the_plan_table_is_the_instance_list():
    """26 rows, in the order of ALL_INSTANCES, and every row is reached by a case of the table through the library's own plan"""
    lib = _abi.lib()
    import ctypes
    n = ctypes.c_int()
    lib.mmdti_plan_table_size(R.PLAN_FAMILY, ctypes.byref(n))
    names = [lib.mmdti_plan_kernel_name(R.PLAN_FAMILY, i).decode() for i in range(n.value)]
    assert names == R.ALL_INSTANCES and lib.mmdti_plan_kernel_name(R.PLAN_FAMILY, n.value) is None
    reached = {R.library_plan(lib, c)["launches"][0][0] for c in R.CASES}
    assert reached == set(names), reached ^ set(names)


@pytest.mark.parametrize("kind", ("ln_fwd", "ln_bwd", "sm_fwd", "sm_bwd"))
def test_the_declared_plan_is_the_librarys_for_every_case(kind):
    lib = _abi.lib()
    n = 0
    for c in R.CASES:
        if c["kind"] == kind:
            got = R.assert_declared_plan(lib, c)
            assert len(got["launches"]) == (2 if "_slab_" in R.instance(c) else 1)
            n += 1
    assert n >= 36


SWEEP_ROWS = (1, 3, 4, 5, 17, 3071, 3072, 3073, 8197, 12293, 65536)


def test_the_declared_plan_is_the_librarys_over_every_width():
    """every D in 4 .. 2048 and every ld in 8 .. 1024 against rows on both sides of a workgroup, of a resident grid (3072 = 4 x 3 x 256
    waves, 2 x 256 workgroups of the wide rows) and far past it; the backward in both dy types, in and out of the deterministic mode,
    with and without a sum to fold"""
    lib = _abi.lib()
    for D in range(4, 2049, 4):
        for rows in SWEEP_ROWS:
            c = dict(kind="ln_fwd", rows=rows, D=D, outs="both", p=0.0)
            assert R.library_plan(lib, c) == R.declared_plan(c), (rows, D)
            for dybf, det, nullg in ((False, False, False), (True, False, True), (False, True, False), (True, True, False), (True, True, True)):
                c = dict(kind="ln_bwd", rows=rows, D=D, dybf=dybf, det=det, nullg=nullg, copy=None, p=0.0)
                got = R.library_plan(lib, c)
                assert got == R.declared_plan(c), (rows, D, dybf, det, nullg)
                assert len(got["launches"]) == (2 if det and not nullg else 1)
    for ld in range(8, 1025, 8):
        for B, heads, Lq in ((1, 1, 1), (1, 1, 5), (2, 3, 7), (64, 8, 128)):
            for k in ("sm_fwd", "sm_bwd"):
                c = dict(kind=k, B=B, heads=heads, Lq=Lq, Lk=ld - (ld // 3) % 8, ld=ld, p=0.0)
                assert R.library_plan(lib, c) == R.declared_plan(c), (k, ld, B)
    # the slab form needs one sum to fold: each of the three alone brings it
    for ptr in (6, 7, 9):
        ptrs = [R.PTR] * 6 + [0, 0, R.PTR, 0]
        ptrs[ptr] = R.PTR
        assert [l[0] for l in R.row_plan(lib, "ln_bwd", ptrs, 37, 0, 0, 0, 516, det=True)["launches"]] == ["ln_bwd_slab_kernel<4, false>", "det_fold_kernel"]
        assert [l[0] for l in R.row_plan(lib, "ln_bwd", ptrs, 37, 0, 0, 0, 516, det=False)["launches"]] == ["ln_bwd_kernel<4, false>"]


def test_the_query_refuses_in_the_launchers_words():
    lib, P = _abi.lib(), R.PTR
    cases = (("layernorm_fwd: need rows>0, D%4==0, D<=2048 \\(D=2052\\)", "ln_fwd", [P] * 5, (3, 0, 0, 0, 2052), {}),
             ("layernorm_fwd: need rows>0", "ln_fwd", [P] * 5, (0, 0, 0, 0, 64), {}),
             ("layernorm_fwd: null pointer", "ln_fwd", [P, P, P, 0, 0], (3, 0, 0, 0, 64), {}),
             ("layernorm_fwd: 16-byte alignment required", "ln_fwd", [P, P + 8, P, P, P], (3, 0, 0, 0, 64), {}),
             ("layernorm_fwd: dropout p out of range", "ln_fwd", [P] * 5, (3, 0, 0, 0, 64), dict(p=1.0)),
             ("layernorm_bwd: need rows>0, D%4==0, D<=2048 \\(D=6\\)", "ln_bwd", [P] * 10, (3, 0, 0, 0, 6), {}),
             ("layernorm_bwd: null pointer", "ln_bwd", [P, P, P, 0] + [P] * 6, (3, 0, 0, 0, 64), {}),
             ("layernorm_bwd: alignment", "ln_bwd", [P + 4] + [P] * 9, (3, 0, 0, 0, 64), {}),
             ("layernorm_bwd: dropout p out of range", "ln_bwd", [P] * 10, (3, 0, 0, 0, 64), dict(p2=-0.5)),
             ("layernorm_bwd: dx_bf16 alignment", "ln_bwd", [P] * 8 + [P + 4, P], (3, 0, 0, 0, 64), {}),
             ("layernorm_bwd: dx_colsum sums the bf16 copy, which was not requested", "ln_bwd", [P] * 8 + [0, P], (3, 0, 0, 0, 64), {}),
             ("softmax_fwd: bad arguments", "sm_fwd", [P, P, P], (1, 0, 4, 8, 8), {}),
             ("softmax_fwd: need Lk <= ld <= 1024, ld % 8 == 0", "sm_fwd", [P, P, P], (1, 2, 4, 1030, 1032), {}),
             ("softmax_fwd: need Lk <= ld", "sm_fwd", [P, P, P], (1, 2, 4, 9, 8), {}),
             ("softmax_fwd: 16-byte alignment required", "sm_fwd", [P, P + 8, P], (1, 2, 4, 8, 8), {}),
             ("softmax_fwd: dropout needs a separate pd buffer", "sm_fwd", [P, P, P], (1, 2, 4, 8, 8), dict(p=0.1)),
             ("softmax_bwd: bad arguments", "sm_bwd", [P, 0, P], (1, 2, 4, 8, 8), {}),
             ("softmax_bwd: need Lk <= ld <= 1024, ld % 8 == 0", "sm_bwd", [P, P, P], (1, 2, 4, 8, 12), {}),
             ("softmax_bwd: dropout p out of range", "sm_bwd", [P, P, P], (1, 2, 4, 8, 8), dict(p=1.5)))
    for msg, kind, ptrs, shape, kw in cases:
        with pytest.raises(_abi.MMDTIError, match=msg):
            R.row_plan(lib, kind, ptrs, *shape, **kw)
    import ctypes
    with pytest.raises(_abi.MMDTIError, match="layernorm_bwd: bad dy dtype"):
        lib.mmdti_row_plan(1, 0, (ctypes.c_void_p * 10)(*[P] * 10), 3, 0, 0, 0, 64, 7, 0.0, 0.0, (ctypes.c_longlong * 13)())
    with pytest.raises(_abi.MMDTIError, match="row_plan: unknown entry 4"):
        lib.mmdti_row_plan(4, 0, (ctypes.c_void_p * 10)(*[P] * 10), 3, 0, 0, 0, 64, 0, 0.0, 0.0, (ctypes.c_longlong * 13)())


def test_both_plan_headers_under_address_and_undefined_sanitizers(tmp_path):
    """tests/plan_sweep_main.cpp: a stand-alone program over csrc/row_plan.h and csrc/stream_plan.h (every width, sizes up to INT_MAX rows
    and 2^40 elements, every key), built with -fsanitize=address,undefined.  Nothing loaded into Python is sanitized."""
    cxx = os.environ.get("HIPCC") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else shutil.which("hipcc"))
    assert cxx, "no hipcc (the compiler the library itself is built with)"
    exe = str(tmp_path / "plan_sweep_main")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "plan_sweep_main.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-600:], r.stderr[-600:])


def test_the_grid_statement_is_the_librarys():
    shapes = {(c["rows"], c["D"]) for c in R.CASES if c["kind"] == "ln_bwd"}
    shapes |= {(rows, D) for rows in (1, 4, 5, 16, 17, 8192, 8193, 12288, 12289, 16385, 50000, 100001) for D in (4, 64, 512, 516, 1024, 1028, 2048)}
    for rows, D in shapes:
        assert ops.det_workspace_bytes("layernorm_bwd", rows, D) == R.ln_grid(rows, D) * 3 * D * 4, (rows, D)
    assert R.ln_rpw(12288, 64) == 4 and R.ln_rpw(12289, 64) == 5 and R.ln_rpw(8192, 516) == 4 and R.ln_rpw(8193, 516) == 5
    assert R.ln_grid(17, 64) == 2                        # a second block whose last three waves own no row


# ------------------------------------------------------------------------------------------------ exact modes, emulation, wrong emulations
def _emulate(c, mut=None):
    t, ref = R.prepared(c["i"])
    got = R.emulate(c, t, mut)
    return t, ref, got, R.evaluate(c, ref, got)


def test_the_exact_modes_are_exact_in_fp32():
    n = 0
    for c in R.CASES:
        if c["kind"].startswith("ln") and c["mode"] == "const":
            t, ref, got, _ = _emulate(c)
            live = torch.ones(c["rows"], dtype=torch.bool) if t["rz"] is None else ~t["rz"]
            if c["kind"] == "ln_fwd":
                assert torch.equal(got["y32"][live], t["beta"].expand(c["rows"], -1)[live]) and torch.equal(ref["y32"][live].to(F32), got["y32"][live])
            else:
                want = t["dres"] if t["dres"] is not None else torch.zeros(c["rows"], c["D"])
                assert torch.equal(got["dx"], want) and torch.equal(ref["dx"], want.to(F64))
                assert c["rows"] < 17 or float(ref["B_dx"].max()) > 1e-3          # (rstd = 1e6 times the summation term of m1)
                if not c["nullg"]:
                    assert torch.equal(got["dbeta"].to(F64), ref["dbeta"]) and float(got["dgamma"].abs().max()) == 0.0
            n += 1
        if c["kind"] == "sm_fwd" and c["key_add"] in ("min_all", "min_half"):
            t, ref, got, _ = _emulate(c)
            per = c["heads"] * c["Lq"]
            if c["key_add"] == "min_all":
                rows = slice((c["B"] - 1) * per, None)
                want = torch.tensor(1.0 / c["Lk"], dtype=F32).to(BF16)
                assert bool((got["p"][rows] == want).all()) and bool((ref["p"][rows] == want).all())
            elif c["Lk"] > 1:
                assert float(got["p"][:per, c["Lk"] // 2:].float().abs().max()) == 0.0 == float(ref["p"][:per, c["Lk"] // 2:].float().abs().max())
            n += 1
    assert n > 40


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_the_emulation_stays_inside_the_bounds(c):
    t, ref, got, res = _emulate(c)
    row = EMU.setdefault(R.instance(c), {})
    for k, (ratio, z) in res.items():
        old = row.get(k, {"ratio": 0.0, "z": 0.0})
        row[k] = {"ratio": max(old["ratio"], ratio), "z": max(old["z"], abs(z))}
        assert ratio <= 1.0 and abs(z) <= R.Z_MAX, (R.case_id(c), k, ratio, z)
    want = {"ln_fwd": {"mean", "rstd", "y32", "y16"}, "sm_fwd": {"p", "pd"}, "sm_bwd": {"ds"}}.get(c["kind"])
    if want is None:
        want = {"dx"} | (set() if c["nullg"] else {"dgamma", "dbeta"}) | ({"dx16"} if c["copy"] else set()) | ({"colsum", "colsum_own"} if c["copy"] and c["copy"][1] else set())
    assert set(res) == want


def _leaves(pred, mut, outputs):
    """the wrong emulation leaves the bound of one of `outputs` on at least one case that pred selects"""
    tried = 0
    for c in R.CASES:
        if not pred(c) or c.get("rows", 0) > 100:
            continue
        tried += 1
        res = _emulate(c, mut)[3]
        if any(res[k][0] > 1.0 for k in outputs if k in res):
            return R.case_id(c)
        if tried >= 6:
            break
    raise AssertionError(f"the wrong emulation {mut} stays inside the bounds on {tried} cases")


def test_the_wrong_emulations_leave_the_bounds():
    fwd = lambda m: (lambda c: c["kind"] == "ln_fwd" and c["mode"] == m and c["rows"] >= 17)
    print(_leaves(fwd("offset"), "one_pass", ("rstd", "y32", "y16")))
    print(_leaves(lambda c: fwd("random")(c) and c["eps"] == 1e-5, "eps_outside", ("rstd",)))
    print(_leaves(fwd("random"), "unbiased", ("rstd", "y32", "y16")))
    print(_leaves(lambda c: c["kind"] == "ln_fwd" and c["rz"] and c["mode"] == "random", "rz_first", ("mean", "rstd")))
    print(_leaves(lambda c: c["kind"] == "ln_bwd" and c["p"] > 0 and not c["nullg"], "dgamma_undropped", ("dgamma",)))
    print(_leaves(lambda c: c["kind"] == "ln_bwd" and c["copy"] is not None and c["copy"][1] and c["mode"] != "const" and c["rows"] >= 17, "colsum_unrounded", ("colsum_own",)))
    print(_leaves(lambda c: c["kind"] == "sm_fwd" and c["ld"] > c["Lk"] and c["key_add"] != "min_all", "norm_ld", ("p",)))
    print(_leaves(lambda c: c["kind"] == "sm_bwd" and c["p"] > 0, "dl_before_dropout", ("ds",)))
