"""What holds for the attention-map kernels (csrc/attn_maps.hip) without a GPU: mmdti_maps_plan answers what tests/maps_cases.py
declares -- for every case and for a sweep of every length --, the case tables reach every row of table MMDTI_PLAN_MAPS, the exact
modes are exact in the fp32 emulation, the emulation stays inside the derived bounds for every case, two wrong emulations (the
mean over H + 1 heads; natural-unit statistics read as base-2) fall outside, and every validation message is raised before a launch."""
import ctypes

import pytest
import torch

from mmdti_hip import _abi
from mmdti_hip._abi import MMDTIError

import maps_cases as M


@pytest.fixture(scope="module")
def lib():
    return _abi.lib()


def test_table_rows(lib):
    n = ctypes.c_int(0)
    lib.mmdti_plan_table_size(M.MAPS_FAMILY, ctypes.byref(n))
    assert n.value == len(M.TABLE)
    assert tuple(lib._dll.mmdti_plan_kernel_name(M.MAPS_FAMILY, i).decode() for i in range(n.value)) == M.TABLE
    assert lib._dll.mmdti_plan_kernel_name(M.MAPS_FAMILY, n.value) is None
    assert lib.const["MMDTI_PLAN_MAPS"] == M.MAPS_FAMILY


def test_plan_of_every_case(lib):
    reached = set()
    for c in M.ATTN_CASES:
        got = M.library_attn_plan(lib, c["B"], c["heads"], c["Lq"], c["Lk"], c["hd"], c["Lq_out"], c["ld_out"],
                                  vargs=(M.PTR, M.PTR, M.PTR, 7) if c["packed"] else (0, 0, 0, 0), add=0 if c["packed"] else M.PTR)
        assert got == M.declared_attn_plan(c["B"], c["Lq_out"], c["ld_out"], c["hd"]), (M.attn_case_id(c), got)
        reached.add(got[0])
    for c in M.PAIR_CASES:
        rag = (M.PTR, M.PTR) if c["lens"] else (0, 0)
        got = M.library_pair_plan(lib, c["B"], c["N"], c["H"], c["ld"], c["ld_out"], c["layout"], key_tiles=rag[0], n_real=rag[1])
        assert got == M.declared_pair_plan(c["B"], c["N"], c["layout"]), (M.pair_case_id(c), got)
        reached.add(got[0])
    assert reached == set(M.TABLE)


def test_plan_sweep(lib):
    """every Lq, Lk in 1..512 (head_dim 32; the other head sizes along Lq = Lk) and every N in 1..320"""
    fn = lib._dll.mmdti_maps_plan
    o = (ctypes.c_int * 6)()
    name = [lib._dll.mmdti_plan_kernel_name(M.MAPS_FAMILY, i).decode() for i in range(len(M.TABLE))]

    def attn(hd, Lq, Lk):
        assert fn(0, M.PTR, M.PTR, 0, M.PTR, M.PTR, 2, 3, Lq, Lk, hd, 3 * hd, 3 * hd, Lq, Lk, -1, 0, 0, 0, 0, 0, 0, 0, 0, o) == 0
        assert (name[o[0]],) + tuple(o[1:]) == M.declared_attn_plan(2, Lq, Lk, hd), (hd, Lq, Lk, list(o))

    for Lq in range(1, 513):
        for Lk in range(1, 513):
            attn(32, Lq, Lk)
    for hd in (16, 64):
        for L in range(1, 513):
            attn(hd, L, L)
    for N in range(1, 321):
        for layout in (0, 1, 3):
            if layout and N > 272:
                with pytest.raises(MMDTIError, match="tiled layouts hold N <= 272"):
                    M.library_pair_plan(lib, 3, N, 3, M.pair_ld(N), N, layout)
                continue
            assert M.library_pair_plan(lib, 3, N, 3, M.pair_ld(N), N, layout) == M.declared_pair_plan(3, N, layout), (N, layout)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("r", M.attn_runs(("selector", "uniform")), ids=M.run_id)
def test_attn_exact_modes(r):
    c, mode = r
    t = M.attn_inputs(c, mode)
    for head in (-1, c["heads"] - 1):
        want = (M.attn_selector_expectation if mode == "selector" else M.attn_uniform_expectation)(c, t, head)
        assert _bits_equal(M.attn_emulate(c, t, head), want), (M.run_id(r), head)
        ref, _ = M.attn_reference(c, t, head)
        assert float((want.double() - ref).abs().max()) <= 2.0 ** -24, (M.run_id(r), head)


@pytest.mark.parametrize("r", M.pair_runs(("selector", "uniform")), ids=M.run_id)
def test_pair_exact_modes(r):
    c, mode = r
    t = M.pair_inputs(c, mode)
    for head in (-1, c["H"] - 1):
        want = (M.pair_selector_expectation if mode == "selector" else M.pair_uniform_expectation)(c, t, head)
        assert _bits_equal(M.pair_emulate(c, t, head), want), (M.run_id(r), head)
        ref, _ = M.pair_reference(c, t, head)
        assert float((want.double() - ref).abs().max()) <= 2.0 ** -24, (M.run_id(r), head)


@pytest.mark.parametrize("r", M.attn_runs(("random",)), ids=M.run_id)
def test_attn_emulation_inside_and_wrong_ones_outside(r):
    c, mode = r
    t = M.attn_inputs(c, mode)
    ref, bnd = M.attn_reference(c, t)
    assert M.worst_ratio(M.attn_emulate(c, t), ref, bnd) <= 1.0, M.run_id(r)
    ref1, bnd1 = M.attn_reference(c, t, 1)
    assert M.worst_ratio(M.attn_emulate(c, t, 1), ref1, bnd1) <= 1.0, M.run_id(r)
    assert M.worst_ratio(M.attn_emulate(c, t, denom=c["heads"] + 1), ref, bnd) > 1.0, M.run_id(r)
    if c["variant"] != "allmask" and c["Lk"] > 1:       # (a uniform row has m = -FLT_MAX, a single key p = 1 whatever m is)
        assert M.worst_ratio(M.attn_emulate(c, t, nat_stats=True), ref, bnd) > 1.0, M.run_id(r)


@pytest.mark.parametrize("r", M.pair_runs(("random",)), ids=M.run_id)
def test_pair_emulation_inside_and_wrong_one_outside(r):
    c, mode = r
    t = M.pair_inputs(c, mode)
    ref, bnd = M.pair_reference(c, t)
    assert M.worst_ratio(M.pair_emulate(c, t), ref, bnd) <= 1.0, M.run_id(r)
    ref1, bnd1 = M.pair_reference(c, t, 1)
    assert M.worst_ratio(M.pair_emulate(c, t, 1), ref1, bnd1) <= 1.0, M.run_id(r)
    assert M.worst_ratio(M.pair_emulate(c, t, denom=c["H"] + 1), ref, bnd) > 1.0, M.run_id(r)


ATTN_OK = dict(q=M.PTR, k=M.PTR, add=0, stats=M.PTR, out=M.PTR, B=2, heads=3, Lq=17, Lk=33, hd=32, ldq=96, ldk=96, Lq_out=17, ld_out=33, head=-1,
               vargs=(0, 0, 0, 0), q_cnt=0)
ATTN_BAD = [
    (dict(q=0), "attn_map: bad arguments"), (dict(k=0), "attn_map: bad arguments"), (dict(stats=0), "stats is required"),
    (dict(out=0), "attn_map: null out"), (dict(hd=48), "head_dim must be 16, 32 or 64"), (dict(Lq=513, Lq_out=513), "at most 512 queries / keys"),
    (dict(Lk=513, ld_out=513), "at most 512 queries / keys"), (dict(ldq=95), "row strides"), (dict(ldk=88), "row strides"),
    (dict(q=M.PTR + 8), "16-byte alignment"), (dict(stats=M.PTR + 4), "stats need 8-byte"), (dict(out=M.PTR + 2), "4-byte alignment"),
    (dict(head=3), "head must be -1"), (dict(head=-2), "head must be -1"), (dict(ld_out=32), r"ld_out \(32\) < Lk \(33\)"),
    (dict(Lq_out=16), r"Lq_out \(16\) < Lq \(17\)"), (dict(vargs=(M.PTR, 0, M.PTR, 5)), "come together"),
    (dict(vargs=(M.PTR, M.PTR, M.PTR, 0)), "packed sequences need q_rows > 0"), (dict(vargs=(M.PTR, M.PTR, M.PTR, 5), add=M.PTR), "take no key_add"),
    (dict(vargs=(0, 0, 0, 5)), "dense sequences take q_rows = 0"),
]
PAIR_OK = dict(s=M.PTR, out=M.PTR, B=3, N=130, H=3, ld=132, ld_out=130, layout=3, head=-1, key_tiles=0, n_real=0)
PAIR_BAD = [
    (dict(s=0), "pair_attn_map: bad arguments"), (dict(out=0), "pair_attn_map: null out"), (dict(layout=2), "layout must be 0"),
    (dict(N=321, ld=324, ld_out=321, layout=0), "exceeds the supported 320"), (dict(N=273, ld=276, ld_out=273), "tiled layouts hold N <= 272"),
    (dict(layout=0, ld=129), r"ld \(129\) < N \(130\)"), (dict(s=M.PTR + 8), "16-byte"), (dict(layout=0, s=M.PTR + 2), "4-byte"),
    (dict(out=M.PTR + 1), "out needs 4-byte"), (dict(head=3), "head must be -1"), (dict(ld_out=129), r"ld_out \(129\) < N \(130\)"),
    (dict(key_tiles=M.PTR, n_real=M.PTR, layout=1), "layout 3 only"), (dict(key_tiles=M.PTR), "key_tiles needs n_real"),
]


@pytest.mark.parametrize("change,msg", ATTN_BAD, ids=[str(i) for i in range(len(ATTN_BAD))])
def test_attn_map_validation(lib, change, msg):
    a = dict(ATTN_OK)
    M.library_attn_plan(lib, a.pop("B"), a.pop("heads"), a.pop("Lq"), a.pop("Lk"), a.pop("hd"), a.pop("Lq_out"), a.pop("ld_out"), **a)
    a = dict(ATTN_OK, **change)
    with pytest.raises(MMDTIError, match=msg):
        M.library_attn_plan(lib, a.pop("B"), a.pop("heads"), a.pop("Lq"), a.pop("Lk"), a.pop("hd"), a.pop("Lq_out"), a.pop("ld_out"), **a)
    # the launch validates with the same function, before anything reaches a device
    a = dict(ATTN_OK, **change)
    with pytest.raises(MMDTIError, match=msg):
        lib.mmdti_attn_map(0, a["q"], a["k"], a["add"], a["stats"], a["out"], a["B"], a["heads"], a["Lq"], a["Lk"], a["hd"], a["ldq"], a["ldk"],
                           a["Lq_out"], a["ld_out"], 1.0, a["head"], *a["vargs"], a["q_cnt"])


@pytest.mark.parametrize("change,msg", PAIR_BAD, ids=[str(i) for i in range(len(PAIR_BAD))])
def test_pair_attn_map_validation(lib, change, msg):
    a = dict(PAIR_OK)
    M.library_pair_plan(lib, a.pop("B"), a.pop("N"), a.pop("H"), a.pop("ld"), a.pop("ld_out"), a.pop("layout"), **a)
    a = dict(PAIR_OK, **change)
    with pytest.raises(MMDTIError, match=msg):
        M.library_pair_plan(lib, a.pop("B"), a.pop("N"), a.pop("H"), a.pop("ld"), a.pop("ld_out"), a.pop("layout"), **a)
    a = dict(PAIR_OK, **change)
    with pytest.raises(MMDTIError, match=msg):
        lib.mmdti_pair_attn_map(0, a["s"], a["out"], a["B"], a["N"], a["H"], a["ld"], a["ld_out"], a["head"], a["layout"], a["key_tiles"], a["n_real"])


def test_plan_needs_plan_out(lib):
    with pytest.raises(MMDTIError, match="null plan_out"):
        lib.mmdti_maps_plan(1, M.PTR, 0, 0, 0, M.PTR, 3, 3, 130, 0, 0, 132, 0, 0, 130, -1, 0, 0, 0, 0, 0, 3, 0, 0, 0)
