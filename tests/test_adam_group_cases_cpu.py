"""The case table of tests/adam_group_cases.py, checked without a GPU: it reaches all eight adam_group_kernel<GUARD, MASK, DECOUPLED>
instantiations, every size, every group layout, the scales 0, 1, 0.37 and the decays 0, 0.01, and stream_cases.ADAM_OPTS' options (clip
scale, step state, shadows, zero data) in each; the large size passes the 4096-workgroup cap once with a ragged tail; the declared instance
and grid of every case are the library's own plan (mmdti_stream_plan); the entry point is declared with the arguments the device test passes; the fp32 emulation stays inside every bound with |gain| <= 6; and four wrong
emulations -- coupled and decoupled decay swapped, the group id read at i >> 2, decoupled decay without lr_i, the table's columns
swapped -- leave the bounds."""
import os

import pytest

from mmdti_hip import _abi

import adam_group_cases as G
import stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_table_reaches_every_instantiation_size_layout_and_table_entry():
    assert {k for c in G.CASES for k in G.instance(c)} == set(G.ALL_KERNELS) and len(G.ALL_KERNELS) == 8
    ids = [G.case_id(c) for c in G.CASES]
    assert len(set(ids)) == len(ids)
    assert {c["n"] for c in G.CASES} == set(G.SIZES) == {1, 5, 8, 8 * 125 + 5, 8388608 + 8 * 129 + 5}
    by = {}
    for c in G.CASES:
        by.setdefault(G.instance(c), []).append(c)
    for name, cs in by.items():
        seen = lambda f: {f(c) for c in cs}
        assert seen(lambda c: c["layout"]) == set(G.LAYOUTS), name
        assert seen(lambda c: c["gs"]) == {None, 0.37} and seen(lambda c: c["state"]) == {True, False} and seen(lambda c: c["zero"]) == {True, False}, name
        assert {("bf16",), ("f16",), ("bf16", "f16"), ()} <= seen(lambda c: c["shadows"]), name
        assert {1, 5, 8, G.MID} <= seen(lambda c: c["n"]), name
        scales = {s for c in cs for s, _ in G.table_of(c)}
        decays = {w for c in cs for _, w in G.table_of(c)}
        assert {0.0, 1.0, 0.37} <= scales and decays == {0.0, 0.01}, name
    for c in G.CASES:                                             # every layout shows what it is named for
        t_ids, ng = G.group_ids(c), len(G.table_of(c))
        assert t_ids.numel() == (c["n"] + 7) // 8
        if c["layout"] == "clamped":
            assert int(t_ids.max()) >= ng
        else:
            assert int(t_ids.max()) < ng
        if c["layout"] == "single" and c["n"] == G.MID:
            k = t_ids.numel() // 2
            assert t_ids[k] == 2 and t_ids[k - 1] == 1 and t_ids[k + 1] == 3 and G.TABLE4[2][0] == 0.0
        if c["layout"] == "last" and c["n"] == G.MID:
            assert c["n"] % 8 == 5 and t_ids[-1] != 0 and bool((t_ids[:-1] == 0).all())
        if c["layout"] == "alternate" and c["n"] >= G.MID:
            assert t_ids[:8].tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    assert {c["layout"] for c in G.CASES if c["n"] == G.MID and c["n"] % 8} >= {"last", "clamped", "single"}
    assert sorted((c["guard"], c["mask"], c["decoupled"]) for c in G.CASES if c["n"] == G.BIGG) == sorted(G.BIG_IN)


def test_the_large_size_crosses_the_grid_cap_once_with_a_tail():
    for c in G.CASES:
        g, per, items = G.launch(c)
        if c["n"] == G.BIGG:
            assert g == G.CAP == 4096 and per == 2048 and G.rounds(c) == 2 and items - g * per == 8 * 129 + 5 and c["n"] % 8 == 5
        else:
            assert g == 1 and G.rounds(c) == 1
    src = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "elementwise.hip")).read()
    assert "const int gid = min((int)group[blk], ngroups - 1);" in src


def test_the_declared_plan_is_the_librarys_for_every_case():
    """instance() and launch() against mmdti_stream_plan, called as the device test calls mmdti_adam_step_grouped: the eight rows are
    reached, each by the (guard, skip, decoupled) the case gives, with the grid launch() states"""
    lib = _abi.lib()
    reached = set()
    for c in G.CASES:
        got = G.assert_declared_plan(lib, c)
        assert len(got["launches"]) == 1 and got["launches"][0][1] == (4096 if c["n"] == G.BIGG else 1)
        reached.add(got["launches"][0][0])
    assert reached == set(G.ALL_KERNELS)
    with pytest.raises(_abi.MMDTIError, match="adam_step_grouped: ngroups must be 1 .. 256"):
        S.stream_plan(lib, "adam_step_grouped", [S.PTR] * 11, 8, a=1, b=0)


def test_the_entry_point_is_declared_as_the_device_test_calls_it():
    rest, argtypes, names = _abi.parse_header()["mmdti_adam_step_grouped"]
    assert names == ["stream", "p", "g", "m", "v", "p_bf16", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale_dev", "step_state_dev", "p_f16", "guard",
                     "skip", "group", "table_dev", "ngroups", "decoupled"]
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2


def _emulate(c, mut=None):
    t, ref = G.prepared(c["i"])
    return t, ref, G.evaluate(c, ref, G.emulate(c, t, mut))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_the_emulation_stays_inside_the_bounds(c):
    t, ref, res = _emulate(c)
    assert set(res) == set(ref) == {"p", "m", "v"}
    for k, (ratio, z) in res.items():
        assert ratio <= 1.0 and abs(z) <= S.Z_MAX, (G.case_id(c), k, ratio, z)
    if c["zero"] and c["layout"] == "one":                           # g = 0, m = v = 0, no decay: nothing moves, bit for bit
        got = G.emulate(c, t)
        assert all(bool((got[k] == t[k]).all()) for k in ("p", "m", "v"))


def _leaves(pred, mut):
    tried = 0
    for c in G.CASES:
        if not pred(c) or c["zero"] or c["n"] != G.MID:
            continue
        tried += 1
        if any(r > 1.0 for r, _ in _emulate(c, mut)[2].values()):
            return G.case_id(c)
    raise AssertionError(f"the wrong emulation {mut} stays inside the bounds on {tried} cases")


def test_the_wrong_emulations_leave_the_bounds():
    assert G.MUTATIONS == ("swap_decay", "gid_shift", "decay_no_lr", "cols_swapped")
    print(_leaves(lambda c: c["decoupled"], "swap_decay"))
    print(_leaves(lambda c: not c["decoupled"], "swap_decay"))
    print(_leaves(lambda c: c["layout"] == "alternate" or c["layout"] == "clamped", "gid_shift"))
    print(_leaves(lambda c: c["decoupled"], "decay_no_lr"))
    print(_leaves(lambda c: c["layout"] != "one", "cols_swapped"))
