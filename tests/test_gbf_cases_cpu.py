"""The case table of tests/gbf_cases.py, checked without a GPU: that the rounding points its reference depends on are verbatim in
csrc/gbf.hip; that the table reaches all 27 kernel instances -- the list is the library's own kernel table -- and every runtime branch
inside them; that the library, asked through the launch-free query mmdti_gbf_plan, plans for every case and for a sweep of shapes
what the table declares, and refuses what the launcher refuses with the launcher's message; that the Python mirror
of tile counts, grids and prefixes agrees with ops and with values computed by hand; that the closed-form gradients of the reference
agree with float64 autograd; that the onehot mode is exact by construction;
that the fp32 emulation of the kernels' rounding points stays inside the bounds with |gain| < 3; and that six wrong emulations (a
dropped tile, two swapped columns of W1, the dstds sign, a halved dmul entry, pi for 3.14159, sigma without its 1e-5) do not.

With MMDTI_GBF_PROFILE=<path> the worst emulation ratio and |gain| per kernel family and output are merged into that JSON file under
"emulation" (profiles/gbf_instances.json holds such a run next to the device's)."""
import ctypes
import json
import math
import os

import pytest
import torch

from mmdti_hip import _abi

import gbf_cases as Gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "mm-dti_amd", "csrc", "gbf.hip")).read()
EMU = {}


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    for k, v in sorted(EMU.items()):
        print(f"emulation {k}: ratio {v['ratio']:.3g} |z| {v['z']:.3g}")
    path = os.environ.get("MMDTI_GBF_PROFILE")
    if path and EMU:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["emulation"] = EMU
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def table_names():
    lib = _abi.lib()
    n = ctypes.c_int()
    lib.mmdti_plan_table_size(1, ctypes.byref(n))
    names = [lib.mmdti_plan_kernel_name(1, i).decode() for i in range(n.value)]
    assert lib.mmdti_plan_kernel_name(1, n.value) is None and lib.mmdti_plan_kernel_name(1, -1) is None
    return names


def test_the_mirrored_lines_are_verbatim_in_the_source():
    for line in Gc.SOURCE_LINES:
        assert line in SRC, line
    assert abs(Gc.GBF_A - (2 * 3.14159) ** 0.5) < 1e-9 and Gc.GBF_SLAB == 16384 + 8192 + 128 + 64 + 256


def test_the_table_reaches_every_instance_of_the_library():
    names = [Gc.canonical(n) for n in table_names()]
    want = set(names)
    assert len(names) == len(want) == 27 and len([i for i in want if i.startswith("gbf_bias_fwd")]) == 9 and len([i for i in want if "full" in i]) == 12
    assert len([i for i in want if i.startswith("gbf_bias_bwd_kernel")]) == 3 and {i for i in want if "<" not in i} == {"gbf_fwd_kernel", "gbf_bwd_kernel", "gbf_bwd_det_kernel"}
    got = {Gc.instance(c) for c in Gc.CASES}
    assert got == want, (got ^ want)
    assert len({Gc.case_id(c) for c in Gc.CASES}) == len(Gc.CASES)
    ids = [Gc.run_id(r) for r in Gc.runs()] + [Gc.run_id(r) for r in Gc.edge_runs()]
    assert len(set(ids)) == len(ids)


def _plan(c, **kw):
    return Gc.library_plan(_abi.lib(), c, **kw)


def test_the_library_plans_what_every_case_declares():
    """instance, workgroup size, grid, tpm, ntiles, ltab, slab use and the slab-reduce launch of every case -- and of every edge-type width"""
    for c in Gc.CASES:
        for esz in (8, 4, 2) if c["kind"] in ("fwd", "bwd", "full") and not c["coords"] else (8,):
            got, want = _plan(c, esz=esz), Gc.declared_plan(c)
            assert {f: got[f] for f in want} == want, (Gc.case_id(c), got, want)
    full = next(c for c in Gc.CASES if c["kind"] == "full" and c["ws"] and not c["det"] and c["N"] == 130)
    need = Gc.launch(full)["grid"] * (Gc.GBF_SLAB + 2 * full["E"]) * 4
    assert _plan(full, ws=need)["slab"] == 1 and _plan(full, ws=need - 1)["slab"] == 0 and _plan(full, ws=need - 1)["reduce_grid"] == 0


SWEEP_E = (1, 961, 1521, 1536, 4096, 4097, 5000)


def _sweep_case(kind, N, layout, B, E, coords=False, save=False, det=False, ws=True):
    V = math.isqrt(E)
    return dict(kind=kind, N=N, layout=layout, B=B, E=E, V=V, coords=coords, save=save, ugrad=False, det=det, ws=ws, lens=None, packed=False, modes=(),
                ld=Gc.pair_ld(N))


def _refusal(c):
    """the launcher's message for a combination it refuses, in the order of its checks; None: it launches"""
    k, E = c["kind"], c["E"]
    if k == "ffwd":
        return None
    if k == "fbwd":
        return "deterministic mode keeps the mul / bias histograms in LDS" if c["det"] and E > Gc.GBF_MAXE else None
    if c["coords"] and c["V"] ** 2 != E:
        return r"V \* V must be the edge-table size"
    if k == "fwd":
        return None
    if k == "bwd":
        if c["det"]:
            return "no fixed-order form yet -- refused in the deterministic mode"
        if E > Gc.GBF_MAXE:
            return r"gbf_bias_bwd: bad shape \(E <= 4096\)"
        # weight images, three rows of 128 floats and four fp32 tables over the edge types in 96 KiB of LDS
        return f"{E} edge types do not fit the LDS tables" if (128 * 136 + 128 * 72) * 2 + (3 * 128 + 4 * E) * 4 > 96 * 1024 else None
    if E > Gc.GBF_FULL_MAXE:
        return r"gbf_bias_bwd_full: bad shape \(E <= 1536\)"
    return "deterministic mode needs the workspace" if c["det"] and not c["ws"] else None


def _sweep():
    for E in SWEEP_E:
        for B in (1, 2, 3, 4, 8):
            for N in range(1, 141):
                yield _sweep_case("ffwd", N, "row", B, E)
                for det in (False, True):
                    yield _sweep_case("fbwd", N, "row", B, E, det=det)
                for lay in ("row", "tiled", "compact"):
                    for save, co in ((False, False), (True, False), (False, True)):
                        yield _sweep_case("fwd", N, lay, B, E, coords=co, save=save)
                    for det in (False, True):
                        yield _sweep_case("bwd", N, lay, B, E, det=det)
                        for co in (False, True):
                            for ws in (True, False):
                                yield _sweep_case("full", N, lay, B, E, coords=co, det=det, ws=ws)


def test_a_sweep_of_shapes_plans_the_declared_launches_or_refuses_as_the_launcher_does():
    """N = 1..140 x B x layouts x save / coords / det x E, with and without workspace: every table row is reached, nothing else is named"""
    seen, refused = set(), set()
    for c in _sweep():
        msg = _refusal(c)
        if msg:
            refused.add(msg)
            with pytest.raises(_abi.MMDTIError, match=msg):
                _plan(c)
            continue
        got, want = _plan(c), Gc.declared_plan(c)
        assert {f: got[f] for f in want} == want, (c, got, want)
        seen.add(got["name"])
    assert seen == {Gc.canonical(n) for n in table_names()} and len(refused) == 7


def test_the_plan_query_validates_like_the_launch():
    c = next(c for c in Gc.CASES if c["kind"] == "fwd" and c["save"] and c["layout"] == "tiled")
    for kw, msg in ((dict(operands=0), "gbf_bias_fwd: null argument"), (dict(aligned=Gc.PTR + 8), "gbf_bias_fwd: 16-byte alignment required"),
                    (dict(esz=3), "edge types must be int64, int32 or int16")):
        with pytest.raises(_abi.MMDTIError, match=msg):
            _plan(c, **kw)
    with pytest.raises(_abi.MMDTIError, match="compact planes .* exist in the tiled layout only"):
        _abi.lib().mmdti_gbf_plan(2, 0, Gc.PTR, Gc.PTR, 0, 0, 0, 0, 0, 0, 0, 3, 5, 8, Gc.K, Gc.F, Gc.H, 961, 31, 0, 8, 4, (ctypes.c_longlong * 10)())   # flags: compact, not tiled
    with pytest.raises(_abi.MMDTIError, match="tile_prefix .* needs the tiled pair layout"):
        _plan(dict(c, layout="row", lens=(5,), save=False))
    f = next(c for c in Gc.CASES if c["kind"] == "ffwd")
    with pytest.raises(_abi.MMDTIError, match="feat must be 16-byte aligned"):
        _plan(f, aligned=Gc.PTR + 2)


def test_every_instance_meets_every_size_mode_and_branch():
    by = {}
    for c in Gc.CASES:
        by.setdefault(Gc.instance(c), []).append(c)
    for inst, cs in by.items():
        fused, planes = inst.startswith("gbf_bias"), not any(c["coords"] for c in cs)
        assert {c["N"] for c in cs} >= set(Gc.NS), inst
        assert {m for c in cs for m in c["modes"]} == set(Gc.MODES), inst
        big = [c for c in cs if c["N"] == 130 and c["lens"] is None]
        assert big and all(Gc.launch(c)["rounds"] >= 2 and Gc.launch(c)["ntiles"] % (Gc.launch(c)["grid"] * (4 if c["kind"] == "bwd" else 8)) for c in big if fused), inst
        if fused:
            Es = {c["E"] for c in cs}
            assert Es >= ({961, 1, 1536} if planes else {961, 1521}), inst
            if "fwd" in inst:
                assert any(c["E"] > Gc.GBF_FWD_MAXE for c in cs), inst                             # ltab off
            if planes:
                assert {r[2] for r in Gc.edge_runs() if Gc.instance(r[0]) == inst} == {4, 2}, inst
            tiled = inst.split("<")[1].split(",")[1 if "fwd" in inst else 0].strip() == "true"
            if tiled and "bias_bwd_kernel" not in inst:
                assert any(c["lens"] is not None and not c["packed"] for c in cs) and any(c["packed"] for c in cs), inst
                for c in cs:
                    if c["lens"] is not None:
                        assert max(c["lens"]) == c["N"] and min(c["lens"]) < 16
        if inst.startswith("gbf_bias_fwd_kernel<true") or inst.startswith("gbf_bias_bwd_kernel"):
            assert {c["ugrad"] for c in cs} == {True, False}, inst
        if "full" in inst:
            det = inst.split(",")[2].strip() == "true"
            assert {c["ws"] for c in cs} == ({True} if det else {True, False}), inst
    assert {c["E"] for c in by["gbf_bwd_kernel"]} >= {961, 1, 5000} and {c["E"] for c in by["gbf_fwd_kernel"]} >= {961, 1, 5000}
    assert any(Gc.launch(c)["rounds"] >= 2 for c in by["gbf_fwd_kernel"]) and all(c["E"] <= Gc.GBF_MAXE for c in by["gbf_bwd_det_kernel"])
    for N in (5, 17, 37):
        assert N * Gc.pair_ld(N) % 16 != 0
    for c, m, esz in Gc.edge_runs():
        assert m in ("random", "clamp") and (m == "clamp" or c["lens"] is None) and esz in (4, 2)


def test_the_mirror_of_tiles_grids_and_prefixes():
    from mmdti_hip import ops
    L = lambda **kw: Gc.launch(dict(dict(kind="fwd", N=5, B=3, layout="row", lens=None, packed=False, det=False, ld=Gc.pair_ld(kw.get("N", 5))), **kw))
    # by hand: N = 5: ld 8, 40 slots -> 3 tiles a molecule; tiled: 2 x 2 blocks.  N = 17: ld 20, 340 slots -> 22; tiled 5 x 5.  N = 130: ld 132, 17160 -> 1073; 33 x 33
    assert (L()["tpm"], L()["ntiles"], L()["grid"], L()["rounds"]) == (3, 9, 2, 1)
    assert L(layout="tiled")["tpm"] == 4 and L(N=17)["tpm"] == 22 and L(N=17, layout="tiled")["tpm"] == 25
    big = L(N=130, B=4)
    assert (big["tpm"], big["ntiles"], big["grid"], big["rounds"]) == (1073, 4292, 512, 2) and L(N=130, B=4, layout="tiled")["ntiles"] == 4356
    assert L(kind="bwd", N=130, B=4) == dict(tpm=1073, ntiles=4292, grid=1024, rounds=2) and L(kind="bwd")["grid"] == 3
    assert L(kind="full", N=130, B=2) == dict(tpm=1073, ntiles=2146, grid=256, rounds=2)
    assert Gc.launch(dict(kind="fbwd", N=37, B=3, det=True))["grid"] == 256 and Gc.launch(dict(kind="fbwd", N=37, B=3, det=False))["grid"] == 257
    for c in Gc.CASES:
        assert Gc.pair_ld(c["N"]) == ops.pair_ld(c["N"]) and Gc.pair_plane(c["N"]) == ops.pair_plane(c["N"])
        if c["lens"] is None:
            continue
        geo = Gc.geometry(Gc.pc_of(c))
        kt = torch.tensor([(n + 15) // 16 for n in c["lens"]])
        if c["packed"]:
            pf, pb, rf, rbk = ops.gbf_tile_prefixes(kt, c["N"], "cpu", torch.tensor(geo["qlive"]))
            assert rf.tolist() == Gc.row_blocks(c, geo) == rbk.tolist()
        else:
            pf, pb = ops.gbf_tile_prefixes(kt, c["N"], "cpu")
        assert pf.tolist() == Gc.prefix(c, geo) == pb.tolist()
        w = Gc.written(c, geo)
        assert int(w[:, ::4, ::4].sum()) + 0 == sum(len(range(0, min(4 * r, c["N"]), 4)) * (min(16 * k, geo["cols"]) // 4) for r, k in zip(Gc.row_blocks(c, geo), geo["ke"])) == Gc.prefix(c, geo)[-1]
    # by hand: N = 37 (10 x 10 blocks, 3 key tiles), lengths (29, 37, 1, 13): covered tiles 2, 3, 1, 1 -> 8, 10, 4, 4 column blocks of 10 row blocks
    c = next(c for c in Gc.CASES if c["lens"] == (29, 37, 1, 13) and not c["packed"])
    assert Gc.prefix(c, Gc.geometry(Gc.pc_of(c))) == [0, 80, 180, 220, 260]
    c = next(c for c in Gc.CASES if c["lens"] == (29, 37, 1, 13) and c["packed"])          # rows 30, 37, 2, 14 -> 8, 10, 1, 4 row blocks
    assert Gc.prefix(c, Gc.geometry(Gc.pc_of(c))) == [0, 64, 164, 168, 184]


@pytest.mark.parametrize("lay,N", [("row", 5), ("tiled", 17), ("compact", 37)])
def test_the_closed_form_gradients_agree_with_float64_autograd(lay, N):
    """the chain without its rounding points against autograd of sum(out G), on the pairs a ragged launch computes where there is one"""
    c = next(c for c in Gc.CASES if c["kind"] == "full" and c["layout"] == lay and c["N"] == N and (c["lens"] is not None or lay == "row"))
    geo = Gc.geometry(Gc.pc_of(c))
    t = dict(Gc.make_inputs(c, "random"), _exact=True)
    ref = Gc.chain(c, t, geo, bounds=False)
    sel = ref["sel"]
    p = {k: t[k].to(Gc.F64).clone().requires_grad_() for k in ("mul", "bias", "means", "stds", "w1", "b1", "w2", "b2")}
    e, d = t["e"].reshape(-1)[sel], t["d"].reshape(-1)[sel].to(Gc.F64)
    sg = p["stds"].abs() + 1e-5
    z = ((p["mul"][e] * d + p["bias"][e]).view(-1, 1) - p["means"]) / sg
    basis = torch.exp(-0.5 * z * z) / ((2 * 3.14159) ** 0.5 * sg)
    u = basis @ p["w1"].t() + p["b1"]
    out = torch.nn.functional.gelu(u) @ p["w2"].t() + p["b2"]
    (out * t["G"].reshape(-1, Gc.H)[sel].to(Gc.F64)).sum().backward()
    for k, n in zip(Gc.GRADS, ("w1", "b1", "w2", "b2", "mul", "bias", "means", "stds")):
        err = float((ref[k] - p[n].grad).abs().max())
        assert err <= 1e-11 * max(1.0, float(p[n].grad.abs().max())), (k, err)


ONEHOT = Gc.runs(("onehot",))


@pytest.mark.parametrize("r", ONEHOT, ids=Gc.run_id)
def test_onehot_is_exact_by_construction(r):
    c, m = r
    t, geo, ref = Gc.prepared(c["i"], m)
    assert Gc.onehot_is_exact(c, t)
    feat, u = Gc.onehot_expectation(c, t)
    sel = ref["sel"]
    fc = dict(c, kind="fwd", save=True, ugrad=False, layout="row" if c["kind"] in ("ffwd", "fbwd") else c["layout"])
    got = Gc.chain(fc, t, geo) if c["kind"] != "ffwd" else dict(ref, u=None)
    assert torch.equal(got["feat"].to(Gc.BF16), feat.reshape(-1, Gc.K)[sel])                 # the float64 reference = the fp32 expectation, bit for bit
    if got["u"] is not None:
        assert torch.equal(got["u"].to(Gc.BF16), u.reshape(-1, Gc.F)[sel])
    emu = Gc.emulate(fc, t, geo, ref) if c["kind"] != "ffwd" else Gc.emulate(c, t, geo, ref)
    assert torch.equal(emu["feat"].to(Gc.BF16), feat.reshape(-1, Gc.K)[sel])
    if "dmul" in ref:                                                                        # mul = 0, z = 0: dy is exactly 0
        assert float(ref["dmul"].abs().max()) == 0.0 and float(ref["dbias"].abs().max()) == 0.0
    for k, v in Gc.evaluate(c, ref, Gc.emulate(c, t, geo, ref)).items():
        assert v[0] < 1.0 and abs(v[1]) < 3.0, (Gc.run_id(r), k, v)


def test_the_boundary_stds_tell_pi_from_3_14159():
    for x in (0.7, 1.1):
        s = torch.tensor(Gc.boundary_std(x), dtype=torch.float32)
        assert abs(float(s) - x) < 0.03
        assert Gc._cf32(s, Gc.GBF_A).to(Gc.BF16) != Gc._cf32(s, (2 * torch.pi) ** 0.5).to(Gc.BF16)


RANDOM = Gc.runs(("random", "clamp"))


@pytest.mark.parametrize("r", RANDOM, ids=Gc.run_id)
def test_the_fp32_emulation_stays_inside_the_bounds(r):
    c, m = r
    t, geo, ref = Gc.prepared(c["i"], m)
    res = Gc.evaluate(c, ref, Gc.emulate(c, t, geo, ref))
    assert set(res) == {k for k in Gc.OUTPUTS[c["kind"]] if c["kind"] != "fwd" or k == "out" or c["save"]}
    for k, (ratio, z, bad, first) in res.items():
        assert ratio < 1.0 and abs(z) < 3.0, (Gc.run_id(r), k, ratio, z, bad, first)
        assert torch.isfinite(ref[k]).all() and torch.isfinite(ref["B_" + k]).all()
        row = EMU.setdefault(f"{c['kind']}.{k}", {"ratio": 0.0, "z": 0.0})
        row["ratio"], row["z"] = max(row["ratio"], ratio), max(row["z"], abs(z))
    if m == "clamp" and c["kind"] == "fwd" and c["layout"] == "compact":
        assert float(ref["out"].max()) == 65504.0
    if m == "clamp" and not c["coords"]:
        assert int((t["et"] < 0).sum()) > 0 and int((t["et"] >= c["E"]).sum()) > 0


def _caught(c, m, mut):
    t, geo, ref = Gc.prepared(c["i"], m)
    res = Gc.evaluate(c, ref, Gc.emulate(c, t, geo, ref, mut=mut))
    return {k: v for k, v in res.items() if not (v[0] <= 1.0 and abs(v[1]) <= Gc.Z_MAX)}


def _pick(kind, N, m, **kw):
    return next(c for c in Gc.CASES if c["kind"] == kind and c["N"] == N and m in c["modes"] and all(c[k] == v for k, v in kw.items()))


@pytest.mark.parametrize("kind,N", [("fwd", 5), ("fwd", 130), ("full", 37), ("full", 130), ("bwd", 17), ("bwd", 130)])
def test_a_dropped_tile_leaves_the_bounds(kind, N):
    hit = _caught(_pick(kind, N, "random", lens=None, E=961), "random", "drop_tile")
    assert hit and ("out" in hit or {"dW2", "db2"} <= set(hit) or "du" in hit), hit


@pytest.mark.parametrize("kind", ["fwd", "full", "bwd"])
def test_two_swapped_columns_of_w1_leave_the_bounds(kind):
    for m in ("onehot", "random"):
        hit = _caught(_pick(kind, 37, m, lens=None), m, "swap_w1")
        assert hit and (m == "onehot" or set(hit) & {"out", "dW1", "dmeans"}), (m, hit)


@pytest.mark.parametrize("kind", ["full", "bwd", "fbwd"])
def test_a_wrong_dstds_sign_leaves_the_bounds(kind):
    for m in ("onehot", "random"):
        assert "dstds" in _caught(_pick(kind, 17, m, lens=None, E=961), m, "dstds_sign"), m


@pytest.mark.parametrize("kind", ["full", "bwd", "fbwd"])
def test_a_halved_dmul_entry_leaves_the_bounds(kind):
    assert set(_caught(_pick(kind, 37, "random", lens=None), "random", "half_dmul")) == {"dmul"}


@pytest.mark.parametrize("kind", ["fwd", "ffwd"])
def test_pi_for_3_14159_leaves_the_bounds(kind):
    """(through the onehot mode: two stds sit where bf16(cf) tells the two constants apart)"""
    c = _pick(kind, 5 if kind == "fwd" else 17, "onehot", **({"save": True} if kind == "fwd" else {}))
    assert "feat" in _caught(c, "onehot", "pi")


@pytest.mark.parametrize("kind", ["fwd", "full", "bwd", "fbwd", "ffwd"])
def test_sigma_without_its_1e_5_leaves_the_bounds(kind):
    """(through the onehot mode, whose two zero stds then divide by zero; with |std| >= 0.05 the 1e-5 is 2e-4 of sigma at most, which
    the saved feat and the unfused backward see and the gradients of the fused backwards do not)"""
    c = _pick(kind, 17 if kind != "fwd" else 5, "onehot")
    assert _caught(c, "onehot", "no_eps")
    if kind in ("fwd", "ffwd", "fbwd"):
        assert _caught(_pick(kind, 37, "random", lens=None), "random", "no_eps")
