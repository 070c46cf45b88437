"""The 27 kernel instances of csrc/gbf.hip (9 fused forwards, 3 per-pair backwards, 12 complete backwards, the unfused forward and its two
backwards; gbf_slab_reduce_kernel behind every complete backward with a workspace) against the float64 reference of tests/gbf_cases.py,
through the C entry points mmdti_gbf_bias_fwd / _fwd_coords / _bwd / _bwd_full / _bwd_full_coords and mmdti_gbf_features_fwd / _bwd.
tests/test_gbf_cases_cpu.py proves on the CPU that the table reaches every instance and branch and that the bounds hold for an fp32
emulation of the kernels' rounding points, and not for six wrong ones.

dist, the edge types, the atom records, G and the saved u are cut from NaN-filled (integers: poisoned) arenas -- G holds NaN in every slot
that no computed pair owns: an invalid lane of the per-pair backward loads nothing (gbf.hip:727), one of the complete backward loads slot
0 of the plane, which is pair (0, 0) (gbf.hip:976) -- ; the out planes, the saved tensors, do / du and the eight gradient buffers (filled
with gbf_cases.FILL: the kernels accumulate) from sentinel-filled ones.  After every launch: no output holds a NaN, every slot the contract
says is written holds no sentinel, the pad columns [N, ld) of row-major planes are exactly 0 and the pad keys of tiled planes exactly -inf,
the blocks behind a ragged molecule's tile prefix and the rows of its pairs there still hold the sentinel, and no sentinel outside a view
has moved.
  test_onehot             feat and u (ugrad off) EQUAL the fp32 expectation, do EQUALS bf16(G); everything else within the bounds
  test_random_and_clamp   elementwise within the bounds, |gain| <= 6; the saturated outputs of compact planes are exactly 65504
  test_edge_sizes         the planes instances again with 4- and 2-byte edge types
Nothing here asserts run-to-run bits (test_deterministic_gpu.py owns that); the deterministic instances run in the mode, which is
switched off again in a finally.

With MMDTI_GBF_PROFILE=<path> the largest |got - ref| / bound and |z| of every instance and output are merged into that JSON file under
"device" (profiles/gbf_instances.json is such a run: on MI355X the largest ratio of an fp32 output is 0.35 -- out of the compact planes
forward --, of the gradients 0.20 (dW1), 0.16 (db2), 0.14 (dmul), 0.12 (dbias), below 0.07 for the rest; the 16-bit outputs (feat, u, h,
du), where the reference rounds too and one flipped rounding is one ulp against a bound of one ulp + L, reach 0.9999; the largest |z| is 0.09;
the CPU emulation's own ratios sit beside them under "emulation".  The 420 tests take 11 to 18 s on the MI355X host, the slowest 1 s.)"""
import json
import os

import pytest
import torch

from mmdti_hip import _abi, ops

import gbf_cases as Gc
import pair_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
F64, BF16, F32, F16 = Gc.F64, Gc.BF16, Gc.F32, Gc.F16
K, F, H = Gc.K, Gc.F, Gc.H
POISON = 29999


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MMDTI_GBF_PROFILE")
    if path:
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc["device"] = REPORT
        with open(path, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(c, res):
    row = REPORT.setdefault(Gc.instance(c), {})
    for k, v in res.items():
        old = row.get(k, {"ratio": 0.0, "z": 0.0})
        row[k] = {"ratio": max(old["ratio"], v[0]), "z": max(old["z"], abs(v[1]))}


def _int_arena(values, dtype, guard=64):
    """integers between two poisoned guards (a kernel that reads one of them computes with edge type / token 29999)"""
    buf = torch.full((values.numel() + 2 * guard,), POISON, dtype=dtype, device=DEV)
    buf[guard:guard + values.numel()] = values.reshape(-1).to(dtype).to(DEV)
    assert (buf.data_ptr() + guard * buf.element_size()) % 16 == 0
    return buf, buf.data_ptr() + guard * buf.element_size()


class Run:
    """the operands of a run on the device, and the launches"""

    def __init__(self, c, t, geo, ref, esz=8):
        self.c, self.t, self.geo, self.ref, self.pc = c, t, geo, ref, Gc.pc_of(c)
        B, N = c["B"], c["N"]
        self.P = B * N * N
        self.keep = []
        dev = lambda x: x.to(DEV).contiguous()
        self.par = {k: dev(t[k]) for k in ("mul", "bias", "means", "stds", "w1", "b1", "w2", "b2")}
        self.esz = esz
        self.rec = self.tp = self.rb = self.dist = self.et = 0
        if c["coords"]:
            rec = ops.pair_records(dev(t["coord"]), dev(t["tok"]))
            buf = torch.full((B * N * 4 + 128,), 0x7FC00000, dtype=torch.int32, device=DEV)
            buf[64:64 + B * N * 4] = rec.reshape(-1)
            self.keep.append(buf)
            self.rec = buf.data_ptr() + 256
            assert self.rec % 16 == 0
        else:
            a, flat, self.dist = Gc.flat_arena(self.P, F32, DEV, out=False)
            flat.copy_(t["d"].reshape(-1).to(DEV))
            ebuf, self.et = _int_arena(t["et"], {8: torch.int64, 4: torch.int32, 2: torch.int16}[esz])
            self.keep += [a, ebuf]
        if c["lens"] is not None:
            kt = torch.tensor([(n + 15) // 16 for n in c["lens"]])
            if c["packed"]:
                pf, pb, rf, rbk = ops.gbf_tile_prefixes(kt, N, DEV, torch.tensor(geo["qlive"]))
                assert rf.tolist() == Gc.row_blocks(c, geo) == rbk.tolist()
                self.rb = (rf if c["kind"] == "fwd" else rbk).data_ptr()
            else:
                pf, pb = ops.gbf_tile_prefixes(kt, N, DEV)
            assert pf.tolist() == Gc.prefix(c, geo) == pb.tolist()
            self.tp = (pf if c["kind"] == "fwd" else pb).data_ptr()
            self.keep += [pf, pb]
        assert c["ld"] == ops.pair_ld(N) and (c["layout"] == "row" or geo["plane"] == ops.pair_plane(N))
        self.n = B * H * geo["plane"]
        self.sel = ref["sel"].view(B, N, N)

    def shape(self):
        c = self.c
        return (c["B"], c["N"], c["ld"], K, F, H, c["E"])

    def params(self, *names):
        return [self.par[k].data_ptr() for k in names]

    # ---- operands
    def g_plane(self):
        c, geo = self.c, self.geo
        a, flat, ptr = Gc.flat_arena(self.n, BF16 if c["layout"] == "compact" else F32, DEV, out=False)
        vals = torch.zeros(c["B"], H, c["N"], geo["cols"])
        vals[..., :c["N"]] = self.t["G"].permute(0, 3, 1, 2)
        where = torch.zeros(c["B"], c["N"], geo["cols"], dtype=torch.bool)
        where[..., :c["N"]] = self.sel
        Gc.scatter_plane(self.pc, geo, flat, vals, where)
        self.keep.append(a)
        return ptr

    def rows_in(self, x):
        a, view = Gc.row_arena(x.shape[0], x.shape[1], x.dtype, DEV, out=False)
        view.copy_(x.to(DEV))
        self.keep.append(a)
        return a.ptr()

    # ---- outputs
    def rows_out(self, cols):
        return Gc.row_arena(self.P, cols, BF16, DEV, out=True)

    def grads(self, names):
        out = {}
        for k in names:
            a, flat, ptr = Gc.flat_arena(self.ref[k].numel(), F32, DEV, out=True)
            flat.fill_(Gc.FILL)
            out[k] = (a, flat, ptr)
        return out

    def read_grads(self, gr, what):
        got = {}
        for k, (a, flat, _) in gr.items():
            assert a.outside_untouched() == 0, (what, k, "a store outside the gradient buffer")
            x = flat.cpu()
            assert not bool(torch.isnan(x).any()), (what, k, "NaN in a gradient")
            got[k] = (x.to(F64) - Gc.FILL).view(self.ref[k].shape)
        return got

    def read_rows(self, a, view, what, exact_sel=True):
        """rows of the computed pairs; the rows of every other pair still hold the sentinel"""
        assert a.outside_untouched() == 0, (what, "a store outside the rows")
        x = view.cpu()
        s = self.sel.reshape(-1)
        assert bool((P.bits(x[~s]) == Gc.SENT16).all()), (what, "a row of a pair the launch does not compute was written")
        assert not bool(torch.isnan(x[s].float()).any()), (what, "NaN or sentinel in a row the launch computes")
        return x[s]

    def read_plane(self, a, flat, what):
        c, geo = self.c, self.geo
        B, N = c["B"], c["N"]
        assert a.outside_untouched() == 0, (what, "a store outside the planes")
        where = Gc.written(c, geo)
        host = flat.cpu().view(B, H, geo["plane"])
        unw = P.unwritten_mask(self.pc, geo, where).view(B, 1, geo["plane"]).expand_as(host)
        assert bool((P.bits(host)[unw] == P.sentinel_of(flat.dtype)).all()), (what, "a store into a slot the launch does not write (alignment tail, blocks behind the prefix)")
        pos = host[:, :, geo["idx"].reshape(-1)].view(B, H, N, geo["cols"])
        w = where.view(B, 1, N, geo["cols"]).expand_as(pos)
        assert not bool(torch.isnan(pos[w].float()).any()), (what, "NaN or sentinel in a slot the launch writes")
        pads = w.clone()
        pads[..., :N] = False
        if bool(pads.any()):
            pv = pos[pads].float()
            assert bool((pv == 0).all() if c["layout"] == "row" else torch.isneginf(pv).all()), (what, "pad columns: exactly 0 (row-major) / -inf (tiled)")
        return pos[..., :N].permute(0, 2, 3, 1).reshape(-1, H)[self.sel.reshape(-1)]


def _launch(c, t, geo, ref, esz=8):
    """-> got {name: CPU tensor shaped as the reference's}"""
    lib, r = _abi.lib(), None
    r = Run(c, t, geo, ref, esz)
    what, kind = Gc.run_id((c, t["mode"])), c["kind"]
    st = ops._stream
    Gc.assert_declared_plan(lib, c, esz)          # (the mode and the workspace the launch below finds are the case's: _run, and the assert on ws)
    if kind in ("ffwd", "fbwd"):
        assert esz == 8
        pm = r.params("mul", "bias", "means", "stds")
        if kind == "ffwd":
            a, view = r.rows_out(K)
            lib.mmdti_gbf_features_fwd(st(), r.dist, r.et, *pm, r.P, K, c["E"], a.ptr())
            torch.cuda.synchronize()
            return dict(feat=r.read_rows(a, view, what))
        if c["det"]:
            assert ops.det_workspace_bytes("gbf_features_bwd", r.P, 2 * c["E"] + 2 * K) <= ops.det_workspace_mb() << 20
        gr = r.grads(Gc.GRADS[4:])
        lib.mmdti_gbf_features_bwd(st(), r.dist, r.et, *pm, r.P, K, c["E"], r.rows_in(t["dfeat"]), *[gr[k][2] for k in Gc.GRADS[4:]])
        torch.cuda.synchronize()
        return r.read_grads(gr, what)
    fl = Gc.flags(c)
    if kind == "fwd":
        oa, oflat, optr = Gc.flat_arena(r.n, F16 if c["layout"] == "compact" else F32, DEV, out=True)
        sv = [r.rows_out(K), r.rows_out(F), r.rows_out(F)] if c["save"] else []
        if c["coords"]:
            lib.mmdti_gbf_bias_fwd_coords(st(), r.rec, c["V"], Gc.PAD, *r.params("mul", "bias", "means", "stds", "w1", "b1", "w2", "b2"), *r.shape(), optr, fl, r.tp, r.rb)
        else:
            lib.mmdti_gbf_bias_fwd(st(), r.dist, r.et, esz, *r.params("mul", "bias", "means", "stds", "w1", "b1", "w2", "b2"), *r.shape(), optr,
                                   *([a.ptr() for a, _ in sv] if sv else [0, 0, 0]), fl, r.tp, r.rb)
        torch.cuda.synchronize()
        got = dict(out=r.read_plane(oa, oflat, what + " out"))
        for k, (a, view) in zip(("feat", "u", "h"), sv):
            got[k] = r.read_rows(a, view, what + " " + k)
        return got
    g = r.g_plane()
    if kind == "bwd":
        (da, dview), (ua, uview) = Gc.row_arena(r.P, H, BF16, DEV, out=True), r.rows_out(F)
        gr = r.grads(Gc.GRADS[4:])
        lib.mmdti_gbf_bias_bwd(st(), g, r.dist, r.et, esz, *r.params("mul", "bias", "means", "stds", "w1", "w2"), r.rows_in(ref["u_in"]), *r.shape(), fl,
                               da.ptr(), ua.ptr(), *[gr[k][2] for k in Gc.GRADS[4:]])
        torch.cuda.synchronize()
        got = r.read_grads(gr, what)
        got["du"] = r.read_rows(ua, uview, what + " du")
        got["do"] = r.read_rows(da, dview, what + " do")
        return got
    ws = torch.empty(lib._dll.mmdti_gbf_bias_bwd_full_workspace(c["E"]), device=DEV, dtype=torch.uint8) if ops.GBF_SLABS else None
    assert (ws is not None) == c["ws"]
    wsp, wsn = (ws.data_ptr(), ws.numel()) if ws is not None else (0, 0)
    gr = r.grads(Gc.GRADS)
    gp = [gr[k][2] for k in Gc.GRADS]
    if c["coords"]:
        lib.mmdti_gbf_bias_bwd_full_coords(st(), g, r.rec, c["V"], Gc.PAD, *r.params("mul", "bias", "means", "stds", "w1", "b1", "w2"), *r.shape(), fl, *gp, r.tp, r.rb, wsp, wsn)
    else:
        lib.mmdti_gbf_bias_bwd_full(st(), g, r.dist, r.et, esz, *r.params("mul", "bias", "means", "stds", "w1", "b1", "w2"), *r.shape(), fl, *gp, r.tp, r.rb, wsp, wsn)
    torch.cuda.synchronize()
    return r.read_grads(gr, what)


def _run(c, m, monkeypatch, esz=8):
    t, geo, ref = Gc.prepared(c["i"], m)
    if c["kind"] == "full" and not c["ws"]:
        monkeypatch.setattr(ops, "GBF_SLABS", False)           # the complete backward without a workspace: fp32 atomics
    if c["det"]:
        ops.set_deterministic(True)
    try:
        got = _launch(c, t, geo, ref, esz)
    finally:
        if c["det"]:
            ops.set_deterministic(False)
    res = Gc.evaluate(c, ref, got)
    _record(c, res)
    want = {k for k in Gc.OUTPUTS[c["kind"]] if c["kind"] != "fwd" or k == "out" or c["save"]}
    assert set(res) == want
    for k, (ratio, z, bad, first) in res.items():
        print(f"{Gc.run_id((c, m))} {Gc.instance(c)} {k}: ratio {ratio:.4g} z {z:.3g}")
    for k, (ratio, z, bad, first) in res.items():
        assert ratio <= 1.0 and abs(z) <= Gc.Z_MAX, f"{Gc.instance(c)} {k}: {bad} elements outside the bound, the first at flat index {first}; worst ratio {ratio:.4g}, gain {z:.3g}"
    if "do" in got:
        assert torch.equal(got["do"], t["G"].reshape(-1, H)[ref["sel"]].to(BF16)), f"{Gc.instance(c)} do: not bf16(G)"
    return t, ref, got


@pytest.mark.parametrize("r", Gc.runs(("onehot",)), ids=Gc.run_id)
def test_onehot(r, monkeypatch):
    c, m = r
    t, ref, got = _run(c, m, monkeypatch)
    if "feat" in got:
        feat, u = Gc.onehot_expectation(c, t)
        sel = ref["sel"]
        bad = (P.bits(got["feat"]) != P.bits(feat.reshape(-1, K)[sel])).flatten().nonzero().flatten()
        assert bad.numel() == 0, f"{Gc.instance(c)} feat: {bad.numel()} elements differ from bf16(cf), the first at flat index {int(bad[0])}"
        if "u" in got and not c["ugrad"]:
            bad = (got["u"].float() != u.reshape(-1, F)[sel].float()).flatten().nonzero().flatten()
            assert bad.numel() == 0, f"{Gc.instance(c)} u: {bad.numel()} elements differ from bf16(W1[f, k] bf16(cf) + b1[f]), the first at flat index {int(bad[0])}"


@pytest.mark.parametrize("r", Gc.runs(("random", "clamp")), ids=Gc.run_id)
def test_random_and_clamp(r, monkeypatch):
    c, m = r
    t, ref, got = _run(c, m, monkeypatch)
    if m == "clamp" and c["kind"] == "fwd" and c["layout"] == "compact":
        sat = got["out"][:, [0, 21, 42, 63]].float()
        assert bool((sat == 65504.0).all()), f"{Gc.instance(c)} out: a saturated output is not exactly 65504"


@pytest.mark.parametrize("r", Gc.edge_runs(), ids=Gc.run_id)
def test_edge_sizes(r, monkeypatch):
    c, m, esz = r
    _run(c, m, monkeypatch, esz)
