"""The 85 forward and 98 backward kernel instances of the pair-bias attention (csrc/pair_attn.hip, pair_attn_bwd.hip,
pair_attn_bwd_mfma.h, pair_attn_bwd_g16.hip) and the 86 bodies of the ragged sweeps in each direction, against the float64 reference of
tests/pair_cases.py, through the C entry points mmdti_pair_attn_fwd / mmdti_pair_attn_bwd.  tests/test_pair_cases_cpu.py proves on
the CPU that the table reaches every instance and body and that the bounds hold for an fp32 emulation of the kernels' rounding
points -- and not for one that drops the low parts of the hi + lo splits or has a softmax denominator wrong by 1 / 256.

q | k | v, dO, the bias (S-in) planes and key_pad are cut from NaN-filled arenas (0xff for key_pad); S-out, O, dqkv and G (in place: G_in
is written into the slots the layout defines, everything else keeps the sentinel) from sentinel-filled ones.  Where a padding mask is
handed in, the bias of the padded keys is NaN as well.  After every launch no slot the layout defines holds a NaN or the sentinel,
and nothing else has changed.  Every slot of a plane is one of
  a real pair                    checked against the reference; a padded key is exactly -inf in S and keeps G_in (0) in G
  a pad key of a real query      (keys N .. N4 - 1 of tiled planes and of the MFMA kernels' row-major rows) exactly -inf in S, exactly 0 in G
  a skipped ragged tile          -inf with rag_store, otherwise untouched; in G untouched
  a slot no kernel writes        the alignment tail of a plane, the row padding past N4 (past N: per-element kernels), the rows past a
                                 packed molecule's representative pad row: still the sentinel
A dense case runs one forward and two backwards (G_in given; g_in_zero on a G full of 7).  A ragged case runs a first layer on the
bias with rag_store = 0, a second layer on the first layer's S-out as it stands -- its skipped tiles still hold the (NaN) sentinel --
with rag_store = 1 and no key_pad, and the backwards on the first layer's S.
  selector, uq, uk            S, O, G, dq, dk, dv EQUAL what the mode requires, bit for bit
  random, saturate, dropout   elementwise within the derived bounds, |gain| <= 6; dropout under the keep mask recovered from the forward
                              kernel through indicator V columns -- which is the test that both directions draw one mask

With MMDTI_PAIR_PROFILE=<path> the largest |got - ref| / bound and |z| of every instance and output are written there as JSON
(profiles/pair_instances.json is such a run: on MI355X the largest ratio is 0.997 -- S of pair_attn_fwd_mfma_kernel<6, true, true, true,
_Float16>; G 0.996, O 0.993, dq / dk / dv 0.99 --, the largest |z| 1.38; the 1573 tests take 63.7 s, the slowest 0.6 s, next to the
4.5 s of the 216 fused-attention tests: 40 ms per test, two to five launches and a float64 reference of up to 27 planes each)."""
import json
import os

import pytest
import torch

from mmdti_hip import _abi, ops
from mmdti_hip._abi import MMDTIError

import pair_cases as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPORT = {}
F64 = P.F64


@pytest.fixture(scope="module", autouse=True)
def _profile():
    yield
    path = os.environ.get("MMDTI_PAIR_PROFILE")
    if path:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
            f.write("\n")


def _record(c, res, fwd_keys=("S", "O"), bwd_keys=("G", "dq", "dk", "dv")):
    fwd, bwd, _ = P.instances(c)
    for inst, keys in ((fwd, fwd_keys), (bwd, bwd_keys)):
        row = REPORT.setdefault(inst, {})
        for k in keys:
            if k in res:
                old = row.get(k, {"ratio": 0.0, "z": 0.0})
                row[k] = {"ratio": max(old["ratio"], res[k][0]), "z": max(old["z"], abs(res[k][1]))}


# ------------------------------------------------------------------------------------------------ placement and launches
class Placed:
    """the operands of a run on the device"""

    def __init__(self, c, t, geo):
        B, N, H = c["B"], c["N"], c["H"]
        D, rows = H * P.HD, geo["rows"]
        self.c, self.t, self.geo = c, t, geo
        self.shift = 1 if c["shift"] else 0
        tr = lambda x: P.token_rows(c, geo, x)
        self.qkv_a, qkv = P.row_arena(rows, 3 * D, P.op_dtype(c), DEV, out=False)
        qkv.copy_(torch.cat([tr(t["q"]), tr(t["k"]), tr(t["v"])], 1).to(DEV))
        self.do_a, do = P.row_arena(rows, D, P.BF16, DEV, out=False)
        do.copy_(tr(t["do"]).to(DEV))
        self.qkv, self.do = self.qkv_a.ptr(), self.do_a.ptr()
        self.kp = 0
        if t["pad"] is not None:
            self.kp_buf = torch.full((rows + 128,), 0xFF, dtype=torch.uint8, device=DEV)
            self.kp_buf[64:64 + rows] = t["pad"].reshape(-1)[geo["gather"]].to(torch.uint8).to(DEV)
            self.kp = self.kp_buf.data_ptr() + 64
        self.kt = self.ro = 0
        if c["lens"] is not None:
            self.kt_t = torch.tensor([P.tiles(n) for n in c["lens"]], dtype=torch.int32, device=DEV)
            self.kt = self.kt_t.data_ptr()
            if c["packed"]:
                self.ro_t = torch.tensor(geo["off"], dtype=torch.int32, device=DEV)
                self.ro = self.ro_t.data_ptr()
        self.n = B * H * geo["plane"]
        # the bias planes: real pairs, -inf at the pad keys of tiled planes; NaN wherever the kernels must not look (padded keys under a
        # mask, tiles that are not covered, queries that do not exist, row padding)
        self.sin_a, self.sin, self.sin_p = P.flat_arena(self.n, P.s_dtype(c), DEV, out=False, shift=self.shift)
        vals = torch.full((B, H, N, geo["cols"]), float("-inf") if c["layout"] & 1 else float("nan"))
        vals[..., :N] = t["bias"] if t["pad"] is None else t["bias"].masked_fill(t["pad"].view(B, 1, 1, N), float("nan"))
        P.scatter_plane(c, geo, self.sin, vals, P.written(c, geo, rag_store=False))

    def s_out(self):
        return P.flat_arena(self.n, P.s_dtype(self.c), DEV, out=True, shift=self.shift)

    def o_out(self):
        return P.row_arena(self.geo["rows"], self.c["H"] * P.HD, P.o_dtype(self.c), DEV, out=True)


def _fwd(pl, s_in_ptr, s_out_ptr, o_ptr, kp, p, rag_store):
    c = pl.c
    P.assert_declared_plan(_abi.lib(), c, False, dict(qkv=pl.qkv, s=s_in_ptr, g=s_out_ptr, o=o_ptr, dqkv=0))
    _abi.lib().mmdti_pair_attn_fwd(ops._stream(), pl.qkv, s_in_ptr, s_out_ptr, o_ptr, kp, c["B"], c["N"], c["H"], c["ld"], pl.t["scale"], p, P.SEED, P.SITE,
                                   c["layout"] & 3, pl.kt, int(rag_store), pl.ro, int(c["f16"]))


def _bwd(pl, s_ptr, g_ptr, dqkv_ptr, gz, p):
    c = pl.c
    P.assert_declared_plan(_abi.lib(), c, True, dict(qkv=pl.qkv, s=s_ptr, g=g_ptr, o=pl.do, dqkv=dqkv_ptr))
    _abi.lib().mmdti_pair_attn_bwd(ops._stream(), pl.qkv, s_ptr, pl.do, g_ptr, dqkv_ptr, c["B"], c["N"], c["H"], c["ld"], pl.t["scale"], int(gz), p, P.SEED, P.SITE,
                                   c["layout"], pl.kt, pl.ro, int(c["f16"]))


def _plane_out(pl, arena, flat, where, what):
    """the accounting of an output plane: everything outside `where` still holds the sentinel, nothing inside is NaN -> [B, H, N, cols]"""
    c, geo = pl.c, pl.geo
    assert arena.outside_untouched() == 0, (what, "a store outside the planes")
    if pl.shift:
        assert int(P.bits(arena.view[0, 0, 0][:pl.shift]).cpu()[0]) == P.sentinel_of(flat.dtype), (what, "a store in front of the planes")
    host = flat.cpu().view(c["B"], c["H"], geo["plane"])
    unw = P.unwritten_mask(c, geo, where).view(c["B"], 1, geo["plane"]).expand_as(host)
    assert bool((P.bits(host)[unw] == P.sentinel_of(flat.dtype)).all()), (what, "a store into a slot no kernel writes (alignment tail, row padding, skipped tile, absent row)")
    pos = host[:, :, geo["idx"].reshape(-1)].view(c["B"], c["H"], c["N"], geo["cols"])
    w = where.view(c["B"], 1, c["N"], geo["cols"]).expand_as(pos)
    assert not bool(torch.isnan(pos[w].float()).any()), (what, "NaN or sentinel in a slot the layout defines")
    return pos, w


def _rows_out(arena, view, what):
    assert arena.outside_untouched() == 0, (what, "a store outside the rows")
    x = view.cpu()
    assert not bool(torch.isnan(x.float()).any()), (what, "NaN: a read outside an operand, or an element never stored")
    return x


def _forward(pl, s_in_ptr, kp, p, rag_store, what):
    """one forward launch -> S by position [B, H, N, cols] (and its defined slots), O rows, the S arena's pointer"""
    c, geo = pl.c, pl.geo
    sa, sflat, sp = pl.s_out()
    oa, oview = pl.o_out()
    _fwd(pl, s_in_ptr, sp, oa.ptr(), kp, p, rag_store)
    torch.cuda.synchronize()
    where = P.written(c, geo, rag_store=rag_store)
    S, w = _plane_out(pl, sa, sflat, where, what + " S")
    pads = w.clone()
    pads[..., :c["N"]] = False
    assert bool(torch.isneginf(S[pads].float()).all()), (what, "pad keys of a real query are exactly -inf")
    if rag_store:                                          # the tiles that are not covered: exactly -inf
        skipped = where & ~P.written(c, geo, rag_store=False)
        assert bool(torch.isneginf(S[skipped.view(c["B"], 1, c["N"], -1).expand_as(S)].float()).all()), (what, "rag_store writes -inf into the skipped tiles")
    return S[..., :c["N"]].to(F64), _rows_out(oa, oview, what + " O"), sp, (sa, sflat)


def _backward(pl, s_ptr, gz, p, what):
    c, t, geo = pl.c, pl.t, pl.geo
    B, N, H = c["B"], c["N"], c["H"]
    ga, gflat, gp = P.flat_arena(pl.n, P.g_dtype(c), DEV, out=True, shift=pl.shift)
    where = P.written(c, geo, rag_store=False)
    vals = torch.zeros(B, H, N, geo["cols"])
    vals[..., :N] = t["gin"]
    if gz:
        vals.fill_(7.0)
    P.scatter_plane(c, geo, gflat, vals, where)
    da, dview = P.row_arena(geo["rows"], 3 * H * P.HD, P.BF16, DEV, out=True)
    _bwd(pl, s_ptr, gp, da.ptr(), gz, p)
    torch.cuda.synchronize()
    G, w = _plane_out(pl, ga, gflat, where, what + " G")
    pads = w.clone()
    pads[..., :N] = False
    assert float(G[pads].float().abs().max() if bool(pads.any()) else 0.0) == 0.0, (what, "pad keys of a real query are exactly 0 in G")
    d = _rows_out(da, dview, what + " dqkv")
    D = H * P.HD
    return dict(G=G[..., :N].to(F64), dq=d[:, :D], dk=d[:, D:2 * D], dv=d[:, 2 * D:])


def _recover_keep(c, geo, p):
    """the forward's keep mask through indicator V columns (q = k = 0, zero bias: every covered key has a positive probability), eight keys
    per pass, with the case's own B, N, H, ld, layout, alignment, key_tiles and row_off -> [B, H, N, N] bool (True where a key is not
    covered or a query does not exist: nothing reads the mask there)"""
    B, N, H = c["B"], c["N"], c["H"]
    D, rows, sh = H * P.HD, geo["rows"], 1 if c["shift"] else 0
    od, sd = P.op_dtype(c), P.s_dtype(c)
    qkv = torch.zeros(rows, 3, H, P.HD, dtype=od, device=DEV)
    n = B * H * geo["plane"]
    bias = torch.full((n + 4,), float("-inf") if c["layout"] & 1 else 0.0, dtype=sd, device=DEV)[sh:sh + n]
    bias.view(B, H, geo["plane"])[:, :, geo["idx"][:, :N].reshape(-1).to(DEV)] = 0.0
    s_out = torch.empty(n + 4, dtype=sd, device=DEV)[sh:sh + n]
    o = torch.empty(rows, H, P.HD, dtype=P.o_dtype(c), device=DEV)
    kt = ro = 0
    if c["lens"] is not None:
        kt_t = torch.tensor([P.tiles(x) for x in c["lens"]], dtype=torch.int32, device=DEV)
        kt = kt_t.data_ptr()
        if c["packed"]:
            ro_t = torch.tensor(geo["off"], dtype=torch.int32, device=DEV)
            ro = ro_t.data_ptr()
    pos = (geo["gather"] % N).to(DEV)
    mol = (geo["gather"] // N)
    keep = torch.ones(B, H, N, N, dtype=torch.bool)
    got = torch.zeros(rows, H, N, dtype=torch.bool, device=DEV)
    for c0 in range(0, N, P.HD):
        r = ((pos >= c0) & (pos < c0 + P.HD)).nonzero().flatten()
        qkv[:, 2] = 0
        qkv[r, 2, :, pos[r] - c0] = 1.0
        _abi.lib().mmdti_pair_attn_fwd(ops._stream(), qkv.data_ptr(), bias.data_ptr(), s_out.data_ptr(), o.data_ptr(), 0, B, N, H, c["ld"], 1.0, p, P.SEED, P.SITE,
                                       c["layout"] & 3, kt, 1, ro, int(c["f16"]))
        w = min(P.HD, N - c0)
        got[:, :, c0:c0 + w] = o[:, :, :w] != 0
    got = got.cpu()
    ql, kl = P._live(c, geo)
    for b in range(B):
        rb = (mol == b).nonzero().flatten()
        keep[b, :, :len(rb)] = got[rb].permute(1, 0, 2)
        if c["packed"]:                                   # keys past the representative pad row are no rows: never kept, never read
            keep[b, :, :, len(rb):] = True
    return keep | ~(ql & kl)


class _det:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = ops.is_deterministic()
        if self.on != self.was:
            ops.set_deterministic(self.on)

    def __exit__(self, *exc):
        if ops.is_deterministic() != self.was:
            ops.set_deterministic(self.was)


def _run(r):
    """every launch of a run -> (placement, keep, layers [(S, O, prev)], backwards {gz: outputs}, the stored logits the backward read)"""
    c, mode, p, mask = r
    t, geo = P.make_inputs(c, mode, mask), P.geometry(c)
    rid = P.run_id(r)
    try:
        return _launches(r, c, t, geo, rid, p)
    except RuntimeError as e:              # a device fault ends the session: nothing more is started on this device
        if isinstance(e, MMDTIError) or not any(w in str(e) for w in ("HIP error", "hipError", "illegal memory access", "CUDA error")):
            raise
        pytest.exit(f"{rid}: {e}", returncode=3)


def _launches(r, c, t, geo, rid, p):
    with _det(c["det"]):
        keep = _recover_keep(c, geo, p) if p else None
        pl = Placed(c, t, geo)
        layers = []
        if c["lens"] is None:
            S, O, sp, hold = _forward(pl, pl.sin_p, pl.kp, p, 0, rid)
            layers.append((S, O, None))
        else:
            S, O, sp, hold = _forward(pl, pl.sin_p, pl.kp, p, 0, rid + " layer 1")
            layers.append((S, O, None))
            S2, O2, _, _ = _forward(pl, sp, 0, p, 1, rid + " layer 2")
            layers.append((S2, O2, S))
        back = {gz: _backward(pl, sp, gz, p, f"{rid} g_in_zero={int(gz)}") for gz in (False, True)}
    return pl, keep, layers, back


def _same(rid, name, got, want):
    bad = got.to(F64) != want.to(F64)
    assert not bool(bad.any()), (rid, name, int(bad.sum()), "first at", bad.nonzero()[0].tolist(), float(got[bad][0]), float(want[bad][0]))


@pytest.mark.parametrize("r", P.runs(("selector", "uq", "uk")), ids=P.run_id)
def test_exact_modes(r):
    c, mode, _, _ = r
    rid = P.run_id(r)
    pl, _, layers, back = _run(r)
    t, geo = pl.t, pl.geo
    ql, kl = P._live(c, geo)
    live = (ql & kl).expand(c["B"], c["H"], c["N"], c["N"])
    for n, (S, O, prev) in enumerate(layers):
        S_ref, _ = P.logits(c, t, geo, prev=prev)
        _same(rid, f"S of layer {n + 1}", S[live], S_ref[live])                      # (-inf at the padded keys included)
    for gz in (False, True):
        if mode == "selector":
            want = P.selector_expectation(c, t, geo, gz)
        else:
            ref = P.reference(c, t, geo, layers[0][0], bounds=False, gz=gz)
            want = {k: P.round16(ref[k], P.o_dtype(c) if k == "O" else P.BF16) for k in ("O", "dq", "dk", "dv")}
            want["G"] = ref["G"]
        for S, O, prev in layers:                                                     # (the second layer's P is the first layer's: one-hot / uniform)
            _same(rid, "O", O, P.token_rows(c, geo, want["O"]))
        _same(rid, "G", back[gz]["G"][live], want["G"].to(P.g_dtype(c))[live])
        for k in ("dq", "dk", "dv"):
            _same(rid, f"{k} g_in_zero={int(gz)}", back[gz][k], P.token_rows(c, geo, want[k]))


def _held(rid, c, res):
    for k, (ratio, z) in res.items():
        assert ratio <= 1.0 and abs(z) <= P.Z_MAX, (rid, k, ratio, z)


@pytest.mark.parametrize("r", P.runs(("random", "saturate", "dropout")), ids=P.run_id)
def test_random_saturate_and_dropout(r):
    c, mode, p, _ = r
    rid = P.run_id(r)
    pl, keep, layers, back = _run(r)
    t, geo = pl.t, pl.geo
    if keep is not None:
        ql, kl = P._live(c, geo)
        live = (ql & kl).expand_as(keep)
        if c["packed"]:                                    # (keys past the representative pad row are no rows: nothing was recovered there)
            live = live & (torch.arange(c["N"]).view(1, 1, 1, -1) < torch.tensor(geo["qlive"]).view(-1, 1, 1, 1))
        n = int(live.sum())
        rate, sd = float(keep[live].sum()) / n, (p * (1 - p) / n) ** 0.5
        assert abs(rate - (1 - p)) <= 4 * sd + 1.0 / 256, (rid, rate)             # (+ the byte generator's threshold step)
    for n, (S, O, prev) in enumerate(layers):
        S_ref, E_S = P.logits(c, t, geo, prev=prev)
        ref = P.reference(c, t, geo, S, p, keep)
        res = P.evaluate(c, geo, ref, dict(S=S, O=O), S_ref, E_S)
        _held(f"{rid} layer {n + 1}", c, res)
        _record(c, res)
        if mode == "saturate":
            fin = S[torch.isfinite(S)]                      # (tiles that are not covered hold the sentinel)
            assert not bool(torch.isposinf(S).any()) and (c["N"] < 8 or float(fin.max()) == 65504.0), rid
    for gz in (False, True):
        ref = P.reference(c, t, geo, layers[0][0], p, keep, gz=gz)
        res = P.evaluate(c, geo, ref, back[gz])
        _held(f"{rid} g_in_zero={int(gz)}", c, res)
        _record(c, res)


# ------------------------------------------------------------------------------------------------ refusals
def test_the_wrappers_refuse_pair_planes_of_another_size():
    """S and G must be planes of the call's own (B, H, N, ld): a smaller one would be read and written past its end, a tiled one of another
    N would be addressed with the wrong plane stride"""
    B, N, H = 2, 20, 3
    ld, D = ops.pair_ld(N), H * 8
    qkv = torch.zeros(B * N, 3 * D, dtype=P.BF16, device=DEV)
    do = torch.zeros(B * N, D, dtype=P.BF16, device=DEV)
    good = torch.zeros(B, H, ops.pair_plane(N), dtype=torch.float16, device=DEV)
    small = torch.zeros(B, H, ops.pair_plane(N - 4), dtype=torch.float16, device=DEV)
    with pytest.raises(MMDTIError):
        ops.pair_attn_fwd(qkv, small, None, B, N, H, ld, 0.35)
    with pytest.raises(MMDTIError):
        ops.pair_attn_fwd(qkv, torch.zeros(B, H, N, ld - 4, device=DEV), None, B, N, H, ld, 0.35)
    s, _ = ops.pair_attn_fwd(qkv, good, None, B, N, H, ld, 0.35)
    with pytest.raises(MMDTIError):
        ops.pair_attn_bwd(qkv, s, do, small.float(), B, N, H, ld, 0.35, False)
    with pytest.raises(MMDTIError):
        ops.pair_attn_bwd(qkv, small, do, small.float(), B, N, H, ld, 0.35, False)
    big = torch.zeros(B, H, ops.pair_plane(N + 4), dtype=torch.float16, device=DEV)
    with pytest.raises(MMDTIError):
        ops.pair_attn_fwd(qkv, big, None, B, N, H, ld, 0.35)                                   # the planes of another N
    with pytest.raises(MMDTIError):
        ops.pair_attn_bwd(qkv, s, do, big.float(), B, N, H, ld, 0.35, False)                   # S and G of unequal size
    with pytest.raises(MMDTIError):
        ops.pair_attn_bwd(qkv, big, do, big.float(), B, N, H, ld, 0.35, False)
    ops.pair_attn_bwd(qkv, s, do, torch.zeros_like(s, dtype=torch.float32), B, N, H, ld, 0.35, False)


def test_the_library_refuses_a_row_stride_below_n_and_serves_any_key_tile_count():
    """ld < N is refused for every layout; a key_tiles entry of 0 runs as one tile and one above the tile count as the tile count (the
    kernels clamp it), identically to the dense run"""
    B, N, H = 2, 40, 3
    ld, D = ops.pair_ld(N), H * 8
    g = torch.Generator().manual_seed(3)
    qkv = torch.randn(B * N, 3 * D, generator=g).to(P.BF16).to(DEV)
    bias = torch.zeros(B, H, ops.pair_plane(N), dtype=torch.float16, device=DEV)
    bias[:, :, ops._tile_index(N, DEV, ld)[:, N:].reshape(-1)] = float("-inf")
    s = torch.empty_like(bias)
    o = torch.empty(B * N, D, dtype=P.BF16, device=DEV)
    with pytest.raises(MMDTIError):
        _abi.lib().mmdti_pair_attn_fwd(ops._stream(), qkv.data_ptr(), bias.data_ptr(), s.data_ptr(), o.data_ptr(), 0, B, N, H, N - 4, 0.35, 0.0, 1, 1, 3, 0, 0, 0, 0)
    s_d, o_d = ops.pair_attn_fwd(qkv, bias, None, B, N, H, ld, 0.35)
    kt = torch.tensor([9, 3], dtype=torch.int32, device=DEV)
    s_r, o_r = ops.pair_attn_fwd(qkv, bias, None, B, N, H, ld, 0.35, key_tiles=kt, rag_store=True)
    assert torch.equal(o_r, o_d) and torch.equal(s_r, s_d)
    kt0 = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    key_pad = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    key_pad[:, 16:] = True
    s_d, o_d = ops.pair_attn_fwd(qkv, bias, key_pad, B, N, H, ld, 0.35)
    s_r, o_r = ops.pair_attn_fwd(qkv, bias, key_pad, B, N, H, ld, 0.35, key_tiles=kt0, rag_store=True)
    assert torch.equal(o_r, o_d) and torch.equal(ops.pair_untile(s_r, N), ops.pair_untile(s_d, N))
