"""The case tables of the attention-map instance tests (csrc/attn_maps.hip), their input builders, float64 references, bounds and an
fp32 emulation of the kernels' rounding points, shared by test_maps_cases_cpu.py (plans, coverage, exactness, the emulation inside
the bounds and two wrong emulations outside) and test_maps_instances_gpu.py (the twelve kernel instances on the device, operands cut
from NaN-filled arenas, outputs from sentinel-filled ones).

FUSED MAP (mmdti_attn_map).  Reference: float64 on the stored bf16 operands, per (sequence, head), logits in base-2 units with the
additive term clamped at -FLT_MAX (attn_cases.reference):
    s2 = log2e scale q.k^T + max(log2e add, -FLT_MAX)     p = 2^(s2 - m) / sum_j 2^(s2 - m)     map = (1/H) sum_h p_h   |   p_h
written positionally into [B, Lq_out, ld_out]; zero wherever the query is not a real query or the key not a real key.
The kernel computes p from the forward's saved (m, 1 / sum): the ingredients of the forward's own p, so attn_cases' rho_ij is its
relative error; the map adds a sum of H terms and one product:
    |got - ref| <= (1/H) sum_h rho_h p_h + (H + 2) 2^-23 ref + 2^-126                       (H = 1 for a single head)
PAIR MAP (mmdti_pair_attn_map).  Reference: float64 softmax over the stored logits (fp16 or fp32, widened exactly; -inf at padded
keys is in them), rho_ij of pair_cases (eps (|m| + 2 |s - m| + 2), its p-weighted row mean, (N + 4) eps), the same sum and product.

EXACT MODES (compare bits):
  selector  one key per query wins by >= 128 natural units: p is one-hot, the mean over heads is count / H: the expectation is
            fp32(count) * fp32(1 / H) (count <= H small: the sum is exact in any order), stated without the reference.
  uniform   n real keys (a power of two), all logits 0: p = 1/n exactly, the sum over heads H / n exactly, times fp32(1 / H)."""
import math

import torch

from attn_cases import EPS, ETA, FLT_MAX, FMIN, LOG2E, _codes, sel_of
from gemm_cases import F64, Arena, worst_ratio  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
PTR = 0x10000          # a fake, 16-byte aligned device address: mmdti_maps_plan never dereferences one
MAPS_FAMILY = 8        # MMDTI_PLAN_MAPS
BLOCK = 256
PAIR_BUCKETS = ((80, 5), (144, 9), (208, 13), (272, 17))          # (largest N, tiles the instance is unrolled for)
TABLE = ("attn_map_kernel<16>", "attn_map_kernel<32>", "attn_map_kernel<64>", "pair_attn_map_rows_kernel") + \
    tuple(f"pair_attn_map_tiled_kernel<{t}, {nt}>" for t in ("float", "_Float16") for _, nt in PAIR_BUCKETS)


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------------------------------------ declared plans
def declared_attn_plan(B, Lq_out, ld_out, hd):
    """(instance, grid, workgroup size, LDS bytes, keyed by, tiles): one workgroup of four waves per (sequence, 16 output rows), the
    waves split the 16-column tiles of the output row; no LDS"""
    return (f"attn_map_kernel<{hd}>", B * cdiv(Lq_out, 16), BLOCK, 0, hd, cdiv(ld_out, 16))


def declared_pair_plan(B, N, layout):
    """one workgroup per (molecule, 16 queries); the tiled forms run the smallest instance whose unrolled row holds N (5 / 9 / 13 / 17 tiles
    for N <= 80 / 144 / 208 / 272) and fold three waves' partial sums through LDS: 64 lanes x tiles x 16 B each"""
    nt = cdiv(N, 16)
    if layout == 0:
        return (TABLE[3], B * nt, BLOCK, 0, 0, nt)
    unrolled = next(u for n, u in PAIR_BUCKETS if N <= n)
    return (f"pair_attn_map_tiled_kernel<{'float' if layout == 1 else '_Float16'}, {unrolled}>", B * nt, BLOCK, 3 * 64 * nt * 16, unrolled, nt)


def _plan_tuple(lib, out):
    p = list(out)
    return (lib._dll.mmdti_plan_kernel_name(MAPS_FAMILY, p[0]).decode(),) + tuple(p[1:])


def library_attn_plan(lib, B, heads, Lq, Lk, hd, Lq_out, ld_out, head=-1, q=PTR, k=PTR, add=0, stats=PTR, out=PTR, ldq=None, ldk=None,
                      vargs=(0, 0, 0, 0), q_cnt=0):
    import ctypes
    D = heads * hd
    o = (ctypes.c_int * 6)()
    lib.mmdti_maps_plan(0, q, k, add, stats, out, B, heads, Lq, Lk, hd, ldq or D, ldk or D, Lq_out, ld_out, head, *vargs, q_cnt, 0, 0, 0, o)
    return _plan_tuple(lib, o)


def library_pair_plan(lib, B, N, H, ld, ld_out, layout, head=-1, s=PTR, out=PTR, key_tiles=0, n_real=0):
    import ctypes
    o = (ctypes.c_int * 6)()
    lib.mmdti_maps_plan(1, s, 0, 0, 0, out, B, H, N, 0, 0, ld, 0, 0, ld_out, head, 0, 0, 0, 0, 0, layout, key_tiles, n_real, o)
    return _plan_tuple(lib, o)


# ------------------------------------------------------------------------------------------------ the fused map's table
ATTN_CASES = []
SHAPES = ((1, 1), (16, 15), (17, 33), (40, 256), (40, 257), (257, 40), (300, 384), (385, 385))
VARIANTS = ("bias", "fmin", "allmask")


def add_attn(hd, Lq, Lk, variant, heads=3, B=2, packed=None, qcnt=None, vec=False, modes=("selector", "uniform", "random")):
    c = dict(hd=hd, heads=heads, B=B, Lq=Lq, Lk=Lk, variant=variant, packed=packed, qcnt=qcnt, vec=vec, modes=tuple(modes))
    if packed is not None:            # (query lengths, key lengths, padded lengths)
        ql, kl, Sq, Sk = packed
        c["B"] = len(ql)
        c["Lq"], c["Lk"] = max(n + (n < Sq) for n in ql), max(kl)
        c["Lq_out"], c["ld_out"] = Sq, Sk
    else:
        c["Lq_out"], c["ld_out"] = Lq, (cdiv(Lk, 4) * 4 + 4 if vec else Lk)
    ATTN_CASES.append(c)
    return c


def _build_attn():
    n = 0
    for hd in (16, 32, 64):
        for Lq, Lk in SHAPES:
            add_attn(hd, Lq, Lk, VARIANTS[n % 3], vec=bool(n % 2))
            n += 1
    add_attn(32, 512, 512, "bias", vec=True, modes=("uniform", "random"))
    add_attn(32, 33, 40, "fmin", heads=16, modes=("selector", "uniform", "random"))                  # the cross block's heads
    pm = ("selector", "random")
    for i, hd in enumerate((16, 32, 64)):
        add_attn(hd, 0, 0, "packed", packed=((1, 17, 33), (16, 1, 40), 33, 40), modes=pm)
        add_attn(hd, 0, 0, "packed", packed=((5, 258, 130), (512, 40, 300), 258, 512), qcnt=(5, 258, 130), modes=pm)
        add_attn(hd, 0, 0, "packed", packed=((17, 1, 33), (16, 1, 32), 40, 40), qcnt=(17, 1, 33), modes=("uniform",))
        # dense rows with a real-query count (the padded layout of a right-padded batch)
        add_attn(hd, 33, 40, "bias", qcnt=(33, 7), modes=("random",))


_build_attn()


def attn_case_id(c):
    f = [f"hd{c['hd']}", f"h{c['heads']}", f"{c['Lq']}x{c['Lk']}", c["variant"]]
    if c["packed"]:
        f.append("_".join(map(str, c["packed"][0])))
    if c["qcnt"]:
        f.append("qcnt")
    if c["vec"]:
        f.append("vec")
    return "-".join(f)


def attn_runs(modes):
    return [(c, m) for c in ATTN_CASES for m in c["modes"] if m in modes]


def run_id(r):
    return (attn_case_id(r[0]) if "hd" in r[0] else pair_case_id(r[0])) + "-" + r[1]


def attn_sequences(c):
    """-> (rows_q, rows_k, [(q0, lq, k0, lk, krows)], packed offsets or None)"""
    if c["packed"] is None:
        Lq, Lk, B = c["Lq"], c["Lk"], c["B"]
        return B * Lq, B * Lk, [(b * Lq, Lq, b * Lk, Lk, Lk) for b in range(B)], None
    from mmdti_hip.packing import PackedRows
    ql, kl, Sq, Sk = c["packed"]
    pq, pk = PackedRows(torch.tensor(ql), Sq), PackedRows(torch.tensor(kl), Sk)
    qo, ko = pq.off_host.tolist(), pk.off_host.tolist()
    seqs = [(qo[b], qo[b + 1] - qo[b], ko[b], kl[b], ko[b + 1] - ko[b]) for b in range(len(ql))]
    return pq.M, pk.M, seqs, dict(q_off=qo, k_off=ko, k_cnt=list(kl))


def attn_inputs(c, mode, seed=0):
    """-> dict: q [rows_q, D], k [rows_k, D] bf16 on the CPU, add [B, Lk] fp32 or None, scale, seqs, packed, sel / n_real"""
    hd, H = c["hd"], c["heads"]
    D = H * hd
    rq, rk, seqs, pk = attn_sequences(c)
    nb = len(seqs)
    g = torch.Generator().manual_seed(977 + seed + 7 * hd + 13 * c["Lq"] + 17 * c["Lk"] + H)
    t = dict(seqs=seqs, packed=pk, rows_q=rq, rows_k=rk, add=None, sel=None, n_real=None)
    if mode == "selector":
        t["scale"] = 1.0
        k, q = torch.zeros(rk, D), torch.zeros(rq, D)
        t["sel"] = []
        for b, (q0, lq, k0, lk, krows) in enumerate(seqs):
            for h in range(H):
                k[k0:k0 + krows, h * hd:(h + 1) * hd] = _codes(krows, hd, 613 * b + 97 * h)
            sel = torch.stack([(sel_of(lq, lk) + h) % lk for h in range(H)])              # [H, lq]: the heads select different keys
            t["sel"].append(sel)
            for h in range(H):
                q[q0:q0 + lq, h * hd:(h + 1) * hd] = 64.0 * k[k0 + sel[h], h * hd:(h + 1) * hd]
    elif mode == "uniform":
        t["scale"] = 0.25
        q, k = torch.zeros(rq, D), torch.randint(-1, 2, (rk, D), generator=g).float()
        t["n_real"] = []
        if pk is None:
            addm = torch.full((nb, c["Lk"]), FMIN)
            for b in range(nb):
                n = 1 << (c["Lk"].bit_length() - 1)
                addm[b, torch.randperm(c["Lk"], generator=g)[:n]] = 0.0
                t["n_real"].append(n)
            t["add"] = addm
        else:
            t["n_real"] = list(pk["k_cnt"])
            assert all(n & (n - 1) == 0 for n in t["n_real"])
    else:
        t["scale"] = 1.0 / math.sqrt(hd)
        q = (torch.randn(rq, D, generator=g) * 1.5).to(BF16).float()
        k = (torch.randn(rk, D, generator=g) * 1.5).to(BF16).float()
    if pk is None and mode != "uniform":
        Lk = c["Lk"]
        if c["variant"] == "bias":
            addm = -4.0 * torch.rand(nb, Lk, generator=g)
        else:
            addm = torch.zeros(nb, Lk)
            if Lk > 2:
                addm[0, Lk - Lk // 3:] = FMIN
        if c["variant"] == "allmask":
            addm[nb - 1, :] = FMIN
        if mode == "selector":           # (a bias of a few units cannot reach the 128-unit margin; finfo.min would: the selector keeps its winners)
            addm = torch.zeros(nb, Lk)
        t["add"] = addm
    t.update(q=q.to(BF16), k=k.to(BF16))
    return t


def _heads(x, r0, n, H, hd, dtype):
    return x[r0:r0 + n].to(dtype).view(n, H, hd).permute(1, 0, 2)          # [H, n, hd]


def _real_queries(c, b, lq):
    return lq if c["qcnt"] is None else min(lq, c["qcnt"][b])


def attn_probs(c, t, dtype, stats=None, nat_stats=False):
    """per sequence [H, lq, lk] probabilities in `dtype` arithmetic (float64: the reference; fp32: the kernels' rounding points, with
    the forward's own (m, 1 / sum) -- or the given stats, list per sequence of ([H, lq], [H, lq])) -> (list of p, list of (m, inv), list of rho)"""
    hd, H, scale = c["hd"], c["heads"], t["scale"]
    ps, sts, rhos = [], [], []
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        Q, K = _heads(t["q"], q0, lq, H, hd, dtype), _heads(t["k"], k0, lk, H, hd, dtype)
        if dtype == F64:
            add2 = torch.zeros(lk, dtype=F64) if t["add"] is None else (t["add"][b, :lk].to(F64) * LOG2E).clamp_min(-FLT_MAX)
            s2 = (LOG2E * scale) * (Q @ K.transpose(1, 2)) + add2
        else:
            sc2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
            add2 = torch.zeros(lk) if t["add"] is None else (t["add"][b, :lk] * torch.tensor(LOG2E, dtype=F32)).clamp_min(-FLT_MAX)
            s2 = (Q @ K.transpose(1, 2)) * sc2 + add2
        m = s2.max(-1, keepdim=True).values
        e = torch.exp2(s2 - m)
        l = e.sum(-1, keepdim=True)
        if dtype == F64:
            p = e / l
            E2 = (hd + 8) * EPS * (LOG2E * abs(scale) * (Q.abs() @ K.abs().transpose(1, 2)) + add2.abs())
            E2 = torch.where(add2 == -FLT_MAX, torch.zeros_like(E2), E2)
            E = E2 + EPS * ((s2 - m).abs() + 4.0)
            rhos.append(math.log(2.0) * (E + (p * E).sum(-1, keepdim=True)) + (lk + 8) * EPS)
        else:
            mi = (m, 1.0 / l) if stats is None else (stats[b][0].unsqueeze(-1), stats[b][1].unsqueeze(-1))
            mm = mi[0] / torch.tensor(LOG2E, dtype=F32) if nat_stats else mi[0]
            p = torch.exp2(s2 - mm) * mi[1]
            m, l = mi[0], 1.0 / mi[1]
        ps.append(p)
        sts.append((m[..., 0], (1.0 / l)[..., 0]))
    return ps, sts, rhos


def attn_reference(c, t, head=-1):
    """-> (ref, bound) float64 [B, Lq_out, ld_out]"""
    H = c["heads"]
    ps, _, rhos = attn_probs(c, t, F64)
    ref = torch.zeros(c["B"], c["Lq_out"], c["ld_out"], dtype=F64)
    bnd = torch.zeros_like(ref)
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        n = _real_queries(c, b, lq)
        p, rho = ps[b][:, :n], rhos[b][:, :n]
        if head < 0:
            ref[b, :n, :lk], bnd[b, :n, :lk] = p.mean(0), (rho * p).mean(0)
            hh = H
        else:
            ref[b, :n, :lk], bnd[b, :n, :lk] = p[head], rho[head] * p[head]
            hh = 1
        bnd[b, :n, :lk] += (hh + 2) * EPS * ref[b, :n, :lk] + ETA
    return ref, bnd


def attn_emulate(c, t, head=-1, stats=None, denom=None, nat_stats=False):
    """the kernel in fp32 torch: p from (m, 1 / sum), the heads added in ascending order, times fp32(1 / H)"""
    H = c["heads"]
    ps, _, _ = attn_probs(c, t, F32, stats, nat_stats)
    out = torch.zeros(c["B"], c["Lq_out"], c["ld_out"], dtype=F32)
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(denom or H), dtype=F32)
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        n = _real_queries(c, b, lq)
        if head < 0:
            acc = torch.zeros(n, lk, dtype=F32)
            for h in range(H):
                acc = acc + ps[b][h, :n]
            out[b, :n, :lk] = acc * inv_h
        else:
            out[b, :n, :lk] = ps[b][head, :n]
    return out


def attn_selector_expectation(c, t, head=-1):
    H = c["heads"]
    out = torch.zeros(c["B"], c["Lq_out"], c["ld_out"], dtype=F32)
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        n = _real_queries(c, b, lq)
        cnt = torch.zeros(lq, lk, dtype=F32)
        for h in (range(H) if head < 0 else (head,)):
            cnt[torch.arange(lq), t["sel"][b][h]] += 1.0
        out[b, :n, :lk] = (cnt * inv_h if head < 0 else cnt)[:n]
    return out


def attn_uniform_expectation(c, t, head=-1):
    H = c["heads"]
    out = torch.zeros(c["B"], c["Lq_out"], c["ld_out"], dtype=F32)
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        n = _real_queries(c, b, lq)
        real = torch.ones(lk, dtype=torch.bool) if t["add"] is None else t["add"][b, :lk] == 0
        nr = int(real.sum())
        assert nr == t["n_real"][b] and nr & (nr - 1) == 0
        v = torch.tensor(float(H) / nr, dtype=F32) * inv_h if head < 0 else torch.tensor(1.0 / nr, dtype=F32)
        out[b, :n, :lk] = torch.where(real, v, torch.tensor(0.0))
    return out


# ------------------------------------------------------------------------------------------------ the pair map's table
PAIR_CASES = []


def pair_ld(N):
    return (N + 3) // 4 * 4


def pair_plane(N):
    return (N * pair_ld(N) + 7) // 8 * 8


def pa_kt_effective(kt, nt):
    step = 1 if nt <= 9 else (2 if nt <= 13 else 4)
    k = (max(int(kt), 1) + step - 1) // step * step
    return nt if k >= nt else k


def supported_counts(nt):
    return sorted({pa_kt_effective(k, nt) for k in range(1, nt + 1)})


def add_pair(N, layout, B=3, H=3, ld=None, lens=None, vec=False, modes=("selector", "uniform", "random")):
    c = dict(N=N, layout=layout, B=B, H=H, ld=(N if ld is None else ld) if layout == 0 else pair_ld(N), lens=lens, vec=vec, modes=tuple(modes),
             ld_out=(cdiv(N, 4) * 4 + 4 if vec else N))
    if lens is not None:
        c["B"] = len(lens)
    PAIR_CASES.append(c)
    return c


def ragged_lens(N):
    """one molecule per supported covered-tile count (its last real atom in the count's last tile), one whose count rounds up, a single atom"""
    nt = cdiv(N, 16)
    lens = [min(16 * k - 3, N) for k in supported_counts(nt)]
    up = next((k for k in range(1, nt) if pa_kt_effective(k, nt) != k), None)
    if up is not None:
        lens.append(16 * up - 5)
    return lens + [1]


def _build_pair():
    n = 0
    for N in (1, 4, 5, 16, 17, 22, 130, 258, 272):
        for layout in (1, 3):
            add_pair(N, layout, vec=bool(n % 2))
            n += 1
    for N in (80, 81, 144, 145, 208, 209):             # each boundary of the size classes csrc/maps_plan.h declares
        for layout in (1, 3):
            add_pair(N, layout, vec=bool(n % 2), modes=("selector", "random"))
            n += 1
    add_pair(130, 3, H=64, modes=("uniform", "random"))
    for N in (1, 13, 273, 320):
        add_pair(N, 0, vec=False)
        add_pair(N, 0, ld=N + 5, vec=True)
    for N in (208, 272, 130):
        add_pair(N, 3, lens=ragged_lens(N), modes=("selector", "random"))


_build_pair()


def pair_case_id(c):
    f = [f"N{c['N']}", f"l{c['layout']}", f"B{c['B']}H{c['H']}"]
    if c["layout"] == 0 and c["ld"] != c["N"]:
        f.append(f"ld{c['ld']}")
    if c["lens"]:
        f.append("ragged")
    if c["vec"]:
        f.append("vec")
    return "-".join(f)


def pair_runs(modes):
    return [(c, m) for c in PAIR_CASES for m in c["modes"] if m in modes]


def pair_dtype(c):
    return F16 if c["layout"] == 3 else F32


def pair_lens(c):
    """real atoms per molecule: ragged cases as listed; dense cases mask a third of the keys of molecule 0 (key padding)"""
    if c["lens"] is not None:
        return list(c["lens"])
    N = c["N"]
    return [N - N // 3 if (b == 0 and N > 2) else N for b in range(c["B"])]


def pair_inputs(c, mode, seed=0):
    """-> dict: S [B, H, N, N] in the storage type's values (fp32 tensor), -inf at padded keys; lens; sel"""
    B, H, N = c["B"], c["H"], c["N"]
    g = torch.Generator().manual_seed(4177 + seed + 11 * N + H)
    lens = pair_lens(c)
    t = dict(lens=lens, sel=None)
    if mode == "selector":
        S = torch.full((B, H, N, N), -200.0)
        sel = torch.stack([torch.stack([(7 * torch.arange(N) + 3 * h + b) % lens[b] for h in range(H)]) for b in range(B)])        # [B, H, N]
        S.scatter_(3, sel.unsqueeze(-1), 0.0)
        t["sel"] = sel
    elif mode == "uniform":
        # (a power-of-two count of real keys: the dense cases of this mode take their own lengths)
        lens = [max(1 << (n.bit_length() - 1), 1) for n in lens]
        t["lens"] = lens
        S = torch.zeros(B, H, N, N)
    else:
        S = torch.randn(B, H, N, N, generator=g) * 3.0
    for b in range(B):
        S[b, :, :, t["lens"][b]:] = float("-inf")
    t["S"] = S.to(pair_dtype(c)).float()
    return t


def pair_rows(c, t, b):
    """query rows of molecule b whose map is asked for: every row of a dense case, the real rows of a ragged one"""
    return t["lens"][b] if c["lens"] is not None else c["N"]


def pair_reference(c, t, head=-1):
    B, H, N = c["B"], c["H"], c["N"]
    S = t["S"].to(F64)
    m = S.max(-1, keepdim=True).values
    e = torch.exp(S - m)
    p = e / e.sum(-1, keepdim=True)
    a = torch.where(p > 0, (S - m).abs(), torch.zeros_like(S))
    ee = EPS * (m.abs() + 2 * a + 2.0)
    rho = ee + (p * ee).sum(-1, keepdim=True) + (N + 4) * EPS
    ref = torch.zeros(B, N, c["ld_out"], dtype=F64)
    bnd = torch.zeros_like(ref)
    if head < 0:
        ref[:, :, :N], bnd[:, :, :N], hh = p.mean(1), (rho * p).mean(1), H
    else:
        ref[:, :, :N], bnd[:, :, :N], hh = p[:, head], (rho * p)[:, head], 1
    bnd[:, :, :N] += (hh + 2) * EPS * ref[:, :, :N] + ETA
    for b in range(B):
        ref[b, pair_rows(c, t, b):] = 0
        bnd[b, pair_rows(c, t, b):] = 0
    return ref, bnd


def pair_head_runs(c, head=-1):
    """the order the kernel adds heads in: layout 0 all heads in order; tiled: four runs of ceil(H / 4) consecutive heads"""
    H = c["H"]
    if head >= 0:
        return [[head]]
    if c["layout"] == 0:
        return [list(range(H))]
    ch = cdiv(H, 4)
    return [list(range(w * ch, min((w + 1) * ch, H))) for w in range(4)]


def pair_emulate(c, t, head=-1, denom=None):
    B, H, N = c["B"], c["H"], c["N"]
    S = t["S"]
    L = torch.tensor(LOG2E, dtype=F32)
    m = S.max(-1, keepdim=True).values
    e = torch.exp2(S * L + (-m * L))
    p = e * (1.0 / e.sum(-1, keepdim=True))
    acc = None
    for run in pair_head_runs(c, head):
        part = torch.zeros(B, N, N, dtype=F32)
        for h in run:
            part = part + p[:, h]
        acc = part if acc is None else acc + part
    if head < 0:
        acc = acc * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(denom or H), dtype=F32))
    out = torch.zeros(B, N, c["ld_out"], dtype=F32)
    out[:, :, :N] = acc
    for b in range(B):
        out[b, pair_rows(c, t, b):] = 0
    return out


def pair_selector_expectation(c, t, head=-1):
    B, H, N = c["B"], c["H"], c["N"]
    cnt = torch.zeros(B, N, N, dtype=F32)
    for h in (range(H) if head < 0 else (head,)):
        cnt.scatter_add_(2, t["sel"][:, h].unsqueeze(-1), torch.ones(B, N, 1))
    if head < 0:
        cnt = cnt * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32))
    out = torch.zeros(B, N, c["ld_out"], dtype=F32)
    out[:, :, :N] = cnt
    for b in range(B):
        out[b, pair_rows(c, t, b):] = 0
    return out


def pair_uniform_expectation(c, t, head=-1):
    B, H, N = c["B"], c["H"], c["N"]
    out = torch.zeros(B, N, c["ld_out"], dtype=F32)
    inv_h = torch.tensor(1.0, dtype=F32) / torch.tensor(float(H), dtype=F32)
    for b in range(B):
        n = t["lens"][b]
        out[b, :pair_rows(c, t, b), :n] = torch.tensor(float(H) / n, dtype=F32) * inv_h if head < 0 else 1.0 / n
    return out


def tile_index(N):
    """[N, N4] flat offsets inside a tiled plane of (query, key slot)"""
    q = torch.arange(N).view(N, 1)
    k = torch.arange(pair_ld(N)).view(1, -1)
    vr = torch.clamp(N - q // 16 * 16, max=16)
    return (q // 16 * 16) * pair_ld(N) + vr * (k - k % 4) + (q % 16) * 4 + k % 4


def pair_store(c, t):
    """the stored form of t['S'] on the CPU: a flat tensor of the storage type with NaN wherever the forward stores nothing the map may
    read -- the skipped key tiles and the rows from n_real on of a ragged case (and the alignment tail of a plane, the padding columns
    of a row-major plane) -- and -inf in the pad key slots N .. N4-1 of a tiled plane; plus key_tiles / n_real lists or None"""
    B, H, N = c["B"], c["H"], c["N"]
    dt = pair_dtype(c)
    nan = float("nan")
    if c["layout"] == 0:
        flat = torch.full((B, H, N, c["ld"]), nan, dtype=dt)
        flat[..., :N] = t["S"].to(dt)
        return flat.reshape(-1), None, None
    N4, nt = pair_ld(N), cdiv(N, 16)
    full = torch.full((B, H, N, N4), float("-inf"), dtype=dt)
    full[..., :N] = t["S"].to(dt)
    kts = nrl = None
    if c["lens"] is not None:
        kts, nrl = [cdiv(n, 16) for n in t["lens"]], list(t["lens"])
        for b in range(B):
            full[b, :, :, 16 * pa_kt_effective(kts[b], nt):] = nan
            full[b, :, nrl[b]:, :] = nan
    flat = torch.full((B, H, pair_plane(N)), nan, dtype=dt)
    flat[:, :, tile_index(N).reshape(-1)] = full.reshape(B, H, N * N4)
    return flat.reshape(-1), kts, nrl
