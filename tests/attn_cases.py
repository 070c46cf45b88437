"""The case table of the fused-attention instance tests, their input builders and their float64 reference, shared by
test_attn_cases_cpu.py (which proves the table's coverage, the exactness conditions and that an fp32 emulation of the kernels'
rounding points stays inside the bounds) and test_attn_instances_gpu.py (which holds the 27 kernel instances of csrc/attn.hip to
the reference on the device, on operands cut from NaN-filled arenas into outputs cut from sentinel-filled arenas).

REFERENCE (reference()): float64 on the stored 16-bit operands, explicit sums, per (sequence, head); c = 1 / (1 - p_drop), kappa the
keep mask.  Logits are carried in base-2 units as the kernels carry them (mathematically the natural-unit softmax; the additive
term is clamped at -FLT_MAX as attn_mask2 clamps it, which only matters at finfo.min, where the probability is 0 or -- all keys
masked -- the row uniform):
    s2 = log2e * scale * q.k^T + max(log2e * add, -FLT_MAX)      m = max_j s2      e = 2^(s2 - m)      p = e / sum_j e
    P' = c kappa p      ctx = P' v      dP = c kappa (do.v^T)      r = sum_j dP p      dS = scale p (dP - r)
    dq = dS k           dk = dS^T q     dv = P'^T do

MODES
  selector  k rows are distinct +-1 codes, q_i = 64 k_sel(i), scale 1: every loser lies 128 * hamming >= 128 natural units below the
            winner, 2^(-184) is 0 in fp32, P is one-hot.  ctx_i = v_sel(i), dq = dk = 0, dv_j = sum of the do_i that selected j,
            stats = (fp32(64 hd) * fp32(log2e), 1) -- bit for bit, stated without the reference.
  uniform   q = 0, a power-of-two number n of real keys (the others carry finfo.min, scattered), k, v, do in {-1, 0, 1}, scale
            2^-2: p = 1/n, every fp32 intermediate is exact, every 16-bit rounding rounds an exact value and the reference
            applies it too (exact=True).  exactness() states the condition: the terms of every final sum are multiples of one
            quantum with sum |term| < 2^24 quanta, so no summation order can matter.  Outputs EQUAL the reference.
  random    the inputs of the older tests (randn * 1.5, do randn, scale hd^-1/2); key_add from [-4, 0] (`bias` cases) or finfo.min
            on the last third of sequence 0's keys; `allmask` cases mask every key of the last sequence (the uniform row).
  large     random with q and k scaled until max |s| = 150 natural units.
  dropout   random at p = 0.1 / 0.35 with the keep mask recovered from the device.

BOUNDS of the non-exact modes (bounds are first-order in eps = 2^-23; u = 2^-8, the relative step of a bf16 operand rounding; R =
gemm_cases.rounding_term of the output; eta = 2^-126 covers fp32 / bf16 underflow of a probability or dS):
  logit      fp32 accumulation of hd exact products, the rounding of scale * log2e, of add * log2e and of the fma:
                 E2_ij = (hd + 8) eps (log2e |scale| sum_d |q||k| + |add2|)            [base-2 units]
             (a key at -FLT_MAX absorbs the product exactly in fp32 and in float64 alike: E2 = 0 there);
             the subtraction of the row max and v_exp_f32 add eps (|s2 - m| + 4):  E_ij = E2_ij + eps (|s2_ij - m_i| + 4).
  p          d ln p_j = ln2 (d_j - sum_l p_l d_l), the sum of lk terms, 1 / sum and the product:
                 rho_ij = ln2 (E_ij + sum_l p_il E_il) + (lk + 8) eps                  [relative error of p_ij]
  stats      |m - m_ref| <= max_j E2_ij;   lse2 = m - log2(inv):  |.| <= sum_j p_ij E_ij + (lk + 8) eps log2e.
  ctx, dv    P' is rounded to bf16 (u), summed in fp32 over lk (lq) terms:
                 u T + [sum rho P' |v| + (L + 8) eps T + eta c sum |v|] + R + eta,   T = sum P' |v|   (dv: |do|, over queries)
  dP         E_dP = (hd + 8) eps sum_d |do||v|
  drow       two nested sums:  E_r = sum_j c kappa p (E_dP + |do.v| rho) + (lk + 8) eps sum_j |dP| p
  dS         the cancellation in dP - r: the errors of dP and of r are absolute, they do not shrink with |dP - r|:
                 E_dS = |scale| [p (c kappa E_dP + E_r + 3 eps (|dP| + |r|)) + rho p |dP - r| + eta (|dP| + |r| + 1)]
  dq, dk     u T + [sum E_dS |k| + (L + 8) eps T] + R + eta,   T = sum |dS| |k|   (dk: |q|, over queries)
GAIN: z = sum (got - ref) ref / sqrt(sum (bound ref)^2) per 16-bit output; |z| <= 6 (Hoeffding: 2 e^-18 for independent zero-mean
errors inside the bound).  This is what sees a 0.2 - 0.4 % systematic error that the elementwise bound only grazes."""
import math

import torch

from gemm_cases import F64, Arena, round16, rounding_term, worst_ratio  # noqa: F401

B, HEADS = 2, 3
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LOG2E = 1.4426950408889634
FLT_MAX = float(torch.finfo(F32).max)
FMIN = float(torch.finfo(F32).min)
EPS, ETA, U16 = 2.0 ** -23, 2.0 ** -126, 2.0 ** -8
SEED, SITE = 987654321, 3
Z_MAX = 6.0
PTR = 0x10000          # a fake, 16-byte aligned device address: mmdti_attn_plan never dereferences one


def attn_nt(Lk):
    return 10 if Lk <= 160 else 16 if Lk <= 256 else 24 if Lk <= 384 else 32


# ------------------------------------------------------------------------------------------------ the table
CASES = []
PLAIN = ("selector", "uniform", "random", "large")


def add(hd, Lq, Lk, entry, layout="tight", ldo4=False, ctx_f16=0, bias=False, allmask=False, modes=PLAIN, packed=None, drop=(0.1,)):
    assert entry == "long" or max(Lq, Lk) <= 256
    assert layout != "fused" or (Lq == Lk and packed is None)
    c = dict(hd=hd, Lq=Lq, Lk=Lk, entry=entry, layout=layout, ldo4=ldo4, ctx_f16=ctx_f16, bias=bias, allmask=allmask, modes=tuple(modes),
             packed=packed, drop=tuple(drop), nt=attn_nt(Lk), lqp=((Lq + 31) // 32) * 32)
    if packed is not None:                     # (query lengths, key lengths, padded lengths): Lq / Lk are what ops.AttnVarlen passes
        ql, kl, Sq, Sk = packed
        c["Lq"], c["Lk"] = max(n + (n < Sq) for n in ql), max(kl)
        c["nt"], c["lqp"] = attn_nt(c["Lk"]), ((c["Lq"] + 31) // 32) * 32
    CASES.append(c)
    return c


def _build():
    for n, hd in enumerate((16, 32, 64)):
        f = lambda i: (i + n) % 2                                        # alternate the context type between the head sizes
        add(hd, 1, 1, "short", "tight", ctx_f16=f(0))
        add(hd, 16, 15, "short", "padded", ldo4=True, ctx_f16=f(1), bias=True)
        add(hd, 17, 17, "short", "fused", ctx_f16=f(0), modes=PLAIN + ("dropout",), drop=(0.35,))
        add(hd, 31, 33, "short", "cross", ctx_f16=f(1), bias=True, allmask=True)
        add(hd, 33, 160, "short", "padded", ctx_f16=f(0), modes=PLAIN + ("dropout",), drop=(0.1, 0.35))
        add(hd, 33, 160, "long", "tight", ldo4=True, ctx_f16=f(1), bias=True)
        add(hd, 129, 161, "short", "cross", ldo4=True, ctx_f16=f(0), allmask=True)
        add(hd, 129, 256, "short", "tight", ctx_f16=f(1), bias=True, modes=PLAIN + ("dropout",))
        add(hd, 257, 256, "long", "padded", ctx_f16=f(0))
        add(hd, 512, 257, "long", "cross", ctx_f16=f(1), bias=True)
        add(hd, 16, 384, "long", "tight", ldo4=True, ctx_f16=f(0), allmask=True)
        add(hd, 17, 385, "long", "padded", ctx_f16=f(1), bias=True, modes=PLAIN + ("dropout",))
        add(hd, 129, 511, "long", "cross", ldo4=True, ctx_f16=f(0), allmask=True)
        add(hd, 512, 512, "long", "fused", ctx_f16=f(1), bias=True)
        add(hd, 33, 384, "long", "tight", ctx_f16=f(0), modes=("random", "dropout"), drop=(0.35,))
        pm = ("selector", "random", "large")
        add(hd, 0, 0, "short", "tight", ctx_f16=f(1), modes=pm, packed=((1, 17, 33), (16, 1, 40), 33, 40))
        add(hd, 0, 0, "long", "padded", ldo4=True, ctx_f16=f(0), modes=pm, packed=((5, 258, 130), (512, 40, 300), 258, 512))
        add(hd, 0, 0, "short", "cross", ctx_f16=f(0), modes=("uniform",), packed=((17, 1, 33), (16, 1, 32), 40, 40))


_build()


def case_id(c):
    f = [f"hd{c['hd']}", f"{c['Lq']}x{c['Lk']}", c["entry"], c["layout"]]
    f += [k for k in ("ldo4", "bias", "allmask") if c[k]]
    f.append("f16" if c["ctx_f16"] else "bf16")
    if c["packed"]:
        f.append("packed" + "_".join(map(str, c["packed"][0])))
    return "-".join(f)


def instances(c):
    return (f"attn_fwd_kernel<{c['hd']}, {c['nt']}>", f"attn_bwd_q_kernel<{c['hd']}, {c['nt']}>", f"attn_bwd_kv_kernel<{c['hd']}>")


def declared_plan(hd, Lq, Lk, nb, backward):
    """what a call is declared to launch, stated independently of csrc/attn_plan.h: (nt, lqp, [(instance, grid, workgroup size, dynamic
    LDS bytes, LDS opt-in)]) -- one workgroup per (sequence, head); K and V (dK/dV: Q and dO) images of hd + 8 columns and one (four)
    fp32 row vectors; the opt-in is the largest image pair of the short (256 rows) or the long (512 rows) entry points."""
    nt, lqp = attn_nt(Lk), ((Lq + 31) // 32) * 32
    short, long_ = 2 * 256 * 80 * 2 + 4 * 256 * 4, 2 * 512 * 72 * 2 + 4 * 512 * 4
    img = 2 * nt * 16 * (hd + 8) * 2 + nt * 16 * 4
    cap = long_ if nt > 16 else short
    if not backward:
        return nt, lqp, [(f"attn_fwd_kernel<{hd}, {nt}>", nb * HEADS, 256 if (hd, nt) == (16, 32) else 512, img, cap)]
    kv = 2 * lqp * (hd + 8) * 2 + 4 * lqp * 4
    return nt, lqp, [(f"attn_bwd_q_kernel<{hd}, {nt}>", nb * HEADS, 1024 if nt > 16 else 256, img, cap),
                     (f"attn_bwd_kv_kernel<{hd}>", nb * HEADS, 512, kv, long_ if kv > short else short)]


def library_plan(lib, backward, long_entry, hd, Lq, Lk, nb, ptr=None, ld=None, add=0, vargs=(0, 0, 0, 0), p_drop=0.0):
    """mmdti_attn_plan's answer in the form of declared_plan.  ptr / ld: the addresses and row strides of a launch (place()); default: fake
    aligned addresses and tight rows."""
    import ctypes
    D = HEADS * hd
    ptr = ptr or {n: PTR for n in ("q", "k", "v", "ctx", "do", "dq", "dk", "dv", "stats", "drow")}
    ld = ld or {n: D for n in ("q", "k", "ctx", "do", "dq", "dk")}
    out = (ctypes.c_int * 13)()
    lib.mmdti_attn_plan(int(backward), int(long_entry), ptr["q"], ptr["k"], ptr["v"], add, ptr["do"] if backward else ptr["ctx"], ptr["stats"], ptr["drow"],
                        ptr["dq"], ptr["dk"], ptr["dv"], nb, HEADS, Lq, Lk, hd, ld["q"], ld["k"], ld["do"] if backward else ld["ctx"], ld["dq"], ld["dk"],
                        p_drop, *vargs, out)
    p = list(out)
    name = lambda i: lib._dll.mmdti_plan_kernel_name(0, i).decode()
    return p[0], p[1], [(name(p[3 + 5 * i]),) + tuple(p[4 + 5 * i:8 + 5 * i]) for i in range(p[2])]


def assert_declared_plan(lib, c, nb, ptr=None, ld=None, add=0, vargs=(0, 0, 0, 0), p_drop=0.0, entry=None):
    """the library plans, for the case's forward and backward, what the table declares"""
    for backward in (False, True):
        got = library_plan(lib, backward, (entry or c["entry"]) == "long", c["hd"], c["Lq"], c["Lk"], nb, ptr, ld, add, vargs, p_drop)
        want = declared_plan(c["hd"], c["Lq"], c["Lk"], nb, backward)
        assert got == want and (got[0], got[1]) == (c["nt"], c["lqp"]), (case_id(c), backward, got, want)
        assert tuple(k[0] for k in got[2]) == (instances(c)[1:] if backward else instances(c)[:1]), (case_id(c), got)


def runs(modes):
    """(case, mode, p_drop) of every run in the given modes"""
    out = []
    for c in CASES:
        for m in c["modes"]:
            if m in modes:
                out += [(c, m, p) for p in (c["drop"] if m == "dropout" else (0.0,))]
    return out


def run_id(r):
    return f"{case_id(r[0])}-{r[1]}" + (f"-p{r[2]}" if r[2] else "")


# ------------------------------------------------------------------------------------------------ inputs
def sequences(c):
    """-> (rows_q, rows_k, [(q0, lq, k0, lk, krows)] per sequence, packed offsets or None)"""
    if c["packed"] is None:
        Lq, Lk = c["Lq"], c["Lk"]
        return B * Lq, B * Lk, [(b * Lq, Lq, b * Lk, Lk, Lk) for b in range(B)], None
    from mmdti_hip.packing import PackedRows
    ql, kl, Sq, Sk = c["packed"]
    pq, pk = PackedRows(torch.tensor(ql), Sq), PackedRows(torch.tensor(kl), Sk)
    qo, ko = pq.off_host.tolist(), pk.off_host.tolist()
    seqs = [(qo[b], qo[b + 1] - qo[b], ko[b], kl[b], ko[b + 1] - ko[b]) for b in range(len(ql))]
    return pq.M, pk.M, seqs, dict(q_off=qo, k_off=ko, k_cnt=list(kl))


def sel_of(lq, lk):
    """the selector's key of every query: pairs of queries share a key, four keys of five stay unselected, the last query takes the
    last key"""
    s = (5 * (torch.arange(lq) // 2)) % lk
    s[-1] = lk - 1
    return s


def _codes(n, hd, salt):
    """n distinct rows of +-1: the 11 bits of (row + 1 + salt), repeated along the head"""
    idx = torch.arange(n) + 1 + salt
    bits = (idx[:, None] >> (torch.arange(hd) % 11)[None, :]) & 1
    return (2 * bits - 1).to(torch.float32)


# The gain's premise -- independent errors -- is weakest in `large`, where the hd outputs of a row share the bf16 rounding of one
# dominant probability.  The condition on the inputs (test_attn_cases_cpu.py: the fp32 emulation's |z| < 3) picks the draw:
SEEDS = {("hd16-512x257-long-cross-bias-f16", "large"): 1}


def make_inputs(c, mode, seed=None):
    """-> dict: q, k, v, do ([rows, D] of the 16-bit operand type, on the CPU), add ([B, Lk] fp32 or None), scale, seqs, ..."""
    seed = SEEDS.get((case_id(c), mode), 0) if seed is None else seed
    hd = c["hd"]
    D = HEADS * hd
    rq, rk, seqs, pk = sequences(c)
    nb = len(seqs)
    g = torch.Generator().manual_seed(4242 + seed + 7 * hd + 13 * c["Lq"] + 17 * c["Lk"])
    ints = lambda rows, r: torch.randint(-r, r + 1, (rows, D), generator=g).to(torch.float32)
    t = dict(seqs=seqs, packed=pk, rows_q=rq, rows_k=rk, add=None, sel=None, n_real=None)
    if mode == "selector":
        t["scale"] = 1.0
        k, q = torch.zeros(rk, D), torch.zeros(rq, D)
        t["sel"] = []
        for b, (q0, lq, k0, lk, krows) in enumerate(seqs):
            for h in range(HEADS):
                k[k0:k0 + krows, h * hd:(h + 1) * hd] = _codes(krows, hd, 613 * b + 97 * h)
            s = sel_of(lq, lk)
            t["sel"].append(s)
            q[q0:q0 + lq] = 64.0 * k[k0 + s]
        v, do = ints(rk, 64) / 8.0, ints(rq, 2)
    elif mode == "uniform":
        t["scale"] = 0.25
        q, k, v, do = torch.zeros(rq, D), ints(rk, 1), ints(rk, 1), ints(rq, 1)
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
        G = lambda s: torch.Generator().manual_seed(s + seed)
        q, k, v, do = (torch.randn(rows, D, generator=G(s)) * a for rows, s, a in ((rq, 1, 1.5), (rk, 2, 1.5), (rk, 3, 1.5), (rq, 4, 1.0)))
        q, k = q.to(BF16).float(), k.to(BF16).float()
        if mode == "large":
            smax = 0.0
            for q0, lq, k0, lk, krows in seqs:
                for h in range(HEADS):
                    sl = slice(h * hd, (h + 1) * hd)
                    smax = max(smax, float((q[q0:q0 + lq, sl].double() @ k[k0:k0 + lk, sl].double().T).abs().max()) * t["scale"])
            f = math.sqrt(150.0 / smax)
            q, k = q * f, k * f
        if pk is None:
            Lk = c["Lk"]
            if c["bias"]:
                addm = -4.0 * torch.rand(nb, Lk, generator=g)
            else:
                addm = torch.zeros(nb, Lk)
                if Lk > 2:
                    addm[0, Lk - Lk // 3:] = FMIN
            if c["allmask"]:
                addm[nb - 1, :] = FMIN
            t["add"] = addm
    t.update(q=q.to(BF16), k=k.to(BF16), v=v.to(BF16), do=do.to(BF16))
    return t


# ------------------------------------------------------------------------------------------------ the reference
def _heads(x, r0, n, hd, dtype):
    return x[r0:r0 + n].to(dtype).view(n, HEADS, hd).permute(1, 0, 2)          # [heads, n, hd]


def _rows(x):
    return x.permute(1, 0, 2).reshape(x.shape[1], -1)                           # [heads, n, hd] -> [n, D]


def reference(c, t, p_drop=0.0, keep=None, exact=False, bounds=True):
    """-> dict of float64 tensors: ctx, dq [rows_q, D], dk, dv [rows_k, D], m2, lse2, inv, r (lists per sequence of [heads, lq]); with
    bounds, B_ctx .. B_dv (without R), tol_m, tol_lse, tol_r.  keep: list per sequence of [heads, lq, lk] bool.  exact: P' and dS
    rounded to bf16 as the kernels round them (the exact modes, where every rounding rounds an exact value)."""
    hd, scale = c["hd"], t["scale"]
    D = HEADS * hd
    cc = 1.0 / (1.0 - p_drop)
    out = {k: torch.zeros(t["rows_q"] if k in ("ctx", "dq", "B_ctx", "B_dq") else t["rows_k"], D, dtype=F64)
           for k in ("ctx", "dq", "dk", "dv", "B_ctx", "B_dq", "B_dk", "B_dv")}
    for k in ("m2", "lse2", "inv", "r", "tol_m", "tol_lse", "tol_r"):
        out[k] = []
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        Q, DO = _heads(t["q"], q0, lq, hd, F64), _heads(t["do"], q0, lq, hd, F64)
        K, V = _heads(t["k"], k0, lk, hd, F64), _heads(t["v"], k0, lk, hd, F64)
        add2 = torch.zeros(lk, dtype=F64) if t["add"] is None else (t["add"][b, :lk].to(F64) * LOG2E).clamp_min(-FLT_MAX)
        s2 = (LOG2E * scale) * (Q @ K.transpose(1, 2)) + add2
        m = s2.max(-1, keepdim=True).values
        e = torch.exp2(s2 - m)
        l = e.sum(-1, keepdim=True)
        p = e / l
        kp = torch.ones_like(p) if keep is None else keep[b].to(F64)
        Pp = cc * kp * p
        dPraw = DO @ V.transpose(1, 2)
        dP = cc * kp * dPraw
        r = (dP * p).sum(-1, keepdim=True)
        dS = scale * p * (dP - r)
        if exact:
            Pp, dS = Pp.to(BF16).to(F64), dS.to(BF16).to(F64)
        qs, ks = slice(q0, q0 + lq), slice(k0, k0 + lk)
        out["ctx"][qs], out["dq"][qs] = _rows(Pp @ V), _rows(dS @ K)
        out["dk"][ks], out["dv"][ks] = _rows(dS.transpose(1, 2) @ Q), _rows(Pp.transpose(1, 2) @ DO)
        out["m2"].append(m[..., 0])
        out["lse2"].append(m[..., 0] + torch.log2(l[..., 0]))
        out["inv"].append(1.0 / l[..., 0])
        out["r"].append(r[..., 0])
        if not bounds:
            continue
        E2 = (hd + 8) * EPS * (LOG2E * abs(scale) * (Q.abs() @ K.abs().transpose(1, 2)) + add2.abs())
        E2 = torch.where(add2 == -FLT_MAX, torch.zeros_like(E2), E2)
        E = E2 + EPS * ((s2 - m).abs() + 4.0)
        Ebar = (p * E).sum(-1, keepdim=True)
        rho = math.log(2.0) * (E + Ebar) + (lk + 8) * EPS
        out["tol_m"].append(E2.max(-1).values)
        out["tol_lse"].append(Ebar[..., 0] + (lk + 8) * EPS * LOG2E)
        E_dP = (hd + 8) * EPS * (DO.abs() @ V.abs().transpose(1, 2))
        E_r = (cc * kp * p * (E_dP + dPraw.abs() * rho)).sum(-1, keepdim=True) + (lk + 8) * EPS * (dP.abs() * p).sum(-1, keepdim=True)
        out["tol_r"].append(E_r[..., 0])
        E_dS = abs(scale) * (p * (cc * kp * E_dP + E_r + 3 * EPS * (dP.abs() + r.abs())) + rho * p * (dP - r).abs() + ETA * (dP.abs() + r.abs() + 1.0))
        rP = rho * Pp
        Va, Ka, Qa, DOa = V.abs(), K.abs(), Q.abs(), DO.abs()
        T = Pp @ Va
        out["B_ctx"][qs] = _rows(U16 * T + rP @ Va + (lk + 8) * EPS * T + ETA * cc * Va.sum(1, keepdim=True)) + ETA
        T = dS.abs() @ Ka
        out["B_dq"][qs] = _rows(U16 * T + E_dS @ Ka + (lk + 8) * EPS * T) + ETA
        T = dS.abs().transpose(1, 2) @ Qa
        out["B_dk"][ks] = _rows(U16 * T + E_dS.transpose(1, 2) @ Qa + (lq + 8) * EPS * T) + ETA
        T = Pp.transpose(1, 2) @ DOa
        out["B_dv"][ks] = _rows(U16 * T + rP.transpose(1, 2) @ DOa + (lq + 8) * EPS * T + ETA * cc * DOa.sum(1, keepdim=True)) + ETA
    return out


def ctx_dtype(c):
    return F16 if c["ctx_f16"] else BF16


def out_bound(c, ref, k):
    return ref["B_" + k] + rounding_term(ref[k], ctx_dtype(c) if k == "ctx" else BF16)


def gain(got, ref, bound):
    num = ((got.to(F64) - ref) * ref).sum()
    den = ((bound * ref) ** 2).sum().sqrt()
    return float(num / den) if float(den) > 0 else 0.0


def evaluate(c, ref, got):
    """got: ctx, dq, dk, dv [rows, D]; m2, inv, r lists per sequence of [heads, lq] -> {name: (worst ratio, z)}"""
    res = {}
    for k in ("ctx", "dq", "dk", "dv"):
        b = out_bound(c, ref, k)
        res[k] = (worst_ratio(got[k], ref[k], b), gain(got[k], ref[k], b))
    cat = lambda xs: torch.cat([x.to(F64).flatten() for x in xs])
    m, inv = cat(got["m2"]), cat(got["inv"])
    res["stats_m"] = (worst_ratio(m, cat(ref["m2"]), cat(ref["tol_m"])), 0.0)
    res["stats_lse"] = (worst_ratio(m - torch.log2(inv), cat(ref["lse2"]), cat(ref["tol_lse"])), 0.0)
    res["drow"] = (worst_ratio(cat(got["r"]), cat(ref["r"]), cat(ref["tol_r"])), 0.0)
    return res


def selector_expectation(c, t):
    """what the selector mode requires, stated without the reference: ctx, dv (fp32 sums of the selecting do rows), the row max"""
    ctx = torch.zeros(t["rows_q"], HEADS * c["hd"], dtype=F64)
    dv = torch.zeros(t["rows_k"], HEADS * c["hd"], dtype=F64)
    for (q0, lq, k0, lk, krows), s in zip(t["seqs"], t["sel"]):
        ctx[q0:q0 + lq] = t["v"][k0 + s].to(F64)
        dv[k0:k0 + krows].index_add_(0, s, t["do"][q0:q0 + lq].to(F64))
    m = float(torch.tensor(64.0 * c["hd"], dtype=F32) * torch.tensor(LOG2E, dtype=F32))
    return ctx, dv.to(BF16).to(F64), m


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def emulate(c, t, p_drop=0.0, keep=None):
    """The kernels' arithmetic in fp32 torch on the CPU with their rounding points: P' and dS to bf16, the outputs to bf16 / fp16."""
    hd, scale = c["hd"], t["scale"]
    D = HEADS * hd
    dsc = torch.tensor(1.0 / (1.0 - p_drop), dtype=F32) if p_drop else torch.tensor(1.0)
    sc2 = torch.tensor(scale, dtype=F32) * torch.tensor(LOG2E, dtype=F32)
    got = {k: torch.zeros(t["rows_q"] if k in ("ctx", "dq") else t["rows_k"], D, dtype=ctx_dtype(c) if k == "ctx" else BF16) for k in ("ctx", "dq", "dk", "dv")}
    got.update(m2=[], inv=[], r=[])
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        Q, DO = _heads(t["q"], q0, lq, hd, F32), _heads(t["do"], q0, lq, hd, F32)
        K, V = _heads(t["k"], k0, lk, hd, F32), _heads(t["v"], k0, lk, hd, F32)
        add2 = torch.zeros(lk) if t["add"] is None else (t["add"][b, :lk] * torch.tensor(LOG2E, dtype=F32)).clamp_min(-FLT_MAX)
        s2 = (Q @ K.transpose(1, 2)) * sc2 + add2
        m = s2.max(-1, keepdim=True).values
        e = torch.exp2(s2 - m)
        inv = 1.0 / e.sum(-1, keepdim=True)
        p = e * inv
        kp = torch.ones_like(p) if keep is None else keep[b].to(F32)
        Pp = (e * (inv * dsc) * kp).to(BF16).float()
        dP = (DO @ V.transpose(1, 2)) * kp
        r = (dP * p).sum(-1, keepdim=True) * dsc
        dS = (p * (dP * dsc - r) * scale).to(BF16).float()
        Pd = (p * dsc * kp).to(BF16).float()
        qs, ks = slice(q0, q0 + lq), slice(k0, k0 + lk)
        got["ctx"][qs] = round16(_rows(Pp @ V), ctx_dtype(c))
        got["dq"][qs] = _rows(dS @ K).to(BF16)
        got["dk"][ks] = _rows(dS.transpose(1, 2) @ Q).to(BF16)
        got["dv"][ks] = _rows(Pd.transpose(1, 2) @ DO).to(BF16)
        got["m2"].append(m[..., 0])
        got["inv"].append(inv[..., 0])
        got["r"].append(r[..., 0])
    return got


# ------------------------------------------------------------------------------------------------ exactness of the uniform mode
def exactness(c, t):
    """-> the largest sum |term| / quantum over the final sums of a uniform case (must stay below 2^24), asserting on the way that
    every term is a multiple of its sum's quantum.  n real keys, integer k, v, do, q = 0, scale a power of two:
      row sum   terms 1                          quantum 1          ctx, dv   terms v / n, do / n           quantum 1 / n
      dP        terms do v                       quantum 1          r         terms dP / n                  quantum 1 / n
      dq        terms bf16(dS) k, dS = scale (n dP - sum dP) / n^2, bf16 rounding keeps a multiple of a power of two a multiple of it
                                                 quantum scale / n^2"""
    hd, scale, worst = c["hd"], t["scale"], 0.0
    assert float(t["q"].float().abs().max()) == 0.0 and math.log2(scale) % 1 == 0
    for b, (q0, lq, k0, lk, krows) in enumerate(t["seqs"]):
        n = t["n_real"][b]
        assert n & (n - 1) == 0
        real = torch.ones(lk, dtype=torch.bool) if t["add"] is None else t["add"][b, :lk] == 0
        assert int(real.sum()) == n
        DO = _heads(t["do"], q0, lq, hd, F64)
        K, V = _heads(t["k"], k0, lk, hd, F64)[:, real], _heads(t["v"], k0, lk, hd, F64)[:, real]
        for x in (DO, K, V):
            assert bool((x == x.round()).all())
        dP = DO @ V.transpose(1, 2)
        dS = (scale * (dP - dP.sum(-1, keepdim=True) / n) / n).to(BF16).to(F64)
        qn = scale / n ** 2
        assert bool(((dS / qn) == (dS / qn).round()).all())
        sums = (float(n), float(V.abs().sum(1).max()), float(DO.abs().sum(1).max()), float((DO.abs() @ V.abs().transpose(1, 2)).max()),
                float(dP.abs().sum(-1).max()), float((dS.abs() @ K.abs()).max() / qn))
        worst = max(worst, *sums)
    return worst


# ------------------------------------------------------------------------------------------------ placement on the device
def _arena(rows, cols, ld, dtype, device, out=False):
    return Arena((rows, cols, ld, 0, 0, rows * ld), (1, 1), dtype, device, out=out)


def place(c, t, device):
    """the operands of a case in NaN-filled arenas, the outputs in sentinel-filled ones, in the case's row layout -> dict with the
    arenas (`arenas`: name -> Arena, outputs in `outs`), views ([rows, D]), pointers and leading dimensions"""
    hd = c["hd"]
    D = HEADS * hd
    rq, rk, lay = t["rows_q"], t["rows_k"], c["layout"]
    A, views, ptr, ld = {}, {}, {}, {}

    def cut(name, arena, col0):
        views[name] = arena.view[0, 0][:, col0:col0 + D]
        ptr[name] = arena.ptr() + col0 * 2
        ld[name] = arena.view.stride(2)

    for grp, out in ((("q", "k", "v"), False), (("dq", "dk", "dv"), True)):
        nq, nk, nv = grp
        if lay == "fused":
            A[nq] = _arena(rq, 3 * D, 3 * D, BF16, device, out)
            for i, n in enumerate(grp):
                cut(n, A[nq], i * D)
        elif lay == "cross":
            A[nq], A[nk] = _arena(rq, D, D, BF16, device, out), _arena(rk, 2 * D, 2 * D, BF16, device, out)
            cut(nq, A[nq], 0), cut(nk, A[nk], 0), cut(nv, A[nk], D)
        else:
            w = D + 8 if lay == "padded" else D
            for n, rows in ((nq, rq), (nk, rk), (nv, rk)):
                A[n] = _arena(rows, D, w, BF16, device, out)
                cut(n, A[n], 0)
    A["do"] = _arena(rq, D, D + 8 if lay == "padded" else D, BF16, device)
    cut("do", A["do"], 0)
    A["ctx"] = _arena(rq, D, D + 4 if c["ldo4"] else D, ctx_dtype(c), device, out=True)
    cut("ctx", A["ctx"], 0)
    nstat = HEADS * rq if t["packed"] else len(t["seqs"]) * HEADS * c["Lq"]
    A["stats"], A["drow"] = _arena(1, 2 * nstat, 2 * nstat, F32, device, out=True), _arena(1, nstat, nstat, F32, device, out=True)
    for n in ("q", "k", "v", "do"):
        views[n].copy_(t[n].to(device))
    if t["add"] is not None:
        A["add"] = _arena(t["add"].shape[0], c["Lk"], c["Lk"], F32, device)
        A["add"].view[0, 0].copy_(t["add"].to(device))
    outs = [n for n in ("dq", "dk", "dv", "ctx", "stats", "drow") if n in A]
    return dict(arenas=A, outs=outs, views=views, ptr=ptr, ld=ld, nstat=nstat)


def split_stats(c, t, x, width):
    """the flat stats / drow buffer -> list per sequence of [heads, lq(, width)]"""
    out = []
    if t["packed"]:
        x = x.view(HEADS, t["rows_q"], width)
        return [x[:, q0:q0 + lq] for (q0, lq, _, _, _) in t["seqs"]]
    x = x.view(len(t["seqs"]), HEADS, c["Lq"], width)
    for b in range(len(t["seqs"])):
        out.append(x[b])
    return out
