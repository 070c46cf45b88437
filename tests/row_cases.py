"""The case table of the LayerNorm and row-softmax instance tests, their input builders, float64 reference, bounds and fp32 emulation,
shared by test_row_cases_cpu.py (which proves that the table reaches all 26 instances, that the grid statement is the library's, that
the exact modes are exact, that the fp32 emulation stays inside the bounds and that nine wrong emulations do not) and
test_row_instances_gpu.py (which holds the kernels of csrc/layernorm.hip and the softmax kernels of csrc/elementwise.hip to the
reference on the device).  Dropout masks come from dropout_rule.py, never from a kernel's output.

INSTANCES (instance(c) and launch(c): an independent statement of the launchers' dispatch and geometry, held against the library's own
answer, mmdti_row_plan, by assert_declared_plan; SOURCE_LINES keeps the rounding points verbatim):
ln_fwd_kernel<NV> NV in 1, 2, 4, 8; ln_bwd_kernel<NV, DY_BF16> and ln_bwd_slab_kernel<NV, DY_BF16> (16); softmax_fwd_kernel<NV> and
softmax_bwd_kernel<NV>, NV in 1, 2, 4: 26.  det_fold_kernel runs behind every slab case and is held through dgamma, dbeta and colsum.
    LayerNorm  nv = ceil(D / 256), 3 -> 4, 5..7 -> 8;   softmax  nv = ceil(ld / 256), 3 -> 4
    LayerNorm backward: rows per wave = max(4, ceil(rows / (4 (3 if nv <= 2 else 2) 256))), grid = ceil(rows / (4 rpw))
    (the slab form runs in the deterministic mode when at least one of dgamma, dbeta, dx_colsum is given)

TABLE.  D = 4 (one live lane), 252 / 256 / 260 (one chunk short of, at, one lane into the second chunk), 512, 516 (NV = 3, served by
<4>), 1024, 1028 (NV = 5, served by <8>), 2044, 2048; rows = 1, 3 (less than a block), 17 (a second block whose last three waves own
no row), 37; rows_per_wave > 4 once per register class, (12293, 64) and (8197, 516).  Options rotate with the case number so that
every instance sees each: row_zero on every 5th row, forward dropout 0.1 / 0.35, y32 / y16 / both, y16 as fp16, fp32 / bf16 dy, dy_add,
dres, backward dropout, the bf16 copy with its own dropout site with and without dx_colsum, null dgamma / dbeta, eps 1e-5 / 1e-12.
The gradient buffers start at FILL (the kernels accumulate).  Softmax: (Lk, ld) of SM_SHAPES, rows = B heads Lq = 1, 5, 2 x 3 x 7;
NaN in the score and dp columns [Lk, ld); key_add none / -10000 or finfo.min on the last half of sequence 0's keys / finfo.min on
every key of the last sequence; dropout 0.1 on both outputs, or none with pd aliased to p.

MODES (LayerNorm)
  random  x = 0.5 + 2 randn
  offset  x = 64 + 2^-4 randn: |mean| / sigma = 2^10 -- what separates the two-pass variance from a one-pass one
  const   the row is all 3.0, eps = 1e-12, gamma = 0.5, dy constant along a row (small integers), no dropout: every partial sum is exact
          in any order, y32 EQUALS beta, the reference dx is exactly dres (0 without) and the device is held to the bound, which here
          is the fp32 summation term of m1 times rstd = 1e6
  sat     (forward) gamma scaled so that some outputs pass 65504: the fp16 copy holds exactly +-65504 there, the bf16 copy is not saturated

REFERENCE.  chain(c, t, dtype): one function, float64 (the reference) and float32 (the emulation).  Rounding points the reference
performs itself: eps, mean and rstd handed to the backward and the dropout scale 1.f / (1.f - p) are fp32 values; the softmax adds
key_add to the score in fp32 (finfo.min absorbs the score: such a row is uniform at 1 / Lk); 16-bit outputs are rounded to nearest
even (fp16 saturating); the bf16 copy's column sums add the ROUNDED values.  The backward reads the reference's own mean and rstd
(float64 rounded to fp32) and the softmax backward the reference's own bf16 p: no backward case depends on a forward kernel.

BOUNDS, from the reference alone; U = 2^-24.  n_s = nv + 9 is the depth of a row sum (3 adds inside a float4, nv accumulations, 6 DPP
steps); the softmax's is 4 nv + 6.
  mean   E_m = n_s U mean|x| + U |mean|            (the conditioning term: it is carried, times rstd, into every output)
  var    E_v = 2 E_m mean|x - mean| + (n_s + 4) U var;      rstd  E_r = rstd (E_v / (2 (var + eps)) + 3 U)
  xhat   E_h = (E_m + U |x - mean|) rstd + |x - mean| E_r + U |xhat|;   y  |gamma| E_h + 2 U (|xhat gamma| + |beta|), x dscale + U |y|
  backward: xhat from the given mean, rstd: 2 U |xhat|; d = dy (+ dy_add) (x dscale): 2 U |d|; dg = d gamma; m1, m2 row sums of depth
  n_s + 1, + 2; t = dg - m1 - xhat m2 with three roundings; dx = rstd t (+ dres).  dgamma, dbeta, colsum: (n + 8) U (sum |terms| + FILL)
  + sum of the terms' own L, n = rows per wave + 4 waves + the grid's partial sums.
  softmax: e = __expf(a), a = v - max: relative (4 |a| + 4) U (the subtraction, the scaling by log2 e, v_exp_f32's ulp) + 2^-126;
  sum: (4 nv + 6) U S; p = e / S: + 2 U.  pd: x dscale + U.  backward: d = dp dscale, dl = sum p d, ds = scale p (d - dl):
  scale (p (L_d + L_dl + U |d - dl|)) + 2 U |ds|  (p is given as stored: L_p = 0).
  A 16-bit output is a rounding point the reference rounds too: bound = L + one ulp of the rounded value.  colsum, a sum of such
  points: L + KAPPA sqrt(Q), Q = sum ulp^2 (gbf_cases' form) -- and, without any Q, `colsum_own`: the device's column sums against the
  float64 sums of the device's OWN bf16 copy, (n + 8) U (sum |terms| + FILL): that is the contract ("sums the ROUNDED values").
Two checks per output: worst |got - ref| / bound <= 1 and |gain| <= Z_MAX (attn_cases.gain)."""
import functools

import numpy as np
import torch

import dropout_rule as DR
from attn_cases import Z_MAX, gain  # noqa: F401
from gbf_cases import KAPPA
from gemm_cases import F64, SENT16, SENT32, Arena, worst_ratio  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U = 2.0 ** -24
ETA = 2.0 ** -126
FILL = 0.75
SEED = 0x5DEECE66D1234567
SITE_LN, SITE_LN2, SITE_SM = 11, 29, 7
FMIN = float(torch.finfo(F32).min)

SOURCE_LINES = {
    "layernorm.hip": (
        "const float mean = wave_sum(s) / (float)D;",
        "const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);",
        "const float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;",
        "Rand4 r = philox4(seed, site, ((uint64_t)row * D + (uint64_t)c * 4) >> 2);",
        "const Rand4 r = philox4(seed, site2, ((uint64_t)row * D + (uint64_t)c * 4) >> 2);",
        "if (zero) o[0] = o[1] = o[2] = o[3] = 0.f;",
        "pk.x = f2h_sat2(o[0], o[1]);",
        "pk.x = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);",
        "if (dx_colsum) {   // sums the ROUNDED values: exactly what a column-sum pass over dx_bf16 would add up",
        "if (cur.zero) d[0] = d[1] = d[2] = d[3] = 0.f;",
    ),
    "elementwise.hip": (
        "v[c][e] = (j + e < Lk) ? tv[e] + (ka ? ka[j + e] : 0.f) : -INFINITY;",
        "v[c][e] = __expf(v[c][e] - m);   // exp(-inf) = 0 in the pad columns",
        "const float inv = 1.0f / wave_sum(sum);",
        "const Rand4 r = philox4(seed, site, (uint64_t)(row * ld + j) >> 2);",
        "if (j + e >= Lk) p[c][e] = d[c][e] = 0.f;   // pad columns of dp are not data",
        "for (int e = 0; e < 4; ++e) o[e] = scale * p[c][e] * (d[c][e] - dl);",
    ),
}

class Bufs:
    """the operands (NaN arenas) and outputs (sentinel arenas) of one launch"""

    def __init__(self, device):
        self.outs, self.dev = {}, device

    def put(self, x, ld=None):
        """a [rows, cols] (or [n]) operand -> pointer; the columns [cols, ld) and the guards hold NaN"""
        if x is None:
            return 0
        x2 = x.view(1, -1) if x.dim() == 1 else x
        rows, cols = x2.shape
        ld = ld or cols
        a = Arena((rows, cols, ld, 0, 0, rows * ld), (1, 1), x.dtype, self.dev, out=False)
        a.view[0, 0].copy_(x2.to(self.dev))
        assert a.ptr() % 16 == 0
        self.outs.setdefault("_in", []).append(a)
        return a.ptr()

    def out(self, name, rows, cols, dtype, fill=None, on=True):
        if not on:
            return 0
        a = Arena((rows, cols, cols, 0, 0, rows * cols), (1, 1), dtype, self.dev, out=True)
        if fill is not None:
            a.view.fill_(fill)
        assert a.ptr() % 16 == 0
        self.outs[name] = a
        return a.ptr()

    def read(self, name, what):
        a = self.outs[name]
        assert a.outside_untouched() == 0, (what, name, "a store outside the output")
        x = a.view[0, 0].cpu()
        assert not bool(torch.isnan(x.float()).any()), (what, name, "NaN or sentinel where the contract gives a value")
        return x


# ------------------------------------------------------------------------------------------------ dispatch, stated independently
LN_DS = (4, 252, 256, 260, 512, 516, 1024, 1028, 2044, 2048)
LN_ROWS = (1, 3, 17, 37)
LN_BIG = ((12293, 64), (8197, 516))
SM_SHAPES = ((1, 8), (13, 16), (130, 136), (250, 256), (256, 256), (257, 264), (512, 512), (513, 520), (768, 768), (1021, 1024),
             (1024, 1024), (130, 152))
SM_ROWS = ((1, 1, 1), (1, 1, 5), (2, 3, 7))
KEY_ADDS = ("none", "m10000", "min_half", "min_all")


def ln_nv(D):
    n = -(-D // 256)
    return 4 if n == 3 else 8 if n >= 5 else n


def sm_nv(ld):
    n = -(-ld // 256)
    return 4 if n >= 3 else n


def ln_rpw(rows, D):
    return max(4, -(-rows // (4 * (3 if ln_nv(D) <= 2 else 2) * 256)))


def ln_grid(rows, D):
    return -(-rows // (4 * ln_rpw(rows, D)))


def tf(x):
    return "true" if x else "false"


def instance(c):
    k = c["kind"]
    if k == "ln_fwd":
        return f"ln_fwd_kernel<{ln_nv(c['D'])}>"
    if k == "ln_bwd":
        slab = c["det"] and (not c["nullg"] or (c["copy"] is not None and c["copy"][1]))
        return f"ln_bwd{'_slab' if slab else ''}_kernel<{ln_nv(c['D'])}, {tf(c['dybf'])}>"
    return f"softmax_{'fwd' if k == 'sm_fwd' else 'bwd'}_kernel<{sm_nv(c['ld'])}>"


ALL_INSTANCES = ([f"ln_fwd_kernel<{n}>" for n in (1, 2, 4, 8)] + [f"ln_bwd{s}_kernel<{n}, {b}>" for s in ("", "_slab") for n in (1, 2, 4, 8) for b in ("false", "true")]
                 + [f"softmax_{d}_kernel<{n}>" for d in ("fwd", "bwd") for n in (1, 2, 4)])

def launch(c, det=None):
    """the launches of the case: [(kernel, grid x, grid y, workgroup size, dynamic LDS bytes)] -- one wave per row, four rows per workgroup;
    the LayerNorm backward keeps [3][4 waves][D] floats in LDS and, in its slab form, is followed by the fold over D columns x 3 sums"""
    k = c["kind"]
    if k == "ln_fwd":
        return [(instance(c), -(-c["rows"] // 4), 1, 256, 0)]
    if k == "ln_bwd":
        name = instance(dict(c, det=c["det"] if det is None else det))
        first = [(name, ln_grid(c["rows"], c["D"]), 1, 256, 12 * c["D"] * 4)]
        return first + ([("det_fold_kernel", -(-c["D"] // 64), 3, 1024, 0)] if "_slab_" in name else [])
    return [(instance(c), -(-sm_rows(c) // 4), 1, 256, 0)]


# ------------------------------------------------------------------------------------------------ the library's answer (mmdti_row_plan)
PLAN_FAMILY = 6                      # MMDTI_PLAN_ROW
ENTRY = {"ln_fwd": 0, "ln_bwd": 1, "sm_fwd": 2, "sm_bwd": 3}
PTR = 0x7F0000001000                 # an address with every alignment; the queries test pointers for null and alignment only


def kernel_name(lib, family, row):
    return "det_fold_kernel" if row == -1 else lib.mmdti_plan_kernel_name(family, row).decode()


def read_plan(lib, family, words, derived):
    """the queries' word array -> dict(launches=[(kernel, grid x, grid y, workgroup size, LDS bytes)], **derived numbers)"""
    v = list(words)
    n = v[0]
    assert all(x == 0 for x in v[1 + 5 * n:11]), v                      # the launches a plan does not make are zero
    launches = [(kernel_name(lib, family, v[1 + 5 * i]),) + tuple(v[2 + 5 * i:6 + 5 * i]) for i in range(n)]
    return dict(launches=launches, **dict(zip(derived, v[11:])))


def row_plan(lib, kind, ptrs, rows_or_B, heads, Lq, Lk, D_or_ld, det=False, dybf=False, p=0.0, p2=0.0):
    """one call of mmdti_row_plan: ptrs in the entry's order (include/mmdti_hip.h)"""
    import ctypes
    out = (ctypes.c_longlong * 13)()
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    lib.mmdti_row_plan(ENTRY[kind], int(det), arr, rows_or_B, heads, Lq, Lk, D_or_ld, 1 if dybf else 0, p, p2, out)
    return read_plan(lib, PLAN_FAMILY, out, ("nv", "rpw"))


def case_ptrs(c):
    """the addresses the case hands to its entry point, null where the case gives none"""
    on = lambda x: PTR if x else 0
    if c["kind"] == "ln_fwd":
        return [PTR, PTR, PTR, on(c["outs"] in ("both", "y32")), on(c["outs"] in ("both", "y16"))]
    if c["kind"] == "ln_bwd":
        copy = c["copy"]
        return [PTR] * 6 + [on(not c["nullg"]), on(not c["nullg"]), on(copy is not None), on(copy is not None and copy[1])]
    return [PTR, PTR, PTR + 0x1000]


def library_plan(lib, c, det=None):
    k = c["kind"]
    if k.startswith("ln"):
        p2 = c["copy"][0] if k == "ln_bwd" and c["copy"] is not None else 0.0
        return row_plan(lib, k, case_ptrs(c), c["rows"], 0, 0, 0, c["D"], det=c.get("det", False) if det is None else det, dybf=c.get("dybf", False), p=c["p"], p2=p2)
    return row_plan(lib, k, case_ptrs(c), c["B"], c["heads"], c["Lq"], c["Lk"], c["ld"], p=c["p"])


def declared_plan(c, det=None):
    """what the case is declared to launch, from instance() and launch(): every field of the library's plan"""
    k = c["kind"]
    return dict(launches=launch(c, det), nv=sm_nv(c["ld"]) if k.startswith("sm") else ln_nv(c["D"]), rpw=ln_rpw(c["rows"], c["D"]) if k == "ln_bwd" else 0)


def assert_declared_plan(lib, c):
    got, want = library_plan(lib, c), declared_plan(c)
    assert got == want, (case_id(c), got, want)
    return got


# ------------------------------------------------------------------------------------------------ the table
CASES = []


def add(kind, **kw):
    c = dict(kind=kind, i=len(CASES), **kw)
    CASES.append(c)
    return c


#               rows = 1     3        17        37           (per D of an instance, in turn)
LN_FWD_MODES = (("random", "offset", "const", "sat"), ("random", "sat", "random", "offset"), ("random", "const", "sat", "random"))


def _ln_fwd(rows, D, j, mode=None):
    """j: the case's number within its instance -- the options rotate with it"""
    mode = mode or LN_FWD_MODES[(j // 4) % 3][LN_ROWS.index(rows)]
    p = 0.0 if mode == "const" else (0.0, 0.1, 0.35)[j % 3]
    k = len([c for c in CASES if c["kind"] == "ln_fwd" and ln_nv(c["D"]) == ln_nv(D) and c["mode"] in ("random", "offset")])
    outs = ("both", "y16", "y32")[k % 3] if mode not in ("sat", "const") else "both"
    add("ln_fwd", rows=rows, D=D, mode=mode, rz=j % 2 == 1, p=p, outs=outs, f16=(j // 2) % 2 == 1, eps=1e-12 if mode == "const" or j % 5 == 4 else 1e-5)


#          mode      dy_add dres   rz     p     copy           nullg  eps
LN_BWD_OPTS = (("random", True, True, True, 0.1, (0.1, True), False, 1e-5),
               ("offset", False, False, False, 0.0, None, True, 1e-12),
               ("const", True, False, True, 0.0, (0.0, True), False, 1e-12),
               ("random", False, True, False, 0.35, (0.35, False), False, 1e-12),
               ("offset", True, True, True, 0.1, (0.0, False), False, 1e-5),
               ("const", False, True, False, 0.0, None, False, 1e-12))


def _ln_bwd(rows, D, j, dybf, det, mode=None):
    m, dy_add, dres, rz, p, copy, nullg, eps = LN_BWD_OPTS[j % 6]
    if det and j % 6 in (1, 2):          # (in the mode, null dgamma and dbeta reach the slab kernel only with dx_colsum)
        copy = LN_BWD_OPTS[3 - j % 6][5]
    if mode is not None and mode != m:
        m, eps = mode, 1e-5
    add("ln_bwd", rows=rows, D=D, mode=m, dybf=dybf, det=det, dy_add=dy_add, dres=dres, rz=rz, p=p, copy=copy, nullg=nullg, eps=eps)


def _build():
    j = {}
    for D in LN_DS:
        for rows in LN_ROWS:
            n = j.setdefault(ln_nv(D), 0)
            _ln_fwd(rows, D, n)
            j[ln_nv(D)] = n + 1
    for rows, D in LN_BIG:
        _ln_fwd(rows, D, 7 if D == 64 else 13, "random")
    j = {}
    for D in LN_DS:
        for dybf in (False, True):
            for det in (False, True):
                for rows in (17, 37) + (((3,) if det else (1,)) if dybf == det else ()):
                    key = (ln_nv(D), dybf, det)
                    n = j.setdefault(key, 0)
                    _ln_bwd(rows, D, n, dybf, det)
                    j[key] = n + 1
    for n, ((rows, D), dybf, det) in enumerate((((12293, 64), False, False), ((12293, 64), True, True), ((8197, 516), True, False), ((8197, 516), False, True))):
        _ln_bwd(rows, D, (0, 3, 4, 0)[n], dybf, det, "random")
    i = 0
    for Lk, ld in SM_SHAPES:
        for B, heads, Lq in SM_ROWS:
            ka = KEY_ADDS[i % 4]
            add("sm_fwd", Lk=Lk, ld=ld, B=B, heads=heads, Lq=Lq, key_add=ka, p=(0.1, 0.0)[(i // 4 + i) % 2])
            add("sm_bwd", Lk=Lk, ld=ld, B=B, heads=heads, Lq=Lq, key_add=ka, p=(0.0, 0.1, 0.1)[i % 3], scale=(1.0, 0.125, 0.17677669)[i % 3])
            i += 1


_build()


def case_id(c):
    k = c["kind"]
    if k.startswith("sm"):
        return f"{k}-Lk{c['Lk']}-ld{c['ld']}-r{c['B'] * c['heads'] * c['Lq']}-{c['key_add']}-p{c['p']}"
    f = [k, f"{c['rows']}x{c['D']}", c["mode"]]
    if k == "ln_fwd":
        f += [c["outs"], "f16" if c["f16"] else "bf16"]
    else:
        f += ["dybf" if c["dybf"] else "dy32", "det" if c["det"] else "atomic"]
    return "-".join(f) + f"-{c['i']}"


def sm_rows(c):
    return c["B"] * c["heads"] * c["Lq"]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(c):
    return torch.Generator().manual_seed(7919 * c["i"] + 13)


def _mask(keep):
    return torch.from_numpy(np.ascontiguousarray(keep))


def ln_x(c, g):
    rows, D, mode = c["rows"], c["D"], c["mode"]
    if mode == "offset":
        return 64.0 + 2.0 ** -4 * torch.randn(rows, D, generator=g)
    if mode == "const":
        return torch.full((rows, D), 3.0)
    return 0.5 + 2.0 * torch.randn(rows, D, generator=g)


def make_inputs(c, salt=0):
    g = _gen(c)
    k = c["kind"]
    rn = lambda *s: torch.randn(*s, generator=g)
    if k.startswith("ln"):
        rows, D = c["rows"], c["D"]
        t = dict(x=ln_x(c, g), gamma=1.0 + 0.2 * rn(D), beta=0.3 * rn(D), eps32=float(np.float32(c["eps"])))
        if c["mode"] == "const":
            t["gamma"] = torch.full((D,), 0.5)
        if c["mode"] == "sat":
            t["gamma"] = t["gamma"] * 30000.0
        t["rz"] = (torch.arange(rows) % 5 == 0) if c["rz"] else None
        t["keep"] = _mask(DR.keep_rows(SEED, SITE_LN, rows, D, c["p"], salt=salt)) if c["p"] > 0 else None
        t["sc"] = DR.dscale(c["p"])
        if k == "ln_bwd":
            if c["mode"] == "const":
                dy = ((torch.arange(rows) % 5) - 2.0).view(rows, 1).expand(rows, D).contiguous()
                da = torch.ones(rows, D)
            else:
                dy, da = rn(rows, D), 0.5 * rn(rows, D)
            t["dy"] = dy.to(BF16) if c["dybf"] else dy
            t["dy_add"] = da if c["dy_add"] else None
            t["dres"] = rn(rows, D) if c["dres"] else None
            fw = ln_fwd_chain(dict(c, kind="ln_fwd", f16=False), dict(t, keep=None, rz=None), F64, bounds=False)
            t["mean32"], t["rstd32"] = fw["mean"].to(F32), fw["rstd"].to(F32)
            if c["copy"] is not None:
                p2 = c["copy"][0]
                t["keep2"] = _mask(DR.keep_rows(SEED, SITE_LN2, rows, D, p2, salt=salt)) if p2 > 0 else None
                t["sc2"] = DR.dscale(p2)
        return t
    rows, Lk, ld, B = sm_rows(c), c["Lk"], c["ld"], c["B"]
    t = dict(s=3.0 * rn(rows, Lk))
    ka = None
    if c["key_add"] != "none":
        ka = torch.zeros(B, Lk)
        if c["key_add"] == "min_all":
            ka[B - 1, :] = FMIN
        else:
            ka[0, Lk // 2:] = -10000.0 if c["key_add"] == "m10000" else FMIN
    t["key_add"] = ka
    t["keep"] = _mask(DR.keep_rows(SEED, SITE_SM, rows, Lk, c["p"], ld=ld, salt=salt)) if c["p"] > 0 else None
    t["sc"] = DR.dscale(c["p"])
    if k == "sm_bwd":
        fw = sm_fwd_chain(dict(c, kind="sm_fwd"), dict(t, keep=None), F64, bounds=False)
        t["p16"] = fw["p"].to(BF16)
        t["dp"] = rn(rows, Lk)
    return t


# ------------------------------------------------------------------------------------------------ the chains
def ulp16(x16):
    """one ulp of a bf16 / fp16 value (the subnormal spacing at 0)"""
    mant, emin = (7, -126) if x16.dtype == BF16 else (10, -14)
    a = x16.abs().to(F64).clamp(min=2.0 ** emin)
    return torch.exp2(torch.floor(torch.log2(a)) - mant)


def round16(v, dtype):
    """to nearest even; fp16 saturates at +-65504 (f2h_sat2)"""
    if dtype == F16:
        v = v.clamp(-65504.0, 65504.0)
    return v.to(dtype)


LN_MUTATIONS = ("one_pass", "eps_outside", "unbiased", "rz_first", "dgamma_undropped", "colsum_unrounded")
SM_MUTATIONS = ("norm_ld", "dl_before_dropout")


def ln_fwd_chain(c, t, dt=F64, mut=None, bounds=True):
    f = lambda v: v.to(dt)
    x, g, b = f(t["x"]), f(t["gamma"]), f(t["beta"])
    D, rz = c["D"], t["rz"]
    eps = torch.tensor(t["eps32"], dtype=dt)
    if mut == "rz_first" and rz is not None:
        x = x.masked_fill(rz.view(-1, 1), 0.0)
    mean = x.sum(1, keepdim=True) / D
    xc = x - mean
    if mut == "one_pass":
        var = (x * x).sum(1, keepdim=True) / D - mean * mean
    else:
        var = (xc * xc).sum(1, keepdim=True) / ((D - 1) if mut == "unbiased" else D)
    rstd = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    xh = xc * rstd
    o = xh * g + b
    sc = torch.tensor(t["sc"], dtype=dt)
    if t["keep"] is not None:
        o = torch.where(t["keep"], o * sc, torch.zeros_like(o))
    if rz is not None:
        o = o.masked_fill(rz.view(-1, 1), 0.0)
    d16 = F16 if c["f16"] else BF16
    out = dict(mean=mean[:, 0], rstd=rstd[:, 0], y32=o, y16=round16(o, d16))
    if dt == F64 and bounds:
        ns = ln_nv(D) + 9
        Em = ns * U * x.abs().mean(1, keepdim=True) + U * mean.abs()
        Ev = 2 * Em * xc.abs().mean(1, keepdim=True) + (ns + 4) * U * var
        Er = rstd * (Ev / (2 * (var + eps)) + 3 * U)
        Eh = (Em + U * xc.abs()) * rstd + xc.abs() * Er + U * xh.abs()
        Eo = g.abs() * Eh + 2 * U * ((xh * g).abs() + b.abs())
        if t["keep"] is not None:
            Eo = torch.where(t["keep"], Eo * sc + U * o.abs(), torch.zeros_like(o))
        if rz is not None:
            Eo = Eo.masked_fill(rz.view(-1, 1), 0.0)
        out.update(B_mean=Em[:, 0], B_rstd=Er[:, 0], B_y32=Eo, B_y16=Eo + ulp16(out["y16"]))
    return out


def ln_acc_count(c):
    return ln_rpw(c["rows"], c["D"]) + 4 + ln_grid(c["rows"], c["D"]) + 8


def ln_bwd_chain(c, t, dt=F64, mut=None, bounds=True):
    f = lambda v: v.to(dt)
    x, g = f(t["x"]), f(t["gamma"])
    D, rz = c["D"], t["rz"]
    mean, rstd = f(t["mean32"]).view(-1, 1), f(t["rstd32"]).view(-1, 1)
    d = f(t["dy"])
    if t["dy_add"] is not None:
        d = d + f(t["dy_add"])
    d_raw = d
    sc = torch.tensor(t["sc"], dtype=dt)
    if t["keep"] is not None:
        d = torch.where(t["keep"], d * sc, torch.zeros_like(d))
    if rz is not None:
        d = d.masked_fill(rz.view(-1, 1), 0.0)
        d_raw = d_raw.masked_fill(rz.view(-1, 1), 0.0)
    xh = (x - mean) * rstd
    tg = (d_raw if mut == "dgamma_undropped" else d) * xh
    dg = d * g
    m1 = dg.sum(1, keepdim=True) / D
    m2 = (dg * xh).sum(1, keepdim=True) / D
    dx = rstd * (dg - m1 - xh * m2)
    if t["dres"] is not None:
        dx = dx + f(t["dres"])
    out = dict(dx=dx)
    if not c["nullg"]:
        out.update(dgamma=tg.sum(0), dbeta=d.sum(0))
    if c["copy"] is not None:
        o = dx
        sc2 = torch.tensor(t["sc2"], dtype=dt)
        if t["keep2"] is not None:
            o = torch.where(t["keep2"], o * sc2, torch.zeros_like(o))
        out["dx16"] = o.to(BF16)
        if c["copy"][1]:
            out["colsum"] = (o if mut == "colsum_unrounded" else out["dx16"].to(dt)).sum(0)
    if dt == F64 and bounds:
        ns, n = ln_nv(D) + 9, ln_acc_count(c)
        Ld = 2 * U * d.abs()
        Eh = 2 * U * xh.abs()
        Ldg = g.abs() * Ld + U * dg.abs()
        E1 = (ns + 1) * U * dg.abs().mean(1, keepdim=True) + Ldg.mean(1, keepdim=True)
        E2 = (ns + 2) * U * (dg * xh).abs().mean(1, keepdim=True) + (Ldg * xh.abs() + dg.abs() * Eh).mean(1, keepdim=True)
        Et = Ldg + E1 + xh.abs() * E2 + m2.abs() * Eh + 3 * U * (dg.abs() + m1.abs() + (xh * m2).abs())
        Edx = rstd * Et + U * dx.abs() + (U * (dx.abs() + f(t["dres"]).abs()) if t["dres"] is not None else 0.0)
        out["B_dx"] = Edx
        acc = lambda terms, L: n * U * (terms.abs().sum(0) + FILL) + L.sum(0)
        if not c["nullg"]:
            out["B_dgamma"] = acc(tg, d.abs() * Eh + xh.abs() * Ld + U * tg.abs())
            out["B_dbeta"] = acc(d, Ld)
        if c["copy"] is not None:
            Eo = Edx
            if t["keep2"] is not None:
                Eo = torch.where(t["keep2"], Edx * sc2 + U * o.abs(), torch.zeros_like(o))
            u16 = ulp16(out["dx16"])
            out["B_dx16"] = Eo + u16
            if c["copy"][1]:
                out["B_colsum"] = acc(out["dx16"].to(dt), Eo) + KAPPA * torch.sqrt((u16 * u16).sum(0))
    return out


def colsum_own(c, dx16, colsum):
    """the device's (or an emulation's) column sums against the float64 sums of its OWN bf16 copy -> (ratio, gain)"""
    v = dx16.to(F64)
    ref, b = v.sum(0), ln_acc_count(c) * U * (v.abs().sum(0) + FILL)
    return worst_ratio(colsum.to(F64), ref, b), gain(colsum.to(F64), ref, b)


def sm_scores(c, t, dt):
    """v = s + key_add, added in fp32 (a rounding point of the kernel: finfo.min absorbs the score)"""
    v = t["s"]
    if t["key_add"] is not None:
        v = v + t["key_add"].repeat_interleave(c["heads"] * c["Lq"], 0)
    return v.to(dt)


def sm_fwd_chain(c, t, dt=F64, mut=None, bounds=True):
    v = sm_scores(c, t, dt)
    Lk, ld = c["Lk"], c["ld"]
    if mut == "norm_ld":                                            # the pad columns take part, as scores of 0
        v = torch.cat([v, torch.zeros(v.shape[0], ld - Lk, dtype=dt)], 1)
    m = v.max(1, keepdim=True).values
    a = v - m
    e = torch.exp(a)
    S = e.sum(1, keepdim=True)
    p = (e * (1.0 / S))[:, :Lk]
    sc = torch.tensor(t["sc"], dtype=dt)
    pd = p if t["keep"] is None else torch.where(t["keep"], p * sc, torch.zeros_like(p))
    out = dict(p=p.to(BF16), pd=pd.to(BF16))
    if dt == F64 and bounds:
        rel = (4 * a.abs() + 4) * U
        ES = (4 * sm_nv(ld) + 6) * U * S + (e * rel).sum(1, keepdim=True) + Lk * ETA
        Lp = p * (rel + ES / S + 2 * U) + ETA / S
        Lpd = Lp if t["keep"] is None else torch.where(t["keep"], Lp * sc + U * pd, torch.zeros_like(p))
        out.update(B_p=Lp + ulp16(out["p"]), B_pd=Lpd + ulp16(out["pd"]))
    return out


def sm_bwd_chain(c, t, dt=F64, mut=None, bounds=True):
    p, dp = t["p16"].to(dt), t["dp"].to(dt)
    sc, scale = torch.tensor(t["sc"], dtype=dt), torch.tensor(float(np.float32(c["scale"])), dtype=dt)
    d = dp if t["keep"] is None else torch.where(t["keep"], dp * sc, torch.zeros_like(dp))
    dl = (p * (dp if mut == "dl_before_dropout" else d)).sum(1, keepdim=True)
    o = scale * p * (d - dl)
    out = dict(ds=o.to(BF16))
    if dt == F64 and bounds:
        Ld = U * d.abs()
        Edl = (4 * sm_nv(c["ld"]) + 7) * U * (p * d).abs().sum(1, keepdim=True) + (p * Ld).sum(1, keepdim=True)
        out["B_ds"] = scale * p * (Ld + Edl + U * (d - dl).abs()) + 2 * U * o.abs() + ulp16(out["ds"])
    return out


CHAIN = {"ln_fwd": ln_fwd_chain, "ln_bwd": ln_bwd_chain, "sm_fwd": sm_fwd_chain, "sm_bwd": sm_bwd_chain}
OUTPUTS = {"ln_fwd": ("mean", "rstd", "y32", "y16"), "ln_bwd": ("dx", "dgamma", "dbeta", "dx16", "colsum"), "sm_fwd": ("p", "pd"), "sm_bwd": ("ds",)}


def chain(c, t, dt=F64, mut=None):
    return CHAIN[c["kind"]](c, t, dt, mut)


def emulate(c, t, mut=None):
    return chain(c, t, F32, mut)


def evaluate(c, ref, got):
    """got: {name: tensor shaped as the reference's} -> {name: (worst ratio, gain)}; 16-bit outputs against the ROUNDED reference"""
    res = {}
    for k in OUTPUTS[c["kind"]]:
        if k not in got or k not in ref:
            continue
        r, b = ref[k].to(F64), ref["B_" + k]
        res[k] = (worst_ratio(got[k].to(F64), r, b), gain(got[k].to(F64), r, b) if r.numel() >= 64 else 0.0)
    if "colsum" in got and "dx16" in got:
        res["colsum_own"] = colsum_own(c, got["dx16"], got["colsum"])
    return res


def saturated(c, ref):
    """(mask, expected): the fp16 outputs that must hold exactly +-65504 (the reference passes it by more than its bound)"""
    o = ref["y32"]
    m = o.abs() - ref["B_y32"] >= 65504.0
    return m, torch.sign(o) * 65504.0


@functools.lru_cache(maxsize=4)
def prepared(i):
    """(inputs, reference) of CASES[i]: computed once, shared by the tests that run the case"""
    c = CASES[i]
    t = make_inputs(c)
    return t, chain(c, t)
