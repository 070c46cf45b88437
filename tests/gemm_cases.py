"""The case table of the GEMM instance tests and their float64 reference, shared by test_gemm_cases_cpu.py (which proves with plan
queries that the table reaches every instance of csrc/gemm.hip's launch table, and pins the reference against an fp32 evaluation of
the same formula) and test_gemm_instances_gpu.py (which holds every instance to the reference on the device).

A case is gemm_plan_helpers.case(...) plus
  opts    the option setting it runs under (mmdti_set_option names; restored to test_gemm_plan_cpu.DEFAULTS afterwards),
  kernel  the instance it DECLARES (the plan must name it, on the CPU and again before the launch),
  expect  further plan fields it declares (mstep, slabs, stream_c, arowsum, grid_x),
  ldr / ld_aux / drop   what the helper's argument list has no word for.

The reference is C = epilogue(alpha * op(A) . op(B)^T) in float64 as epi_elem of gemm.hip spells it, on the operands exactly as
stored (an fp16 B of a `bcvt` case rounded to bf16, to nearest even, first).

EXACT inputs: integers in [-r, r] with r = min(cap, floor(sqrt(2^23 / (K * mag)))) (cap 255 for bf16, 2047 for fp16 operands; mag
collects |alpha| > 1, the dropout scale and the aux multiplier), integer bias / residual / C0 below 2^20, alpha and beta powers
of two: every product, every partial sum in any order and every epilogue value is a multiple of `gran` (0.5 or 1) below
2^24 * gran, which fp32 holds exactly -- whatever the tiling, split or atomic order, the output must EQUAL the reference.
RANDOM inputs: randn rounded to the operand type; held to the worst-case bound of fp32 summation in any order (bound())."""
import ctypes
import math

import torch

from gemm_plan_helpers import ACT_GELU, ACT_GELU_BWD, ACT_GELU_G, ACT_MUL_AUX, ACT_NONE, case, kernel_name, r8  # noqa: F401

F64 = torch.float64
GUARD_ROWS = 256                      # NaN / sentinel rows in front of and behind every operand and output (one tile of the largest kernel)
SENT32, SENT16 = 0x7FC05A5A, 0x7FC5   # sentinel bit patterns: NaN as fp32, as bf16 and as fp16
SEED, SITE = 0x5EED1234, 7

# |device gelu_erf - float64 gelu| and |device gelu_erf_grad - float64 gelu'| over [-8, 8], measured on MI355X by
# test_gemm_instances_gpu.py::test_gelu_error_G (profiles/gemm_instances.json "gelu_G"); the GELU bands carry four times these.
# A priori both are below GELU_G_CAP: the erf approximation (Abramowitz-Stegun 7.1.26) is within 1.5e-7, times |x| / 2 <= 4, plus
# a few fp32 roundings of values <= 8.
GELU_G_MEASURED = {"gelu": 4.51e-7, "gelu_grad": 2.28e-7}
GELU_G_CAP = 1e-5


# ------------------------------------------------------------------------------------------------ the table
def _name(fam, c, fast=None):
    b = lambda v: "true" if v else "false"
    ta, tb, f16, bc = c["tA"], c["tB"], c["ab16"], c["bcvt"]
    if fam == "reg":
        return f"gemm_bf16_kernel<{b(ta)}, {b(tb)}, {b(fast)}, {b(f16)}, {b(bc)}>"
    if fam in ("glds0", "dbuf", "deep"):
        return f"gemm_glds_kernel<{b(ta)}, {b(tb)}, {('glds0', 'dbuf', 'deep').index(fam)}, {b(f16)}, {b(bc)}>"
    if fam == "tall":
        return f"gemm_glds_tall_kernel<{b(tb)}, {b(f16)}>"
    if fam == "small":
        return f"gemm_small_kernel<{b(tb)}, {b(f16)}>"
    assert fam == "big"
    return f"gemm_big_kernel<{b(ta)}, {b(tb)}, {b(f16)}, {b(bc)}, false>"


CASES = []


def add(label, fam, opts, M, N, K, fast=None, expect=None, ldr=None, ld_aux=None, drop=0.0, modes=("exact", "random"), big_ld=False, **kw):
    c = case(M, N, K, **kw)
    c.update(label=f"{fam}{'-fast' if fast else ''}:{label}", fam=fam, opts=dict(opts), kernel=_name(fam, c, fast), expect=dict(expect or {}),
             ldr=ldr, ld_aux=ld_aux, drop=drop, modes=tuple(modes), big_ld=big_ld)
    CASES.append(c)
    return c


def _epilogues(fam, opts, M, N, K, fast=None, tA=0, tB=0, colsum=True, splitk=0, gelu=True, stream=True, ab16=True, expect=None):
    """the cases every family gets at one of its shapes (M, N, K): the linear epilogue at once, in three output types and with every
    leading dimension off its natural value; colsum; bias and alpha under a K split; the aux multiply; dropout; GELU; streaming
    stores"""
    e = dict(expect or {})
    kw = dict(fast=fast, tA=tA, tB=tB, expect=e)
    lda, ldb = r8(M if tA else K) + 8, r8(N if tB else K) + 16
    for out, ldc in (("f32", N + 4), ("bf16", N + 8), ("f16", N + 8)):
        add(f"linear-{out}", fam, opts, M, N, K, out=out, alpha=0.5, beta=1.0 if out == "f32" else 0.0, bias=1, residual=1, lda=lda, ldb=ldb,
            ldc=ldc, ldr=N + 12, **kw)
    if ab16 and not tA and not tB:
        add("linear-ab16", fam, opts, M, N, K, ab16=1, out="f16", alpha=0.5, bias=1, residual=1, ldc=N + 8, ldr=N + 4, **kw)
    if colsum:
        add("colsum-f32", fam, opts, M, N, K, out="f32", colsum=1, bias=1, **kw)
        add("colsum-bf16", fam, opts, M, N, K, out="bf16", colsum=1, **kw)
    add("mulaux", fam, opts, M, N, K, out="f32", act=ACT_MUL_AUX, aux_in=1, ld_aux=N + 8, bias=1, **kw)
    add("dropout", fam, opts, M, N, K, out="f32", bias=1, drop=0.5, **kw)
    add("dropout-bf16", fam, opts, M, N, K, out="bf16", bias=1, drop=0.5, **kw)
    if gelu:
        add("gelu", fam, opts, M, N, K, out="bf16", bias=1, act=ACT_GELU, aux_out=1, ld_aux=N + 8, modes=("random",), **kw)
        add("gelu_g", fam, opts, M, N, K, out="f32", bias=1, act=ACT_GELU_G, aux_out=1, modes=("random",), **kw)
        add("gelu_bwd", fam, opts, M, N, K, out="bf16", act=ACT_GELU_BWD, aux_in=1, modes=("random",), **kw)
    if stream:
        so = dict(opts, gemm_stream_mb=0)
        add("stream-f32", fam, so, M, N, K, out="f32", bias=1, fast=fast, tA=tA, tB=tB, expect=dict(e, stream_c=1))
        add("stream-bf16", fam, so, M, N, K, out="bf16", residual=1, fast=fast, tA=tA, tB=tB, expect=dict(e, stream_c=1))
        add("stream-beta", fam, so, M, N, K, out="f32", beta=1.0, fast=fast, tA=tA, tB=tB, expect=dict(e, stream_c=0))
    if splitk:
        add(f"sk{splitk}-bias-alpha2", fam, opts, M, N, K, out="atomic", sk=splitk, alpha=2.0, bias=1, residual=1, ldr=N + 4, **kw)


def _build():
    D = {}
    tt = ((0, 0), (0, 1), (1, 0), (1, 1))
    # ---- the issue's table ------------------------------------------------------------------------------------------------
    for ta, tb in tt:
        add("table", "reg", D, 130, 50, 72, tA=ta, tB=tb, out="f32")
    add("table", "reg", D, 130, 56, 72, ab16=1, out="f16")
    add("table", "reg", D, 136, 72, 200, tA=1, tB=1, sk=2, out="atomic", bcvt=1)
    add("table-arowsum", "dbuf", D, 264, 136, 192, tA=1, tB=1, sk=3, out="atomic", arowsum=1, expect=dict(arowsum=1))
    add("table-arowsum-pass", "reg", D, 264, 136, 200, tA=1, tB=1, sk=3, out="atomic", arowsum=1, expect=dict(arowsum=2))
    add("table", "dbuf", D, 264, 136, 192, tA=1, tB=1, sk=3, out="atomic", bcvt=1)
    for kw in (dict(tB=0), dict(tB=1), dict(ab16=1, out="f16")):
        add("table", "small", D, 200, 136, 320, **kw)
        add("table", "tall", D, 4500, 4096, 64, expect=dict(mstep=141, grid_x=1024), **kw)
    G0 = {"gemm_glds": 0}
    for ta, tb in tt:
        add("table", "reg", G0, 264, 136, 192, fast=True, tA=ta, tB=tb)
    add("table", "reg", G0, 264, 136, 192, fast=True, ab16=1, out="f16")
    add("table", "reg", G0, 264, 136, 192, fast=True, tA=1, tB=1, sk=3, out="atomic", bcvt=1, arowsum=1, expect=dict(arowsum=2))
    S0D0, S0, G3, B2 = {"gemm_small": 0, "gemm_deep": 0}, {"gemm_small": 0}, {"gemm_glds": 3}, {"gemm_big": 2}
    for ta, tb in tt:
        add("table", "glds0", S0D0, 264, 136, 320, tA=ta, tB=tb)
        add("table", "deep", S0, 264, 136, 320, tA=ta, tB=tb)
        add("table", "dbuf", G3, 264, 136, 320, tA=ta, tB=tb)
        add("table", "big", B2, 256, 512, 192, tA=ta, tB=tb)
    add("table", "glds0", S0D0, 264, 136, 320, ab16=1, out="f16")
    add("table", "deep", S0, 264, 136, 320, ab16=1, out="f16")
    add("table", "big", B2, 256, 512, 192, ab16=1, out="f16")
    add("table-bcvt-arowsum", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", bcvt=1, arowsum=1, expect=dict(arowsum=1, slabs=0))
    add("table-slabs", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", ws=4 * 256 * 512 * 4, expect=dict(slabs=1))
    add("table-atomics", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", expect=dict(slabs=0))

    # ---- edges, per family that admits them ---------------------------------------------------------------------------------
    # register-staged, predicated form: every K tail, M and N below a chunk, scalar epilogue, ragged k-major chunks
    for K in (8, 24, 56, 72, 120):                                                   # K < 64; K % 64 in {8, 56}
        for ta, tb in tt:
            add(f"K{K}", "reg", D, 129, 65, K, tA=ta, tB=tb, out="f32")
    add("K200-bcvt-sk1", "reg", D, 129, 65, 200, tA=1, tB=1, out="atomic", bcvt=1)
    add("K56-ab16", "reg", D, 129, 72, 56, ab16=1, out="f16")
    for ta, tb in tt:
        add("M4", "reg", D, 4, 257, 64, tA=ta, tB=tb, out="f32")
        add("N4", "reg", D, 257, 4, 64, tA=ta, tB=tb, out="bf16")
    add("tA-M%8", "reg", D, 260, 256, 128, tA=1, out="f32")
    add("tB-N%8", "reg", D, 256, 260, 128, tB=1, out="bf16")
    add("N%8-f16out", "reg", D, 129, 50, 72, out="f16", bias=1)
    add("ldc%4", "reg", D, 130, 64, 72, out="f32", ldc=65)
    _epilogues("reg", D, 130, 56, 72, ab16=True, splitk=2)                            # vector epilogue on the predicated form
    _epilogues("reg", D, 130, 50, 72, tB=1, colsum=False, stream=False, ab16=False)   # scalar epilogue (N % 8 != 0), k-major B
    add("dropout-scalar", "reg", D, 128, 50, 72, out="f32", bias=1, drop=0.5)         # same element counters as dropout-vector below
    add("dropout-vector", "reg", D, 100, 64, 72, out="f32", bias=1, drop=0.5)
    # register-staged, bare loads (gemm_glds = 0)
    for K in (64, 192, 320):
        for ta, tb in tt:
            add(f"K{K}", "reg", G0, 136 if ta else 129, 264 if tb else 257, K, fast=True, tA=ta, tB=tb, out="f32")
    add("M8N8", "reg", G0, 8, 8, 64, fast=True, out="f32")
    add("N%8", "reg", G0, 257, 50, 64, fast=True, out="f32", bias=1)
    add("ldc%4", "reg", G0, 257, 64, 64, fast=True, out="f32", ldc=67)
    _epilogues("reg", G0, 256, 512, 256, fast=True, splitk=2)
    _epilogues("reg", G0, 264, 136, 128, fast=True, tA=1, colsum=False, gelu=False, stream=False, ab16=False)
    # LDS-DMA single-buffered (small and deep off), four-stage ring (small off), double-buffered (gemm_glds = 3)
    for fam, opts, Ks in (("glds0", S0D0, (64, 192, 320)), ("deep", S0, (256, 320, 1024)), ("dbuf", G3, (64, 192, 320))):
        for K in Ks:
            for ta, tb in tt:
                M, N = (136 if ta else 129), (264 if tb else 257)
                add(f"K{K}", fam, opts, M, N, K, tA=ta, tB=tb, out="f32")
        add("M8N8", fam, opts, 8, 8, Ks[1], out="f32")
        add("N%8", fam, opts, 257, 50, Ks[1], out="bf16", bias=1)
        add("ldc%4", fam, opts, 257, 64, Ks[1], out="f32", ldc=67)
        # (fp16 operands under gemm_glds = 3 are left out: that measurement switch plans the bf16 double-buffered instance for them)
        _epilogues(fam, opts, 256, 512, 256 if fam == "deep" else 192, splitk=2 if fam == "dbuf" else 0, ab16=fam != "dbuf")
        _epilogues(fam, opts, 264, 136, Ks[1], tA=1, tB=1, colsum=False, gelu=False, stream=False, ab16=False, splitk=3 if fam == "dbuf" else 0)
    add("K64-ab16", "glds0", S0D0, 129, 136, 64, ab16=1, out="f16")
    add("K256-ab16", "deep", S0, 129, 136, 256, ab16=1, out="f16")
    add("sk2-K128", "dbuf", G3, 136, 264, 128, tA=1, tB=1, sk=2, out="atomic")       # one K-tile per split
    add("sk3-K320", "dbuf", G3, 136, 264, 320, tA=1, tB=1, sk=3, out="atomic", arowsum=1, expect=dict(arowsum=1))   # uneven splits
    add("sk3-K320-bcvt", "dbuf", D, 136, 264, 320, tA=1, tB=1, sk=3, out="atomic", bcvt=1, arowsum=1, expect=dict(arowsum=1))
    add("sk1-bcvt", "dbuf", D, 136, 264, 64, tA=1, tB=1, out="atomic", bcvt=1)
    # 64 x 64: one row / column past a tile, the ring at 1, 3, 4, 5 and 16 K-tiles
    for K in (64, 192, 256, 320, 1024):
        add(f"K{K}", "small", D, 65, 72, K, out="f32")
        add(f"K{K}", "small", D, 129, 136, K, tB=1, out="bf16")
    add("K64-ab16", "small", D, 65, 72, 64, ab16=1, out="f16")
    add("M8N8", "small", D, 8, 8, 64, out="f32")
    _epilogues("small", D, 256, 512, 256, colsum=False)
    _epilogues("small", D, 200, 136, 320, tB=1, colsum=False, gelu=False, stream=False, ab16=False)
    # tall tiles: only at 4500 x 4096 (more than 1024 tiles of 128 x 128); row tiles of 141 end at row 4500 / 4497 mid-tile
    tall = dict(mstep=141, grid_x=1024)
    add("ragged", "tall", D, 4497, 4088, 64, out="f32", bias=1, expect=tall)
    add("K192", "tall", D, 4500, 4096, 192, tB=1, out="bf16", expect=tall)
    _epilogues("tall", D, 4500, 4096, 64, expect=tall, ab16=True)
    add("dropout", "glds0", {"gemm_tall": 0}, 4500, 4096, 64, out="f32", bias=1, drop=0.5)      # the tall case's mask on another kernel
    # 256 x 256
    for K in (64, 320):
        for ta, tb in tt:
            add(f"K{K}", "big", B2, 512 if ta else 256, 256 if ta else 512, K, tA=ta, tB=tb, out="f32")
    add("K64-ab16", "big", B2, 256, 256, 64, ab16=1, out="f16")
    _epilogues("big", B2, 256, 512, 256, colsum=False, splitk=2)
    _epilogues("big", B2, 512, 256, 192, tA=1, tB=1, colsum=False, gelu=False, stream=False, ab16=False)
    add("slabs-uneven", "big", B2, 256, 256, 576, tA=1, tB=1, sk=3, out="atomic", ws=4 * 256 * 256 * 2, expect=dict(slabs=1, splitk=2))   # 5 + 4 K-tiles
    add("slabs-bcvt-arowsum", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", bcvt=1, arowsum=1, ws=4 * 256 * 512 * 4,
        expect=dict(slabs=1, arowsum=1))
    add("slabs-ldc", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", ws=4 * 256 * 512 * 4, ldc=520, expect=dict(slabs=1))
    add("ws-too-small", "big", B2, 256, 512, 1024, tA=1, tB=1, sk=4, out="atomic", ws=4 * 256 * 512 * 4 - 16, expect=dict(slabs=0))
    # ---- batches (2, 3): distinct outer and inner strides with gaps between the items -----------------------------------------
    bt = dict(batch=(2, 3))
    for fam, opts, fast, K in (("reg", D, False, 72), ("reg", G0, True, 128), ("glds0", S0D0, None, 192), ("deep", S0, None, 320), ("dbuf", G3, None, 192)):
        add("batch", fam, opts, 129, 136, K, fast=fast, out="f32", alpha=0.5, beta=1.0, bias=1, **bt)
        add("batch-tB", fam, opts, 136, 72, K, fast=fast, tB=1, out="bf16", **bt)
        add("batch-tA", fam, opts, 136, 72, K, fast=fast, tA=1, out="f16", bias=1, **bt)
    add("batch-sk2", "reg", D, 136, 136, 128, fast=True, tA=1, tB=1, sk=2, out="atomic", **bt)
    add("batch-sk2-tail", "reg", D, 130, 136, 136, tA=1, tB=1, sk=2, out="atomic", **bt)
    add("batch-sk2", "dbuf", G3, 136, 136, 256, tA=1, tB=1, sk=2, out="atomic", alpha=2.0, bias=1, **bt)
    # ---- 32-bit operand offsets: ~2.2 GB arenas, only the K used columns written ---------------------------------------------------
    add("A-under-2^31", "small", D, 8184, 64, 64, out="f32", lda=131072, big_ld=True, modes=("exact",))
    add("A-over-2^31", "reg", D, 8200, 64, 64, out="f32", lda=131080, big_ld=True, modes=("exact",))


_build()
BIG_LD_CASES = [c for c in CASES if c["big_ld"]]
PLAIN_CASES = [c for c in CASES if not c["big_ld"]]


def case_id(c):
    f = [c["label"], f"{c['M']}x{c['N']}x{c['K']}"]
    f += [k for k in ("tA", "tB", "ab16", "bcvt") if c[k]]
    if c["sk"] > 1:
        f.append(f"sk{c['sk']}")
    f.append(c["out"])
    return "-".join(f)


# the gemm_ln instances: gemm_ln_kernel<4 | 5, fp16 operands?> from gemm_ln_rows 64 / 80
LN_CASES = [dict(rows=rows, f16=f16, M=M, K=K, residual=res)
            for rows in (64, 80) for f16 in (0, 1) for (M, K, res) in ((1, 64, 0), (63, 320, 1), (64, 64, 1), (81, 320, 0), (161, 64, 0), (161, 320, 1))]


# ------------------------------------------------------------------------------------------------ geometry and arguments
def geometry(c):
    """where every operand and output of a case lies: per tensor (rows, cols, ld, outer stride, inner stride, span), elements"""
    M, N, K = c["M"], c["N"], c["K"]
    bo, bi = c["batch"]
    ar, ac = (K, M) if c["tA"] else (M, K)
    br, bc = (K, N) if c["tB"] else (N, K)
    g = {"A": [ar, ac, c["lda"] or r8(ac)], "B": [br, bc, c["ldb"] or r8(bc)], "C": [M, N, c["ldc"] or N]}
    ldc = g["C"][2]
    g["residual"] = [M, N, c["ldr"] or ldc]
    g["aux_in"] = g["aux_out"] = [M, N, c["ld_aux"] or N]
    for k, (rows, cols, ld) in list(g.items()):
        si = rows * ld + 16 if bo * bi > 1 else 0                   # a 16-element gap between the items of a batch,
        so = bi * si + 40 if bo * bi > 1 else 0                     # 40 more between the outer groups (multiples of 8)
        g[k] = (rows, cols, ld, so, si, (bo - 1) * so + (bi - 1) * si + rows * ld)
    return g


DT = {"f32": 0, "bf16": 1, "atomic": 2, "f16": 3}


def call_args(c, ptr):
    """the argument list of mmdti_gemm_bf16 without the stream (= mmdti_gemm_plan's without plan_out); ptr: name -> address"""
    g = geometry(c)
    p = lambda k: ptr[k] if c.get(k) else 0
    dt = DT[c["out"]] | (16 if c["ab16"] else 0) | (32 if c["bcvt"] else 0)
    bo, bi = c["batch"]
    return [ptr["A"], ptr["B"], ptr["C"], c["M"], c["N"], c["K"], g["A"][2], g["B"][2], g["C"][2], c["tA"], c["tB"], bo, bi,
            g["A"][3], g["A"][4], g["B"][3], g["B"][4], g["C"][3], g["C"][4], c["sk"], c["alpha"], c["beta"], p("bias"), p("residual"),
            g["residual"][2], c["act"], p("aux_in"), p("aux_out"), g["aux_in"][2], dt, c["drop"], SEED, SITE, p("colsum"), p("arowsum"),
            p("ws"), c["ws"]]


def operand_dtype(c, which):
    if c["ab16"] or (which == "B" and c["bcvt"]):
        return torch.float16
    return torch.bfloat16


def out_dtype(c):
    return {"f32": torch.float32, "atomic": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c["out"]]


# ------------------------------------------------------------------------------------------------ inputs
class Arena:
    """a flat buffer pre-filled with NaN (operands) or a sentinel bit pattern (outputs), and the strided view of the tensor cut from
    it: GUARD_ROWS rows of the filling in front and behind, the padding columns [cols, ld) and the gaps of a batch in between"""

    def __init__(self, geo, batch, dtype, device, out=False, guard=True):
        rows, cols, ld, so, si, span = geo
        self.guard = (GUARD_ROWS * ld if ld <= 8192 else 4096) if guard else 0    # (the split-K workspace, one long row: 4096 elements)
        n = self.guard + span + self.guard
        self.out, self.dtype = out, dtype
        self.ibits = torch.int32 if dtype == torch.float32 else torch.int16
        self.sent = SENT32 if dtype == torch.float32 else SENT16
        if guard:
            self.buf = torch.empty(n, dtype=self.ibits, device=device).fill_(self.sent).view(dtype) if out else torch.full((n,), float("nan"), dtype=dtype, device=device)
        else:
            self.buf = torch.empty(n, dtype=dtype, device=device)
        bo, bi = batch
        self.view = self.buf.as_strided((bo, bi, rows, cols), (so, si, ld, 1), self.guard)
        self.iview = self.buf.view(self.ibits).as_strided((bo, bi, rows, cols), (so, si, ld, 1), self.guard)

    def ptr(self):
        return self.buf.data_ptr() + self.guard * self.buf.element_size()

    def outside_untouched(self):
        """every sentinel outside the view still in place (the view itself is overwritten with the sentinel on a copy)"""
        chk = self.buf.view(self.ibits).clone()
        chk.as_strided(self.iview.shape, self.iview.stride(), self.guard).fill_(self.sent)
        return int((chk != self.sent).sum())


def _ints(shape, r, g, dtype, device):
    return torch.randint(-r, r + 1, shape, generator=g).to(dtype).to(device)


def exact_r(c):
    """-> (r, gran): the operand range of the exact inputs and the granularity of every value involved"""
    cap = 2047 if c["ab16"] else 255
    mag = max(1.0, abs(c["alpha"])) * (1.0 / (1.0 - c["drop"])) * (2.0 if c["aux_in"] else 1.0)
    r = min(cap, int(math.isqrt(int((1 << 23) / (c["K"] * mag)))))
    if c["arowsum"]:
        r = min(r, ((1 << 24) - 1) // c["K"])
    if c["colsum"]:                     # sum over M rows of |C| stays below 2^24 (bias below 2^10 there: see make_inputs)
        r = min(r, int(math.isqrt(max(1, ((1 << 23) // c["M"]) // c["K"]))))
    if c["out"] == "f16":               # most outputs inside fp16's range (3 sigma at 65504), some saturated
        r = min(r, max(1, int(math.sqrt(65504.0 / math.sqrt(c["K"])))))
    gran = min(1.0, abs(c["alpha"])) * (0.5 if c["drop"] else 1.0)
    return max(r, 1), gran


def make_inputs(c, mode, device, seed=0):
    """-> dict of Arenas (A, B, C and whatever else the case takes); C holds NaN where the kernel must store every element
    (beta == 0, not atomic), else C0.  mode: "exact" (integers) or "random" (randn rounded to the operand type)."""
    g = torch.Generator().manual_seed(1000 + seed + hash((c["M"], c["N"], c["K"], c["tA"], c["tB"])) % 1000)
    geo, batch = geometry(c), c["batch"]
    guard = not c["big_ld"]
    t = {}
    r, _ = exact_r(c)
    small = 1 << 10 if c["colsum"] else 1 << 20
    for k in ("A", "B"):
        a = Arena(geo[k], batch, operand_dtype(c, k), device, guard=guard)
        shape = a.view.shape
        a.view.copy_(_ints(shape, r, g, a.dtype, device) if mode == "exact" else torch.randn(shape, generator=g).to(a.dtype).to(device))
        t[k] = a
    f32 = torch.float32

    def fvals(shape, dtype, lim):
        if mode == "exact":
            return _ints(shape, lim - 1, g, dtype, device)
        return torch.randn(shape, generator=g).to(dtype).to(device)

    M, N = c["M"], c["N"]
    if c["bias"]:
        a = Arena((1, N, r8(N), 0, 0, r8(N)), (1, 1), f32, device)
        a.view.copy_(torch.full((1, 1, 1, N), 0.5, device=device) if c["drop"] else fvals((1, 1, 1, N), f32, small))
        t["bias"] = a
    if c["residual"]:
        a = Arena(geo["residual"], (1, 1), f32, device)
        a.view.copy_(fvals(a.view.shape, f32, small))
        t["residual"] = a
    if c["aux_in"]:
        a = Arena(geo["aux_in"], (1, 1), torch.bfloat16, device)
        a.view.copy_(_ints(a.view.shape, 2, g, torch.bfloat16, device) if mode == "exact" else torch.randn(a.view.shape, generator=g).to(torch.bfloat16).to(device))
        t["aux_in"] = a
    if c["aux_out"]:
        t["aux_out"] = Arena(geo["aux_out"], (1, 1), torch.bfloat16, device, out=True)
    C = Arena(geo["C"], batch, out_dtype(c), device, out=True)
    t["C0"] = None
    if c["beta"] != 0.0 or c["out"] == "atomic":
        t["C0"] = fvals(C.view.shape, f32, small)
        C.view.copy_(t["C0"])
    t["C"] = C
    for k, n in (("colsum", N), ("arowsum", M)):
        if c[k]:
            a = Arena((1, n, r8(n), 0, 0, r8(n)), (1, 1), f32, device, out=True)
            t[k + "0"] = fvals((1, 1, 1, n), f32, 1 << 10)          # the kernels add into these
            a.view.copy_(t[k + "0"])
            t[k] = a
    if c["ws"]:
        a = Arena((1, c["ws"] // 4, c["ws"] // 4, 0, 0, c["ws"] // 4), (1, 1), f32, device, out=True)
        t["ws"] = a
    return t


def pointers(t):
    return {k: a.ptr() for k, a in t.items() if isinstance(a, Arena)}


FAKE_PTRS = {k: 0x10000 for k in ("A", "B", "C", "bias", "residual", "aux_in", "aux_out", "colsum", "arowsum", "ws")}


# ------------------------------------------------------------------------------------------------ the reference
def gelu64(x):
    return x * 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def round16(v, dtype):
    """float64 -> the 16-bit type, to nearest even; fp16 saturates at 65504 (f2h_sat).  (Every value rounded here is either
    an fp32-exact number or compared within a band that covers the double rounding.)"""
    if dtype == torch.float16:
        v = v.clamp(-65504.0, 65504.0)
    return v.to(dtype)


def reference(c, t, keep=None, dtype=F64):
    """-> dict: C (in `dtype`, before the rounding of a 16-bit output), C_out (as stored), T (the magnitude sum of the bound), pre (the
    pre-activation), aux_out, colsum, arowsum.  keep: the dropout mask [.., M, N] (bool) -- taken from the device's output, its
    law is checked apart.  dtype float32 gives the fp32 evaluation of the same formula that pins this function on the CPU."""
    A, B = t["A"].view, t["B"].view
    if c["bcvt"]:
        B = B.to(torch.bfloat16)
    A, B = A.to(dtype), B.to(dtype)
    opA = A.transpose(-1, -2) if c["tA"] else A                     # [.., M, K]
    opB = B.transpose(-1, -2) if c["tB"] else B                     # [.., N, K]
    alpha, beta = c["alpha"], c["beta"]
    v = alpha * (opA @ opB.transpose(-1, -2))
    T = abs(alpha) * (opA.abs() @ opB.abs().transpose(-1, -2))
    out = {}
    if c["bias"]:
        b = t["bias"].view.to(dtype)
        v, T = v + b, T + b.abs()
    out["pre"] = v
    act = c["act"]
    if act == ACT_GELU:
        out["aux_out"] = v
        v = gelu64(v)
    elif act == ACT_GELU_G:
        out["aux_out"] = gelu_grad64(v)
        v = gelu64(v)
    elif act == ACT_GELU_BWD:
        v = v * gelu_grad64(t["aux_in"].view.to(dtype))
    elif act == ACT_MUL_AUX:
        x = t["aux_in"].view.to(dtype)
        v, T = v * x, T * x.abs()
    if c["drop"]:
        s = 1.0 / (1.0 - c["drop"])
        v, T = torch.where(keep, v * s, torch.zeros_like(v)), T * s
    if c["residual"]:
        rr = t["residual"].view.to(dtype)
        v, T = v + rr, T + rr.abs()
    if t["C0"] is not None:
        c0 = t["C0"].to(dtype) * (1.0 if c["out"] == "atomic" else beta)
        v, T = v + c0, T + c0.abs()
    out["C"], out["T"] = v, T
    od = out_dtype(c)
    out["C_out"] = v.to(od) if od == torch.float32 else round16(v, od)
    if c["colsum"]:
        out["colsum"] = t["colsum0"].to(dtype) + out["C_out"].to(dtype).sum(-2, keepdim=True)
        out["colsum_T"] = t["colsum0"].to(dtype).abs() + out["C_out"].to(dtype).abs().sum(-2, keepdim=True)
    if c["arowsum"]:
        out["arowsum"] = t["arowsum0"].to(dtype) + opA.sum(-1).reshape(1, 1, 1, -1)
        out["arowsum_T"] = t["arowsum0"].to(dtype).abs() + opA.abs().sum(-1).reshape(1, 1, 1, -1)
    return out


def rounding_term(ref, dtype):
    """R of the bound: the rounding of a 16-bit output"""
    if dtype == torch.bfloat16:
        return 2.0 ** -8 * ref.abs()
    if dtype == torch.float16:
        return 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return torch.zeros_like(ref)


def bound(c, ref):
    """|got - ref| <= (K + 8) * 2^-23 * T + R elementwise: fp32 summation of K products and the epilogue's few terms in any order,
    rounding or truncating adders; GELU epilogues carry the bound through the function (|gelu'| <= 1.13) plus four times the
    measured error of the device's gelu_erf / gelu_erf_grad."""
    u = (c["K"] + 8) * 2.0 ** -23
    b = u * ref["T"]
    if c["act"] in (ACT_GELU, ACT_GELU_G):
        b = 1.13 * b + 4 * GELU_G_MEASURED["gelu"]
    elif c["act"] == ACT_GELU_BWD:
        b = 1.13 * b + ref["pre"].abs() * 4 * GELU_G_MEASURED["gelu_grad"]
    return b + rounding_term(ref["C"], out_dtype(c))


def aux_out_bound(c, ref):
    u = (c["K"] + 8) * 2.0 ** -23
    b = u * ref["T"] if c["act"] == ACT_GELU else 1.13 * u * ref["T"] + 4 * GELU_G_MEASURED["gelu_grad"]
    return b + rounding_term(ref["aux_out"], torch.bfloat16)


# ------------------------------------------------------------------------------------------------ plans
class options:
    """writes a case's option setting, then the library's documented defaults back (as test_gemm_plan_cpu.options)"""

    def __init__(self, lib, setting, defaults):
        self.lib, self.setting, self.defaults = lib, setting, defaults

    def __enter__(self):
        for k, v in self.setting.items():
            self.lib.mmdti_set_option(k.encode(), v)

    def __exit__(self, *exc):
        for k in self.setting:
            self.lib.mmdti_set_option(k.encode(), self.defaults[k])


def plan(lib, c, ptr=None):
    """the launch plan of a case under the options in force, as a dict"""
    out = (ctypes.c_int * 15)()
    lib.mmdti_gemm_plan(*call_args(c, ptr or FAKE_PTRS), out)
    p = list(out)
    return dict(kernel=kernel_name(p), grid_x=p[6], grid_z=p[7], block=p[8], lds=p[9], splitk=p[10], mstep=p[11], slabs=p[12], stream_c=p[13],
                arowsum=p[14])


def assert_declared_plan(lib, c, ptr=None):
    p = plan(lib, c, ptr)
    assert p["kernel"] == c["kernel"], (case_id(c), p)
    for k, v in c["expect"].items():
        assert p[k] == v, (case_id(c), k, p)
    if c["big_ld"]:                                                  # the bare-load predicate, on either side of 2^31 bytes
        under = c["M"] * c["lda"] * 2 < 0x7fffffff
        assert under == (not c["kernel"].startswith("gemm_bf16_kernel<false, false, false")), (case_id(c), p)
    return p


# ------------------------------------------------------------------------------------------------ Linear + LayerNorm
LN_N, LN_EPS = 512, 1e-5


def ln_inputs(lc, mode, device, seed=0):
    """A [M, K] and W [512, K] (16-bit, NaN-guarded arenas with padded rows), bias, residual [M, 516], gamma, beta"""
    g = torch.Generator().manual_seed(77 + seed + lc["M"] + lc["K"])
    M, K = lc["M"], lc["K"]
    dt = torch.float16 if lc["f16"] else torch.bfloat16
    r = min(2047 if lc["f16"] else 255, math.isqrt((1 << 23) // K))
    t = {}
    for k, rows, ld in (("A", M, K + 8), ("W", LN_N, K + 16)):
        a = Arena((rows, K, ld, 0, 0, rows * ld), (1, 1), dt, device)
        a.view.copy_(_ints(a.view.shape, r, g, dt, device) if mode == "exact" else torch.randn(a.view.shape, generator=g).to(dt).to(device))
        t[k] = a
    f32 = torch.float32
    vals = lambda shape: (_ints(shape, (1 << 20) - 1, g, f32, device) if mode == "exact" else torch.randn(shape, generator=g).to(device))
    t["bias"] = Arena((1, LN_N, LN_N, 0, 0, LN_N), (1, 1), f32, device)
    t["bias"].view.copy_(vals((1, 1, 1, LN_N)))
    if lc["residual"]:
        t["residual"] = Arena((M, LN_N, LN_N + 4, 0, 0, M * (LN_N + 4)), (1, 1), f32, device)
        t["residual"].view.copy_(vals((1, 1, M, LN_N)))
    t["gamma"] = (1.0 + 0.25 * torch.randn(LN_N, generator=g)).to(device)
    t["beta"] = (0.25 * torch.randn(LN_N, generator=g)).to(device)
    for k, shape, dtype in (("x_out", (M, LN_N), f32), ("ln_f32", (M, LN_N), f32), ("ln_16", (M, LN_N), dt), ("mean", (1, M), f32), ("rstd", (1, M), f32)):
        t[k] = Arena((shape[0], shape[1], shape[1], 0, 0, shape[0] * shape[1]), (1, 1), dtype, device, out=True)
    return t


def ln_reference(t, dtype=F64):
    """x = residual + A . W^T + bias, its row mean and 1 / sqrt(var + eps), LN(x) * gamma + beta -- all in `dtype`; T as in reference()"""
    A, W, b = t["A"].view[0, 0].to(dtype), t["W"].view[0, 0].to(dtype), t["bias"].view[0, 0].to(dtype)
    x, T = A @ W.T + b, A.abs() @ W.abs().T + b.abs()
    if "residual" in t:
        rr = t["residual"].view[0, 0].to(dtype)
        x, T = x + rr, T + rr.abs()
    return dict(x=x, T=T, **ln_of(x, t, dtype))


def ln_of(x, t, dtype):
    x = x.to(dtype)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    return dict(mean=mean, rstd=rstd, ln=(x - mean[:, None]) * rstd[:, None] * t["gamma"].to(dtype) + t["beta"].to(dtype))


def colsum_bound(c, ref):
    """column sums of the stored C: every term within its own bound (a 16-bit term may round the other way: R covers one step), and
    the fp32 sum over M rows in any order"""
    return bound(c, ref).sum(-2, keepdim=True) + (c["M"] + 8) * 2.0 ** -23 * ref["colsum_T"]


def arowsum_bound(c, ref):
    return (c["K"] + 8) * 2.0 ** -23 * ref["arowsum_T"]


def side_bound(c, ref, k):
    return {"colsum": colsum_bound, "arowsum": arowsum_bound, "aux_out": aux_out_bound}[k](c, ref)


def worst_ratio(got, ref, b):
    """max |got - ref| / b; an element whose bound is zero admits only the reference itself"""
    d = (got.to(F64) - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    q = torch.where(b > 0, d / b, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
    return float(q.max())
