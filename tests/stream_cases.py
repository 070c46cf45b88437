"""The case table of the stream-kernel instance tests (the casts, dropout_f32, axpy, GELU, column sums, sum of squares, Adam and the step
state of csrc/elementwise.hip), their input builders, float64 references, bounds and fp32 emulations, shared by test_stream_cases_cpu.py
(which proves that the table reaches every kernel and every Adam and sumsq instantiation, that the sizes cross each launcher's grid cap,
that the exact modes are exact in the emulation, that the emulation stays inside the bounds and that six wrong emulations do not) and
test_stream_instances_gpu.py (which holds the kernels to the references on the device).  Masks come from dropout_rule.py.

SIZES.  grid_for caps a launch at 4096 workgroups of 256; every kernel runs at n = 1, 3, 1027 (1003) and at the smallest size that passes
the cap once with a ragged tail: the fp32 -> 16-bit casts (4 elements per thread) at 4194304 + 4 x 257 + 3, the one-element-per-thread
kernels at 1048576 + 1027, the fp16 -> bf16 cast (8 per thread, row stride) at 2049 x 4104, ldx 4112; Adam (at most 1024 elements per
workgroup of 256: always a grid-stride loop of four rounds) at 1048576 + 8 x 129 + 5.

WHAT IS HELD
  casts     EQUAL, as bit patterns, the value rounded to nearest even (fp16: saturating at +-65504); with dropout the fp32 product
            x * (1.f / (1.f - p)) is a rounding point of the kernel and the reference performs it; -0.0 stays -0.0, a dropped element is +0
  dropout   EQUAL the same fp32 product or +0;   bf16 -> fp32 EQUAL;   fp16 -> bf16 EQUAL x.float().bfloat16()
  axpy      2 U (|a x| + |y|): one fused-or-not rounding pair.   GELU: 4 GELU_G_MEASURED["gelu"] + one bf16 ulp (gelu_erf, common.h)
  colsum    exact mode (small integers) EQUAL; random: (n + 8) U (sum |terms| + FILL), n = a thread's rows + the 8 row lanes + the row groups
  sumsq     integers EQUAL; randn (n + 8) U sum g^2, n = the depth of the chain (a thread's terms, 6 DPP steps, 4 waves, the partials);
            the non-finite count EQUAL; the guard's five words EQUAL the table's values
  Adam      a float64 statement of the kernel's update over three steps; the errors of p, m, v are carried from step to step:
                g' = g gs + wd p: 3 U (|g gs| + |wd p|) + wd L_p       m: 3 U (|b1 m| + |(1 - b1) g'|) + b1 L_m + (1 - b1) L_g
                v: 3 U (b2 v + (1 - b2) g'^2) + b2 L_v + 2 (1 - b2) |g'| L_g       r = sqrt(v): L_v / (2 r) (sqrt(L_v) at v = 0) + U r
                den = r / bc2 + eps: L_r / bc2 + 2 U den + den E_bc2 / bc2      step = (lr / bc1) m / den: |step| (3 U + E_bc1 / bc1 + L_den / den) + (lr / bc1) L_m / den
                p: L_p + L_step + U |p|
            (1 - b1), (1 - b2) are fp32 differences and the reference takes them as such.  lr, bc1, bc2 read through the step state or the
            guard are inputs; by value, the library's host powf is allowed 2 ulp: E_bc1 = 4 U b1^t + U bc1, E_bc2 likewise through the root.
            The shadows EQUAL the rounding of the device's OWN fp32 p (fp16 saturating).  Masked groups of 8 keep their bits in all five
            buffers; a set guard flag leaves every buffer untouched.  With g = 0 and m = v = 0: at wd = 0 nothing moves, bit for bit.
  step      counter, salt pair EQUAL a host splitmix64; lr EQUALS the same two fp32 operations; bias corrections within the 2-ulp-of-powf bound"""
import functools
import math

import numpy as np
import torch

import dropout_rule as DR
from attn_cases import Z_MAX, gain  # noqa: F401
from gemm_cases import F64, GELU_G_MEASURED, SENT16, SENT32, gelu64, worst_ratio  # noqa: F401
from row_cases import PTR, Bufs, read_plan, round16, ulp16  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
U = 2.0 ** -24
FILL = 0.75
SEED, SITE = 0x7A5C3E1F2B4D6978, 17
CAP = 4096
BIG1 = 1048576 + 1027
BIG4 = 4194304 + 4 * 257 + 3
BIGA = 1048576 + 8 * 129 + 5
SUMSQ_WGS = 2048
NF_T, NF_SKIPPED, NF_FLAG, NF_BC1, NF_BC2 = range(5)

SOURCE_LINES = (
    "if (thresh) o = dropout_keep(seed, site, (uint64_t)i, thresh) ? o * dscale : 0.f;",
    "Rand4 r = philox4(seed, site, (uint64_t)i);",
    "y[i] = f2bf(gelu_erf(bf2f(u[i])));",
    "y[i] += a * x[i];",
    "for (int i = 0; i < cols - c0; ++i) acc[i] += bf2f(p[i]);",
    "__device__ __forceinline__ unsigned nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }",
    "const int i = min((int)t, table_steps) - 1;      // (the host sizes the table to every step it has enqueued)",
    "if (guard[NF_FLAG] != 0.f) return;",
    "if (skip[i >> 3]) continue;",
    "float gi = g[i] * gs;",
    "if (wd != 0.f) gi += wd * pi;",
    "float mi = b1 * m[i] + (1.f - b1) * gi;",
    "float vi = b2 * v[i] + (1.f - b2) * gi * gi;",
    "const float denom = sqrtf(vi) / bc2_sqrt + eps;",
    "pi -= (lr / bc1) * mi / denom;",
    "if (pb) pb[i] = f2bf(pi);",
    "if (ph) ph[i] = f2h_sat(pi);      // the fp16 shadow the forward GEMMs read (fp16 forward-operand mode)",
    "const float lam = k < warmup ? (float)k / (float)max(1, warmup) : fmaxf(0.f, (float)(total - k) / (float)max(1, total - warmup));",
    "st[1] = base_lr * lam;",
    "unsigned long long x = *salt + 0x9E3779B97F4A7C15ull;       // splitmix64: a fresh, well-mixed word per step",
)
PLAN_LINES = ("constexpr int SUMSQ_WGS = 2048;",)           # (csrc/stream_plan.h: the constant this file restates)

ALL_KERNELS = ("cast_f32_bf16_kernel<false>", "cast_f32_bf16_kernel<true>", "cast_f16_bf16_kernel", "cast_bf16_f32_kernel", "dropout_f32_kernel", "axpy_kernel",
               "gelu_bf16_kernel", "colsum_bf16_kernel", "colsum_bf16_slab_kernel", "sumsq_kernel", "sumsq_part_kernel<false>", "sumsq_fold_kernel<false>",
               "sumsq_part_kernel<true>", "sumsq_fold_kernel<true>", "adam_kernel<false, false>", "adam_kernel<true, false>", "adam_kernel<false, true>",
               "adam_kernel<true, true>", "step_state_advance_kernel")


def grid_for(n, per):
    return max(1, min(CAP, -(-n // per)))


# ------------------------------------------------------------------------------------------------ the table
CASES = []


def add(kind, **kw):
    c = dict(kind=kind, i=len(CASES), **kw)
    CASES.append(c)
    return c


COLSUM_SHAPES = ((1, 8, 8), (63, 50, 56), (333, 200, 200), (333, 257, 264), (65536 + 197, 8, 8))
SUMSQ_FORMS = ("atomic", "part", "check", "guard", "guard_table")
SUMSQ_WS3 = 3 * 256 * 4 * 2 + 7
#            n     wd    gs    state  shadows   zero
ADAM_OPTS = ((BIGA, 0.0, None, False, ("bf16",), False),
             (1003, 0.01, 0.37, True, ("f16",), False),
             (1, 0.01, None, True, ("bf16", "f16"), False),
             (3, 0.0, 0.37, False, (), False),
             (1003, 0.0, None, False, ("bf16", "f16"), True),
             (1003, 0.01, 0.37, True, ("bf16",), True))


def _build():
    for f16 in (False, True):
        for n in (1, 3, 1027, BIG4):
            for p in (0.0, 0.1):
                add("cast", f16=f16, n=n, p=p)
    for shape in ((1, 8, 8), (3, 8, 16), (2049, 4104, 4112)):
        add("cast_hb", rows=shape[0], cols=shape[1], ldx=shape[2])
    for n in (1, 3, 1027, BIG1):
        add("cast_b32", n=n)
        add("dropout", n=n, p=0.35)
        add("axpy", n=n, a=(0.37, -1.5)[n % 2])
        add("gelu", n=n)
    for rows, cols, ld in COLSUM_SHAPES:
        for det in (False, True):
            for mode in ("exact", "random"):
                add("colsum", rows=rows, cols=cols, ld=ld, det=det, mode=mode)
    for form in SUMSQ_FORMS:
        for j, n in enumerate((1, 3, 1003, 1048576 + 7)):
            add("sumsq", form=form, n=n, ws=4096, mode=("exact", "random")[j % 2], special=None)
            add("sumsq", form=form, n=n, ws=4096, mode=("random", "exact")[j % 2], special=None)
        if form != "atomic":
            add("sumsq", form=form, n=SUMSQ_WS3, ws=3 if form == "part" else 6, mode="exact", special=None)      # many rounds of three workgroups
            add("sumsq", form=form, n=SUMSQ_WS3, ws=3 if form == "part" else 6, mode="random", special=None)
        if form not in ("atomic", "part"):
            for special in ("body", "tail", "last_wg", "denormal", "overflow"):
                add("sumsq", form=form, n=1048576 + 7 if special == "last_wg" else 1003, ws=4096, mode="exact", special=special)
    for guard in (False, True):
        for mask in (False, True):
            for n, wd, gs, state, shadows, zero in ADAM_OPTS:
                add("adam", guard=guard, mask=mask, n=n, wd=wd, gs=gs, state=state, shadows=shadows, zero=zero)
    add("step", steps=12, warmup=3, total=10, base_lr=3e-4)


_build()


def instance(c):
    """the kernels the entry point launches for the case"""
    k = c["kind"]
    if k == "cast":
        return (f"cast_f32_bf16_kernel<{'true' if c['f16'] else 'false'}>",)
    if k == "colsum":
        return ("colsum_bf16_slab_kernel",) if c["det"] else ("colsum_bf16_kernel",)
    if k == "sumsq":
        chk = "false" if c["form"] == "part" else "true"
        return ("sumsq_kernel",) if c["form"] == "atomic" else (f"sumsq_part_kernel<{chk}>", f"sumsq_fold_kernel<{chk}>")
    if k == "adam":
        return (f"adam_kernel<{'true' if c['guard'] else 'false'}, {'true' if c['mask'] else 'false'}>",)
    return ({"cast_hb": "cast_f16_bf16_kernel", "cast_b32": "cast_bf16_f32_kernel", "dropout": "dropout_f32_kernel", "axpy": "axpy_kernel", "gelu": "gelu_bf16_kernel",
             "step": "step_state_advance_kernel"}[k],)


def launch(c):
    """(workgroups, work items per workgroup and round, work items): rounds = ceil(items / (workgroups x per))"""
    k = c["kind"]
    if k == "cast":
        return grid_for(c["n"] // 4 + 1, 256), 256, c["n"] // 4
    if k == "cast_hb":
        n8 = c["rows"] * (c["cols"] // 8)
        return grid_for(n8, 256), 256, n8
    if k == "adam":
        return grid_for(c["n"], 1024), 256, c["n"]
    if k == "sumsq":
        if c["form"] == "atomic":
            return grid_for(c["n"], 2048), 256, c["n"]
        return sumsq_wgs(c), 256, c["n"] // 4
    return grid_for(c["n"], 256), 256, c["n"]


def rounds(c):
    g, per, items = launch(c)
    return -(-items // (g * per))


def sumsq_wgs(c):
    return min(min(c["ws"] if c["form"] == "part" else c["ws"] // 2, SUMSQ_WGS), (c["n"] // 4 + 255) // 256 + 1)


def sumsq_depth(c):
    """the longest chain of additions a term passes through"""
    if c["form"] == "atomic":
        g = grid_for(c["n"], 2048)
        return -(-c["n"] // (g * 256)) + 6 + 4 + g
    w = sumsq_wgs(c)
    return -(-(c["n"] // 4) // (w * 256)) + 3 + 1 + 6 + 4 + -(-w // 256) + 8


def colsum_gy(rows):
    return min(1024, -(-rows // 64))


def colsum_depth(rows):
    gy = colsum_gy(rows)
    return -(-rows // (gy * 8)) + 8 + gy


# ------------------------------------------------------------------------------------------------ the library's answer (mmdti_stream_plan)
PLAN_FAMILY = 7                      # MMDTI_PLAN_STREAM
ENTRY = {name: i for i, name in enumerate(("cast_f32_bf16", "cast_f32_f16", "cast_f16_bf16", "cast_bf16_f32", "dropout_f32", "axpy_f32", "gelu_fwd_bf16", "colsum_bf16",
                                           "sumsq_f32", "sumsq_check_f32", "adam_step", "adam_step_guarded", "adam_step_masked", "adam_step_grouped", "ema_update",
                                           "ema_swap", "step_state_advance"))}
FLAT_ENTRY = {"cast_b32": "cast_bf16_f32", "dropout": "dropout_f32", "axpy": "axpy_f32", "gelu": "gelu_fwd_bf16"}


def stream_plan(lib, entry, ptrs, n=0, a=0, b=0, c=0, f=0.0, det=False):
    """one call of mmdti_stream_plan: ptrs in the entry's order (include/mmdti_hip.h) -> dict(launches, wgs)"""
    import ctypes
    out = (ctypes.c_longlong * 12)()
    lib.mmdti_stream_plan(ENTRY[entry], int(det), (ctypes.c_void_p * len(ptrs))(*ptrs), n, a, b, c, f, out)
    return read_plan(lib, PLAN_FAMILY, out, ("wgs",))


def flat(name, grid):
    return [(name, grid, 1, 256, 0)]


def adam_entry(c):
    """(entry, ptrs): the entry point the case goes through and the addresses it gives -- p, g, m, v, then the entry's optional ones"""
    on = lambda x: PTR if x else 0
    if c["mask"]:
        return "adam_step_masked", [PTR] * 4 + [on(c["state"]), on(c["guard"]), PTR]
    if c["guard"]:
        return "adam_step_guarded", [PTR] * 5
    return "adam_step", [PTR] * 4 + [on(c["state"])]


def library_plan(lib, c, det=None):
    k = c["kind"]
    det = c.get("det", False) if det is None else det
    if k == "cast":
        return stream_plan(lib, "cast_f32_f16" if c["f16"] else "cast_f32_bf16", [PTR, PTR], c["n"], f=c["p"])
    if k == "cast_hb":
        return stream_plan(lib, "cast_f16_bf16", [PTR, PTR], a=c["rows"], b=c["cols"], c=c["ldx"])
    if k in FLAT_ENTRY:
        return stream_plan(lib, FLAT_ENTRY[k], [PTR, PTR], c["n"], f=c.get("p", 0.0))
    if k == "colsum":
        return stream_plan(lib, "colsum_bf16", [PTR, PTR], a=c["rows"], b=c["cols"], c=c["ld"], det=det)
    if k == "sumsq":
        if c["form"] in ("atomic", "part"):
            return stream_plan(lib, "sumsq_f32", [PTR, PTR, PTR if c["form"] == "part" else 0], c["n"], a=c["ws"] if c["form"] == "part" else 0, det=det)
        table = c["form"] == "guard_table"
        return stream_plan(lib, "sumsq_check_f32", [PTR, PTR, PTR, PTR if table else 0], c["n"], a=c["ws"], b=3 if table else 0)
    if k == "adam":
        entry, ptrs = adam_entry(c)
        return stream_plan(lib, entry, ptrs, c["n"], a=7 if c["state"] or c["guard"] else 1)
    assert k == "step"
    return stream_plan(lib, "step_state_advance", [PTR, PTR], a=c["warmup"], b=c["total"])


def declared_plan(c, det=None):
    """what the case is declared to launch, from instance() and launch(): every field of the library's plan"""
    k, names = c["kind"], instance(c)
    det = c.get("det", False) if det is None else det
    wgs = 0
    if k == "colsum":
        name = "colsum_bf16_slab_kernel" if det else "colsum_bf16_kernel"
        launches = [(name, -(-c["cols"] // 256), colsum_gy(c["rows"]), 256, 0)] + ([("det_fold_kernel", -(-c["cols"] // 64), 1, 1024, 0)] if det else [])
    elif k == "sumsq" and c["form"] != "atomic":
        wgs = sumsq_wgs(c)
        launches = flat(names[0], wgs) + flat(names[1], 1)
    elif k == "step":
        launches = [(names[0], 1, 1, 1, 0)]
    else:
        launches = flat(names[0], launch(c)[0])
    return dict(launches=launches, wgs=wgs)


def assert_declared_plan(lib, c):
    got, want = library_plan(lib, c), declared_plan(c)
    assert got == want, (case_id(c), got, want)
    return got


def case_id(c):
    skip = ("kind", "i")
    f = [c["kind"]]
    for k, v in c.items():
        if k in skip or v is None or v is False or v == ():
            continue
        f.append(k if v is True else f"{k}{'+'.join(v) if isinstance(v, tuple) else v}")
    return "-".join(f) + f"-{c['i']}"


# ------------------------------------------------------------------------------------------------ inputs
def _gen(c):
    return torch.Generator().manual_seed(104729 * c["i"] + 5)


F16_SPECIALS = (65504.0, -65504.0, 65520.0, -65520.0, 65519.99, 1e6, -1e6, float("inf"), float("-inf"), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, -2.0 ** -25, 1e-7,
                6.1e-5, 2.0 ** -14, 1e-40, -0.0, 0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.3895314e38, -3.3961775e38)


def make_inputs(c):
    g = _gen(c)
    k = c["kind"]
    rn = lambda *s: torch.randn(*s, generator=g)
    if k in ("cast", "dropout"):
        n = c["n"]
        x = rn(n) * torch.exp2(torch.randint(-20, 17, (n,), generator=g).float())
        sp = torch.tensor(F16_SPECIALS, dtype=F32)
        if n >= 1027:
            x[7:7 + sp.numel()] = sp
            x[n - sp.numel():] = sp.flip(0)                        # the specials in the n % 4 tail and the last workgroup too
        elif n == 3:
            x[:] = torch.tensor([65520.0, -0.0, float("-inf")])
        keep = DR.keep_flat(SEED, SITE, n, c["p"])
        return dict(x=x, keep=torch.from_numpy(keep) if c["p"] > 0 else None, sc=DR.dscale(c["p"]))
    if k == "cast_hb":
        bits = torch.randint(0, 1 << 16, (c["rows"], c["cols"]), generator=g, dtype=torch.int32)
        bits = torch.where((bits & 0x7C00) == 0x7C00, bits & ~0x03FF, bits)                 # (inf stays, NaN payloads are not part of the contract)
        return dict(x=(bits - ((bits >= 32768).int() << 16)).to(torch.int16).view(F16))
    if k == "cast_b32":
        bits = torch.randint(0, 1 << 16, (c["n"],), generator=g, dtype=torch.int32)
        bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x007F, bits)
        return dict(x=(bits - ((bits >= 32768).int() << 16)).to(torch.int16).view(BF16))
    if k == "axpy":
        return dict(x=rn(c["n"]), y=rn(c["n"]) * 3)
    if k == "gelu":
        u = (torch.rand(c["n"], generator=g) * 20 - 10).to(BF16)
        if c["n"] >= 3:
            u[0], u[1], u[2] = 0.0, -0.0, 10.0
        if c["n"] >= 1027:
            u[3], u[-1] = -10.0, -10.0
        return dict(u=u)
    if k == "colsum":
        rows, cols = c["rows"], c["cols"]
        x = torch.randint(-3, 4, (rows, cols), generator=g).float() if c["mode"] == "exact" else rn(rows, cols)
        return dict(x=x.to(BF16))
    if k == "sumsq":
        n = c["n"]
        x = torch.randint(-2, 3, (n,), generator=g).float() if c["mode"] == "exact" else rn(n)
        sp = c["special"]
        if sp == "body":
            x[5], x[300], x[777] = float("inf"), float("-inf"), float("nan")
        elif sp == "tail":
            x[n - 1], x[n - 2] = float("nan"), float("inf")            # n = 1003: the n % 4 tail is elements 1000 .. 1002
        elif sp == "last_wg":
            x[n - 6], x[n - 3000], x[n - 1] = float("-inf"), float("nan"), float("inf")     # (n - 6: the one float4 of the last workgroup that has any; n - 1: the tail)
        elif sp == "denormal":
            x[11] = 1e-40
        elif sp == "overflow":
            x[11] = 3e38
        return dict(x=x)
    if k == "adam":
        n = c["n"]
        t = dict(p=rn(n), m=0.1 * rn(n), v=(0.1 * rn(n)) ** 2, g=[rn(n) * 0.3 for _ in range(3)])
        if n >= 1003:
            t["p"][3], t["p"][n - 2] = 1e5, -1e5                     # past the fp16 range: the fp16 shadow saturates
            t["v"][5] = 0.0
        if c["zero"]:
            t["m"].zero_(); t["v"].zero_()
            t["g"] = [torch.zeros(n) for _ in range(3)]
        if c["mask"]:
            t["skip"] = (torch.rand((n + 7) // 8, generator=g) < 0.3).to(torch.uint8)
            t["skip"][-1] = c["i"] % 2                                  # the last, partial group: skipped in one case, taken in the next
        b1, b2 = np.float32(0.9), np.float32(0.999)
        t["steps"] = []
        for s in range(3):
            step = s + 1
            lr = np.float32(1e-3) * np.float32(1.0 - 0.2 * s)
            bc1, bc2 = 1.0 - float(b1) ** step, math.sqrt(1.0 - float(b2) ** step)
            st = dict(step=step, lr=float(lr), flag=int(c["guard"] and s == 1))
            if c["state"] or c["guard"]:                                # read through pointers: inputs, fp32
                st.update(bc1=float(np.float32(bc1)), bc2=float(np.float32(bc2)), E1=0.0, E2=0.0)
            else:                                                       # by value: the library's host powf, 2 ulp
                st.update(bc1=bc1, bc2=bc2, E1=4 * U * float(b1) ** step + U * bc1, E2=(4 * U * float(b2) ** step + U * bc2 * bc2) / (2 * bc2) + U * bc2)
            t["steps"].append(st)
        return t
    return {}


# ------------------------------------------------------------------------------------------------ roundings restated (the emulation's own)
def bf16_bits_rne(x32, truncate=False):
    """fp32 tensor -> bf16 bit patterns (int32 holding 16 bits), round to nearest even in integer arithmetic"""
    b = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if not truncate:
        b = b + 0x7FFF + ((b >> 16) & 1)
    return ((b >> 16) & 0xFFFF).to(torch.int32)


def f16_bits_sat(x32, truncate=False):
    """fp32 tensor -> fp16 bit patterns, to nearest even and saturating (numpy's conversion; truncate: toward zero)"""
    a = np.clip(x32.numpy().astype(np.float64), -65504.0, 65504.0)
    h = a.astype(np.float16)
    if truncate:
        over = np.abs(h.astype(np.float64)) > np.abs(a)
        h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return torch.from_numpy(h.view(np.int16).astype(np.int32) & 0xFFFF)


def bits16(x):
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


# ------------------------------------------------------------------------------------------------ references and emulations
def dropped(c, t):
    """the fp32 value the kernel rounds or stores: x, or x * dscale in fp32 (a rounding point), or +0"""
    x = t["x"]
    if t["keep"] is None:
        return x
    return torch.where(t["keep"], x * torch.tensor(t["sc"], dtype=F32), torch.zeros_like(x))


def reference(c, t):
    """-> {name: (value, bound)}; bound None: EQUAL (16-bit values: as bit patterns)"""
    k = c["kind"]
    if k == "cast":
        return dict(y=(bits16(round16(dropped(c, t).to(F64), F16 if c["f16"] else BF16)), None))
    if k == "dropout":
        return dict(y=(dropped(c, t), None))
    if k == "cast_hb":
        return dict(y=(bits16(t["x"].float().bfloat16()), None))
    if k == "cast_b32":
        return dict(y=(torch.from_numpy((bits16(t["x"]).numpy().astype(np.uint32) << 16).view(np.float32)), None))       # the bits, 16 places up
    if k == "axpy":
        ax, y = float(np.float32(c["a"])) * t["x"].to(F64), t["y"].to(F64)            # (a reaches the kernel as a C float)
        return dict(y=(ax + y, 2 * U * (ax.abs() + y.abs())))
    if k == "gelu":
        r = gelu64(t["u"].to(F64)).to(BF16)
        return dict(y=(r.to(F64), 4 * GELU_G_MEASURED["gelu"] + ulp16(r)))
    if k == "colsum":
        v = t["x"].to(F64)
        s = v.sum(0)
        return dict(out=(s, None if c["mode"] == "exact" else colsum_depth(c["rows"]) * U * (v.abs().sum(0) + FILL)))
    if k == "sumsq":
        x = t["x"].to(F64)
        fin = torch.isfinite(t["x"])
        cnt = int((~fin).sum())
        x32sq = t["x"] * t["x"]                                    # (fp32: a finite 3e38 squares to inf)
        s = float("nan") if cnt else (float("inf") if bool(torch.isinf(x32sq).any()) else float((x * x).sum()))
        b = None if c["mode"] == "exact" or cnt or math.isinf(s) else (sumsq_depth(c) + 8) * U * s
        return dict(sum=(s, b), count=(cnt, None))
    if k == "adam":
        return adam_chain(c, t, F64)
    raise KeyError(k)


def emulate(c, t, mut=None):
    """the same operations in fp32 (mut: a wrong build the checks must see) -> {name: value}"""
    k = c["kind"]
    if k == "cast":
        v = dropped(c, t)
        return dict(y=f16_bits_sat(v, mut == "truncate") if c["f16"] else bf16_bits_rne(v, mut == "truncate"))
    if k == "dropout":
        return dict(y=dropped(c, t))
    if k == "cast_hb":
        return dict(y=bf16_bits_rne(torch.from_numpy(t["x"].view(torch.int16).numpy().view(np.float16).astype(np.float32))))
    if k == "cast_b32":
        return dict(y=t["x"].float())
    if k == "axpy":
        return dict(y=t["y"] + torch.tensor(c["a"], dtype=F32) * t["x"])
    if k == "gelu":
        u = t["u"].float()
        return dict(y=(u * 0.5 * (1.0 + torch.erf(u * 0.70710678118654752440))).to(BF16).to(F64))
    if k == "colsum":
        x = t["x"].float()
        if mut == "over_ld":                                     # the rows taken as cols elements apart: the NaN padding enters the sums
            pad = torch.cat([x, torch.full((c["rows"], c["ld"] - c["cols"]), float("nan"))], 1).reshape(-1)
            x = pad[:c["rows"] * c["cols"]].view(c["rows"], c["cols"])
        return dict(out=x.sum(0).to(F64))
    if k == "sumsq":
        x = t["x"]
        cnt = int((x != x).sum()) if mut == "nan_only" else int(((x.view(torch.int32) & 0x7F800000) == 0x7F800000).sum())
        return dict(sum=float((x * x).sum()), count=cnt)
    if k == "adam":
        return {n: v[0] for n, v in adam_chain(c, t, F32, mut).items()}
    raise KeyError(k)


ADAM_MUTATIONS = ("eps_inside", "bc2_on_v", "adamw")


def adam_chain(c, t, dt=F64, mut=None):
    """three steps -> {p, m, v: (value, bound)} after the last (masked elements and flagged steps keep what they held)"""
    f = lambda x: x.to(dt)
    T = lambda x: torch.tensor(float(x), dtype=dt)
    p, m, v = f(t["p"]), f(t["m"]), f(t["v"])
    Lp, Lm, Lv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-8)
    ob1, ob2 = T(np.float32(1) - b1), T(np.float32(1) - b2)                # fp32 differences, as the kernel forms them
    b1, b2, eps = T(b1), T(b2), T(eps)
    wd, gs = T(np.float32(c["wd"])), T(np.float32(c["gs"] if c["gs"] is not None else 1.0))
    live = torch.ones(p.shape, dtype=torch.bool) if not c["mask"] else ~t["skip"].bool().repeat_interleave(8)[:p.numel()]
    for st, g in zip(t["steps"], t["g"]):
        if st["flag"]:
            continue
        lr, bc1, bc2 = T(np.float32(st["lr"])), T(st["bc1"]), T(st["bc2"])
        if dt == F32 and not st["E1"] == 0.0:
            bc1, bc2 = T(np.float32(1) - np.power(np.float32(0.9), np.float32(st["step"]))), T(np.sqrt(np.float32(1) - np.power(np.float32(0.999), np.float32(st["step"]))))
        gsc = f(g) * gs
        gi = gsc + wd * p if c["wd"] != 0 and mut != "adamw" else gsc
        mi = b1 * m + ob1 * gi
        vi = b2 * v + ob2 * gi * gi
        r = torch.sqrt(vi)
        if mut == "eps_inside":
            den = torch.sqrt(vi + eps) / bc2
        elif mut == "bc2_on_v":
            den = torch.sqrt(vi / bc2) + eps
        else:
            den = r / bc2 + eps
        step = (lr / bc1) * mi / den
        pn = p - step
        if mut == "adamw" and c["wd"] != 0:
            pn = pn - lr * wd * p
        if dt == F64:
            Lg = 3 * U * (gsc.abs() + (wd * p).abs()) + wd * Lp
            Lmn = 3 * U * ((b1 * m).abs() + (ob1 * gi).abs()) + b1 * Lm + ob1 * Lg
            Lvn = 3 * U * (b2 * v + ob2 * gi * gi) + b2 * Lv + 2 * ob2 * gi.abs() * Lg
            Lr = torch.where(vi > 0, Lvn / (2 * r.clamp(min=1e-300)), torch.sqrt(Lvn)) + U * r
            Lden = Lr / bc2 + 2 * U * den + den * st["E2"] / bc2
            Lstep = step.abs() * (3 * U + st["E1"] / bc1 + Lden / den) + (lr / bc1) * Lmn / den
            Lpn = Lp + Lstep + U * pn.abs()
            Lp, Lm, Lv = torch.where(live, Lpn, Lp), torch.where(live, Lmn, Lm), torch.where(live, Lvn, Lv)
        p, m, v = torch.where(live, pn, p), torch.where(live, mi, m), torch.where(live, vi, v)
    return dict(p=(p, Lp), m=(m, Lm), v=(v, Lv))


def evaluate(c, ref, got):
    """-> {name: (ratio, gain)}: an EQUAL output scores 0 or inf"""
    res = {}
    for k, (r, b) in ref.items():
        g = got[k]
        if not torch.is_tensor(r):
            same = (g == r) or (isinstance(r, float) and math.isnan(r) and math.isnan(g))
            res[k] = ((0.0 if same else float("inf")) if b is None else (abs(g - r) / b if b > 0 else (0.0 if g == r else float("inf"))), 0.0)
        elif b is None:
            same = torch.equal(g.view(torch.int32), r.view(torch.int32)) if r.dtype == F32 else torch.equal(g.to(r.dtype), r)
            res[k] = (0.0 if same else float("inf"), 0.0)
        else:
            res[k] = (worst_ratio(g.to(F64), r, b), gain(g.to(F64), r, b) if r.numel() >= 64 else 0.0)
    return res


@functools.lru_cache(maxsize=2)
def prepared(i):
    c = CASES[i]
    t = make_inputs(c)
    return t, reference(c, t)


# ------------------------------------------------------------------------------------------------ the step state
M64 = (1 << 64) - 1


def splitmix64(x):
    """-> (the advanced state, the mixed word): step_state_advance_kernel's salt pair"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return x, z ^ (z >> 31)


def step_lr(k, base_lr, warmup, total):
    """the learning rate of scheduler step k in the kernel's two fp32 operations: a correctly rounded division, one product"""
    f = np.float32
    lam = f(k) / f(max(1, warmup)) if k < warmup else max(f(0), f(total - k) / f(max(1, total - warmup)))
    return f(base_lr) * f(lam)


def step_bias(t, b1=0.9, b2=0.999):
    """float64 (1 - b1^t, sqrt(1 - b2^t)) of the fp32 betas, and the bound 2 ulp of powf carries through them"""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    bc1, bc2 = 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t)
    return (bc1, 4 * U * b1 ** t + U * bc1), (bc2, (4 * U * b2 ** t + U * bc2 * bc2) / (2 * bc2) + U * bc2)
