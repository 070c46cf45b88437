"""The LoRA kernels' case table, an independent statement of their launch plans, and the float64 reference of their contract.

Shared by tests/test_lora_cpu.py (the library's mmdti_lora_plan against `expected_plan` for every case and a sweep past them; the
case table reaches every row of the MMDTI_PLAN_LORA table) and tests/test_lora_instances_gpu.py (every case on the device against the
reference below).  Nothing here imports the library.

Contract (include/mmdti_hip.h): x [T, in], A [r, in], B [out, r], s = alpha / r.
    forward   t = bf16(x.A^T);  y <- round16(float(y) + s.t.B^T), an element whose update is zero keeps its bits
    backward  u = bf16(s.dy.B);  dB += s.dy^T.t;  dA += u^T.x
    dx        dx += u.A (fp32, or bf16 rounded to nearest even)
The reference works on the operands exactly as the kernel reads them: the second product of the forward reads the t the first one
STORED (in the fp16 mode converted to fp16), dA and dx read the stored u -- each product is held to its own bound.

Bound (the method of tests/gemm_cases.py): |got - v| <= (K + 8) * 2^-23 * T + R elementwise, v the UNROUNDED float64 value, K the accumulation length (in, r,
out or the token rows), T the sum of the magnitudes of the products and of what is accumulated onto, R the rounding of a 16-bit
output (gemm_cases.rounding_term).
"""
import torch

LORA_FAMILY = 9         # MMDTI_PLAN_LORA
LORA_KERNELS = 27
RANKS = (8, 16, 32)
ROWS = 128              # forward / dx: token rows per workgroup
COLS = 256              # columns per staged block
DET_WGS = 64
CUS = 256

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64


def C(entry, T, n_in, n_out, r, flag=False, sliced=False, det=False, small_ws=False):
    return dict(entry=entry, T=T, n_in=n_in, n_out=n_out, r=r, flag=flag, sliced=sliced, det=det, small_ws=small_ws)


def case_id(c):
    return (f"{c['entry']}-T{c['T']}-in{c['n_in']}-out{c['n_out']}-r{c['r']}" + (f"-flag{int(c['flag'])}" if c["flag"] else "") + ("-slice" if c["sliced"] else "")
            + ("-det" if c["det"] else ""))


# flag: a saved fp16 x beside the bf16 dy (bwd), a bf16 dx (dx); fwd: 0 bf16, 1 fp16 operands and y, 2 fp16 operands beside a bf16 y.
#  sliced: y / dy is the middle third of a
# [T, 3 out] buffer.  T: one row, a ragged last tile, more than one workgroup; 16385 / 32769: the 128- and 256-row chunks of the
# backward; 4161 in the deterministic mode: more chunks than workgroups.  320: a staged block of 256 columns and a remainder of 64.
FWD_CASES = [
    C("fwd", 1, 64, 64, 8), C("fwd", 63, 512, 512, 16, flag=True, sliced=True), C("fwd", 130, 512, 1536, 32),
    C("fwd", 257, 64, 1536, 8, flag=True), C("fwd", 257, 512, 64, 32, flag=True, sliced=True), C("fwd", 130, 64, 512, 16, sliced=True),
    C("fwd", 63, 64, 64, 8, flag=2, sliced=True), C("fwd", 257, 512, 1536, 16, flag=2, sliced=True), C("fwd", 130, 64, 512, 32, flag=2),
]
BWD_CASES = [
    C("bwd", 1, 64, 64, 8), C("bwd", 63, 512, 512, 16, flag=True, sliced=True), C("bwd", 130, 512, 1536, 32, sliced=True),
    C("bwd", 257, 64, 1536, 8, flag=True), C("bwd", 257, 512, 64, 32, flag=True), C("bwd", 130, 64, 512, 16),
    C("bwd", 130, 320, 320, 16),
    C("bwd", 16385, 64, 64, 8), C("bwd", 32769, 64, 64, 16, flag=True),
    C("bwd", 257, 512, 512, 8, det=True), C("bwd", 63, 64, 64, 8, flag=True, det=True),
    C("bwd", 130, 64, 1536, 16, flag=True, sliced=True, det=True), C("bwd", 257, 320, 64, 16, det=True),
    C("bwd", 257, 512, 64, 32, det=True), C("bwd", 130, 64, 512, 32, flag=True, det=True),
    C("bwd", 4161, 64, 64, 32, det=True),
]
DX_CASES = [
    C("dx", 1, 64, 64, 8), C("dx", 63, 512, 64, 16, flag=True), C("dx", 130, 512, 64, 32), C("dx", 257, 64, 64, 8, flag=True),
    C("dx", 257, 512, 64, 32, flag=True), C("dx", 130, 64, 64, 16), C("dx", 130, 320, 64, 16, sliced=True),
]
CASES = FWD_CASES + BWD_CASES + DX_CASES
# refused before a launch: (r, in, out, the words the message must hold)
REFUSED = [(12, 64, 64, "rank must be 8, 16 or 32"), (8, 72, 64, "in must be a multiple of 64"), (8, 64, 100, "out must be a multiple of 64")]


# ------------------------------------------------------------------------------------------------ plans
def rank_index(r):
    return RANKS.index(r)


def kernel_name(entry, r, flag, det=False):
    b = lambda v: "true" if v else "false"   # noqa: E731
    if entry == "fwd":
        return f"lora_fwd_kernel<{r}, {b(flag)}, {b(int(flag) == 1)}>"
    if entry == "bwd":
        return f"lora_bwd_kernel<{r}, {b(flag)}, {b(det)}>"
    return f"lora_dx_kernel<{r}, {b(flag)}>"


def kernel_key(entry, r, flag, det=False):
    if entry == "fwd":
        return 3 * rank_index(r) + int(flag)
    if entry == "bwd":
        return 9 + 4 * rank_index(r) + 2 * int(flag) + int(det)
    return 21 + 2 * rank_index(r) + int(flag)


def bwd_chunk_rows(T):
    """the fewest of 64, 128, 256 token rows per chunk that leave at most one chunk per CU (256 past that)"""
    for rows in (64, 128):
        if -(-T // rows) <= CUS:
            return rows
    return 256


def expected_plan(entry, T, n_in, n_out, r, flag=False, det=False):
    """what ops.lora_plan must return"""
    key = kernel_key(entry, r, flag, det and entry == "bwd")
    if entry in ("fwd", "dx"):
        lds = (ROWS if entry == "fwd" else COLS) * (r + 8) * 2
        return {"nlaunch": 1, "launches": [dict(key=key, gx=-(-T // ROWS), gy=1, block=256, lds=lds)], "chunk_rows": ROWS, "slab_floats": 0}
    rows = bwd_chunk_rows(T)
    chunks = -(-T // rows)
    lds = (64 * (COLS + 8) + r * (COLS + 8) + 64 * (r + 8) + 256 * (r + 8)) * 2
    k0 = dict(key=key, gx=min(chunks, DET_WGS) if det else chunks, gy=1, block=256, lds=lds)
    if not det:
        return {"nlaunch": 1, "launches": [k0], "chunk_rows": rows, "slab_floats": 0}
    fold = lambda n: dict(key=-1, gx=-(-n // 64), gy=1, block=1024, lds=0)   # noqa: E731
    return {"nlaunch": 3, "launches": [k0, fold(n_out * r), fold(r * n_in)], "chunk_rows": rows, "slab_floats": r * (n_in + n_out)}


def det_workspace_bytes(T, n_in, n_out, r):
    p = expected_plan("bwd", T, n_in, n_out, r, det=True)
    return p["launches"][0]["gx"] * p["slab_floats"] * 4


# ------------------------------------------------------------------------------------------------ operands and reference
def act_dtype(flag):
    return F16 if flag else BF16


def operands(c, seed=0):
    """seeded host tensors of a case (16-bit values exactly representable in their type; gradients start non-zero)"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * c["T"] + c["n_in"] + 3 * c["n_out"] + c["r"])
    T, n_in, n_out, r = c["T"], c["n_in"], c["n_out"], c["r"]
    rnd = lambda *s: torch.randn(*s, generator=g)   # noqa: E731
    o = {"scale": 16.0 / r}
    if c["entry"] == "fwd":
        dt = act_dtype(c["flag"])
        o["x"], o["A"], o["B"] = rnd(T, n_in).to(dt), (rnd(r, n_in) * n_in ** -0.5).to(dt), (rnd(n_out, r) * 0.2).to(dt)
        o["ybuf"] = rnd(T, 3 * n_out if c["sliced"] else n_out).to(F16 if int(c["flag"]) == 1 else BF16)
    elif c["entry"] == "bwd":
        o["x"] = rnd(T, n_in).to(act_dtype(c["flag"]))
        o["dybuf"] = (rnd(T, 3 * n_out if c["sliced"] else n_out) * 0.1).to(BF16)
        o["t"], o["B"] = rnd(T, r).to(BF16), (rnd(n_out, r) * 0.2).to(BF16)
        o["dA"], o["dB"] = rnd(r, n_in), rnd(n_out, r)
    else:
        o["u"], o["A"] = (rnd(T, r) * 0.1).to(BF16), (rnd(r, n_in) * n_in ** -0.5).to(BF16)
        dxbuf = rnd(T, n_in + 64 if c["sliced"] else n_in)
        o["dxbuf"] = dxbuf.to(BF16) if c["flag"] else dxbuf
    return o


def view(c, buf, cols):
    """the [T, cols] matrix a case's kernel sees of its buffer (a column slice when the case says so)"""
    if not c["sliced"]:
        return buf
    return buf[:, cols:2 * cols] if c["entry"] != "dx" else buf[:, 64:64 + cols]


def rounding_term(ref, dtype):
    if dtype == BF16:
        return 2.0 ** -8 * ref.abs()
    if dtype == F16:
        return 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return torch.zeros_like(ref)


def product(a, b, acc0=None, scale=1.0):
    """scale * a.b^T (+ acc0) in float64, and the sum of magnitudes its bound needs"""
    a, b = a.to(F64), b.to(F64)
    v, T = scale * (a @ b.T), abs(scale) * (a.abs() @ b.abs().T)
    if acc0 is not None:
        v, T = v + acc0.to(F64), T + acc0.to(F64).abs()
    return v, T


def unit(K):
    return (K + 8) * 2.0 ** -23


def ref_t(o):
    v, T = product(o["x"], o["A"])
    return v, unit(o["x"].shape[1]) * T + rounding_term(v, BF16)


def ref_y(c, o, t_stored):
    """y after the update, from the t the kernel stored"""
    dt = o["ybuf"].dtype
    t_op = t_stored.to(F16) if o["x"].dtype == F16 else t_stored
    y0 = view(c, o["ybuf"], c["n_out"])
    d, Td = product(t_op, o["B"], scale=o["scale"])
    v = y0.to(F64) + d
    return v, unit(c["r"]) * (Td + y0.to(F64).abs()) + torch.where(d == 0, torch.zeros_like(v), rounding_term(v, dt))


def ref_u(c, o):
    dy = view(c, o["dybuf"], c["n_out"])
    v, T = product(dy, o["B"].T, scale=o["scale"])
    return v, unit(c["n_out"]) * T + rounding_term(v, BF16)


def x_as_read(o):
    """the backward reads a saved fp16 activation rounded to bf16"""
    return o["x"].to(F32).to(BF16)


def ref_dB(c, o):
    dy = view(c, o["dybuf"], c["n_out"])
    v, T = product(dy.T, o["t"].T, acc0=o["dB"], scale=o["scale"])
    return v, unit(c["T"]) * T


def ref_dA(c, o, u_stored):
    v, T = product(u_stored.T, x_as_read(o).T, acc0=o["dA"])
    return v, unit(c["T"]) * T


def ref_dx(c, o):
    dx0 = view(c, o["dxbuf"], c["n_in"])
    v, T = product(o["u"], o["A"].T, acc0=dx0)
    dt = dx0.dtype
    return v, unit(c["r"]) * T + rounding_term(v, dt)
