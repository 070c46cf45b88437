"""The case table of the pair-attention instance tests, their input builders, float64 reference, bounds and fp32 emulation, shared by
test_pair_cases_cpu.py (which proves that the table reaches every kernel instance and every ragged body, that the reference agrees
with float64 autograd, that the exact modes are exact, and that an fp32 emulation of the kernels' rounding points stays inside the
bounds while two wrong emulations do not) and test_pair_instances_gpu.py (which holds the kernel instances of csrc/pair_attn.hip,
pair_attn_bwd.hip, pair_attn_bwd_mfma.h and pair_attn_bwd_g16.hip to the reference on the device).

INSTANCES (instances() / blocks(): the independent statement of what each case is declared to run; the CPU test holds the library's own
answer, mmdti_pair_attn_plan, to it for every case and for a sweep of every size, the GPU suite before every launch; SOURCE_LINES keeps
the device-side rules it mirrors verbatim).  MFMA kernels serve ld % 4 == 0, 16-byte aligned planes and N <= 272; everything else runs the per-element
kernels <NCH = ceil(N / 64)> (backward: x deterministic mode).  fp32 planes (layout 0 row-major, 1 tiled) run the buckets NT = 5 / 9 /
13 / 17, tiled ones FULL when ceil(N / 16) == NT; compact planes (3: fp16 logits, 7: bf16 gradients too) have one instantiation per
tile count, dense and ragged, the forward also for fp16 q | k | v.  The backward's NW (3 or 4 waves) follows its workgroup size.
85 forward + 98 backward instances; the ragged kernels branch into one of 86 (tile count, covered tiles) bodies per direction.

TABLE.  Tile count k of the compact planes runs five kinds -- dense, dense with fp16 q | k | v and bf16 G, ragged with bf16 G, ragged with
fp16 q | k | v, ragged on packed token rows --, each kind (so each instance) at the three edge sizes N = 16 (k - 1) + 1 (one query and one
key group in the last block), 16 (k - 1) + 6 (N % 4 != 0) and 16 k (no EDGE block): every mode at one of them, rotating from one tile
count to the next, the exact modes and `random` at the other two (k = 1: every kind at N = 1 and 16 and at one of 4, 5, 12, 13).  A ragged batch holds one molecule
per supported covered-tile count of its kernel, one whose count rounds up to the next supported one, and one of a single atom.
B = H = 3 (xcd_chunk has a remainder) but for one case at H = 64 and one at B H = 16.

PACKED ROWS (read off the kernels): molecule b owns rows [row_off[b], row_off[b + 1]) -- its n real tokens and, if n < N, ONE pad row,
position n.  That row is computed as a query like any other and is a padded key; its dk / dv rows are written, as zeros.  Queries
past it do not exist: their S / G rows keep what they held, no O / dqkv row belongs to them, they add nothing to dk / dv.

REFERENCE (reference()): float64 on the stored 16-bit operands, per (molecule, head); c = 1 / (1 - p_drop), kappa the keep mask:
    S = bias + scale q.k^T   (-inf at padded keys; compact planes: min(S, 65504) rounded to fp16)       [logits(), checked on its own]
  and, on the logits the DEVICE stored, widened exactly (what the kernels themselves read back):
    p = softmax(S_stored)    P' = c kappa p    O = P' v    dP = c kappa (dO.v^T)    delta = sum_j dP p
    G_out = p (dP - delta) + G_in     dq = scale G_out k     dk = scale G_out^T q     dv = P'^T dO
  (layout 7 stores bf16(G_out), the products use the unrounded value; with fp16 q | k | v the backward multiplies their bf16 roundings).

MODES
  selector  bias 0 at one key per query and -200 elsewhere, q, k, v, dO, G_in small integers, scale 2^-2, k[7] = 1 and q[7] chosen so
            that the winner's logit is 0, +-1 or 2: m log2e is then exact in fp32, the fma against it is 0 and exp2 gives 1; every
            loser lies >= 183 below, exp2(-264) is 0 in fp32.  P is one-hot: S, O = v_sel, dv, G_out = G_in, dq, dk bit for bit.
  uniform   bias 0 on n <= 16 real keys (a power of two, scattered), the rest padded; integer operands, q = 0 (`uq`: dq live) or
            k = 0 (`uk`: dk live): S = 0, p = 1 / n, every term a multiple of 2^-10 (exactness()).  Outputs EQUAL the reference.
  random    randn q, k, v, dO, G_in, bias 3 randn, scale 8^-1/2.
  saturate  (compact) random with q x 16 and some bias entries at 65504: the stored logits saturate, nothing is NaN or +inf.
  dropout   random at p = 0.1 / 0.35 with the keep mask recovered from the device's forward.

BOUNDS (first-order in eps = 2^-23; u = 2^-16 for the bf16 hi + lo pairs of the MFMA kernels, 2^-22 (+ 2^-24 absolute per term: fp16
underflow) for the fp16 pairs of the fp16-operand forward, 0 in the per-element kernels; R = gemm_cases.rounding_term of the output;
eta = 2^-126 covers the flush of a denormal probability, low part or gradient -- v_exp_f32 and the matrix pipe flush them, float64 and
the CPU keep them: O, dv + eta c sum |v| (|dO|), E_G + eta (|dP| + |delta| + 1)):
  S          8 exact products accumulated in fp32, scaled, added to the bias:   E_S = 10 eps (|scale| sum_d |q||k| + |bias|)
             (compact: + half an fp16 step, rounding_term(fp16))
  e          exp2(fma(S, log2e, -fl(m log2e))) / __expf(S - m): rounding of m log2e, of the fma, of log2e itself, v_exp_f32:
                 eps_ij = eps (|m_i| + 2 |S_ij - m_i| + 2)                                      [relative]
  p          row sum over N terms, dscale / lsum, the product:   rho_ij = eps_ij + sum_l p_il eps_il + (N + 4) eps
  O, dv      u T + sum rho P' |v| + (N + 24) eps T + R,   T = sum P' |v|      (dv: |dO|, over queries -- query blocks, then waves)
  dP         E_dP = c kappa 8 eps sum_d |dO||v| + eps |dP|
  delta      E_d = sum_j p (E_dP + |dP| (rho + eps)) + (N + 8) eps sum_j |dP| p
  G          the cancellation in dP - delta: absolute errors
                 E_G = p (E_dP + E_d + 2 eps (|dP| + |delta|)) + rho p |dP - delta| + 2 eps (p |dP - delta| + |G_in|)
             (layout 7: + rounding_term(bf16) on the stored value only)
  dq, dk     |scale| (u T + sum E_G |k| + (N + 24) eps T) + R,   T = sum |G_out| |k|    (dk: |q|, over queries)
GAIN: attn_cases.gain, |z| <= Z_MAX = 6 on every 16-bit output: what sees a systematic 2^-9.  (O rows of a query with ONE real key are
left out of the gain, not of the elementwise bound: each is the same c v row, rounded the same way -- N copies of one error.)"""
import torch

from gemm_cases import F64, SENT16, SENT32, Arena, round16, rounding_term, worst_ratio  # noqa: F401
from attn_cases import EPS, ETA, Z_MAX, gain  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
HD = 8
PA_MAX_NT = 17
SEED, SITE = 20240607, 5
LOG2E32 = torch.tensor(1.44269504088896340736, dtype=F32)

# the device-side rules (pa_kt_effective, the size limit) that instances() and geometry() mirror; what the launchers choose is asked of the
# library (library_plan)
SOURCE_LINES = {
    "pair_attn_plan.h": (
        "__host__ __device__ constexpr int pa_kt_step(int nt) { return nt <= 9 ? 1 : (nt <= 13 ? 2 : 4); }",
        "const int s = pa_kt_step(nt), k = ((kt < 1 ? 1 : kt) + s - 1) / s * s;",
        "return k >= nt ? nt : k;",
    ),
    "pair_attn.h": ("MMDTI_REQUIRE(N <= 320,",),
}
PTR = 0x10000          # a fake, 16-byte aligned device address: mmdti_pair_attn_plan never dereferences one


# ------------------------------------------------------------------------------------------------ layout arithmetic (mirrors of ops / common.h)
def pair_ld(N):
    return (N + 3) // 4 * 4


def pair_plane(N):
    return (N * pair_ld(N) + 7) // 8 * 8


def tiles(N):
    return (N + 15) // 16


def pa_kt_step(nt):
    return 1 if nt <= 9 else (2 if nt <= 13 else 4)


def pa_kt_effective(kt, nt):
    s = pa_kt_step(nt)
    k = (max(kt, 1) + s - 1) // s * s
    return nt if k >= nt else k


def supported_counts(nt):
    """the covered-tile counts pa_dispatch_kt<NT, NT> has a body for"""
    s = pa_kt_step(nt)
    return [k for k in range(s, nt, s)] + [nt]


def fwd_block(nqb):
    return 192 if nqb % 3 == 0 else (64 * nqb if nqb < 4 else 256)


def bwd_block(nqb):
    return 192 if (nqb % 3 == 0 or nqb >= 16 or nqb == 5) else (64 * nqb if nqb < 4 else 256)


def mfma(c):
    return c["ld"] % 4 == 0 and not c["shift"] and c["N"] <= 16 * PA_MAX_NT


def instances(c):
    """-> (forward kernel, backward kernel, {(tile count, covered tiles)} of the ragged bodies the case's molecules branch into)"""
    N, lay = c["N"], c["layout"]
    tiled, compact, g16 = lay & 1, (lay >> 1) & 1, (lay >> 2) & 1
    nqb = tiles(N)
    if not mfma(c):
        assert lay == 0 and c["lens"] is None and not c["f16"]
        nch = min((N + 63) // 64, 5)
        return f"pair_attn_fwd_kernel<{nch}>", f"pair_attn_bwd_kernel<{nch}, {'true' if c['det'] else 'false'}>", set()
    nw = 3 if bwd_block(nqb) == 192 else 4
    if compact:
        rag = "true" if c["lens"] is not None else "false"
        fwd = f"pair_attn_fwd_mfma_kernel<{nqb}, true, true, {rag}, _Float16{', true' if c['f16'] else ''}>"
        bwd = f"pair_attn_bwd_mfma_kernel<{nqb}, true, true, {nw}, {rag}, _Float16, {'__bf16' if g16 else 'float'}>"
        bodies = set() if c["lens"] is None else {(nqb, pa_kt_effective(min(tiles(n), nqb), nqb)) for n in c["lens"]}
        return fwd, bwd, bodies
    assert c["lens"] is None and not c["f16"]
    nt = 5 if nqb <= 5 else 9 if nqb <= 9 else 13 if nqb <= 13 else 17
    tl, fl = ("true", "true" if nqb == nt else "false") if tiled else ("false", "false")
    return (f"pair_attn_fwd_mfma_kernel<{nt}, {tl}, {fl}, false, float>", f"pair_attn_bwd_mfma_kernel<{nt}, {tl}, {fl}, {nw}, false, float, float>", set())


def blocks(c):
    """workgroup sizes of the two launches"""
    return (fwd_block(tiles(c["N"])), bwd_block(tiles(c["N"]))) if mfma(c) else (256, 256)


def declared_plan(c, backward):
    """what a case is declared to launch, from instances() and blocks(): (kernel, grid, workgroup size, nqb, NW)"""
    f, b, _ = instances(c)
    nqb = tiles(c["N"]) if mfma(c) else 0
    nw = (3 if bwd_block(nqb) == 192 else 4) if backward and nqb else 0
    return (b if backward else f, c["B"] * c["H"], blocks(c)[int(backward)], nqb, nw)


def library_plan(lib, c, backward, ptr=None):
    """mmdti_pair_attn_plan's answer in the form of declared_plan.  ptr: the addresses of a launch (qkv, s, g, o, dqkv: for the forward s is
    bias_in, g is s_out); default: fake aligned ones, the planes 4 bytes off in a `shift` case."""
    import ctypes
    plane = PTR + (4 if c["shift"] else 0)
    ptr = ptr or dict(qkv=PTR, s=plane, g=plane, o=PTR, dqkv=PTR)
    out = (ctypes.c_int * 6)()
    lib.mmdti_pair_attn_plan(int(backward), int(c["det"]), ptr["qkv"], ptr["s"], ptr["o"], ptr["g"], ptr["dqkv"], c["B"], c["N"], c["H"], c["ld"], 0.0,
                             c["layout"] if backward else c["layout"] & 3, PTR if c["lens"] is not None else 0, PTR if c["packed"] else 0, int(c["f16"]), out)
    family, key, grid, block, nqb, nw = list(out)
    name = lib.mmdti_plan_kernel_name(2 + family, key).decode()
    if name.startswith("pair_attn_bwd_kernel<") and "," not in name:          # (the table leaves the defaulted DET = false out)
        name = name[:-1] + ", false>"
    return (name, grid, block, nqb, nw)


def assert_declared_plan(lib, c, backward, ptr=None):
    got, want = library_plan(lib, c, backward, ptr), declared_plan(c, backward)
    assert got == want, (case_id(c), backward, got, want)


# ------------------------------------------------------------------------------------------------ the table
CASES = []
MODES32 = ("selector", "uq", "uk", "random", "dropout")
MODES16 = MODES32 + ("saturate",)
EDGE_MODES = ("selector", "uq", "uk", "random")     # what an instance runs at its two other edge sizes
# the padding mask of a dense run, by mode (uniform modes pad everything but their n real keys; ragged cases pad by length):
MASK_OF = {"selector": None, "uq": "third", "uk": None, "random": "third", "saturate": None, 0.1: "third", 0.35: None}


def add(N, layout, B=3, H=3, ld=None, lens=None, packed=False, f16=False, det=False, shift=False, one=False, modes=None):
    c = dict(N=N, layout=layout, B=B if lens is None else len(lens), H=H, ld=pair_ld(N) if ld is None else ld, lens=lens, packed=packed, f16=f16,
             det=det, shift=shift, one=one, modes=modes or (MODES16 if layout & 2 else MODES32), drop=(0.1, 0.35))
    assert not packed or lens is not None
    CASES.append(c)
    return c


def ragged_lens(N):
    """one molecule per supported covered-tile count, one whose count rounds up (where counts are skipped), one single atom"""
    nt = tiles(N)
    lens = [N if ke == nt else 16 * ke - 3 for ke in supported_counts(nt)]
    s = pa_kt_step(nt)
    if s > 1:
        lens.append(16 * s + 2)                      # s + 1 tiles: runs as 2 s
    if len(lens) < 9 and N > 1:
        lens.append(1)
    if len(lens) < 2:
        lens.append(max(1, N - 1))
    return tuple(lens[1:] + lens[:1])


def _edges(k):
    return (16 * (k - 1) + 1, 16 * (k - 1) + 6, 16 * k)


def _build():
    kinds = (dict(layout=3), dict(layout=7, f16=True), dict(layout=7, rag=True), dict(layout=3, f16=True, rag=True), dict(layout=3, rag=True, packed=True))
    small = (1, 4, 5, 12, 13, 16)
    for k in range(1, PA_MAX_NT + 1):
        for i, kind in enumerate(kinds):
            kw = dict(kind)
            rag = kw.pop("rag", False)
            if k == 1:                                   # every kind at N = 1 and 16 and at one size in between; all modes at the kind's own size
                Ns = sorted({1, small[i], 16} | ({5} if i == 0 else set()))
                full = small[i]
            else:                                        # every kind at the three edge sizes; all modes at one of them, rotating
                Ns, full = _edges(k), _edges(k)[(k + i) % 3]
            for N in Ns:
                add(N, lens=ragged_lens(N) if rag else None, one=(k % 4 == 2 and not rag and N == full), modes=None if N == full else EDGE_MODES, **kw)
    add(130, 3, B=1, H=64)
    add(70, 7, B=2, H=8)
    # fp32 planes on the MFMA kernels: row-major, tiled, tiled FULL at every (NT, NW) the launchers reach
    for N in (13, 33, 70, 100, 96, 150, 192, 210, 241):
        add(N, 0, one=(N == 100))
    add(54, 0, ld=pair_ld(54) + 4)
    add(7, 0, ld=8)
    for N in (37, 64, 81, 110, 180, 145, 240, 214):
        add(N, 1)
    for N in (65, 80, 130, 200, 258, 272):
        add(N, 1, one=(N == 130))
    # the per-element kernels: by misalignment, by size, by a plane pointer 4 bytes off; each with and without the deterministic mode
    for det in (False, True):
        for N in (9, 70, 130, 200, 258):        # (N = 7 at ld = 8 has aligned rows: it is an MFMA case, added above)
            add(N, 0, ld=N + 1, det=det)
        for N in (273, 300, 320):
            add(N, 0, det=det)
        add(64, 0, shift=True, det=det)
        add(130, 0, shift=True, det=det, one=True)


_build()


def case_id(c):
    f = [f"N{c['N']}", f"L{c['layout']}"]
    if c["ld"] != pair_ld(c["N"]):
        f.append(f"ld{c['ld']}")
    if (c["B"], c["H"]) != (3, 3) and c["lens"] is None:
        f.append(f"B{c['B']}H{c['H']}")
    f += [k for k in ("f16", "det", "shift", "packed") if c[k]]
    if c["lens"] is not None and not c["packed"]:
        f.append("rag")
    return "-".join(f)


def runs(modes=None):
    """(case, mode, p_drop, mask) of every run"""
    out = []
    for c in CASES:
        for m in c["modes"]:
            if modes is not None and m not in modes:
                continue
            if m == "dropout":
                out += [(c, m, p, MASK_OF[p]) for p in c["drop"]]
            else:
                out.append((c, m, 0.0, MASK_OF[m]))
                if m == "random" and c["one"]:
                    out.append((c, m, 0.0, "one"))
    return out


def run_id(r):
    return f"{case_id(r[0])}-{r[1]}" + (f"-p{r[2]}" if r[2] else "") + (f"-{r[3]}" if r[3] else "")


def all_instances():
    """the instantiations the launchers can reach, from the template parameter ranges: (forward set, backward set)"""
    fwd, bwd = set(), set()
    for nch in range(1, 6):
        fwd.add(f"pair_attn_fwd_kernel<{nch}>")
        bwd |= {f"pair_attn_bwd_kernel<{nch}, {d}>" for d in ("false", "true")}
    for nt, lo in ((5, 1), (9, 6), (13, 10), (17, 14)):
        for tl, fl in (("false", "false"), ("true", "false"), ("true", "true")):
            fwd.add(f"pair_attn_fwd_mfma_kernel<{nt}, {tl}, {fl}, false, float>")
            nqbs = (nt,) if fl == "true" else range(lo, nt) if tl == "true" else range(lo, nt + 1)
            for nw in {3 if bwd_block(n) == 192 else 4 for n in nqbs}:
                bwd.add(f"pair_attn_bwd_mfma_kernel<{nt}, {tl}, {fl}, {nw}, false, float, float>")
    for nt in range(1, PA_MAX_NT + 1):
        nw = 3 if (nt % 3 == 0 or nt >= 16 or nt == 5) else 4
        for rag in ("false", "true"):
            fwd |= {f"pair_attn_fwd_mfma_kernel<{nt}, true, true, {rag}, _Float16{h}>" for h in ("", ", true")}
            bwd |= {f"pair_attn_bwd_mfma_kernel<{nt}, true, true, {nw}, {rag}, _Float16, {g}>" for g in ("float", "__bf16")}
    return fwd, bwd


def all_bodies():
    return {(nt, k) for nt in range(1, PA_MAX_NT + 1) for k in supported_counts(nt)}


# ------------------------------------------------------------------------------------------------ geometry of a case
def op_dtype(c):
    return F16 if c["f16"] else BF16


def s_dtype(c):
    return F16 if c["layout"] & 2 else F32


def g_dtype(c):
    return BF16 if c["layout"] & 4 else F32


def geometry(c):
    """-> dict: qlive [B] (query rows that exist), ke [B] (key tiles the kernels cover), cols (keys per row a kernel may write), plane
    (elements per (molecule, head)), idx [N, cols] (flat offset of (query, key) in a plane), rows (token rows), gather [rows] (padded
    position b N + i of every token row), off [B + 1]"""
    N, B, nt = c["N"], c["B"], tiles(c["N"])
    lens = c["lens"]
    ke = [nt if lens is None else pa_kt_effective(min(tiles(n), nt), nt) for n in (lens or [0] * B)]
    qlive = [min(n + 1, N) if c["packed"] else N for n in (lens or [N] * B)]
    q = torch.arange(N).view(N, 1)
    if c["layout"] & 1:
        cols, plane = pair_ld(N), pair_plane(N)
        k = torch.arange(cols).view(1, -1)
        vr = torch.clamp(N - q // 16 * 16, max=16)
        idx = (q // 16 * 16) * pair_ld(N) + vr * (k - k % 4) + (q % 16) * 4 + k % 4
    else:
        cols, plane = (pair_ld(N) if mfma(c) else N), N * c["ld"]
        idx = q * c["ld"] + torch.arange(cols).view(1, -1)
    off = [0]
    for n in qlive:
        off.append(off[-1] + n)
    gather = torch.cat([b * N + torch.arange(qlive[b]) for b in range(B)])
    return dict(qlive=qlive, ke=ke, cols=cols, plane=plane, idx=idx, rows=off[-1], gather=gather, off=off)


def written(c, geo, rag_store=True):
    """[B, N, cols] bool: the slots of a plane that a launch stores (S with rag_store, G without)"""
    N, B = c["N"], c["B"]
    w = torch.zeros(B, N, geo["cols"], dtype=torch.bool)
    for b in range(B):
        w[b, :geo["qlive"][b], :(geo["cols"] if (rag_store or geo["ke"][b] == tiles(N)) else min(16 * geo["ke"][b], geo["cols"]))] = True
    return w


# ------------------------------------------------------------------------------------------------ inputs
def _gen(c, mode, seed, salt=0):
    return torch.Generator().manual_seed(1000003 * seed + 7919 * c["N"] + 31 * c["layout"] + 17 * c["ld"] + 5 * c["B"] + 3 * c["H"] + 101 * salt
                                         + 11 * c["f16"] + 13 * c["packed"] + {"selector": 1, "uq": 2, "uk": 3, "random": 4, "saturate": 5, "dropout": 6}[mode] * 977)


SEEDS = {}            # (case id, mode, mask) -> seed, where the default draw does not give the emulation |z| < 3 (test_pair_cases_cpu.py): none needed


def padding(c, mode, mask, g):
    """[B, N] bool (True: padded key) or None, and for the uniform modes the number of real keys per molecule"""
    B, N = c["B"], c["N"]
    pad = None
    if c["lens"] is not None:
        pad = torch.arange(N).view(1, N) >= torch.tensor(c["lens"]).view(B, 1)
    elif mask == "third":
        pad = torch.zeros(B, N, dtype=torch.bool)
        if N >= 3:
            pad[0, N - N // 3:] = True
    elif mask == "one":
        pad = torch.zeros(B, N, dtype=torch.bool)
        pad[B - 1] = True
        pad[B - 1, N // 2] = False
    n_real = None
    if mode in ("uq", "uk"):
        base = torch.zeros(B, N, dtype=torch.bool) if pad is None else pad
        pad, n_real = torch.ones(B, N, dtype=torch.bool), []
        for b in range(B):
            real = (~base[b]).nonzero().flatten()
            n = 1 << (min(16, real.numel()).bit_length() - 1)
            pad[b, real[torch.randperm(real.numel(), generator=g)[:n]]] = False
            n_real.append(n)
    return pad, n_real


def make_inputs(c, mode, mask=None, seed=None):
    """-> dict: q, k, v [B, N, H, 8], do [B, N, H, 8] (fp32 holding values of the 16-bit operand type), bias, gin [B, H, N, N] fp32 (values of
    the plane's type; gin 0 at padded keys), pad [B, N] bool or None, scale, sel / n_real of the exact modes"""
    seed = SEEDS.get((case_id(c), mode, mask), 0) if seed is None else seed
    B, N, H = c["B"], c["N"], c["H"]
    g = _gen(c, mode, seed)
    ints = lambda shape, r: torch.randint(-r, r + 1, shape, generator=g).to(F32)
    pad, n_real = padding(c, mode, mask, g)
    t = dict(pad=pad, n_real=n_real, sel=None, mode=mode)
    od, sd, gd = op_dtype(c), s_dtype(c), g_dtype(c)
    if mode == "selector":
        t["scale"] = 0.25
        k, q = ints((B, N, H, HD), 2), ints((B, N, H, HD), 2)
        k[..., 7] = 1.0
        sel = torch.zeros(B, H, N, dtype=torch.int64)
        for b in range(B):
            real = torch.arange(N) if pad is None else (~pad[b]).nonzero().flatten()
            for h in range(H):
                sel[b, h] = real[(5 * (torch.arange(N) // 2) + h) % real.numel()]
        ksel = torch.gather(k.permute(0, 2, 1, 3), 2, sel.unsqueeze(-1).expand(B, H, N, HD)).permute(0, 2, 1, 3)      # [B, N, H, 8]: k of the query's key
        target = torch.tensor([0.0, 4.0, -4.0, 8.0])[torch.arange(N) % 4].view(1, N, 1)
        q[..., 7] = target - (q[..., :7] * ksel[..., :7]).sum(-1)
        bias = torch.full((B, H, N, N), -200.0)
        bias.scatter_(3, sel.unsqueeze(-1), 0.0)
        v, do, gin = ints((B, N, H, HD), 8), ints((B, N, H, HD), 2), ints((B, H, N, N), 2)
        t["sel"] = sel
    elif mode in ("uq", "uk"):
        t["scale"] = 0.25
        q, k, v, do = (ints((B, N, H, HD), 1) for _ in range(4))
        (q if mode == "uq" else k).zero_()
        bias, gin = torch.zeros(B, H, N, N), ints((B, H, N, N), 1)
    else:
        t["scale"] = 8 ** -0.5
        rn = lambda *shape: torch.randn(*shape, generator=g)
        q, k, v, do = rn(B, N, H, HD), rn(B, N, H, HD), rn(B, N, H, HD), rn(B, N, H, HD)
        bias, gin = 3.0 * rn(B, H, N, N), rn(B, H, N, N)
        if mode == "saturate":
            q = q * 16.0
            bias[:, :, :, ::7] = torch.where(torch.rand(B, H, N, (N + 6) // 7, generator=g) < 0.3, torch.tensor(65504.0), bias[:, :, :, ::7])
    rnd = lambda x, d: x.to(d).to(F32)
    q, k, v, do = rnd(q, od), rnd(k, od), rnd(v, od), rnd(do, BF16)
    bias, gin = rnd(bias, sd), rnd(gin, gd)
    if pad is not None:
        gin = gin.masked_fill(pad.view(B, 1, 1, N), 0.0)
    t.update(q=q, k=k, v=v, do=do, bias=bias, gin=gin)
    return t


# ------------------------------------------------------------------------------------------------ the reference
def _bh(x, dtype=F64):
    return x.to(dtype).permute(0, 2, 1, 3)                    # [B, N, H, 8] -> [B, H, N, 8]


def _live(c, geo):
    """[B, 1, N, 1] query exists, [B, 1, 1, N] key lies in a covered tile"""
    N, B = c["N"], c["B"]
    ar = torch.arange(N)
    ql = torch.stack([ar < geo["qlive"][b] for b in range(B)]).view(B, 1, N, 1)
    kl = torch.stack([ar < 16 * geo["ke"][b] for b in range(B)]).view(B, 1, 1, N)
    return ql, kl


def logits(c, t, geo, prev=None):
    """-> (S [B, H, N, N] float64, -inf at padded keys, compact planes saturated at 65504 -- NOT rounded to fp16: the device rounds its
    fp32 value, which is held to the fp32 bound plus half an fp16 step of this one; that bound).  prev: the stored logits of the layer below (the second layer of the ragged cases) instead of the case's bias"""
    B, N = c["B"], c["N"]
    Q, K = _bh(t["q"]), _bh(t["k"])
    bias = t["bias"].to(F64) if prev is None else prev
    S = bias + t["scale"] * (Q @ K.transpose(2, 3))
    E = 10 * EPS * (abs(t["scale"]) * (Q.abs() @ K.abs().transpose(2, 3)) + bias.abs())
    if t["pad"] is not None and prev is None:
        S = S.masked_fill(t["pad"].view(B, 1, 1, N), float("-inf"))
    E = torch.where(torch.isfinite(S), E, torch.zeros_like(E))
    if c["layout"] & 2:
        S = S.clamp(max=65504.0)                                             # (pa_round4: saturating above only; -inf stays)
        E = E + torch.where(torch.isfinite(S), rounding_term(S, F16), torch.zeros_like(S))
    return S, E


def reference(c, t, geo, S_st, p_drop=0.0, keep=None, bounds=True, gz=False):
    """S_st [B, H, N, N] float64: the stored logits (whatever sits at queries that do not exist or in tiles that are not covered is
    ignored).  -> float64 O, dq, dk, dv [B, N, H, 8], G [B, H, N, N] (unrounded), and with bounds B_O .. B_dv (without R), B_G."""
    B, N, H, scale = c["B"], c["N"], c["H"], t["scale"]
    cc = 1.0 / (1.0 - p_drop)
    ql, kl = _live(c, geo)
    S = torch.where(ql & kl, S_st, torch.full_like(S_st, float("-inf")))
    S = torch.where(ql, S, torch.zeros_like(S))                                # (rows that do not exist: anything finite, weighted 0 below)
    qw = ql.to(F64)
    rb = (lambda x: x.to(BF16)) if c["f16"] else (lambda x: x)               # the backward's operands with fp16 q | k | v
    V, DO = _bh(t["v"]), _bh(t["do"])
    Qb, Kb, Vb = _bh(rb(t["q"])), _bh(rb(t["k"])), _bh(rb(t["v"]))
    m = S.max(-1, keepdim=True).values
    e = torch.exp(S - m)
    p = e / e.sum(-1, keepdim=True)
    kp = torch.ones_like(p) if keep is None else keep.to(F64)
    Pp = cc * kp * p * qw
    dPraw = DO @ Vb.transpose(2, 3)
    dP = cc * kp * dPraw
    dl = (dP * p).sum(-1, keepdim=True)
    Gin = torch.zeros_like(p) if gz else t["gin"].to(F64)
    G = (p * (dP - dl) + Gin) * qw * kl.to(F64)
    back = lambda x: x.permute(0, 2, 1, 3)
    out = dict(O=back(Pp @ V), dq=back(scale * (G @ Kb)), dk=back(scale * (G.transpose(2, 3) @ Qb)), dv=back(Pp.transpose(2, 3) @ DO), G=G, p=p)
    if not bounds:
        return out
    if not mfma(c):
        u, uabs = 0.0, 0.0
    elif c["f16"]:
        u, uabs = 2.0 ** -22, 2.0 ** -24
    else:
        u, uabs = 2.0 ** -16, 0.0
    a = torch.where(p > 0, (S - m).abs(), torch.zeros_like(S))
    ee = EPS * (m.abs() + 2 * a + 2.0)
    rho = ee + (p * ee).sum(-1, keepdim=True) + (N + 4) * EPS
    Va, DOa, Ka, Qa = V.abs(), DO.abs(), Kb.abs(), Qb.abs()
    T = Pp @ Va
    out["B_O"] = back(u * T + (rho * Pp) @ Va + (N + 24) * EPS * T + uabs * (Pp > 0).to(F64) @ Va + ETA * cc * Va.sum(2, keepdim=True)) + ETA
    ub = 0.0 if not mfma(c) else 2.0 ** -16
    T = Pp.transpose(2, 3) @ DOa
    out["B_dv"] = back(ub * T + (rho * Pp).transpose(2, 3) @ DOa + (N + 24) * EPS * T + ETA * cc * (DOa * qw).sum(2, keepdim=True)) + ETA
    E_dP = cc * kp * 8 * EPS * (DOa @ Vb.abs().transpose(2, 3)) + EPS * dP.abs()
    E_d = (p * (E_dP + dP.abs() * (rho + EPS))).sum(-1, keepdim=True) + (N + 8) * EPS * (dP.abs() * p).sum(-1, keepdim=True)
    E_G = (p * (E_dP + E_d + 2 * EPS * (dP.abs() + dl.abs())) + rho * p * (dP - dl).abs() + 2 * EPS * (p * (dP - dl).abs() + Gin.abs())
           + ETA * (dP.abs() + dl.abs() + 1.0)) * qw * kl.to(F64)
    out["B_G"] = E_G + ETA
    T = G.abs() @ Ka
    out["B_dq"] = back(abs(scale) * (ub * T + E_G @ Ka + (N + 24) * EPS * T)) + ETA
    T = G.abs().transpose(2, 3) @ Qa
    out["B_dk"] = back(abs(scale) * (ub * T + E_G.transpose(2, 3) @ Qa + (N + 24) * EPS * T)) + ETA
    return out


def o_dtype(c):
    return F16 if c["f16"] else BF16


def out_bound(c, ref, k):
    return ref["B_" + k] + rounding_term(ref[k], o_dtype(c) if k == "O" else BF16)


def g_bound(c, ref):
    return ref["B_G"] + (rounding_term(ref["G"], BF16) if c["layout"] & 4 else 0.0)


def token_rows(c, geo, x):
    """[B, N, H, 8] -> [rows, H * 8]: the token rows that exist, in the order the device holds them"""
    return x.reshape(c["B"] * c["N"], c["H"] * HD)[geo["gather"]]


def evaluate(c, geo, ref, got, S_ref=None, E_S=None, only=None):
    """got: O, dq, dk, dv [rows, D], G, S [B, H, N, N] (positional, fp32 / float64) -> {name: (worst ratio, z)} over what is defined"""
    res = {}
    ql, kl = _live(c, geo)
    live = (ql & kl).expand(c["B"], c["H"], c["N"], c["N"])
    for k in ("O", "dq", "dk", "dv"):
        if k in got and (only is None or k in only):
            r, b = token_rows(c, geo, ref[k]), token_rows(c, geo, out_bound(c, ref, k))
            if k == "O":     # (a query with ONE real key copies c v of that key: the same rounding error in every such row -- not the independent errors the gain is about)
                w = token_rows(c, geo, (ref["p"].max(-1).values < 1.0).permute(0, 2, 1).unsqueeze(-1).expand(-1, -1, -1, HD))
                res[k] = (worst_ratio(got[k], r, b), gain(got[k][w], r[w], b[w]))
                continue
            res[k] = (worst_ratio(got[k], r, b), gain(got[k], r, b))
    if "G" in got:
        res["G"] = (worst_ratio(got["G"][live], ref["G"][live], g_bound(c, ref)[live]), 0.0)
    if "S" in got:
        fin = torch.isfinite(S_ref) & live
        assert torch.equal(torch.isneginf(got["S"].to(F64)) & live, torch.isneginf(S_ref) & live), "padded keys are exactly -inf, nothing else is"
        res["S"] = (worst_ratio(got["S"][fin], S_ref[fin], E_S[fin]), 0.0)
    return res


# ------------------------------------------------------------------------------------------------ the exact modes
def selector_expectation(c, t, geo, gz=False):
    """what the selector mode requires, stated without the reference: S, O, dv, G_out, dq, dk (float64, positional)"""
    B, N, H = c["B"], c["N"], c["H"]
    Q, K, V, DO = _bh(t["q"]), _bh(t["k"]), _bh(t["v"]), _bh(t["do"])
    ql, kl = _live(c, geo)
    S = t["bias"].to(F64) + 0.25 * (Q @ K.transpose(2, 3))
    if t["pad"] is not None:
        S = S.masked_fill(t["pad"].view(B, 1, 1, N), float("-inf"))
    sel = t["sel"]
    O = torch.gather(V, 2, sel.unsqueeze(-1).expand(B, H, N, HD))
    dv = torch.zeros(B, H, N, HD, dtype=F64)
    dv.scatter_add_(2, sel.unsqueeze(-1).expand(B, H, N, HD), DO * ql.to(F64))
    G = (torch.zeros_like(S) if gz else t["gin"].to(F64)) * ql.to(F64) * kl.to(F64)
    back = lambda x: x.permute(0, 2, 1, 3)
    r16 = lambda x: x.to(BF16).to(F64)
    return dict(S=S, O=back(O), dv=back(r16(dv)), G=G, dq=back(r16(0.25 * (G @ K))), dk=back(r16(0.25 * (G.transpose(2, 3) @ Q))))


def selector_is_one_hot(c, t):
    """the conditions of the selector mode: the winner's logit in {0, +-1, 2} (m log2e exact in fp32), every loser >= 183 below, every
    value an integer (S a multiple of 1/4) exactly representable in its storage type"""
    B, N = c["B"], c["N"]
    S = t["bias"].to(F64) + 0.25 * (_bh(t["q"]) @ _bh(t["k"]).transpose(2, 3))
    if t["pad"] is not None:
        S = S.masked_fill(t["pad"].view(B, 1, 1, N), float("-inf"))
    win = torch.gather(S, 3, t["sel"].unsqueeze(-1))
    assert bool(torch.isin(win, torch.tensor([0.0, 1.0, -1.0, 2.0], dtype=F64)).all())
    rest = S.scatter(3, t["sel"].unsqueeze(-1), float("-inf"))
    assert float((rest - win).max()) <= -183.0
    fin = torch.isfinite(S)
    assert bool((S[fin] == S[fin].to(s_dtype(c)).to(F64)).all()) and bool(((4 * S[fin]) == (4 * S[fin]).round()).all())
    for n in ("q", "k", "v", "do", "gin"):
        assert bool((t[n] == t[n].round()).all()) and float(t[n].abs().max()) <= 64
    mL = (win.to(F32) * LOG2E32).to(F64)
    assert bool((mL == win * LOG2E32.to(F64)).all())                      # fl(m log2e) = m log2e: the fma against it gives 0, exp2(0) = 1
    return True


def exactness(c, t, geo, ref):
    """the uniform modes: n real keys, n a power of two <= 16, integer operands, one of q, k zero, scale 2^-2.  p = 1 / n;
      row sum   terms 1            quantum 1            O, dv    terms v / n, dO / n                quantum 1 / 16
      dP        terms dO v         quantum 1            delta    terms dP / n                       quantum 1 / 16
      G         (dP - delta) / n + G_in                 quantum 2^-8, |G| < 2^3: 11 bits, inside the 16 the hi + lo split carries
      dq, dk    terms scale G k, scale G q              quantum 2^-10
    -> the largest sum |term| / quantum over the final sums (must stay below 2^24), asserting the quanta and the split on the way"""
    assert t["scale"] == 0.25 and (float(t["q"].abs().max()) == 0.0 or float(t["k"].abs().max()) == 0.0)
    assert all(n & (n - 1) == 0 and 1 <= n <= 16 for n in t["n_real"])
    for b, n in enumerate(t["n_real"]):
        assert int((~t["pad"][b]).sum()) == n
    for x in ("q", "k", "v", "do", "gin"):
        assert bool((t[x] == t[x].round()).all())
    G = ref["G"]
    hi = G.to(BF16).to(F64)
    lo = (G - hi).to(BF16).to(F64)
    assert bool((hi + lo == G).all()) and bool(((G * 256) == (G * 256).round()).all())
    Ga = G.abs()
    sums = (ref["p"] > 0).sum(-1).max(), (_bh(t["v"]).abs().sum(2) * 16).max(), (_bh(t["do"]).abs().sum(2) * 16).max(), \
        ((Ga @ _bh(t["k"]).abs()) * 1024).max(), ((Ga.transpose(2, 3) @ _bh(t["q"]).abs()) * 1024).max()
    for k in ("O", "dv"):
        assert bool(((ref[k] * 16) == (ref[k] * 16).round()).all())
    for k in ("dq", "dk"):
        assert bool(((ref[k] * 1024) == (ref[k] * 1024).round()).all())
    return max(float(s) for s in sums)


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _split(x, dtype, drop_lo):
    hi = x.to(dtype).to(F32)
    return hi if drop_lo else hi + (x - hi).to(dtype).to(F32)


def emulate(c, t, geo, p_drop=0.0, keep=None, gz=False, drop_lo=False, denom=1.0):
    """The kernels' arithmetic in fp32 torch with their rounding points: the fp16 rounding of S (compact), the hi + lo split of P, Pd and G
    in the MFMA kernels, 16-bit outputs.  drop_lo / denom: the two wrong builds the bounds must see (the low part of every split
    dropped; every softmax denominator too large by the factor)."""
    B, N, scale = c["B"], c["N"], torch.tensor(t["scale"], dtype=F32)
    dsc = torch.tensor(1.0 / (1.0 - p_drop), dtype=F32) if p_drop else torch.tensor(1.0)
    ql, kl = _live(c, geo)
    Q, K, V, DO = (_bh(t[n], F32) for n in ("q", "k", "v", "do"))
    S = t["bias"] + scale * (Q @ K.transpose(2, 3))
    if t["pad"] is not None:
        S = S.masked_fill(t["pad"].view(B, 1, 1, N), float("-inf"))
    if c["layout"] & 2:
        S = S.clamp(max=65504.0).to(F16).to(F32)
    Sm = torch.where(kl, S, torch.full_like(S, float("-inf")))
    m = Sm.max(-1, keepdim=True).values
    e = torch.exp2(Sm * LOG2E32 - m * LOG2E32)
    lsum = e.sum(-1, keepdim=True) * torch.tensor(denom, dtype=F32)
    kp = torch.ones_like(e) if keep is None else keep.to(F32)
    qw = ql.to(F32)
    use_split = mfma(c)
    sp = (lambda x, d=BF16: _split(x, d, drop_lo)) if use_split else (lambda x, d=None: x)
    P1 = sp(e * (dsc / lsum) * kp, op_dtype(c))
    back = lambda x: x.permute(0, 2, 1, 3)
    got = dict(S=S, O=token_rows(c, geo, back(round16((P1 @ V).to(F64), o_dtype(c)).to(F32))).to(o_dtype(c)))
    if c["f16"]:
        Q, K, V = (x.to(BF16).to(F32) for x in (Q, K, V))
    p = e * (1.0 / lsum)
    dP = (DO @ V.transpose(2, 3)) * dsc * kp
    dl = (dP * p).sum(-1, keepdim=True)
    G = (p * (dP - dl) + (torch.zeros_like(p) if gz else t["gin"])) * qw * kl.to(F32)
    Gs, Pd = sp(G), sp(p * kp * dsc * qw)
    got["G"] = G.to(g_dtype(c)).to(F32)
    for k, x in (("dq", (Gs @ K) * scale), ("dk", (Gs.transpose(2, 3) @ Q) * scale), ("dv", Pd.transpose(2, 3) @ DO)):
        got[k] = token_rows(c, geo, back(x)).to(BF16)
    return got


def random_keep(c, p, seed=5):
    g = torch.Generator().manual_seed(seed + c["N"])
    return torch.rand(c["B"], c["H"], c["N"], c["N"], generator=g) >= p


# ------------------------------------------------------------------------------------------------ placement on the device
def flat_arena(n, dtype, device, out, shift=0):
    """a flat buffer of n elements inside a NaN-filled (operand) or sentinel-filled (output) arena; shift: elements in front of it that
    move its pointer off the 16-byte boundary -> (arena, the n elements, pointer)"""
    a = Arena((1, n + shift, n + shift, 0, 0, n + shift), (1, 1), dtype, device, out=out)
    assert a.ptr() % 16 == 0
    return a, a.view[0, 0, 0][shift:], a.ptr() + shift * a.buf.element_size()


def row_arena(rows, cols, dtype, device, out):
    a = Arena((rows, cols, cols, 0, 0, rows * cols), (1, 1), dtype, device, out=out)
    assert a.ptr() % 16 == 0
    return a, a.view[0, 0]


def scatter_plane(c, geo, flat, values, where):
    """write values [B, H, N, cols] into the planes of `flat` at the slots where [B, N, cols] is set"""
    B, H = c["B"], c["H"]
    planes = flat.view(B, H, geo["plane"])
    for b in range(B):
        sel = where[b]
        planes[b][:, geo["idx"][sel].to(flat.device)] = values[b][:, sel].to(flat.device).to(flat.dtype)


def gather_plane(c, geo, flat):
    """the planes of `flat` by position -> [B, H, N, cols] on the CPU"""
    return flat.view(c["B"], c["H"], geo["plane"])[:, :, geo["idx"].reshape(-1).to(flat.device)].view(c["B"], c["H"], c["N"], geo["cols"]).cpu()


def unwritten_mask(c, geo, where):
    """[B, plane] bool: the slots of a plane outside `where` (the alignment tail, row padding, rows and tiles no kernel stores)"""
    m = torch.ones(c["B"], geo["plane"], dtype=torch.bool)
    for b in range(c["B"]):
        m[b, geo["idx"][where[b]]] = False
    return m


def sentinel_of(dtype):
    return SENT32 if dtype == F32 else SENT16


def bits(x):
    return x.view(torch.int32 if x.dtype == F32 else torch.int16)
