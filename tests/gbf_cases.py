"""The case table of the pair-bias (GBF) instance tests, their input builders, float64 reference, bounds and fp32 emulation, shared by
test_gbf_cases_cpu.py (which proves that the table reaches every kernel instance of csrc/gbf.hip and every runtime branch, that the
exact mode is exact, that an fp32 emulation of the kernels' rounding points stays inside the bounds and that six wrong emulations do
not) and test_gbf_instances_gpu.py (which holds the kernels to the reference on the device).

INSTANCES (instance() and launch(), the independent statement of what each case is declared to run; test_gbf_cases_cpu.py holds the
library's own answer, mmdti_gbf_plan, to it for every case and for a sweep of shapes; SOURCE_LINES keeps the rounding points and
device-side rules the reference depends on verbatim): 9 gbf_bias_fwd_kernel<SAVE, TILED, OT, COORDS>, 3 gbf_bias_bwd_kernel<TILED, GT>,
12 gbf_bias_bwd_full_kernel<TILED, GT, DET, COORDS>, gbf_fwd_kernel, gbf_bwd_kernel, gbf_bwd_det_kernel: 27.  gbf_slab_reduce_kernel
runs behind every complete backward that is handed a workspace and is held through its outputs.

TABLE.  Every instance at N = 1, 5, 17, 37, 130 (a single pair; less than one 16-pair tile; N % 4 = N % 16 = 1; two ragged row blocks;
past 128), B = 3 (N ld % 16 != 0: molecule boundaries fall inside a row-major tile) -- N = 130 with the batch that makes the persistent
grid go round more than once with a ragged last round (forward, per-pair backward: B = 4, > 8 x 512 and > 4 x 1024 tiles; complete
backward: B = 2, > 8 x 256).  All modes at one of N = 5, 17, 37 (rotating), `random` at the others, `onehot` at N = 1 too.  On top:
ugrad on the saving forwards and the per-pair backward; E = 1, 1536 (coords: V = 39, E = 1521) and -- where the entry point takes it --
5000 / 5041 (no LDS tables in the forward, global atomics in gbf_bwd_kernel); tile_prefix alone and with row_blocks (lengths of
pair_cases.ragged_lens) on the tiled and compact forwards and complete backwards; the complete backward without a workspace (fp32
atomics); edge types of 4 and 2 bytes on every planes instance (edge_runs()).  In a dense case molecule 0 is N // 3 atoms short.

PAIRS.  A pad atom carries NaN coordinates and the pad token 0; the host pair rule (gbf.hip gbf_pair_rule) gives (e, d) = (pad, 0) when
either atom is pad, else (tok_i V + tok_j, |c_i - c_j|) -- computed in float64 from the fp32 coordinates and rounded to fp32 (within
an ulp of the device's value: coords cases carry 4 more ulp of d in the bound of y); planes cases receive these planes.

MODES
  onehot  mul = 0, bias[e] = means[k(e)] bit for bit, means 64 apart (>= 42 sigma): y - mu is exactly 0 for one kernel, the exp2 argument
          of every other one below -1000 (v_exp_f32 gives 0).  stds mix signs, at least two are 0 (sigma = 1e-5, cf = 4e4), and two sit where
          bf16(cf) differs between a = sqrt(2 x 3.14159) and sqrt(2 pi) (boundary_std()) -- these four on the kernels the batch uses most.  feat is bf16(cf_k) at one position, u[f] one
          exact bf16 x bf16 product plus b1[f]: one fp32 rounding.  The saved feat and u EQUAL onehot_expectation() (fp32 on the CPU:
          1.0f / x there and on the device is the correctly rounded division -- csrc/Makefile passes neither -ffast-math nor
          -fno-hip-fp32-correctly-rounded-divide-sqrt, and hipcc's default is the correctly rounded one).  k(e) = (37 e + 11) % 128 and
          random weights: pairs of different kernels have different output rows (128 kernels cannot tell 961 edge types apart further).
  random  parameters as _gbf_params of test_pair_inputs_gpu.py draws them, |std| >= 0.05; G ~ N(0, 1) (bf16 values for the compact kernels).
  clamp   random with about 1 % of the edge types (at least one each) out of range (-3, E + 5) on planes cases, four b1 entries at +-10 (GELU tails) and, on
          compact forwards, four b2 entries at 70000: those outputs are exactly 65504.

REFERENCE (chain(), float64; emulate() is the same function in fp32 -- one statement of the arithmetic, two precisions; without its
rounding points it agrees with float64 autograd of sum(out G) to 1e-11, test_gbf_cases_cpu.py):
    y = mul[e] d + bias[e]    val = exp(-z^2 / 2) / (a sigma), z = (y - mu) / sigma, sigma = |std| + 1e-5    basis = bf16(val)   [gbf.hip:379, 67]
    u = W1 basis + b1         h = bf16(gelu(u)) [:615, :611]          out = W2 h + b2  (compact: min(., 65504) as fp16 [:388])
    saved: feat = basis, u = bf16(u) or bf16(gelu'(u)) [:607, :605], h
    dO = bf16(G) in the per-pair kernel [:749]; the complete kernel carries fp32 G as a bf16 hi + lo pair [:1019-1026] (bf16 G: exact)
    du = bf16((dO W2) gp) [:775, :1064], gp = u_in | gelu'(u_in) (per-pair) or bf16(gelu'(u)) of the recomputed fp32 u (complete [:1062])
    dW1 = du^T basis, db1 = sum du, dW2 = dO^T h, db2 = sum dO           dbasis = du W1 -- bf16 in the per-pair kernel only [:796; :1112 stays fp32]
    t = dbasis val (val unrounded), zs = z / sigma: dy = -sum_k t zs, dmeans = sum_p t zs, dstds = sign(std) sum_p t (z zs - 1 / sigma),
    dmul[e] = sum dy d, dbias[e] = sum dy.        The gradient buffers start at FILL and are accumulated into.

BOUNDS, from the reference alone.  Every tensor carries L (worst case, first order: fp32 roundings) and Q (a variance: bf16 rounding
points).  U = 2^-24.
  y       4 U (|mul d| + |bias|): the product and the sum, fused or not (this file is built with opportunistic contraction)
  val     relative |z| dz + 2 U z^2 + 8 U: dz the error of z (y, the subtraction, 4 roundings in 1 / sigma or GBF_SQ / sigma), the square and its
          scaling by log2(e) / 2, v_exp_f32 / __expf (1 ulp = 2 U) and the four roundings of cf; + 2^-126 cf (a flushed denormal)
  bf16    a rounding point the reference rounds too differs from the device's by 0 or ONE bf16 ulp of the rounded value: Q += ulp^2,
          carried to what it is multiplied by (W^2 in a product, gelu'^2 through the activation) and summed over the contraction
  sums    (n + 8) U sum |terms|: n = 128 (64) for the MFMA chains of a pair; for the sums over pairs n = the pairs a workgroup
          adds up in any order + the partial sums that then meet (slabs, atomics): acc_count()
  GELU    4 GELU_G_MEASURED (gemm_cases: the same gelu_erf2 / gelu_erf_both2 / gelu_erf_grad), scaled by |u| / 8 beyond |u| = 8
  bound = L + KAPPA sqrt(Q) (+ one ulp of a 16-bit output that is itself such a rounding point); onehot: L = Q = 0 at the basis, by
  construction, and the saved feat and u admit only the expectation.  KAPPA = 4: the error of the rounding points is a sum of independent
  terms, each 0 or +-a_i with sum a_i^2 = Q; whatever the probability of a flip, Hoeffding gives P(|sum| > 4 sqrt(Q)) <= 2 exp(-8), and
  a site flips only when the fp32 error before it (some 2^-17 of the value) crosses a rounding boundary (2^-8 apart): a few per cent of the
  sites, which makes 4 sqrt(Q) some twenty standard deviations -- sqrt(Q) alone is crossed by the EMULATION in a few of 10^6 elements.
  What the factor costs is measured by the six wrong emulations of test_gbf_cases_cpu.py, which all leave the bounds.
Two checks per output: the worst |got - ref| / bound <= 1 and |gain| <= Z_MAX = 6 (attn_cases.gain)."""
import functools
import math

import torch

import pair_cases as PC
from attn_cases import Z_MAX, gain  # noqa: F401
from gemm_cases import F64, GELU_G_CAP, GELU_G_MEASURED, SENT16, SENT32, Arena, gelu64, gelu_grad64, rounding_term, worst_ratio  # noqa: F401
from pair_cases import flat_arena, gather_plane, geometry, pair_ld, pair_plane, ragged_lens, row_arena, scatter_plane  # noqa: F401

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
K, F, H = 128, 128, 64
GBF_MAXE, GBF_FWD_MAXE, GBF_FULL_MAXE = 4096, 4096, 1536
GBF_SLAB = F * K + H * F + F + H + 2 * K
GBF_A = 2.5066272160
U = 2.0 ** -24
ETA = 2.0 ** -126
FILL = 0.75
KAPPA = 4.0
PAD = 0
NS = (1, 5, 17, 37, 130)
MODES = ("onehot", "random", "clamp")

SOURCE_LINES = (
    "constexpr float GBF_A = 2.5066272160f;  // sqrt(2*3.14159) -- truncated pi exactly as mm_model.py:222-223",
    "__device__ __forceinline__ float gbf_sigma(float sd) { return fabsf(sd) + 1e-5f; }",          # the one definition of sigma ...
    "__device__ __forceinline__ float gbf_coef(float sg) { return 1.0f / (GBF_A * sg); }",         # ... of 1 / (a sigma) ...
    "#define GBF_CLAMP_EDGE(X, E) ((X) < 0 ? 0 : ((X) >= (E) ? (E) - 1 : (X)))",                    # ... and of the edge clamp
    "return gbf_pack8(v);",                                                           # the basis leaves gbf_basis8 as bf16
    "hB[u] = gbf_pack8(hv[0], hv[1]);",                                               # h before the second product
    "if (SAVE && valid) *reinterpret_cast<uint2*>(u_out + p * GBF_F + 16 * ft + 4 * g) = gbf_pack4(acc);",
    "oB[c] = gbf_pack8(gv + 8 * c);",                                                 # per-pair: dO = bf16(G)
    "for (int j = 0; j < 16; ++j) lo[j] = gv[j] - (float)oB[j >> 3][j & 7];",           # complete: hi + lo
    "if (valid) *reinterpret_cast<uint2*>(du_out + p * GBF_F + 16 * ft + 4 * g) = gbf_pack4(acc);",
    "*reinterpret_cast<uint2*>(GBF_SWZ(r1lo, r1hi, 16 * ft) + 4 * g) = gbf_pack4(acc);",
    "const uint2 gb = gbf_pack4(gf32x4{g0[0], g0[1], g1[0], g1[1]});",                 # complete: gelu' through bf16
    "const float dvr = __uint_as_float(((uint32_t)f2bf(acc[r])) << 16);   // dbasis passes through bf16 like the unfused chain",
    "gf32x2 dy2 = {0.f, 0.f};                          // (dbasis stays fp32 on its way into the Gaussian backward)",
    "atomicAdd(dstds + k, stds[k] < 0.f ? -sgv : sgv);   // d|std|/dstd",
    "const float ds = stds[k] < 0.f ? -sgv : sgv;        // d|std|/dstd",
    "for (int j = 0; j < 8; ++j) gv[c * 8 + j] = valid ? gbf_get(gp + (long long)(32 * c + 8 * g + j) * plane) : 0.f;",   # an invalid lane loads nothing
    "const unsigned voff = (unsigned)(8 * g) * (unsigned)plane + (unsigned)(valid ? q : 0);",                               # ... or slot 0: pair (0, 0)
)


# ------------------------------------------------------------------------------------------------ the table
CASES = []
V_OF = {961: 31, 1: 31, 1536: 39, 1521: 39, 5000: 70, 5041: 71}


def add(kind, N, layout="row", B=3, E=961, coords=False, save=False, ugrad=False, det=False, ws=True, lens=None, packed=False, modes=("random",)):
    c = dict(kind=kind, N=N, layout=layout, B=B if lens is None else len(lens), E=E, V=V_OF[E], coords=coords, save=save, ugrad=ugrad, det=det, ws=ws,
             lens=lens, packed=packed, modes=tuple(modes), ld=pair_ld(N))
    assert not coords or E == c["V"] ** 2
    assert lens is None or layout != "row"
    c["i"] = len(CASES)
    CASES.append(c)
    return c


FWD = [(s, lay, False) for s in (True, False) for lay in ("tiled", "row", "compact")] + [(False, lay, True) for lay in ("tiled", "row", "compact")]
BWD = ("tiled", "row", "compact")
FULL = [(lay, det, co) for lay in ("tiled", "row", "compact") for det in (False, True) for co in (False, True)]


def _modes(N, i):
    if N == (5, 17, 37)[i % 3]:
        return MODES
    return ("onehot", "random") if N == 1 else ("random",)


def _build():
    i = 0
    for save, lay, co in FWD:
        for N in NS:
            add("fwd", N, lay, B=4 if N == 130 else 3, coords=co, save=save, modes=_modes(N, i))
        if save:
            for N in (5, 37):
                add("fwd", N, lay, save=True, ugrad=True, modes=("onehot", "random"))
        add("fwd", 17, lay, E=5041 if co else 5000, coords=co, save=save)                      # no LDS tables
        add("fwd", 17, lay, E=1521 if co else 1536, coords=co, save=save)
        if not co:
            add("fwd", 17, lay, E=1, save=save)
        if lay != "row":
            add("fwd", 17, lay, coords=co, save=save, lens=ragged_lens(17))
            add("fwd", 37, lay, coords=co, save=save, lens=ragged_lens(37), modes=("random", "clamp"))
            add("fwd", 37, lay, coords=co, save=save, lens=ragged_lens(37), packed=True)
        i += 1
    for lay in BWD:
        for N in NS:
            add("bwd", N, lay, B=4 if N == 130 else 3, modes=_modes(N, i))
        for N in (5, 37):
            add("bwd", N, lay, ugrad=True, modes=("onehot", "random"))
        for E in (1, 1536):
            add("bwd", 17, lay, E=E)
        i += 1
    for lay, det, co in FULL:
        for N in NS:
            add("full", N, lay, B=2 if N == 130 else 3, coords=co, det=det, modes=_modes(N, i))
        if not det:
            for N in (5, 37):
                add("full", N, lay, coords=co, ws=False, modes=("onehot", "random"))         # fp32 atomics
        add("full", 17, lay, E=1521 if co else 1536, coords=co, det=det)
        if not co:
            add("full", 17, lay, E=1, det=det)
        if lay != "row":
            add("full", 17, lay, coords=co, det=det, lens=ragged_lens(17))
            add("full", 37, lay, coords=co, det=det, lens=ragged_lens(37), modes=("random", "clamp"))
            add("full", 37, lay, coords=co, det=det, lens=ragged_lens(37), packed=True)
        i += 1
    for N in NS:
        add("ffwd", N, modes=_modes(N, 1))
    add("ffwd", 130, B=8)                                            # 135 200 pairs: past the 256 x 32 workgroups of 16
    add("ffwd", 17, E=5000)
    add("ffwd", 17, E=1)
    for det in (False, True):
        for N in NS:
            add("fbwd", N, det=det, modes=_modes(N, 1))
        add("fbwd", 17, E=1, det=det)
    add("fbwd", 17, E=5000)                                          # global atomics


_build()


def tf(x):
    return "true" if x else "false"


def instance(c):
    """the kernel the entry point launches for the case"""
    k, tiled, compact = c["kind"], c["layout"] != "row", c["layout"] == "compact"
    if k == "fwd":
        assert not (c["coords"] and c["save"])
        return f"gbf_bias_fwd_kernel<{tf(c['save'])}, {tf(tiled)}, {'_Float16' if compact else 'float'}, {tf(c['coords'])}>"
    if k == "bwd":
        assert c["E"] <= GBF_MAXE and not c["det"]
        return f"gbf_bias_bwd_kernel<{tf(tiled)}, {'__bf16' if compact else 'float'}>"
    if k == "full":
        assert c["E"] <= GBF_FULL_MAXE and (c["ws"] or not c["det"])
        return f"gbf_bias_bwd_full_kernel<{tf(tiled)}, {'__bf16' if compact else 'float'}, {tf(c['det'])}, {tf(c['coords'])}>"
    if k == "ffwd":
        return "gbf_fwd_kernel"
    assert not c["det"] or c["E"] <= GBF_MAXE
    return "gbf_bwd_det_kernel" if c["det"] else "gbf_bwd_kernel"


def flags(c):
    """the flag word of the fused entry points: bit 0 tiled, bit 1 ugrad, bit 2 compact"""
    return int(c["layout"] != "row") | (2 if c["ugrad"] else 0) | (4 if c["layout"] == "compact" else 0)


def pc_of(c):
    """the case as pair_cases sees it (geometry, scatter_plane, gather_plane)"""
    lay = {"row": 0, "tiled": 1, "compact": 3 if c["kind"] == "fwd" else 7}[c["layout"]]
    return dict(N=c["N"], B=c["B"], H=H, layout=lay, ld=c["ld"], lens=c["lens"], packed=c["packed"], f16=False, det=False, shift=False)


def row_blocks(c, geo):
    nb = (c["N"] + 3) // 4
    return [min((geo["qlive"][b] + 3) // 4, nb) if c["packed"] else nb for b in range(c["B"])]


def prefix(c, geo):
    """tile_prefix [B + 1] of a ragged case: the 4x4 blocks of each molecule's covered key tiles (and packed rows)"""
    nb = (c["N"] + 3) // 4
    pre = [0]
    for b, r in enumerate(row_blocks(c, geo)):
        pre.append(pre[-1] + r * min(4 * geo["ke"][b], nb))
    return pre


def launch(c, geo=None):
    """tpm, ntiles (what the kernel enumerates), grid, pairs per workgroup and round, rounds"""
    N, B, k = c["N"], c["B"], c["kind"]
    if k in ("ffwd", "fbwd"):
        P = B * N * N
        blocks = (P + 15) // 16
        grid = min(blocks, 256 * 32) if k == "ffwd" else (max(1, min(blocks, 256)) if c["det"] else min(blocks, 256 * 8))
        return dict(tpm=0, ntiles=blocks, grid=grid, rounds=-(-blocks // grid))
    nb = (N + 3) // 4
    tpm = nb * nb if c["layout"] != "row" else -(-N * c["ld"] // 16)
    host = B * tpm
    ntiles = host if c["lens"] is None else prefix(c, geo or geometry(pc_of(c)))[-1]
    per, cap = {"fwd": (8, 512), "full": (8, 256), "bwd": (4, 1024)}[k]
    grid = min(host // 4 + 1, cap) if k == "bwd" else min((host + 7) // 8, cap)
    return dict(tpm=tpm, ntiles=ntiles, grid=grid, rounds=-(-ntiles // (per * grid)))


ENTRY = {"ffwd": 0, "fbwd": 1, "fwd": 2, "bwd": 3, "full": 4}
PTR = 0x10000          # a fake, 16-byte aligned device address: mmdti_gbf_plan never dereferences one
PLAN_FIELDS = ("name", "grid", "block", "lds", "lds_cap", "tpm", "ntiles", "ltab", "slab", "reduce_grid")


def workspace_bytes(E):
    """mmdti_gbf_bias_bwd_full_workspace: one slab per workgroup of the largest grid"""
    return 256 * (GBF_SLAB + 2 * E) * 4


def canonical(name):
    """a table name with its defaulted template arguments written out, as instance() spells it"""
    if "<" not in name:
        return name
    kern, args = name[:-1].split("<")
    args = args.split(", ")
    full = {"gbf_bias_fwd_kernel": 4, "gbf_bias_bwd_kernel": 2, "gbf_bias_bwd_full_kernel": 4}[kern]
    return f"{kern}<{', '.join(args + ['false'] * (full - len(args)))}>"


def library_plan(lib, c, esz=8, det=None, ws=None, operands=PTR, aligned=PTR):
    """mmdti_gbf_plan's answer for a case (any dict with the keys of add()) -> dict of PLAN_FIELDS.  ws: workspace bytes handed to the
    complete backward (default: what the case declares)."""
    import ctypes
    k, N = c["kind"], c["N"]
    ws = (workspace_bytes(c["E"]) if c["ws"] else 0) if ws is None else ws
    p = lambda on: PTR if on else 0
    out = (ctypes.c_longlong * 10)()
    lib.mmdti_gbf_plan(ENTRY[k], int(c["det"] if det is None else det), operands, aligned, p(c["save"]), p(c["coords"]), p(c["lens"] is not None), p(c["packed"]),
                       p(ws and k == "full"), ws, c["B"] * N * N, c["B"], N, c["ld"], K, F, H, c["E"], c["V"], PAD, esz, flags(c), out)
    v = list(out)
    return dict(zip(PLAN_FIELDS, [canonical(lib.mmdti_plan_kernel_name(1, v[0]).decode())] + v[1:]))


def declared_plan(c):
    """what the case is declared to launch, from instance() and launch(): every field of the library's plan but the LDS sizes"""
    k = c["kind"]
    L = launch(c)
    host = L["ntiles"] if c["lens"] is None else c["B"] * L["tpm"]       # (the host does not see a ragged batch's prefix)
    slab = int(c["det"]) if k == "fbwd" else int(bool(c["ws"])) if k == "full" else 0
    return dict(name=instance(c), grid=L["grid"], block={"fwd": 512, "full": 512}.get(k, 256), tpm=L["tpm"], ntiles=host,
                ltab=int(k == "fwd" and c["E"] <= GBF_FWD_MAXE), slab=slab, reduce_grid=-(-(GBF_SLAB + 2 * c["E"]) // 64) if slab and k == "full" else 0)


def assert_declared_plan(lib, c, esz=8):
    got, want = library_plan(lib, c, esz), declared_plan(c)
    assert {f: got[f] for f in want} == want, (case_id(c), got, want)
    return got


def acc_count(c, t=None):
    """n of the sums over pairs: the pairs one workgroup adds up (in any order) + the partial sums that meet afterwards.  The grid is the
    library's (mmdti_gbf_plan); the rounds follow from it and the tiles the kernel enumerates."""
    from mmdti_hip import _abi
    grid = library_plan(_abi.lib(), c)["grid"]
    per = {"fwd": 8, "full": 8, "bwd": 4}.get(c["kind"], 1)
    L = dict(grid=grid, rounds=-(-launch(c)["ntiles"] // (per * grid)))
    if c["kind"] == "full":
        return 256 * L["rounds"] + L["grid"] + 8              # (128 pairs a round, twice the products with the hi + lo pair)
    if c["kind"] == "bwd":
        return 64 * L["rounds"] + 4 * L["grid"] + 8           # (one atomic per wave)
    n = 16 * L["rounds"] + 4 * L["grid"] + 8
    if c["E"] > GBF_MAXE and t is not None:                     # global atomics: a bin's pairs in any order
        n += int(torch.bincount(t["e"].flatten()).max())
    return n


def case_id(c):
    f = [c["kind"], c["layout"], f"N{c['N']}"]
    if c["B"] != 3 and c["lens"] is None:
        f.append(f"B{c['B']}")
    if c["E"] != 961:
        f.append(f"E{c['E']}")
    f += [k for k in ("coords", "save", "ugrad", "det", "packed") if c[k]]
    if not c["ws"]:
        f.append("atomics")
    if c["lens"] is not None and not c["packed"]:
        f.append("prefix")
    return "-".join(f)


def runs(modes=MODES):
    return [(c, m) for c in CASES for m in c["modes"] if m in modes]


def edge_runs():
    """every planes instance of the fused kernels with 4- and 2-byte edge types: `random` at N = 17, the clamp at N = 37 (ragged where the instance has it)"""
    out = []
    for c in CASES:
        if c["kind"] in ("ffwd", "fbwd") or c["coords"] or c["E"] != 961 or c["ugrad"] or not c["ws"] or c["packed"]:
            continue
        if (c["N"] == 17 and c["lens"] is None) or (c["N"] == 37 and c["lens"] is not None):
            m = "clamp" if "clamp" in c["modes"] else "random"
            out += [(c, m, 4), (c, m, 2)]
    return out


def run_id(r):
    return f"{case_id(r[0])}-{r[1]}" + (f"-e{r[2]}" if len(r) > 2 else "")


# ------------------------------------------------------------------------------------------------ which pairs and slots a launch touches
def written(c, geo):
    """[B, N, cols] bool: the slots of an output plane the forward stores (the blocks behind a ragged molecule's prefix keep what they held)"""
    N, B = c["N"], c["B"]
    w = torch.zeros(B, N, geo["cols"], dtype=torch.bool)
    for b, r in enumerate(row_blocks(c, geo)):
        if c["lens"] is None:
            w[b] = True
        else:
            w[b, :min(4 * r, N), :min(16 * geo["ke"][b], geo["cols"])] = True
    return w


def pairs(c, geo):
    """[B, N, N] bool: the pairs a launch computes"""
    return written(c, geo)[:, :, :c["N"]]


# ------------------------------------------------------------------------------------------------ inputs
SEEDS = {}            # (case id, mode) -> seed, where the default draw does not give the emulation |gain| < 3 (test_gbf_cases_cpu.py)


def _gen(c, mode, seed):
    return torch.Generator().manual_seed(1000003 * seed + 7919 * c["N"] + 131 * c["E"] + 17 * c["B"] + MODES.index(mode) * 977
                                         + {"fwd": 1, "bwd": 2, "full": 3, "ffwd": 4, "fbwd": 5}[c["kind"]] * 31 + (0 if c["lens"] is None else 7 + c["packed"]))


def _cf32(std, a):
    """fp32, as the kernels compute it: 1.0f / (a * (fabsf(std) + 1e-5f))"""
    return 1.0 / (torch.tensor(a, dtype=F32) * (std.abs() + torch.tensor(1e-5, dtype=F32)))


@functools.lru_cache(maxsize=None)
def boundary_std(target):
    """an fp32 std near `target` whose bf16(cf) is the same in fp32 and float64 with a = GBF_A, and another value with a = sqrt(2 pi)"""
    x = torch.tensor(target, dtype=F32)
    ulp = float(torch.nextafter(x, x * 2) - x)
    cand = (x.to(F64) + torch.arange(-200000, 200000, dtype=F64) * ulp).to(F32)
    want = _cf32(cand, GBF_A).to(BF16)
    c64 = lambda a: (1.0 / (a * (cand.to(F64).abs() + 1e-5))).to(BF16)
    ok = (want == c64(math.sqrt(2 * 3.14159))) & (want != c64(math.sqrt(2 * math.pi))) & (want == c64(GBF_A))
    # (and safely so: the neighbours agree, so that one ulp of the device's own cf does not decide)
    ok = ok & torch.roll(ok, 1) & torch.roll(ok, -1)
    i = ok.nonzero().flatten()
    assert i.numel() > 0
    return float(cand[i[i.numel() // 2]])


def kmap(E):
    return (37 * torch.arange(E) + 11) % K


def make_inputs(c, mode, seed=None):
    seed = SEEDS.get((case_id(c), mode), 0) if seed is None else seed
    g = _gen(c, mode, seed)
    B, N, E, V = c["B"], c["N"], c["E"], c["V"]
    rn = lambda *s: torch.randn(*s, generator=g)
    lens = list(c["lens"]) if c["lens"] is not None else [N - N // 3] + [N] * (B - 1)
    real = torch.arange(N).view(1, N) < torch.tensor(lens).view(B, 1)
    tok = torch.where(real, torch.randint(1, V, (B, N), generator=g), torch.tensor(PAD))
    coord = torch.where(real.unsqueeze(-1), 1.5 * rn(B, N, 3), torch.tensor(float("nan")))
    both = real.view(B, N, 1) & real.view(B, 1, N)
    cz = torch.nan_to_num(coord).to(F64)
    d = torch.where(both, (cz.view(B, N, 1, 3) - cz.view(B, 1, N, 3)).pow(2).sum(-1).sqrt(), torch.zeros(1, dtype=F64)).to(F32)
    et = torch.where(both, tok.view(B, N, 1) * V + tok.view(B, 1, N), torch.tensor(PAD))
    if mode == "clamp" and not c["coords"]:
        at = torch.randperm(B * N * N, generator=g)[:2 * max(1, B * N * N // 200)]          # about 1 %, at least one of each
        et = et.clone()
        et.view(-1)[at[0::2]] = -3
        et.view(-1)[at[1::2]] = E + 5
    t = dict(mode=mode, tok=tok, coord=coord, d=d, et=et, e=et.clamp(0, E - 1), lens=lens)
    if mode == "onehot":
        means = 64.0 * torch.arange(K, dtype=F32)
        stds = (0.3 + 1.2 * torch.rand(K, generator=g)) * torch.where(torch.arange(K) % 3 == 1, -1.0, 1.0)
        stds[5], stds[77] = 0.0, -0.0
        ks, cnt = torch.unique(kmap(E)[t["e"]], return_counts=True)                    # ... on the kernels the batch uses most
        ks = ks[torch.argsort(cnt, descending=True, stable=True)].tolist()
        for k, v in zip(ks, (boundary_std(0.7), -boundary_std(1.1), 0.0, -0.0)):
            stds[k] = v
        mul, bias = torch.zeros(E), means[kmap(E)].clone()
    else:
        mul, bias = 1 + 0.1 * rn(E), 0.1 * rn(E)
        means, stds = torch.rand(K, generator=g) * 3, torch.rand(K, generator=g) * 3 - 1.5
        stds = torch.where(stds.abs() < 0.05, torch.where(stds < 0, -0.05, 0.05), stds)
    w1, b1 = (rn(F, K) * 0.2).to(BF16), rn(F) * 0.1
    w2, b2 = (rn(H, F) * 0.2).to(BF16), rn(H) * 0.1
    if mode == "clamp":
        b1[torch.tensor([3, 40, 77, 126])] = torch.tensor([10.0, -10.0, 10.0, -10.0])
        if c["kind"] == "fwd" and c["layout"] == "compact":
            b2[torch.tensor([0, 21, 42, 63])] = 70000.0
    G = rn(B, N, N, H)
    if c["layout"] == "compact":
        G = G.to(BF16).to(F32)
    t.update(mul=mul, bias=bias, means=means, stds=stds, w1=w1, b1=b1, w2=w2, b2=b2, G=G)
    if c["kind"] == "fbwd":
        t["dfeat"] = rn(B * N * N, K).to(BF16)
    return t


def onehot_is_exact(c, t):
    """the conditions of the onehot mode"""
    assert float(t["mul"].abs().max()) == 0.0 and torch.equal(t["bias"], t["means"][kmap(c["E"])])
    sg = t["stds"].abs() + 1e-5
    gap = (t["means"].view(-1, 1) - t["means"].view(1, -1)).abs() + torch.eye(K) * 1e9
    assert float((gap / sg.view(1, -1)).min()) >= 40.0 and float(((gap / sg.view(1, -1)) ** 2).min()) * 0.72 > 150.0
    assert int((t["stds"] == 0).sum()) >= 2 and bool((t["stds"] < 0).any()) and bool((t["stds"] > 0).any())
    return True


def onehot_expectation(c, t):
    """feat, u [B, N, N, 128] as bf16, in fp32 on the CPU"""
    k = kmap(c["E"])[t["e"]]                                   # [B, N, N]
    cf = _cf32(t["stds"], GBF_A).to(BF16)                      # [K]
    feat = torch.zeros(*k.shape, K, dtype=BF16)
    feat.scatter_(-1, k.unsqueeze(-1), cf[k].unsqueeze(-1))
    u = t["w1"].to(F32).t()[k] * cf.to(F32)[k].unsqueeze(-1) + t["b1"]       # one exact product, one rounded sum
    return feat, u.to(BF16)


# ------------------------------------------------------------------------------------------------ the chain: reference (float64, bounds) and emulation (fp32)
def ulp16(x):
    """one bf16 ulp of a bf16 value"""
    a = x.abs().to(F64)
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp(min=2.0 ** -133))) - 7), torch.zeros_like(a))


def bm(a, b):
    """a product of the BOUNDS (non-negative terms, three digits wanted): in fp32, which is what makes the reference of a 130-atom batch
    take a second; 1 % on top covers the fp32 summation of up to 2^17 non-negative terms"""
    return (a.to(F32) @ b.to(F32)).to(F64) * 1.01


def _gelu_g2(u):
    return torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi) * (2.0 - u * u)


def _gscale(u):
    return torch.clamp(u.abs() / 8.0, min=1.0)


MUTATIONS = ("drop_tile", "swap_w1", "dstds_sign", "half_dmul", "pi", "no_eps")


PER_PAIR = ("out", "feat", "u", "h", "do", "du")
CHUNK = 8192          # pairs per pass of the chain: its [pairs, 128] float64 temporaries stay below the allocator's mmap threshold


def chain(c, t, geo, dt=F64, mut=None, u_in=None, bounds=True):
    """-> dict of the case's outputs over the pairs the launch computes (rows in (b, i, j) order), dtype dt, and for float64 their bounds
    B_<name> (bounds=False: the values alone).  dt = float32 is the emulation; mut one of MUTATIONS (a wrong build the bounds must see)."""
    kind, N, B = c["kind"], c["N"], c["B"]
    sel = pairs(c, geo).reshape(-1) if kind not in ("ffwd", "fbwd") else torch.ones(B * N * N, dtype=torch.bool)
    n = int(sel.sum())
    nacc = acc_count(c, t) if kind in ("bwd", "full", "fbwd") else 0
    parts = [_part(c, t, dt, mut, u_in, bounds, sel, lo, min(lo + CHUNK, n), n) for lo in range(0, n, CHUNK)]
    out = dict(sel=sel, n=n)
    for k, v in parts[0].items():
        if k == "_acc":
            continue
        out[k] = torch.cat([p[k] for p in parts]) if k.replace("B_", "") in PER_PAIR else sum((p[k] for p in parts[1:]), v)
    if mut == "half_dmul":
        out["dmul"] = out["dmul"].clone()
        out["dmul"][t["_worst_e"]] *= 0.5
    for k in parts[0].get("_acc", {}):
        T, L, Q = (sum((p["_acc"][k][i] for p in parts[1:]), parts[0]["_acc"][k][i]) for i in range(3))
        out["B_" + k] = nacc * U * (T + FILL) + L + KAPPA * torch.sqrt(Q)
    return out


def _part(c, t, dt, mut, u_in, bounds, sel, lo, hi, n):
    """the chain over the computed pairs [lo, hi): per-pair outputs, partial sums of the gradients, and the (sum |terms|, L, Q) of their bounds"""
    kind, E = c["kind"], c["E"]
    is64 = dt == F64
    ref = is64 and bounds
    f = lambda x: x.to(dt)
    rb = (lambda x: x) if t.get("_exact") else (lambda x: x.to(BF16).to(dt))       # (_exact: no rounding point -- the chain as calculus has it)
    e, d = t["e"].reshape(-1)[sel][lo:hi], f(t["d"].reshape(-1)[sel][lo:hi])
    drop = (torch.arange(lo, hi) >= n // 2) & (torch.arange(lo, hi) < n // 2 + 16)
    mul, bias, means, stds = f(t["mul"]), f(t["bias"]), f(t["means"]), f(t["stds"])
    W1, W2, b1, b2 = f(t["w1"]), f(t["w2"]), f(t["b1"]), f(t["b2"])
    if mut == "swap_w1":
        W1 = W1.clone()
        W1[:, [3, 4]] = W1[:, [4, 3]]
    a = (math.sqrt(2 * math.pi) if mut == "pi" else (math.sqrt(2 * 3.14159) if is64 else GBF_A))
    a = torch.tensor(a, dtype=dt)
    sg = stds.abs() + (0.0 if mut == "no_eps" else torch.tensor(1e-5, dtype=dt))
    onehot = t["mode"] == "onehot"
    md = mul[e] * d
    y = md + bias[e]
    z = (y.view(-1, 1) - means) / sg
    val = torch.exp(-0.5 * z * z) * (1.0 / (a * sg))
    basis = rb(val)
    out = {}
    if ref:
        E_y = 4 * U * (md.abs() + bias[e].abs()) + (8 * U * md.abs() if c["coords"] else 0.0)
        dz = (E_y.view(-1, 1) + U * (y.view(-1, 1) - means).abs()) / sg + 4 * U * z.abs()
        L_val = val * (z.abs() * dz + 2 * U * z * z + 8 * U) + ETA / (a * sg)
        L_b = torch.zeros_like(val) if onehot else L_val
        Q_b = torch.zeros_like(val) if onehot else ulp16(basis) ** 2
    if kind == "ffwd":
        out["feat"] = basis
        if ref:
            out["B_feat"] = L_b + (0.0 if onehot else ulp16(basis))          # (onehot: EQUAL)
        return out
    W1a, W2a = W1.abs(), W2.abs()
    if kind in ("fwd", "full"):
        u = basis @ W1.t() + b1
        if onehot and is64:
            u = u.to(F32).to(F64)                        # one exact product + b1[f]: THE fp32 rounding is part of the expectation
        g1 = gelu_grad64(u)
        h = rb(gelu64(u))
        if ref:
            L_u = (K + 8) * U * (bm(basis.abs(), W1a.t()) + b1.abs()) + bm(L_b, W1a.t())
            Q_u = bm(Q_b, (W1 * W1).t())
            L_h = 1.13 * L_u + 4 * GELU_G_MEASURED["gelu"] * _gscale(u)
            Q_h = g1 * g1 * Q_u + ulp16(h) ** 2
    if kind == "fwd":
        o = h @ W2.t() + b2
        if c["layout"] == "compact":
            o = o.clamp(max=65504.0)
            if not is64:
                o = o.to(F16).to(dt)
        if mut == "drop_tile":
            o = o.masked_fill(drop.view(-1, 1), 0.0)
        out["out"] = o
        if c["save"]:
            usv = rb(g1) if c["ugrad"] else rb(u)
            out.update(feat=basis, u=usv, h=h)
        if ref:
            out["B_out"] = (F + 8) * U * (bm(h.abs(), W2a.t()) + b2.abs()) + bm(L_h, W2a.t()) + KAPPA * torch.sqrt(bm(Q_h, (W2 * W2).t()))
            if c["layout"] == "compact":
                out["B_out"] = out["B_out"] + rounding_term(o, F16)
            if c["save"]:
                out["B_feat"] = L_b + (0.0 if onehot else ulp16(basis))
                out["B_h"] = L_h + g1.abs() * KAPPA * torch.sqrt(Q_u) + ulp16(h)
                if c["ugrad"]:
                    out["B_u"] = _gelu_g2(u).abs() * (L_u + KAPPA * torch.sqrt(Q_u)) + 4 * GELU_G_MEASURED["gelu_grad"] + ulp16(usv)
                else:
                    out["B_u"] = torch.zeros_like(u) if onehot else L_u + KAPPA * torch.sqrt(Q_u) + ulp16(usv)
        return out
    # ---- the backwards
    if kind == "fbwd":
        dbasis = f(t["dfeat"][lo:hi])
        if ref:
            L_db, Q_db = torch.zeros_like(val), torch.zeros_like(val)
    else:
        G = f(t["G"].reshape(-1, H)[sel][lo:hi])
        if mut == "drop_tile":
            G = G.masked_fill(drop.view(-1, 1), 0.0)
        split = kind == "full" and c["layout"] != "compact"
        dO = G if (split or c["layout"] == "compact") else rb(G)
        dr = dO @ W2
        if kind == "bwd":
            uin = f(u_in[lo:hi])
            gp = uin if c["ugrad"] else gelu_grad64(uin)
        else:
            gp = rb(g1)
        du = rb(dr * gp)
        out["do"], out["du"] = dO, du
        if ref:
            L_dO = 2.0 ** -17 * G.abs() if split else torch.zeros_like(G)
            L_dr = ((H + 8) * U + (2.0 ** -17 if split else 0.0)) * bm(dO.abs(), W2a)
            if kind == "bwd":
                L_gp = torch.zeros_like(gp) if c["ugrad"] else 4 * GELU_G_MEASURED["gelu_grad"] + 0.0 * gp
                Q_gp = torch.zeros_like(gp)
            else:
                L_gp = _gelu_g2(u).abs() * L_u + 4 * GELU_G_MEASURED["gelu_grad"]
                Q_gp = _gelu_g2(u) ** 2 * Q_u + ulp16(gp) ** 2
            L_du = gp.abs() * L_dr + dr.abs() * L_gp + U * du.abs()
            Q_pre = dr * dr * Q_gp
            Q_du = Q_pre + ulp16(du) ** 2
            out["B_du"] = L_du + KAPPA * torch.sqrt(Q_pre) + ulp16(du)
        dbasis = du @ W1
        if kind == "bwd":
            dbasis = rb(dbasis)
        if ref:
            L_db = (F + 8) * U * bm(du.abs(), W1a) + bm(L_du, W1a)
            Q_db = bm(Q_du, W1 * W1) + (ulp16(dbasis) ** 2 if kind == "bwd" else 0.0)
    tt = dbasis * val
    isg = 1.0 / sg
    zs = z * isg
    t1 = tt * zs
    w = z * zs - isg
    t2 = tt * w
    dy = -t1.sum(1)
    dsig = t2.sum(0)
    dstds = dsig if mut == "dstds_sign" else torch.where(stds < 0, -dsig, dsig)
    zero = torch.zeros(E, dtype=dt)
    dmul, dbias = zero.index_add(0, e, dy * d), zero.index_add(0, e, dy)
    out.update(dmeans=t1.sum(0), dstds=dstds, dmul=dmul, dbias=dbias)
    if kind == "full":
        out.update(dW1=du.t() @ basis, db1=du.sum(0), dW2=dO.t() @ h, db2=dO.sum(0))
    if ref:
        L_t = val * L_db + dbasis.abs() * L_val + U * tt.abs()
        Q_t = val * val * Q_db
        dzs = dz * isg + 2 * U * zs.abs()
        L_1 = zs.abs() * L_t + tt.abs() * dzs + U * t1.abs()
        dw = zs.abs() * dz + z.abs() * dzs + 3 * U * ((z * zs).abs() + isg)
        L_2 = w.abs() * L_t + tt.abs() * dw + U * t2.abs()
        acc = out["_acc"] = {}
        acc["dmeans"] = (t1.abs().sum(0), L_1.sum(0), (zs * zs * Q_t).sum(0))
        acc["dstds"] = (t2.abs().sum(0), L_2.sum(0), (w * w * Q_t).sum(0))
        T_dy = t1.abs().sum(1)
        L_dy = (K + 8) * U * T_dy + L_1.sum(1)
        Q_dy = (zs * zs * Q_t).sum(1)
        ix = lambda v: torch.zeros(E, dtype=F64).index_add(0, e, v)
        acc["dbias"] = (ix(T_dy), ix(L_dy), ix(Q_dy))
        acc["dmul"] = (ix(T_dy * d.abs()), ix(L_dy * d.abs() + U * (dy * d).abs()), ix(Q_dy * d * d))
        if kind == "full":
            ba, da, ha, oa = basis.abs(), du.abs(), h.abs(), dO.abs()
            acc["dW1"] = (bm(da.t(), ba), bm(L_du.t(), ba) + bm(da.t(), L_b), bm(Q_du.t(), basis * basis) + bm((du * du).t(), Q_b))
            acc["db1"] = (da.sum(0), L_du.sum(0), Q_du.sum(0))
            acc["dW2"] = (bm(oa.t(), ha), bm(L_dO.t(), ha) + bm(oa.t(), L_h), bm((dO * dO).t(), Q_h))
            acc["db2"] = (oa.sum(0), L_dO.sum(0), torch.zeros(H, dtype=F64))
    return out


GRADS = ("dW1", "db1", "dW2", "db2", "dmul", "dbias", "dmeans", "dstds")
OUTPUTS = {"fwd": ("out", "feat", "u", "h"), "bwd": ("du",) + GRADS[4:], "full": GRADS, "ffwd": ("feat",), "fbwd": GRADS[4:]}


def saved_u(c, t, geo):
    """what the per-pair backward is handed as the forward's saved tensor: bf16(u), or bf16(gelu'(u)) with ugrad -- of the float64 forward"""
    fc = dict(c, kind="fwd", save=True)
    r = chain(fc, t, geo, bounds=False)
    return r["u"].to(BF16)


def reference(c, t, geo):
    u_in = saved_u(c, t, geo) if c["kind"] == "bwd" else None
    ref = chain(c, t, geo, u_in=u_in)
    ref["u_in"] = u_in
    return ref


def emulate(c, t, geo, ref, mut=None):
    if mut == "half_dmul":
        t = dict(t, _worst_e=int((ref["dmul"].abs() / ref["B_dmul"]).argmax()))
    return chain(c, t, geo, dt=F32, mut=mut, u_in=ref.get("u_in"))


def evaluate(c, ref, got):
    """got: {name: tensor shaped as the reference's} -> {name: (worst ratio, gain, bad elements, first bad index)}"""
    res = {}
    for k in OUTPUTS[c["kind"]]:
        if k not in got or k not in ref:
            continue
        g, r, b = got[k].to(F64), ref[k], ref["B_" + k]
        q = (g - r).abs() / torch.where(b > 0, b, torch.full_like(b, 1e-300))
        q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
        bad = (q > 1.0).flatten().nonzero().flatten()
        res[k] = (worst_ratio(g, r, b), gain(g, r, b) if r.numel() >= 64 else 0.0, int(bad.numel()), int(bad[0]) if bad.numel() else -1)
    return res


@functools.lru_cache(maxsize=6)
def prepared(i, mode):
    """(inputs, geometry, reference) of CASES[i] in a mode: computed once, shared by the tests that run the case (the edge-size runs too)"""
    c = CASES[i]
    geo = geometry(pc_of(c))
    t = make_inputs(c, mode)
    return t, geo, reference(c, t, geo)
