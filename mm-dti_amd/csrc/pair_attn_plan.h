// Which kernel a pair-attention call runs, with which grid and workgroup size -- decided here, in plain host C++17 (no HIP types), and
// nowhere else.  pair_attn.hip / pair_attn_bwd.hip validate, ask pair_attn_fwd_plan / pair_attn_bwd_plan, and launch what the plan
// names from one table per direction, indexed by the plan's key; mmdti_pair_attn_plan returns the same plan without launching
// (tests/test_pair_cases_cpu.py asks it for every case and sweeps every N).  The kernels use static LDS only: no opt-in.
#pragma once

namespace mmdti {

// key tiles of 16 the MFMA kernels are instantiated for: 17 covers the reference's crop (max_atoms = 256 -> N <= 258, data/conformer.py:53,199-204)
constexpr int PA_MAX_NT = 17;

// ---- families and their dense keys ----
enum PairAttnFamily {
  PA_FWD_MFMA = 0,   // pair_attn_fwd_mfma_kernel: 80 instances
  PA_BWD_MFMA = 1,   // pair_attn_bwd_mfma_kernel: 88 instances
  PA_FWD_ELEM = 2,   // pair_attn_fwd_kernel<NCH>: N > 272 or rows / planes that are not 16-byte aligned
  PA_BWD_ELEM = 3,   // pair_attn_bwd_kernel<NCH, DET>
};
constexpr int PA_FWD_MFMA_KERNELS = 80, PA_BWD_MFMA_KERNELS = 88, PA_FWD_ELEM_KERNELS = 5, PA_BWD_ELEM_KERNELS = 10;
// the 5 / 9 / 13 / 17-tile instantiations of the fp32 planes
constexpr int pa_bucket(int nqb) { return nqb <= 5 ? 0 : nqb <= 9 ? 1 : nqb <= 13 ? 2 : 3; }
constexpr int pa_bucket_nt(int b) { return 5 + 4 * b; }
// forward MFMA: compact planes 0..67 by (tiles, fp16 operands, ragged); fp32 planes 68..79 by (bucket, row-major | tiled | tiled FULL)
constexpr int pa_fwd_compact_key(int nt, int f16, int rag) { return (nt - 1) * 4 + f16 * 2 + rag; }
constexpr int pa_fwd_f32_key(int bucket, int tiled, int full) { return 68 + bucket * 3 + (full ? 2 : tiled ? 1 : 0); }
// backward MFMA: compact planes 0..33 (fp32 G) and 34..67 (bf16 G: the rows of pair_attn_bwd_g16.hip) by (tiles, ragged); fp32 planes
// 68..87 by (bucket, row-major 3 | 4 waves, tiled 3 | 4 waves, tiled FULL)
constexpr int PA_BWD_COMPACT_ROWS = 34;
constexpr int pa_bwd_compact_key(int g16, int nt, int rag) { return g16 * PA_BWD_COMPACT_ROWS + (nt - 1) * 2 + rag; }
constexpr int pa_bwd_f32_key(int bucket, int tiled, int full, int nw) { return 68 + bucket * 5 + (full ? 4 : (tiled ? 2 : 0) + (nw == 4)); }
// ragged batches: the key-tile counts the sweeps are unrolled for (pair_attn.h, "Ragged batches"; attn_maps.hip covers the same tiles)
__host__ __device__ constexpr int pa_kt_step(int nt) { return nt <= 9 ? 1 : (nt <= 13 ? 2 : 4); }
// smallest supported count >= kt
__host__ __device__ constexpr int pa_kt_effective(int kt, int nt) {
  const int s = pa_kt_step(nt), k = ((kt < 1 ? 1 : kt) + s - 1) / s * s;
  return k >= nt ? nt : k;
}
// per-element kernels: 64-key chunks 1..5; the backward's deterministic form behind the plain one
constexpr int pa_elem_nch(int N) { return (N + 63) / 64 < 5 ? (N + 63) / 64 : 5; }
constexpr int pa_fwd_elem_key(int nch) { return nch - 1; }
constexpr int pa_bwd_elem_key(int nch, int det) { return det * 5 + nch - 1; }

// workgroup sizes of the MFMA kernels, by query blocks of 16
constexpr int pa_fwd_block(int nqb) { return nqb % 3 == 0 ? 192 : (nqb < 4 ? 64 * nqb : 256); }
// (16 and 17 tiles: three waves and a register cap for two workgroups per CU -- with four waves the per-wave dK / dV accumulators
//  leave LDS for one workgroup, and 251 + 12 registers for one wave per SIMD: N = 250 / 258 took 4.2 / 3.9 ms against 2.15 at N = 240)
// (5 blocks: 2,2,1 on three waves beats 2,1,1,1 on four)
constexpr int pa_bwd_block(int nqb) { return (nqb % 3 == 0 || nqb >= 16 || nqb == 5) ? 192 : (nqb < 4 ? 64 * nqb : 256); }
// the backward kernel's NW template argument: its per-wave LDS images are sized for three waves or for four
constexpr int pa_bwd_nw(int nqb) { return pa_bwd_block(nqb) == 192 ? 3 : 4; }

struct PairAttnPlan {
  int family;   // PairAttnFamily
  int key;      // the row of the family's table
  int grid, block;
  int nqb;      // query blocks of 16 (MFMA families; else 0)
  int nw;       // NW of the backward MFMA kernel (else 0)
};
constexpr int PAIR_ATTN_PLAN_INTS = sizeof(PairAttnPlan) / sizeof(int);

// (same eligibility rule in both directions: the two MFMA kernels share one dropout-mask generator)
// planes_aligned: the two pair tensors of the call are 16-byte aligned
static inline bool pa_mfma_ok(int N, int ld, bool planes_aligned) { return ld % 4 == 0 && planes_aligned && N <= 16 * PA_MAX_NT; }

// (arguments already validated by the entry point)
static inline PairAttnPlan pair_attn_fwd_plan(int B, int N, int H, int ld, int tiled, int compact, bool planes_aligned, bool ragged, bool qkv_f16) {
  PairAttnPlan p = {};
  p.grid = B * H;
  if (!pa_mfma_ok(N, ld, planes_aligned)) {
    p.family = PA_FWD_ELEM; p.key = pa_fwd_elem_key(pa_elem_nch(N)); p.block = 256;
    return p;
  }
  const int nqb = (N + 15) / 16;
  p.family = PA_FWD_MFMA; p.nqb = nqb; p.block = pa_fwd_block(nqb);
  // The hot path (compact planes) has an instantiation for EVERY tile count: all its tiles exist, the interior ones run
  // without predicates (FULL).  In a kernel instantiated for more tiles than N has, the surplus tiles are predicated off but
  // still walked and no tile takes the fast path -- 25-45 % more time per real tile (N = 96 / 113 / 128 on the 9-tile kernel).
  if (compact) p.key = pa_fwd_compact_key(nqb, qkv_f16, ragged);
  else p.key = pa_fwd_f32_key(pa_bucket(nqb), tiled, tiled && nqb == pa_bucket_nt(pa_bucket(nqb)));
  return p;
}

static inline PairAttnPlan pair_attn_bwd_plan(int B, int N, int H, int ld, int tiled, int compact, int g16, bool planes_aligned, bool ragged, bool det) {
  PairAttnPlan p = {};
  p.grid = B * H;
  if (!pa_mfma_ok(N, ld, planes_aligned)) {
    // the deterministic mode: the waves of a workgroup add in wave order
    p.family = PA_BWD_ELEM; p.key = pa_bwd_elem_key(pa_elem_nch(N), det); p.block = 256;
    return p;
  }
  const int nqb = (N + 15) / 16;
  p.family = PA_BWD_MFMA; p.nqb = nqb; p.block = pa_bwd_block(nqb); p.nw = pa_bwd_nw(nqb);
  // (compact planes -- the hot path -- have one instantiation per tile count, for fp32 and for bf16 gradients)
  if (compact) p.key = pa_bwd_compact_key(g16, nqb, ragged);
  else p.key = pa_bwd_f32_key(pa_bucket(nqb), tiled, tiled && nqb == pa_bucket_nt(pa_bucket(nqb)), p.nw);
  return p;
}

}  // namespace mmdti
