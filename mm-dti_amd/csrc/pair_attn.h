// pair_attn.h -- shared by pair_attn.hip (forward) and pair_attn_bwd.hip (backward): element types of the pair tensors and their
// load / store / rounding helpers, the bf16 hi + lo split, the ragged key-tile dispatch.  (Two translation units so that the ~200
// kernel instantiations compile in parallel.)
#pragma once
#include <type_traits>

#include "common.h"
#include "pair_attn_plan.h"

namespace mmdti {

constexpr int HD = 8;

__device__ __forceinline__ void load8_bf16(const bf16_t* p, float (&o)[8]) { unpack8_bf16(*reinterpret_cast<const uint4*>(p), o); }
__device__ __forceinline__ void store8_bf16(bf16_t* p, const float (&v)[8]) {
  uint4 u;
  pack8_bf16(v, u);
  *reinterpret_cast<uint4*>(p) = u;
}


// =====================================================================================================================
// MFMA-tiled forward.  One wave owns a block of 16 queries and walks the key tiles of 16: the score tile is computed
// TRANSPOSED, S^T[key][query] = K.Q^T (one v_mfma_f32_16x16x16_bf16 on the raw bf16 q / k rows: head_dim 8 zero-padded
// to k = 16, exact products, fp32 accumulation), scaled and added to the bias tile in the accumulator layout, so bias
// add, S write-out and softmax all happen on that layout
// (lane = query column, 4 consecutive keys per lane-group in registers): pair traffic is one 16-byte load + one 16-byte
// store per lane per tile, the row softmax needs only two cross-lane steps per query block, and P^T is already the B
// operand of the P.V product (O^T = V^T.P^T) -- no data movement between the two matrix products.
// Dropout element index = (bh*N + query)*ld + key (ld % 4 == 0: one RNG call per 4 keys).
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Matrix products of both MFMA kernels: Q, K, V, dO are bf16 in memory, so they enter v_mfma_f32_16x16x16_bf16 exactly as
// loaded; an fp32 factor (the probabilities, G) is split into bf16 high + bf16 low parts (x = hi + lo + O(2^-17 |x|)) and
// its product runs twice -- fp32-class products with fp32 accumulation at a quarter of the matrix-pipe time and a third
// of the LDS instructions of the fp32 16x16x4 form.
typedef short pa_s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 pa_bf16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) pa_s16x4 pa_lds_s16x4;

__device__ __forceinline__ pa_s16x4 pa_pack4(const f32x4& v) {
  pa_bf16x4 h;
  h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
  return __builtin_bit_cast(pa_s16x4, h);
}
// x = hi + lo with hi = bf16(x), lo = bf16(x - hi)
__device__ __forceinline__ void pa_split4(const f32x4& v, pa_s16x4& hi, pa_s16x4& lo) {
  pa_bf16x4 h;
  h[0] = (__bf16)v[0]; h[1] = (__bf16)v[1]; h[2] = (__bf16)v[2]; h[3] = (__bf16)v[3];
  f32x4 r;
  r[0] = v[0] - (float)h[0]; r[1] = v[1] - (float)h[1]; r[2] = v[2] - (float)h[2]; r[3] = v[3] - (float)h[3];
  hi = __builtin_bit_cast(pa_s16x4, h);
  lo = pa_pack4(r);
}
#define PA_MFMA16(A, B, C) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(A, B, C, 0, 0, 0)
// The forward kernel also exists for q | k | v stored as fp16 (F16: the opt-in fp16 forward-operand mode -- three more mantissa
// bits in the operands of q.k^T and P.v; the raw 16-bit LDS images are the same, only the MFMA and the split of P change)
typedef _Float16 pa_h16x4 __attribute__((ext_vector_type(4)));
template <bool F16>
__device__ __forceinline__ f32x4 pa_mfma16(const pa_s16x4& a, const pa_s16x4& b, const f32x4& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(pa_h16x4, a), __builtin_bit_cast(pa_h16x4, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}
// x = hi + lo in the operand type of the product (bf16, or fp16 when F16: 22 mantissa bits kept of the fp32 factor)
template <bool F16>
__device__ __forceinline__ void pa_split4_t(const f32x4& v, pa_s16x4& hi, pa_s16x4& lo) {
  if constexpr (F16) {
    pa_h16x4 h, l;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      h[r] = (_Float16)v[r];
      l[r] = (_Float16)(v[r] - (float)h[r]);
    }
    hi = __builtin_bit_cast(pa_s16x4, h);
    lo = __builtin_bit_cast(pa_s16x4, l);
  } else {
    pa_split4(v, hi, lo);
  }
}
#define PA_LOG2E 1.44269504088896340736f

// Element types of the pair tensors.  Row-major planes and the round-1 tiled planes hold fp32.  The COMPACT tiled planes
// hold the logits chain S as fp16 (same [nKB][nKB][256] element order: a lane's 4 keys are 8 contiguous bytes, a tile
// 512 B): the pair kernels are bound by this traffic -- the forward's halves, the backward's drops from 12 to 10 B per
// pair and head.  The gradient chain G stays fp32 by default; bf16 is an opt-in (layout bit 2) that costs gradient
// fidelity where sums over pairs cancel ("tried").
//   S (fp16, round to nearest even): what the reference's own AMP path carries between layers (its attn_weights are fp16
//     under autocast); the softmax of the layer that produced a value runs on the ROUNDED value, so the forward and the
//     backward's recomputation see the same logits.  Values above the fp16 range saturate at 65504 instead of becoming
//     +inf (a -inf row mask stays -inf).
//   G (bf16, opt-in): fp16 would flush the small gradients the reference protects with its GradScaler; bf16 keeps fp32's
//     range.  The dQ / dK products of a layer use the unrounded fp32 G of that layer; only what is handed to the previous
//     layer is rounded.
typedef _Float16 pa_f16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f32x4 pa_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 pa_load4_nt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
__device__ __forceinline__ void pa_store4_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }
__device__ __forceinline__ f32x4 pa_round4(f32x4& keep, f32x4 v) { keep = v; return v; }

__device__ __forceinline__ f32x4 pa_widen_f16(const pa_f16x4& h) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (float)h[r];
  return v;
}
__device__ __forceinline__ pa_f16x4 pa_narrow_f16(const f32x4& v) {
  pa_f16x4 h;
#pragma unroll
  for (int r = 0; r < 4; ++r) h[r] = (_Float16)v[r];
  return h;
}
__device__ __forceinline__ f32x4 pa_load4(const _Float16* p) { return pa_widen_f16(*reinterpret_cast<const pa_f16x4*>(p)); }
__device__ __forceinline__ f32x4 pa_load4_nt(const _Float16* p) { return pa_widen_f16(__builtin_nontemporal_load(reinterpret_cast<const pa_f16x4*>(p))); }
__device__ __forceinline__ void pa_store4_nt(_Float16* p, const f32x4& v) {   // (v already went through pa_round4: the conversion is exact)
  __builtin_nontemporal_store(pa_narrow_f16(v), reinterpret_cast<pa_f16x4*>(p));
}
// round a quad of logits to its storage type; `keep` receives the stored form so that the store does not convert again.
// (v_med3_f32 against (-inf, 65504) is min(v, 65504) without fminf's NaN-canonicalising v_max_f32 in front)
__device__ __forceinline__ f32x4 pa_round4(pa_f16x4& keep, const f32x4& v) {
  f32x4 c;
#pragma unroll
  for (int r = 0; r < 4; ++r) c[r] = __builtin_amdgcn_fmed3f(v[r], -INFINITY, 65504.f);
  keep = pa_narrow_f16(c);
  return pa_widen_f16(keep);
}
__device__ __forceinline__ void pa_store4_nt(_Float16* p, const pa_f16x4& h) { __builtin_nontemporal_store(h, reinterpret_cast<pa_f16x4*>(p)); }

__device__ __forceinline__ f32x4 pa_widen_bf16(const pa_s16x4& h) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = __builtin_bit_cast(float, (uint32_t)(uint16_t)h[r] << 16);
  return v;
}
__device__ __forceinline__ f32x4 pa_load4(const __bf16* p) { return pa_widen_bf16(*reinterpret_cast<const pa_s16x4*>(p)); }
__device__ __forceinline__ f32x4 pa_load4_nt(const __bf16* p) { return pa_widen_bf16(__builtin_nontemporal_load(reinterpret_cast<const pa_s16x4*>(p))); }
__device__ __forceinline__ void pa_store4_nt(__bf16* p, const f32x4& v) { __builtin_nontemporal_store(pa_pack4(v), reinterpret_cast<pa_s16x4*>(p)); }

// Ragged batches: the number of key tiles a molecule's sweeps cover is a COMPILE-TIME constant of the code that runs them.  A
// workgroup reads its molecule's count and branches ONCE into the body unrolled for it; per-tile `if (t >= kt) skip` branches
// inside one body unrolled for all NT tiles were measured at + 20-40 % per processed tile (they keep the loads of later tiles
// from being issued ahead).  Supported counts: every k up to 9 tiles, every 2nd up to 13, every 4th beyond, and NT itself -- a
// count in between runs as the next supported one (the extra tiles are ordinary all-padding tiles: -inf logits, zero gradient,
// read and written like any other), identically in every layer and in both directions.
// (pa_kt_step / pa_kt_effective, the supported counts: pair_attn_plan.h -- the attention-map kernels round a count the same way)
// f(std::integral_constant<int, ke>) for a count ke that pa_kt_effective produced (K walks down the supported counts)
template <int NT, int K, typename F>
__device__ __forceinline__ void pa_dispatch_kt(int ke, F&& f) {
  constexpr int step = pa_kt_step(NT);
  constexpr int below = (K == NT) ? ((NT - 1) / step) * step : K - step;   // the next supported count below K (0: none)
  if constexpr (below < 1) {
    f(std::integral_constant<int, K>{});
  } else {
    if (ke >= K) f(std::integral_constant<int, K>{});
    else pa_dispatch_kt<NT, below>(ke, f);
  }
}

// ---- The pieces pair_attn_fwd_mfma_kernel (pair_attn.hip) and pair_attn_bwd_mfma_kernel (pair_attn_bwd_mfma.h) share, one definition
// each.  Both kernels are held to the instruction streams they had before the pieces were shared (profiles/pair_kernels_shared_isa.txt).
// The pieces that declare or name the state of a kernel body are macros: that state lives in the captures of the kernels' body lambdas.

// Workgroup prologue.  Declares bh / b / h (the 64 heads of a token share 128-byte q / k / v lines, 8 heads per line: xcd_chunk keeps a
// molecule's heads on one XCD), D / D3, tid / lane / wave / nwaves, nKB, kt (wave-uniform: one molecule per workgroup; rounded up to a
// count the sweeps are unrolled for) and the token rows of molecule b: row0 / rows / base.
// PACKED token rows (RAG only, row_off != null): molecule b owns rows [row_off[b], row_off[b+1]) of qkv / o / key_pad -- its real
// tokens followed by at most ONE representative pad row (every pad row of a molecule is the same row at dropout 0: zeroed
// input, constant bias row, same keys) -- instead of rows [b*N, (b+1)*N).  Pair planes stay indexed by position.
// Names the kernel's RAG, NT, qkv, N, H, key_tiles, row_off.
#define PA_WG_PROLOGUE()                                                                                                   \
  const int bh = xcd_chunk(blockIdx.x, gridDim.x), b = bh / H, h = bh - b * H;                                             \
  const int D = H * HD, D3 = 3 * D;                                                                                        \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;                                 \
  const int nKB = (N + 15) >> 4;                                                                                           \
  const int kt = RAG ? pa_kt_effective(min(__builtin_amdgcn_readfirstlane(key_tiles[b]), nKB), NT) : NT;                   \
  const bool packed = RAG && row_off != nullptr;                                                                           \
  const int row0 = packed ? __builtin_amdgcn_readfirstlane(row_off[b]) : b * N;                                            \
  const int rows = packed ? __builtin_amdgcn_readfirstlane(row_off[b + 1]) - row0 : N;                                     \
  const bf16_t* base = qkv + (long long)row0 * D3 + h * HD

// Layouts (TILED): row-major [N][ld] planes, or the blocked-row planes of common.h whose 16x16 tiles are stored in accumulator
// order -- a wave's access to a tile is then one contiguous KiB at a compile-time offset from the query block's base,
// and, because every pad slot of a tiled S holds -inf (written by mmdti_gbf_bias_fwd, preserved by every S store) and every pad slot
// of a tiled G holds 0, interior tiles need no predicate and no pad masking at all.  Only the last query block (EDGE) and the last
// key tile keep per-lane predicates.  FULL: nKB == NT, so "last tile" is a compile-time index.
// PA_LAST_TILE: declares nlast, colok and the dropout key rk of the (molecule, head) plane (common.h).  Names nKB, g, N, seed, site, bh.
#define PA_LAST_TILE()                                 \
  const int nlast = nKB - 1;                           \
  const bool colok = 4 * g < N - 16 * nlast;           \
  const Rng24 rk = rng24_key(seed, site, (uint32_t)bh)
// Query-block addressing of a body (query block qb, EDGE), in three parts so that each kernel keeps the order of its statements (moving the
// kernels' own loads and pointers across them changes the schedule).  PA_QROW declares qi, this query row's drop threshold t8, qvalid and
// rowoff (row-major: the lane's 4 keys of tile t start at rowoff + 16t + 4g; also the dropout counter base); PA_QTILE vr and tbase;
// PA_TILE_STEP TSTEP and goff.
// (tiled planes, common.h "blocked rows": the block of 16 queries starts at 16 qb N4, a lane's 4 keys of tile t sit at
//  vr (16 t + 4 g) + 4 c16 -- 256 t + 4 lane in a complete block; lanes past the last query of an incomplete block point at query 0,
//  key groups past N4 -- N <= 12 only -- at group 0: whatever a predicate-off lane reads lies inside the plane)
// Names qb, c16, g, thresh, rk, rows, bh, N, ld.
#define PA_QROW()                                                                                                          \
  const int qi = qb * 16 + c16;                                                                                            \
  const uint32_t t8 = thresh ? rng24_row_t8(rk, (uint32_t)qi, thresh) : 0u;                                                \
  const bool qvalid = EDGE ? qi < rows : true;                                                                             \
  const long long rowoff = ((long long)bh * N + (qvalid ? qi : 0)) * ld
#define PA_QTILE()                                                                                                         \
  const int vr = EDGE ? min(16, N - qb * 16) : 16;                                                                         \
  const long long tbase = (long long)bh * pair_plane(N) + (long long)qb * 16 * pair_n4(N) + ((4 * g < pair_n4(N) ? g : 0) * vr + (qvalid ? c16 : 0)) * 4
#define PA_TILE_STEP()                                                                                                     \
  const int TSTEP = TILED ? (EDGE ? vr * 16 : 256) : 16;                                                                   \
  const int goff = TILED ? 0 : 4 * g
// the predicate of this lane's 4 keys of tile T, and "interior tile of a complete query block: no predicate" (FULL only: as a
// wave-uniform run-time branch it doubles the unrolled code and the NT = 13 backward fell out of the instruction cache, 1.2 -> 3.3 ms).
// Name TILED, FULL, EDGE, NT, qvalid, g, N, nlast, colok.
#define PA_PRED(T) (!TILED ? (qvalid && (T) * 16 + 4 * g < N) \
                           : (qvalid && (FULL ? ((T) < NT - 1 || colok) : ((T) < nlast || ((T) == nlast && colok)))))
#define PA_FAST(T) (TILED && !EDGE && (FULL ? (T) < NT - 1 : false))
// (Statement macros are one statement each -- a comma expression or a do { } while (0) -- and are written with their semicolon.)
// DST = the lane's 4 values of tile T of the plane at PTR: a non-temporal load on the fast path, else predicated -- a lane whose
// predicate is off reads the first 16 bytes at PTR (always inside the tensor) and takes FILL.  PA_LOAD4_IF: only where COND (uniform:
// the backward's "there is an incoming gradient") holds, FILL elsewhere.  Names TSTEP, goff.
// (PA_LOAD4_: AND_COND is "&& (COND)", or nothing where COND is true -- "PA_PRED(T) && (true)" gives the non-FULL tiled instances of both
//  kernels other instruction streams, and "(COND) ? PA_PRED(T) : false" every backward instance.)
#define PA_LOAD4_(DST, PTR, T, FILL, COND, AND_COND)                             \
  do {                                                                           \
    if (PA_FAST(T)) {                                                            \
      const f32x4 ld4 = pa_load4_nt((PTR) + ((COND) ? (T) * TSTEP + goff : 0));  \
      DST = (COND) ? ld4 : f32x4{FILL, FILL, FILL, FILL};                        \
    } else {                                                                     \
      const bool pr = PA_PRED(T) AND_COND;                                       \
      const f32x4 ld4 = pa_load4((PTR) + (pr ? (T) * TSTEP + goff : 0));         \
      DST = pr ? ld4 : f32x4{FILL, FILL, FILL, FILL};                            \
    }                                                                            \
  } while (0)
#define PA_LOAD4(DST, PTR, T, FILL) PA_LOAD4_(DST, PTR, T, FILL, true, )
#define PA_LOAD4_IF(DST, PTR, T, FILL, COND) PA_LOAD4_(DST, PTR, T, FILL, COND, && (COND))
// ... and the store of V to them
#define PA_STORE4(PTR, T, V)                                                     \
  do {                                                                           \
    if (PA_FAST(T)) {                                                            \
      pa_store4_nt((PTR) + (T) * TSTEP + goff, V);                               \
    } else if (PA_PRED(T)) {                                                     \
      pa_store4_nt((PTR) + (T) * TSTEP + goff, V);                               \
    }                                                                            \
  } while (0)
// Row softmax of the KT quads X[t] a lane holds of its query's row.  PA_ROW_MAX finishes the row max M over the lane groups;
// PA_ROW_EXP2 declares mneg and lsum, replaces X by exp(X - M) as exp2(X * log2(e) - M * log2(e)) -- one FMA + v_exp_f32 per element,
// the same in both directions -- and sums the row.  (What an all -inf row does to M and what becomes of 1 / lsum is the kernels' own.)
#define PA_ROW_MAX(M) ((M) = fmaxf((M), __shfl_xor((M), 16, 64)), (M) = fmaxf((M), __shfl_xor((M), 32, 64)))
#define PA_ROW_EXP2(X, M)                                                        \
  const float mneg = -M * PA_LOG2E;                                              \
  float lsum = 0.f;                                                              \
  _Pragma("unroll")                                                              \
  for (int t = 0; t < KT; ++t) {                                                 \
    {                                                                            \
      _Pragma("unroll")                                                          \
      for (int r = 0; r < 4; ++r) {                                              \
        const float e = __builtin_amdgcn_exp2f(fmaf(X[t][r], PA_LOG2E, mneg));   \
        X[t][r] = e;                                                             \
        lsum += e;                                                               \
      }                                                                          \
    }                                                                            \
  }                                                                              \
  lsum += __shfl_xor(lsum, 16, 64);                                              \
  lsum += __shfl_xor(lsum, 32, 64)
// the dropout word of the lane's 4 keys of tile T (the counter: the element's index in the row-major plane).  Names rk, qi, ld, g.
#define PA_DROP_WORD(T) rng24_word(rk, ((uint32_t)qi * (uint32_t)ld + (T) * 16 + 4 * g) >> 2)
// what a wave has written to its LDS patches is visible to its other lanes
__device__ __forceinline__ void pa_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The kernels' tail: every wave takes query blocks wave, wave + nwaves, .. (packed: the pad rows past the representative one are not
// computed), a complete block of a tiled plane without the EDGE predicates; ragged kernels branch once into the body unrolled for kt.
// Names body, packed, rows, nKB, wave, nwaves, kt.
#define PA_RUN_QUERY_BLOCKS()                                                    \
  const int nQB = packed ? (rows + 15) >> 4 : nKB;                               \
  auto run = [&](auto kt_c) {                                                    \
    for (int qb = wave; qb < nQB; qb += nwaves) {                                \
      if (TILED && qb * 16 + 16 <= rows) body(qb, std::false_type{}, kt_c);      \
      else body(qb, std::true_type{}, kt_c);                                     \
    }                                                                            \
  };                                                                             \
  if constexpr (RAG) pa_dispatch_kt<NT, NT>(kt, run);                            \
  else run(std::integral_constant<int, NT>{})

}  // namespace mmdti


static inline int check_common(const char* fn, int B, int N, int H, int ld) {
  MMDTI_REQUIRE(B > 0 && N > 0 && H > 0, "%s: B,N,H must be positive", fn);
  MMDTI_REQUIRE(N <= 320, "%s: N=%d exceeds the supported 320 atoms (+BOS/EOS)", fn, N);
  MMDTI_REQUIRE(ld >= N, "%s: ld (%d) < N (%d)", fn, ld, N);
  MMDTI_REQUIRE((long long)B * H <= 2147483647LL, "%s: grid too large", fn);
  return MMDTI_OK;
}


namespace mmdti {
// pair_attn.hip: the forward's two tables (PA_FWD_MFMA / PA_FWD_ELEM) and the validation + plan its launch shares with mmdti_pair_attn_plan
const KernelRow* pair_attn_fwd_table(int family, int* n);
int pair_attn_fwd_prepare(PairAttnPlan& plan, const void* qkv_bf16, const void* bias_in, const void* s_out, const void* o_bf16, int B, int N, int H,
                          int ld, float drop_p, int layout, const void* key_tiles, const void* row_off, int qkv_f16);
}  // namespace mmdti
