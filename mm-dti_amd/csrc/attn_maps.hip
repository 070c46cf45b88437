// Attention maps for gfx950: the probabilities of an attention, reduced over heads, written as [B, Lq, Lk] fp32 -- what a person reads
// (mm_module.py:497-514 attention_probs of the cross-modal block, modeling_roberta.py:158-183 attn_weights of the ChemBERTa tower,
// transformers.py:137-139 the pair attention of the Uni-Mol tower) -- without the [B, heads, Lq, Lk] tensor ever existing.
//
//   mmdti_attn_map       recomputes the probabilities of one fused attention (attn.hip) from q, k and the row statistics its forward
//                        saved: p = exp2(s2 - m) * inv, the expression of the backward kernels (attn.hip, attn_prob).  One workgroup per
//                        (sequence, block of 16 output rows); a wave owns 16 x 16 output tiles and walks the heads in ascending order,
//                        adding each head's tile in registers.  q and k fragments come straight from global memory (a head's K rows
//                        are re-read once per query block, from L2): no LDS.
//   mmdti_pair_attn_map  streams one layer's stored pair logits once.  One workgroup per (molecule, block of 16 queries): in the tiled
//                        layouts that block of one head is ONE contiguous run of 16 N4 elements in MFMA accumulator order, so a lane
//                        holds 4 keys per 16-key tile of its query's row and the row softmax needs two cross-lane steps.  The four
//                        waves split the heads into four runs of consecutive heads, each adds its heads in ascending order, and the
//                        four partial sums meet in wave order through LDS: ((w0 + w1) + w2) + w3.  Row-major planes: a wave per query
//                        row, the heads in ascending order.
// Every element of `out` is written exactly once, by one thread, from a sum in a fixed order: no atomics, two calls give the same bits.
// Neither kernel reads what the forward does not store: keys past a sequence's real keys, query rows past its real queries, key tiles
// past a ragged molecule's covered count and query rows past n_real are never loaded -- their outputs are written as zeros.
#include "common.h"
#include "maps_plan.h"
#include "attn_shared.h"      // the forward's own mask clamp, probability and fragment load (attn.hip)
#include "pair_attn_plan.h"   // pa_kt_effective: the key tiles a ragged molecule covers

namespace mmdti {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

struct AttnMapArgs {
  const bf16_t* q;
  const bf16_t* k;
  const float* key_add;
  const float* stats;
  float* out;
  const int* q_off;
  const int* k_off;
  const int* k_cnt;
  const int* q_cnt;
  int heads, Lq, Lk, ldq, ldk, Lq_out, ld_out, q_rows, head, vec;
  float scale2, inv_heads;
};

__device__ __forceinline__ void am_store4(float* out_row, int col, int ld_out, bool vec, const f32x4& v) {
  if (vec) {
    if (col < ld_out) *reinterpret_cast<f32x4*>(out_row + col) = v;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (col + r < ld_out) out_row[col + r] = v[r];
  }
}

template <int HD>
__global__ __launch_bounds__(MAPS_BLOCK) void attn_map_kernel(AttnMapArgs a) {
  constexpr int KC = HD < 32 ? 1 : HD / 32;
  const int nqt = (a.Lq_out + 15) >> 4;
  const int b = blockIdx.x / nqt, qt = blockIdx.x - b * nqt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  int q0, lq, k0, lk;      // (attn.hip, attn_seq: the same decode; sharing it costs this kernel an instruction, so it stays here)
  if (a.q_off) {
    q0 = __builtin_amdgcn_readfirstlane(a.q_off[b]);
    lq = __builtin_amdgcn_readfirstlane(a.q_off[b + 1]) - q0;
    k0 = __builtin_amdgcn_readfirstlane(a.k_off[b]);
    lk = min(__builtin_amdgcn_readfirstlane(a.k_cnt[b]), __builtin_amdgcn_readfirstlane(a.k_off[b + 1]) - k0);
  } else {
    q0 = b * a.Lq; lq = a.Lq; k0 = b * a.Lk; lk = a.Lk;
  }
  lq = min(lq, a.Lq);
  lk = min(max(lk, 0), a.Lk);
  if (a.q_cnt) lq = min(lq, max(__builtin_amdgcn_readfirstlane(a.q_cnt[b]), 0));
  const int qi = qt * 16 + i;
  const bool qv = qi < lq;                                   // a real query of this sequence
  const bool qblock = qt * 16 < lq;                          // (uniform) the block holds one
  const int h0 = a.head < 0 ? 0 : a.head, h1 = a.head < 0 ? a.heads : a.head + 1;
  float* out_row = a.out + ((long long)b * a.Lq_out + (qi < a.Lq_out ? qi : 0)) * a.ld_out;
  const bf16_t* qrow = a.q + ((long long)q0 + (qv ? qi : 0)) * a.ldq;
  const int nt_out = (a.ld_out + 15) >> 4;
  for (int t = wave; t < nt_out; t += nw) {
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (qblock && t * 16 < lk) {                             // (uniform)
      const int key = t * 16 + i;                            // the key row this lane supplies to the product
      const bool kv = key < lk;
      const bf16_t* krow = a.k + ((long long)k0 + (kv ? key : 0)) * a.ldk;
      f32x4 ka;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kr = t * 16 + 4 * g + r;                   // the keys of this lane's accumulator registers
        ka[r] = kr < lk ? (a.key_add ? attn_mask2(a.key_add[(long long)b * a.Lk + kr]) : 0.f) : -INFINITY;
      }
      // (a head's operands -- K rows, Q rows, the row statistics -- are loaded while the head before it is computed)
      bf16x8 kf[KC], qf[KC], kfn[KC], qfn[KC];
      float2 st = make_float2(0.f, 0.f), stn = make_float2(0.f, 0.f);
      const long long srow0 = a.q_off ? (long long)q0 + qi : (long long)b * a.heads * a.Lq + qi;
      const long long sstep = a.q_off ? (long long)a.q_rows : (long long)a.Lq;
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        kf[c] = attn_frag_global<HD>(krow + h0 * HD, kv, c, lane);
        qf[c] = attn_frag_global<HD>(qrow + h0 * HD, qv, c, lane);
      }
      if (qv) st = *reinterpret_cast<const float2*>(a.stats + (srow0 + h0 * sstep) * 2);
      for (int h = h0; h < h1; ++h) {
        if (h + 1 < h1) {                                    // (uniform)
#pragma unroll
          for (int c = 0; c < KC; ++c) {
            kfn[c] = attn_frag_global<HD>(krow + (h + 1) * HD, kv, c, lane);
            qfn[c] = attn_frag_global<HD>(qrow + (h + 1) * HD, qv, c, lane);
          }
          if (qv) stn = *reinterpret_cast<const float2*>(a.stats + (srow0 + (h + 1) * sstep) * 2);
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[c], qf[c], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) sum[r] += attn_prob(acc[r], a.scale2, ka[r], st.x, st.y);
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          kf[c] = kfn[c];
          qf[c] = qfn[c];
        }
        st = stn;
      }
      if (a.head < 0) sum = sum * a.inv_heads;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (!qv || t * 16 + 4 * g + r >= lk) sum[r] = 0.f;
    }
    if (qi < a.Lq_out) am_store4(out_row, t * 16 + 4 * g, a.ld_out, a.vec != 0, sum);
  }
}

// ------------------------------------------------------------------------------------------------------ pair map
struct PairMapArgs {
  const void* s;
  float* out;
  const int* key_tiles;
  const int* n_real;
  int N, H, ld, ld_out, head, vec;
  float inv_heads;
};

__device__ __forceinline__ f32x4 am_load4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 am_load4(const _Float16* p) {
  const f16x4 h = *reinterpret_cast<const f16x4*>(p);
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = (float)h[r];            // (exact)
  return v;
}

// tiled planes (layouts 1 and 3), N <= 272.  NT: the 16-key tiles the instance is unrolled for (maps_plan.h: 5, 9, 13 or 17 -- the buckets of
// the fp32 pair-attention kernels); a row of NT tiles is 4 NT registers per lane, three times (this head, the next head's loads in flight,
// the sum over heads).  A head's loads are all issued before the first is used, and the next head's before this head's softmax.
template <typename T, int NT>
__device__ __forceinline__ void pair_map_load_row(f32x4 (&X)[NT], const T* run, int kte, bool qv, int g, int i, int vr, int N4) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    X[t] = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const int jg = 4 * t + g;                                // this lane's 4-key group of the row
    if (t < kte && qv && 4 * jg < N4) X[t] = am_load4(run + 4 * (vr * jg + i));
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(MAPS_BLOCK) void pair_attn_map_tiled_kernel(PairMapArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char am_smem[];
  f32x4* fold = reinterpret_cast<f32x4*>(am_smem);     // [3][nt][64]
  const int N = a.N, H = a.H;
  const int nt = (N + 15) >> 4, N4 = pair_n4(N);
  const int b = blockIdx.x / nt, qb = blockIdx.x - b * nt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, i = lane & 15;
  const int vr = min(16, N - qb * 16);
  const int qi = qb * 16 + i;
  const int nreal = a.n_real ? min(max(__builtin_amdgcn_readfirstlane(a.n_real[b]), 0), N) : N;
  const int kte = a.key_tiles ? pa_kt_effective(min(__builtin_amdgcn_readfirstlane(a.key_tiles[b]), nt), nt) : nt;
  const bool qv = i < vr && qi < nreal;                      // a row this molecule stores
  const bool live = qb * 16 < nreal;                         // (uniform)
  const int nheads = a.head < 0 ? H : 1, hbase = a.head < 0 ? 0 : a.head;
  const int chunk = (nheads + 3) >> 2;
  const int hw0 = hbase + min(wave * chunk, nheads), hw1 = hbase + min((wave + 1) * chunk, nheads);
  f32x4 ACC[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) ACC[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (live) {
    const long long plane = pair_plane(N);
    const T* run = reinterpret_cast<const T*>(a.s) + ((long long)b * H + hw0) * plane + (long long)qb * 16 * N4;
    f32x4 X[NT], Xn[NT];
    if (hw0 < hw1) pair_map_load_row<T, NT>(X, run, kte, qv, g, i, vr, N4);
    for (int h = hw0; h < hw1; ++h) {
      run += plane;
      if (h + 1 < hw1) pair_map_load_row<T, NT>(Xn, run, kte, qv, g, i, vr, N4);      // (uniform) the next head's row, in flight under this one's softmax
      float m = -INFINITY;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) X[t][r] = 16 * t + 4 * g + r < N ? X[t][r] : -INFINITY;      // (the pad key slots N .. N4-1)
        m = fmaxf(fmaxf(m, fmaxf(X[t][0], X[t][1])), fmaxf(X[t][2], X[t][3]));
      }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      const float mneg = m == -INFINITY ? 0.f : -m * ATTN_LOG2E;
      float lsum = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(X[t][r], ATTN_LOG2E, mneg));
          X[t][r] = e;
          lsum += e;
        }
      }
      lsum += __shfl_xor(lsum, 16, 64);
      lsum += __shfl_xor(lsum, 32, 64);
      const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        ACC[t] += X[t] * inv;
        X[t] = Xn[t];
      }
    }
    if (wave > 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (t < nt) fold[((wave - 1) * nt + t) * 64 + lane] = ACC[t];
    }
  }
  __syncthreads();
  if (wave != 0) return;
  float* out_row = a.out + ((long long)b * N + (i < vr ? qi : 0)) * a.ld_out;
  const int nt_out = (a.ld_out + 15) >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (t < nt && t < nt_out) {
      f32x4 v = ACC[t];
      if (live) {
        v += fold[(0 * nt + t) * 64 + lane];
        v += fold[(1 * nt + t) * 64 + lane];
        v += fold[(2 * nt + t) * 64 + lane];
        if (a.head < 0) v = v * a.inv_heads;
      }
      if (!qv) v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (i < vr) am_store4(out_row, t * 16 + 4 * g, a.ld_out, a.vec != 0, v);
    }
  }
  for (int t = nt; t < nt_out; ++t)
    if (i < vr) am_store4(out_row, t * 16 + 4 * g, a.ld_out, a.vec != 0, f32x4{0.f, 0.f, 0.f, 0.f});
}

// row-major fp32 planes (layout 0), N <= 320: a wave per query row, 64 keys per step
__global__ __launch_bounds__(MAPS_BLOCK) void pair_attn_map_rows_kernel(PairMapArgs a) {
  constexpr int NC = (MAPS_PAIR_MAX_N + 63) / 64;
  const int N = a.N, H = a.H;
  const int nt = (N + 15) >> 4;
  const int b = blockIdx.x / nt, qb = blockIdx.x - b * nt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int nreal = a.n_real ? min(max(__builtin_amdgcn_readfirstlane(a.n_real[b]), 0), N) : N;
  const int h0 = a.head < 0 ? 0 : a.head, h1 = a.head < 0 ? H : a.head + 1;
  const float* sp = reinterpret_cast<const float*>(a.s);
  for (int qi = qb * 16 + wave; qi < min(qb * 16 + 16, N); qi += nw) {
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    if (qi < nreal) {                                        // (uniform)
      for (int h = h0; h < h1; ++h) {
        const float* row = sp + (((long long)b * H + h) * N + qi) * a.ld;
        float x[NC];
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int j = c * 64 + lane;
          x[c] = j < N ? row[j] : -INFINITY;
          m = fmaxf(m, x[c]);
        }
        m = wave_max(m);
        const float mneg = m == -INFINITY ? 0.f : -m * ATTN_LOG2E;
        float lsum = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          x[c] = __builtin_amdgcn_exp2f(__builtin_fmaf(x[c], ATTN_LOG2E, mneg));
          lsum += x[c];
        }
        lsum = wave_sum(lsum);
        const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += x[c] * inv;
      }
    }
    float* out_row = a.out + ((long long)b * N + qi) * a.ld_out;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int j = c * 64 + lane;
      if (j < a.ld_out) out_row[j] = j < N ? (a.head < 0 ? acc[c] * a.inv_heads : acc[c]) : 0.f;
    }
    for (int j = NC * 64 + lane; j < a.ld_out; j += 64) out_row[j] = 0.f;
  }
}

// every instance, at the row maps_plan.h gives it
static KernelRow g_maps_kernels[MAPS_KERNELS] = {
    KROW(maps_attn_key(16), attn_map_kernel<16>), KROW(maps_attn_key(32), attn_map_kernel<32>), KROW(maps_attn_key(64), attn_map_kernel<64>),
    KROW(maps_pair_key(0, 1), pair_attn_map_rows_kernel),
#define MAPS_TILED_ROWS(LAYOUT, T) \
  KROW(maps_pair_key(LAYOUT, 80), pair_attn_map_tiled_kernel<T, 5>), KROW(maps_pair_key(LAYOUT, 144), pair_attn_map_tiled_kernel<T, 9>), \
  KROW(maps_pair_key(LAYOUT, 208), pair_attn_map_tiled_kernel<T, 13>), KROW(maps_pair_key(LAYOUT, 272), pair_attn_map_tiled_kernel<T, 17>)
    MAPS_TILED_ROWS(1, float), MAPS_TILED_ROWS(3, _Float16),
#undef MAPS_TILED_ROWS
};
const KernelRow* maps_kernel_table(int* n) { *n = MAPS_KERNELS; return g_maps_kernels; }

// What the launches and mmdti_maps_plan share: validate, plan.  Pointers are tested for null and alignment only.
static int attn_map_prepare(MapsPlan& plan, const void* q_bf16, const void* k_bf16, const float* key_add, const float* stats, const float* out, int B,
                            int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int Lq_out, int ld_out, int head, const int* q_off,
                            const int* k_off, const int* k_cnt, int q_rows, const int* q_cnt) {
  (void)q_cnt;
  MMDTI_REQUIRE(q_bf16 && k_bf16 && B > 0 && heads > 0 && Lq > 0 && Lk > 0, "attn_map: bad arguments");
  MMDTI_REQUIRE(stats != nullptr, "attn_map: stats is required (the row statistics the forward of this attention saved)");
  MMDTI_REQUIRE(out != nullptr, "attn_map: null out");
  MMDTI_REQUIRE(head_dim == 16 || head_dim == 32 || head_dim == 64, "attn_map: head_dim must be 16, 32 or 64 (got %d)", head_dim);
  MMDTI_REQUIRE(Lq <= MAPS_ATTN_MAX_LEN && Lk <= MAPS_ATTN_MAX_LEN, "attn_map: at most %d queries / keys per head (got %d / %d)",
                MAPS_ATTN_MAX_LEN, Lq, Lk);
  MMDTI_REQUIRE(ldq >= heads * head_dim && ldk >= heads * head_dim && ldq % 8 == 0 && ldk % 8 == 0,
                "attn_map: row strides must cover heads*head_dim and be multiples of 8");
  MMDTI_REQUIRE(aligned16(q_bf16) && aligned16(k_bf16), "attn_map: q and k need 16-byte alignment");
  MMDTI_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0 &&
                    (reinterpret_cast<uintptr_t>(key_add) & 3) == 0, "attn_map: stats need 8-byte, out and key_add 4-byte alignment");
  MMDTI_REQUIRE(head >= -1 && head < heads, "attn_map: head must be -1 (the mean over heads) or a head below %d (got %d)", heads, head);
  MMDTI_REQUIRE(ld_out >= Lk, "attn_map: ld_out (%d) < Lk (%d)", ld_out, Lk);
  MMDTI_REQUIRE(Lq_out >= Lq, "attn_map: Lq_out (%d) < Lq (%d)", Lq_out, Lq);
  const int n = (q_off ? 1 : 0) + (k_off ? 1 : 0) + (k_cnt ? 1 : 0);
  MMDTI_REQUIRE(n == 0 || n == 3, "attn_map: q_off, k_off and k_cnt come together (packed sequences) or not at all");
  MMDTI_REQUIRE(n == 0 ? q_rows == 0 : (q_rows > 0 && !key_add),
                "attn_map: packed sequences need q_rows > 0 and take no key_add; dense sequences take q_rows = 0");
  MMDTI_REQUIRE((long long)B * ((Lq_out + 15) / 16) <= 2147483647LL, "attn_map: grid too large");
  plan = attn_map_plan(B, Lq_out, ld_out, head_dim);
  return MMDTI_OK;
}

static int pair_map_prepare(MapsPlan& plan, const void* s, const float* out, int B, int N, int H, int ld, int ld_out, int head, int layout,
                            const int* key_tiles, const int* n_real) {
  MMDTI_REQUIRE(s && B > 0 && N > 0 && H > 0, "pair_attn_map: bad arguments");
  MMDTI_REQUIRE(out != nullptr, "pair_attn_map: null out");
  MMDTI_REQUIRE(layout == 0 || layout == 1 || layout == 3, "pair_attn_map: layout must be 0 (row-major fp32), 1 (tiled fp32) or 3 (compact fp16), got %d",
                layout);
  MMDTI_REQUIRE(N <= MAPS_PAIR_MAX_N, "pair_attn_map: N=%d exceeds the supported %d atoms (+BOS/EOS)", N, MAPS_PAIR_MAX_N);
  MMDTI_REQUIRE(layout == 0 || N <= MAPS_PAIR_MAX_TILED, "pair_attn_map: the tiled layouts hold N <= %d (got %d)", MAPS_PAIR_MAX_TILED, N);
  MMDTI_REQUIRE(layout != 0 || ld >= N, "pair_attn_map: ld (%d) < N (%d)", ld, N);
  MMDTI_REQUIRE(layout == 0 ? (reinterpret_cast<uintptr_t>(s) & 3) == 0 : aligned16(s),
                "pair_attn_map: s needs 4-byte (row-major) or 16-byte (tiled) alignment");
  MMDTI_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "pair_attn_map: out needs 4-byte alignment");
  MMDTI_REQUIRE(head >= -1 && head < H, "pair_attn_map: head must be -1 (the mean over heads) or a head below %d (got %d)", H, head);
  MMDTI_REQUIRE(ld_out >= N, "pair_attn_map: ld_out (%d) < N (%d)", ld_out, N);
  MMDTI_REQUIRE(!key_tiles || layout == 3, "pair_attn_map: key_tiles (ragged batches) exist for layout 3 only");
  MMDTI_REQUIRE(!key_tiles || n_real, "pair_attn_map: key_tiles needs n_real (the query rows a ragged molecule stores)");
  MMDTI_REQUIRE((long long)B * ((N + 15) / 16) <= 2147483647LL, "pair_attn_map: grid too large");
  plan = pair_attn_map_plan(B, N, layout);
  return MMDTI_OK;
}

static inline bool maps_vec_ok(const float* out, int ld_out) { return ld_out % 4 == 0 && aligned16(out); }

}  // namespace mmdti
using namespace mmdti;

extern "C" int mmdti_attn_map(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const float* key_add, const float* stats,
                              float* out, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int Lq_out, int ld_out,
                              float scale, int head, const int* q_off, const int* k_off, const int* k_cnt, int q_rows, const int* q_cnt) {
  MapsPlan plan;
  if (int e = attn_map_prepare(plan, q_bf16, k_bf16, key_add, stats, out, B, heads, Lq, Lk, head_dim, ldq, ldk, Lq_out, ld_out, head, q_off, k_off,
                               k_cnt, q_rows, q_cnt))
    return e;
  AttnMapArgs a = {};
  a.q = reinterpret_cast<const bf16_t*>(q_bf16); a.k = reinterpret_cast<const bf16_t*>(k_bf16);
  a.key_add = key_add; a.stats = stats; a.out = out;
  a.q_off = q_off; a.k_off = k_off; a.k_cnt = k_cnt; a.q_cnt = q_cnt;
  a.heads = heads; a.Lq = Lq; a.Lk = Lk; a.ldq = ldq; a.ldk = ldk; a.Lq_out = Lq_out; a.ld_out = ld_out; a.q_rows = q_rows; a.head = head;
  a.vec = maps_vec_ok(out, ld_out) ? 1 : 0;
  a.scale2 = scale * ATTN_LOG2E;
  a.inv_heads = 1.0f / (float)heads;
  void* args[] = {&a};
  (void)hipLaunchKernel(g_maps_kernels[plan.key].fn, dim3(plan.grid), dim3(plan.block), args, (size_t)plan.lds, (hipStream_t)stream);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_pair_attn_map(mmdti_stream_t stream, const void* s, float* out, int B, int N, int H, int ld, int ld_out, int head,
                                   int layout, const int* key_tiles, const int* n_real) {
  MapsPlan plan;
  if (int e = pair_map_prepare(plan, s, out, B, N, H, ld, ld_out, head, layout, key_tiles, n_real)) return e;
  PairMapArgs a = {};
  a.s = s; a.out = out; a.key_tiles = key_tiles; a.n_real = n_real;
  a.N = N; a.H = H; a.ld = ld; a.ld_out = ld_out; a.head = head;
  a.vec = maps_vec_ok(out, ld_out) ? 1 : 0;
  a.inv_heads = 1.0f / (float)H;
  void* args[] = {&a};
  (void)hipLaunchKernel(g_maps_kernels[plan.key].fn, dim3(plan.grid), dim3(plan.block), args, (size_t)plan.lds, (hipStream_t)stream);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_maps_plan(int pair, const void* q_or_s, const void* k_bf16, const float* key_add, const float* stats, const float* out,
                               int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int Lq_out, int ld_out, int head,
                               const int* q_off, const int* k_off, const int* k_cnt, int q_rows, const int* q_cnt, int layout,
                               const int* key_tiles, const int* n_real, int* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr, "maps_plan: null plan_out");
  MapsPlan plan;
  if (pair) {
    if (int e = pair_map_prepare(plan, q_or_s, out, B, Lq, heads, ldq, ld_out, head, layout, key_tiles, n_real)) return e;
  } else {
    if (int e = attn_map_prepare(plan, q_or_s, k_bf16, key_add, stats, out, B, heads, Lq, Lk, head_dim, ldq, ldk, Lq_out, ld_out, head, q_off,
                                 k_off, k_cnt, q_rows, q_cnt))
      return e;
  }
  static_assert(MAPS_PLAN_INTS == 6, "mmdti_hip.h documents 6 ints");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}
