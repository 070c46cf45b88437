// Fused BERT-style multi-head attention for gfx950 (head_dim 16, 32 or 64; mmdti_attn_*: up to 256 queries x 256 keys per head,
// mmdti_attn_long_*: up to 512 x 512 -- the same kernels with 24- / 32-tile score rows and 512-row LDS images, see attn_nt).
//
// Replaces, for the ChemBERTa tower (HF eager_attention_forward, modeling_roberta.py:158-183, called through
// mm_model.py:562) and the cross-modal layers (BertCoAttention, mm_module.py:470-514), the chain
//   scores GEMM -> row softmax (+ key mask, + dropout) -> context GEMM                     (forward)
//   dP GEMM, dV GEMM, softmax backward, dQ GEMM, dK GEMM                                   (backward)
// which moves the [B, heads, Lq, Lk] score tensor through HBM eight times per layer.  Here the scores never leave
// registers: one workgroup (8 waves) owns one (molecule, head), keeps that head's K and V (or Q and dO) rows in LDS, and
// each wave walks 16-row tiles.
//
// Layout trick shared by all three kernels: the score tile is produced with the CONTRACTED index of the next product on
// the accumulator's register/row axis, so that two consecutive 16x16 accumulator tiles ARE one 16x16x32 bf16 MFMA
// operand (k-slot 8g+j <-> tile row 4g+j of the first / second tile).  The other operand of that product is read from
// the row-major LDS image with ds_read_b64_tr_b16, which hands each lane the matching four rows of one column.  No
// shuffles, no LDS round trip between the two matrix products.
//   forward / dQ kernel : S^T[key][query] = K.Q^T   (lane = query, 4 consecutive keys per register quad)
//   dK/dV kernel        : S[query][key]   = Q.K^T   (lane = key,   4 consecutive queries per register quad)
//
// Numerics (same rounding points as the unfused path and the oracle's bf16 mode): bf16 operands, fp32 accumulate,
// fp32 scale/mask/softmax over the WHOLE row (two passes in registers -- not an online softmax), probabilities and dS
// rounded to bf16 only as MFMA operands.  The backward recomputes the probabilities from the saved row statistics
// (max, 1/sum) in fp32, and the row term sum_j dP'_ij p_ij exactly in registers (no O.dO shortcut).
// Dropout: per-element hash of (seed, site, head, query, key) -- the same function in all three kernels.
#include "common.h"
#include "attn_plan.h"
#include "attn_shared.h"   // the pieces attn_maps.hip shares: typedefs, ATTN_LOG2E, attn_mask2, attn_frag_global, attn_prob

namespace mmdti {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// row stride (elements) of the LDS images: head_dim + 8 -> 144-B / 80-B rows.  (head_dim + 16 is conflict-free for both the
// row-major ds_read_b128 fragments and the ds_read_b64_tr_b16 fragments, this one is 2-way -- but it brings the 256-key image
// pair of a head under 80 KB, so TWO workgroups share a CU: forward 149 -> 109 us, dK/dV 220 -> 175 us.)
template <int HD>
struct AttnShape {
  static constexpr int STR = HD + 8;
  static constexpr int KC = HD < 32 ? 1 : HD / 32;  // 32-wide k chunks of a head_dim contraction (head_dim 16: one chunk, upper half zero)
  static constexpr int NB = HD / 16;  // 16-wide head_dim blocks of an output
};

// Dropout of the probabilities: the shared generator of common.h (Rng24: a key per (sequence, head) plane, one word per four
// consecutive keys of a query, a threshold per query row) -- the same function in all three kernels.
typedef Rng24 AttnRng;
__device__ __forceinline__ AttnRng attn_rng_key(uint64_t seed, uint32_t site, uint32_t bh) { return rng24_key(seed, site, bh); }
__device__ __forceinline__ uint32_t attn_hash24(const AttnRng& k, uint32_t ctr) { return rng24_word(k, ctr); }
__device__ __forceinline__ uint32_t attn_row_t8(const AttnRng& k, uint32_t row, uint32_t thresh) { return rng24_row_t8(k, row, thresh); }
// bit r of the result: element r of the quad is kept
__device__ __forceinline__ uint32_t attn_keep4(const AttnRng& k, uint32_t quad, uint32_t t8) {
  const uint32_t h = rng24_word(k, quad);
  return ((h & 0xffu) >= t8 ? 1u : 0u) | (((h >> 8) & 0xffu) >= t8 ? 2u : 0u) | (((h >> 16) & 0xffu) >= t8 ? 4u : 0u) | ((h >> 24) >= t8 ? 8u : 0u);
}
// Variable-length (packed) sequences.  q_off / k_off: [B+1] int32 row offsets of every sequence in the query-side / key-side row
// arrays (sequence b owns rows [off[b], off[b+1]) -- its real tokens, then at most one representative pad row); k_cnt: [B]
// int32, the REAL keys of sequence b (the representative pad row of the key side is no key: the reference masks padded keys,
// additively, to a probability of exactly 0).  Every row of the query side is a query.  Null pointers: the dense layout
// (sequence b = rows [b*L, (b+1)*L), masked keys through key_add).  q_rows: total rows of the query side (stats / drow are
// then [heads, q_rows] instead of [B, heads, Lq]).
struct AttnVarlen {
  const int* q_off;
  const int* k_off;
  const int* k_cnt;
  int q_rows;
};
struct AttnSeq {
  int q0, lq, k0, lk, krows;
};
__device__ __forceinline__ AttnSeq attn_seq(const AttnVarlen& vl, int b, int Lq, int Lk) {
  AttnSeq s;
  if (vl.q_off) {
    s.q0 = __builtin_amdgcn_readfirstlane(vl.q_off[b]);
    s.lq = __builtin_amdgcn_readfirstlane(vl.q_off[b + 1]) - s.q0;
    s.k0 = __builtin_amdgcn_readfirstlane(vl.k_off[b]);
    s.krows = __builtin_amdgcn_readfirstlane(vl.k_off[b + 1]) - s.k0;
    s.lk = __builtin_amdgcn_readfirstlane(vl.k_cnt[b]);
  } else {
    s.q0 = b * Lq; s.lq = Lq; s.k0 = b * Lk; s.lk = Lk; s.krows = Lk;
  }
  return s;
}
// index of query row qi of (sequence b, head h) in stats / drow
__device__ __forceinline__ long long attn_stat_row(const AttnVarlen& vl, const AttnSeq& sq, int bh, int h, int Lq, int qi) {
  return vl.q_off ? (long long)h * vl.q_rows + sq.q0 + qi : (long long)bh * Lq + qi;
}

template <int HD>
__device__ __forceinline__ void attn_fill_rows(bf16_t* lds, const bf16_t* g, int L, int rows, int ld, int tid, int nthreads) {
  constexpr int CPR = HD / 8, STR = AttnShape<HD>::STR;
  for (int c = tid; c < rows * CPR; c += nthreads) {
    const int row = c / CPR, col = (c % CPR) * 8;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row < L) v = *reinterpret_cast<const uint4*>(g + (long long)row * ld + col);
    *reinterpret_cast<uint4*>(lds + row * STR + col) = v;
  }
}
// rows row0..row0+15 as an MFMA operand (lane = row, 8 consecutive k): one ds_read_b128
template <int HD>
__device__ __forceinline__ bf16x8 attn_frag_rm(const bf16_t* lds, int row0, int c, int lane) {
  if (HD < 32 && 8 * (lane >> 4) >= HD) return bf16x8{0, 0, 0, 0, 0, 0, 0, 0};   // k-slots past a 16-wide head: zeros
  return *reinterpret_cast<const bf16x8*>(lds + (row0 + (lane & 15)) * AttnShape<HD>::STR + 32 * c + 8 * (lane >> 4));
}
// columns n0..n0+15 as an MFMA operand (lane = column) whose k-slots 8g+j are rows r0+4g+j (j<4) and r1+4g+(j-4)
template <int HD>
__device__ __forceinline__ bf16x8 attn_frag_tr(const bf16_t* lds, int r0, int r1, int n0, int lane) {
  constexpr int STR = AttnShape<HD>::STR;
  const int off = (4 * (lane >> 4) + ((lane & 15) >> 2)) * STR + n0 + 4 * (lane & 3);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + r0 * STR + off));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds + r1 * STR + off));
  const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ bf16x8 attn_pack(const f32x4& a, const f32x4& b) {
  bf16x8 r;
  r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3];
  r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
  return r;
}
__device__ __forceinline__ void attn_store4(bf16_t* dst, const f32x4& a) {
  uint2 pk;
  pk.x = (uint32_t)f2bf(a[0]) | ((uint32_t)f2bf(a[1]) << 16);
  pk.y = (uint32_t)f2bf(a[2]) | ((uint32_t)f2bf(a[3]) << 16);
  *reinterpret_cast<uint2*>(dst) = pk;
}
#define ATTN_MFMA(A, B, C) __builtin_amdgcn_mfma_f32_16x16x32_bf16(A, B, C, 0, 0, 0)
// Images of more than 256 rows (NT > 16) pass the 64 KiB that a ds_read's immediate offset reaches.  Left alone, the compiler gives
// every fragment address past it a register of its own, hoists them all out of the query-tile loop and spills them to scratch.  So
// the second image, and the rows from 256 on of each, are addressed from bases whose distance the compiler does not see (an empty
// asm on the row count): one more address register per fragment pattern, immediates for the rest.  NT <= 16: nothing changes.
template <int NT>
__device__ __forceinline__ int attn_far_rows(int r) {
  if constexpr (NT > 16) asm volatile("" : "+s"(r));
  return r;
}
#define ATTN_IMG(lo, hi, t) ((t) < 16 ? (lo) : (hi))

// ------------------------------------------------------------------------------------------------------ forward
// (NT > 16, the long entry points: a row of 24 / 32 score tiles is 96 / 128 registers per lane and the 384- / 512-key image pair
//  fills most of a CU's LDS, so one workgroup owns the CU: 2 waves per SIMD, a 256-register ceiling)
//  -- except head_dim 16 with 32 tiles, which the compiler cannot hold in 256: that one instantiation runs 4 waves per workgroup,
//  one per SIMD, and keeps its overflow in the accumulation registers instead of scratch)
template <int HD, int NT>
constexpr int attn_fwd_min_waves() {      // per SIMD: what the register budget is sized for
  if (NT <= 16) return HD == 16 ? 2 : 4;
  return HD == 16 && NT == 32 ? 1 : 2;
}
template <int HD, int NT>
__global__ __launch_bounds__((attn_fwd_threads(HD, NT)), (attn_fwd_min_waves<HD, NT>())) void attn_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                       const bf16_t* __restrict__ v, const float* __restrict__ key_add,
                                                       bf16_t* __restrict__ ctx, float* __restrict__ stats, int heads, int Lq,
                                                       int Lk, int ldq, int ldk, int ldo, float scale, uint32_t thresh16,
                                                       float dscale, uint64_t seed, uint32_t site, AttnVarlen vl, int ctx_f16) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int STR = AttnShape<HD>::STR, KC = AttnShape<HD>::KC, NB = AttnShape<HD>::NB, NP = NT * 16;
  bf16_t* sK = reinterpret_cast<bf16_t*>(attn_smem);
  bf16_t* sV = sK + attn_far_rows<NT>(NP) * STR;
  float* sKA = reinterpret_cast<float*>(sV + NP * STR);
  const int hi = attn_far_rows<NT>(256);
  const bf16_t* sKh = sK + hi * STR;
  const bf16_t* sVh = sV + hi * STR;
  const float* sKAh = sKA + hi;
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const AttnSeq sq = attn_seq(vl, b, Lq, Lk);
  attn_fill_rows<HD>(sK, k + (long long)sq.k0 * ldk + h * HD, sq.lk, NP, ldk, tid, blockDim.x);
  attn_fill_rows<HD>(sV, v + (long long)sq.k0 * ldk + h * HD, sq.lk, NP, ldk, tid, blockDim.x);
  for (int t = tid; t < NP; t += blockDim.x) sKA[t] = t < sq.lk ? (key_add ? attn_mask2(key_add[(long long)b * Lk + t]) : 0.f) : -INFINITY;
  __syncthreads();
  const AttnRng rkey = attn_rng_key(seed, site, (uint32_t)bh);
  const float scale2 = scale * ATTN_LOG2E;
  const int g = lane >> 4, i = lane & 15;
  const int nqt = (sq.lq + 15) >> 4;
  for (int qt = wave; qt < nqt; qt += nw) {
    const int qi = qt * 16 + i;
    const bool qv = qi < sq.lq;
    const bf16_t* qrow = q + ((long long)sq.q0 + (qv ? qi : 0)) * ldq + h * HD;
    bf16x8 qf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) qf[c] = attn_frag_global<HD>(qrow, qv, c, lane);
    f32x4 S[NT];
    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < KC; ++c) acc = ATTN_MFMA(attn_frag_rm<HD>(ATTN_IMG(sK, sKh, t), (t & 15) * 16, c, lane), qf[c], acc);
      const f32x4 ka = *reinterpret_cast<const f32x4*>(&ATTN_IMG(sKA, sKAh, t)[(t & 15) * 16 + 4 * g]);
      acc = acc * scale2 + ka;     // (vector form: two v_pk_fma_f32)
      m = fmaxf(fmaxf(m, fmaxf(acc[0], acc[1])), fmaxf(acc[2], acc[3]));
      S[t] = acc;
      __builtin_amdgcn_sched_barrier(0);  // keep the unrolled tiles in order: hoisted LDS fragments would spill
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    f32x4 ls4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const f32x4 d = S[t] - m;    // (two v_pk_add_f32)
      f32x4 e;
#pragma unroll
      for (int r = 0; r < 4; ++r) e[r] = __builtin_amdgcn_exp2f(d[r]);
      S[t] = e;
      ls4 += e;
    }
    float lsum = (ls4[0] + ls4[1]) + (ls4[2] + ls4[3]);
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const float inv = 1.0f / lsum;
    if (g == 0 && qv) *reinterpret_cast<float2*>(stats + attn_stat_row(vl, sq, bh, h, Lq, qi) * 2) = make_float2(m, inv);
    f32x4 o[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) o[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    // (the NORMALISED probabilities are what is rounded to bf16 for the MFMA -- the rounding site of the oracle's contract.  Folding
    //  1 / sum into the 16 outputs of a lane instead saves 24 packed multiplies per query block, changes nothing in time -- the
    //  kernel is latency-bound -- and moved the regression contrastive loss from 1.0e-3 to 1.3e-3 of the oracle's: not taken)
    const float invd = thresh16 ? inv * dscale : inv;
    const uint32_t t8 = thresh16 ? attn_row_t8(rkey, (uint32_t)qi, thresh16) : 0u;
#pragma unroll
    for (int u = 0; u < NT / 2; ++u) {
      f32x4 p0 = S[2 * u] * invd, p1 = S[2 * u + 1] * invd;
      if (thresh16) {
        const uint32_t q4 = (uint32_t)qi * (NP / 4) + (2 * u) * 4 + g;
        const uint32_t h0 = attn_hash24(rkey, q4), h1 = attn_hash24(rkey, q4 + 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p0[r] = ((h0 >> (8 * r)) & 0xffu) >= t8 ? p0[r] : 0.f;
          p1[r] = ((h1 >> (8 * r)) & 0xffu) >= t8 ? p1[r] : 0.f;
        }
      }
      const bf16x8 pf = attn_pack(p0, p1);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
        o[nb] = ATTN_MFMA(attn_frag_tr<HD>(ATTN_IMG(sV, sVh, 2 * u), 32 * (u & 7), 32 * (u & 7) + 16, nb * 16, lane), pf, o[nb]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (qv) {
      bf16_t* dst = ctx + ((long long)sq.q0 + qi) * ldo + h * HD + 4 * g;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (ctx_f16) {   // the context feeds the output projection's forward GEMM: fp16 in the fp16 forward-operand mode
          uint2 pk;
          pk.x = f2h_sat2(o[nb][0], o[nb][1]);
          pk.y = f2h_sat2(o[nb][2], o[nb][3]);
          *reinterpret_cast<uint2*>(dst + nb * 16) = pk;
        } else {
          attn_store4(dst + nb * 16, o[nb]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------ backward: dQ
template <int HD, int NT>
__global__ __launch_bounds__(NT > 16 ? 1024 : 512) void attn_bwd_q_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                         const bf16_t* __restrict__ v, const float* __restrict__ key_add,
                                                         const bf16_t* __restrict__ dout, const float* __restrict__ stats,
                                                         bf16_t* __restrict__ dq, float* __restrict__ drow, int heads, int Lq,
                                                         int Lk, int ldq, int ldk, int ldo, int lddq, float scale,
                                                         uint32_t thresh16, float dscale, uint64_t seed, uint32_t site, AttnVarlen vl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int STR = AttnShape<HD>::STR, KC = AttnShape<HD>::KC, NB = AttnShape<HD>::NB, NP = NT * 16;
  bf16_t* sK = reinterpret_cast<bf16_t*>(attn_smem);
  bf16_t* sV = sK + NP * STR;
  float* sKA = reinterpret_cast<float*>(sV + NP * STR);
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const AttnSeq sq = attn_seq(vl, b, Lq, Lk);
  attn_fill_rows<HD>(sK, k + (long long)sq.k0 * ldk + h * HD, sq.lk, NP, ldk, tid, blockDim.x);
  attn_fill_rows<HD>(sV, v + (long long)sq.k0 * ldk + h * HD, sq.lk, NP, ldk, tid, blockDim.x);
  for (int t = tid; t < NP; t += blockDim.x) sKA[t] = t < sq.lk ? (key_add ? attn_mask2(key_add[(long long)b * Lk + t]) : 0.f) : -INFINITY;
  __syncthreads();
  const AttnRng rkey = attn_rng_key(seed, site, (uint32_t)bh);
  const float scale2 = scale * ATTN_LOG2E;
  const int g = lane >> 4, i = lane & 15;
  const int nqt = (sq.lq + 15) >> 4;
  for (int qt = wave; qt < nqt; qt += nw) {
    const int qi = qt * 16 + i;
    const bool qv = qi < sq.lq;
    const bf16_t* qrow = q + ((long long)sq.q0 + (qv ? qi : 0)) * ldq + h * HD;
    const bf16_t* orow = dout + ((long long)sq.q0 + (qv ? qi : 0)) * ldo + h * HD;
    bf16x8 qf[KC], dof[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      qf[c] = attn_frag_global<HD>(qrow, qv, c, lane);
      dof[c] = attn_frag_global<HD>(orow, qv, c, lane);
    }
    float2 st = make_float2(0.f, 0.f);
    if (qv) st = *reinterpret_cast<const float2*>(stats + attn_stat_row(vl, sq, bh, h, Lq, qi) * 2);
    const uint32_t t8 = thresh16 ? attn_row_t8(rkey, (uint32_t)qi, thresh16) : 0u;
    f32x4 da[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) da[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (NT <= 16) {
      // sweep 1: probabilities (kept in registers, sign bit = "dropped") and the row term D = sum_j dP'_ij p_ij
      f32x4 P[NT];
      float dsum = 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          acc = ATTN_MFMA(attn_frag_rm<HD>(sK, t * 16, c, lane), qf[c], acc);
          dacc = ATTN_MFMA(attn_frag_rm<HD>(sV, t * 16, c, lane), dof[c], dacc);
        }
        const f32x4 ka = *reinterpret_cast<const f32x4*>(&sKA[t * 16 + 4 * g]);
        // (the quad's four uniform bytes are compared where they are used -- one byte compare + select per element, as in the forward;
        //  building a 4-bit mask first and testing its bits cost three more instructions per element and spilled compare results.
        //  Without dropout t8 == 0: every byte keeps.)
        const uint32_t hw = thresh16 ? attn_hash24(rkey, (uint32_t)qi * (NP / 4) + t * 4 + g) : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = attn_prob(acc[r], scale2, ka[r], st.x, st.y);
          const bool keep = ((hw >> (8 * r)) & 0xffu) >= t8;
          dsum += keep ? dacc[r] * p : 0.f;
          acc[r] = keep ? p : -p;
        }
        P[t] = acc;
        __builtin_amdgcn_sched_barrier(0);
      }
      dsum *= dscale;
      dsum += __shfl_xor(dsum, 16, 64);
      dsum += __shfl_xor(dsum, 32, 64);
      if (g == 0 && qv) drow[attn_stat_row(vl, sq, bh, h, Lq, qi)] = dsum;
      // sweep 2: dP again (two MFMAs per tile are cheaper than 64 more live registers), dS, dQ^T += K^T.dS^T
#pragma unroll
      for (int u = 0; u < NT / 2; ++u) {
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          s0 = ATTN_MFMA(attn_frag_rm<HD>(sV, 32 * u, c, lane), dof[c], s0);
          s1 = ATTN_MFMA(attn_frag_rm<HD>(sV, 32 * u + 16, c, lane), dof[c], s1);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p0 = P[2 * u][r], p1 = P[2 * u + 1][r];
          s0[r] = fabsf(p0) * ((__float_as_uint(p0) >> 31 ? 0.f : s0[r] * dscale) - dsum) * scale;
          s1[r] = fabsf(p1) * ((__float_as_uint(p1) >> 31 ? 0.f : s1[r] * dscale) - dsum) * scale;
        }
        const bf16x8 sf = attn_pack(s0, s1);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) da[nb] = ATTN_MFMA(attn_frag_tr<HD>(sK, 32 * u, 32 * u + 16, nb * 16, lane), sf, da[nb]);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      // NT > 16 (mmdti_attn_long_bwd): a row of 24 / 32 probability tiles next to the rest of this kernel does not fit 256 registers, so
      // nothing is kept: sweep 2 computes K.Q^T and the probabilities again -- the same expressions on the same operands in the same
      // order, hence the same values as above.  Both sweeps are real loops (dynamic LDS addresses; unrolled, the compiler would
      // merge the two sweeps' products and keep them all live).
      float dsum = 0.f;
#pragma unroll 1
      for (int t = 0; t < NT; ++t) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          acc = ATTN_MFMA(attn_frag_rm<HD>(sK, t * 16, c, lane), qf[c], acc);
          dacc = ATTN_MFMA(attn_frag_rm<HD>(sV, t * 16, c, lane), dof[c], dacc);
        }
        const f32x4 ka = *reinterpret_cast<const f32x4*>(&sKA[t * 16 + 4 * g]);
        const uint32_t hw = thresh16 ? attn_hash24(rkey, (uint32_t)qi * (NP / 4) + t * 4 + g) : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = attn_prob(acc[r], scale2, ka[r], st.x, st.y);
          const bool keep = ((hw >> (8 * r)) & 0xffu) >= t8;
          dsum += keep ? dacc[r] * p : 0.f;
        }
      }
      dsum *= dscale;
      dsum += __shfl_xor(dsum, 16, 64);
      dsum += __shfl_xor(dsum, 32, 64);
      if (g == 0 && qv) drow[attn_stat_row(vl, sq, bh, h, Lq, qi)] = dsum;
#pragma unroll 1
      for (int u = 0; u < NT / 2; ++u) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          a0 = ATTN_MFMA(attn_frag_rm<HD>(sK, 32 * u, c, lane), qf[c], a0);
          a1 = ATTN_MFMA(attn_frag_rm<HD>(sK, 32 * u + 16, c, lane), qf[c], a1);
          s0 = ATTN_MFMA(attn_frag_rm<HD>(sV, 32 * u, c, lane), dof[c], s0);
          s1 = ATTN_MFMA(attn_frag_rm<HD>(sV, 32 * u + 16, c, lane), dof[c], s1);
        }
        const f32x4 ka0 = *reinterpret_cast<const f32x4*>(&sKA[32 * u + 4 * g]);
        const f32x4 ka1 = *reinterpret_cast<const f32x4*>(&sKA[32 * u + 16 + 4 * g]);
        const uint32_t q4 = (uint32_t)qi * (NP / 4) + (2 * u) * 4 + g;
        const uint32_t h0 = thresh16 ? attn_hash24(rkey, q4) : 0u, h1 = thresh16 ? attn_hash24(rkey, q4 + 4) : 0u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p0 = attn_prob(a0[r], scale2, ka0[r], st.x, st.y);
          const float p1 = attn_prob(a1[r], scale2, ka1[r], st.x, st.y);
          s0[r] = p0 * ((((h0 >> (8 * r)) & 0xffu) >= t8 ? s0[r] * dscale : 0.f) - dsum) * scale;
          s1[r] = p1 * ((((h1 >> (8 * r)) & 0xffu) >= t8 ? s1[r] * dscale : 0.f) - dsum) * scale;
        }
        const bf16x8 sf = attn_pack(s0, s1);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) da[nb] = ATTN_MFMA(attn_frag_tr<HD>(sK, 32 * u, 32 * u + 16, nb * 16, lane), sf, da[nb]);
      }
    }
    if (qv) {
      bf16_t* dst = dq + ((long long)sq.q0 + qi) * lddq + h * HD + 4 * g;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) attn_store4(dst + nb * 16, da[nb]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------ backward: dK, dV
template <int HD>
__global__ __launch_bounds__(512, 4) void attn_bwd_kv_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                          const bf16_t* __restrict__ v, const float* __restrict__ key_add,
                                                          const bf16_t* __restrict__ dout, const float* __restrict__ stats,
                                                          const float* __restrict__ drow, bf16_t* __restrict__ dk,
                                                          bf16_t* __restrict__ dv, int heads, int Lq, int Lk, int ldq, int ldk,
                                                          int ldo, int lddk, float scale, uint32_t thresh16, float dscale,
                                                          uint64_t seed, uint32_t site, int key_stride, AttnVarlen vl) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int STR = AttnShape<HD>::STR, KC = AttnShape<HD>::KC, NB = AttnShape<HD>::NB;
  const int LQP_MAX = ((Lq + 31) >> 5) << 5;       // (the images are sized for the longest sequence of the launch)
  bf16_t* sQ = reinterpret_cast<bf16_t*>(attn_smem);
  bf16_t* sO = sQ + LQP_MAX * STR;
  float* sM = reinterpret_cast<float*>(sO + LQP_MAX * STR);
  float* sI = sM + LQP_MAX;
  float* sD = sI + LQP_MAX;
  uint32_t* sT = reinterpret_cast<uint32_t*>(sD + LQP_MAX);    // dropout threshold of every query row (see attn_row_t8)
  const int bh = blockIdx.x, b = bh / heads, h = bh - b * heads;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const AttnSeq sq = attn_seq(vl, b, Lq, Lk);
  const AttnRng rkey = attn_rng_key(seed, site, (uint32_t)bh);
  const int LQP = ((sq.lq + 31) >> 5) << 5;        // this sequence's queries, in 32-row steps
  attn_fill_rows<HD>(sQ, q + (long long)sq.q0 * ldq + h * HD, sq.lq, LQP, ldq, tid, blockDim.x);
  attn_fill_rows<HD>(sO, dout + (long long)sq.q0 * ldo + h * HD, sq.lq, LQP, ldo, tid, blockDim.x);
  for (int t = tid; t < LQP; t += blockDim.x) {
    float2 st = make_float2(0.f, 0.f);
    float d = 0.f;
    if (t < sq.lq) {
      st = *reinterpret_cast<const float2*>(stats + attn_stat_row(vl, sq, bh, h, Lq, t) * 2);
      d = drow[attn_stat_row(vl, sq, bh, h, Lq, t)];
    }
    sM[t] = st.x;
    sI[t] = st.y;
    sD[t] = d;
    sT[t] = thresh16 ? attn_row_t8(rkey, (uint32_t)t, thresh16) : 0u;
  }
  __syncthreads();
  const int g = lane >> 4, i = lane & 15;
  // (packed rows: the representative pad row of the key side is visited too -- as a masked key, so that its dk / dv rows are
  //  WRITTEN, as zeros)
  const int nkt = (sq.krows + 15) >> 4;
  for (int kt = wave; kt < nkt; kt += nw) {
    const int key = kt * 16 + i;
    const bool kv = key < sq.lk, kstore = key < sq.krows;
    const bf16_t* krow = k + ((long long)sq.k0 + (kv ? key : 0)) * ldk + h * HD;
    const bf16_t* vrow = v + ((long long)sq.k0 + (kv ? key : 0)) * ldk + h * HD;
    bf16x8 kf[KC], vf[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      kf[c] = attn_frag_global<HD>(krow, kv, c, lane);
      vf[c] = attn_frag_global<HD>(vrow, kv, c, lane);
    }
    const float ka = kv ? (key_add ? attn_mask2(key_add[(long long)b * Lk + key]) : 0.f) : -INFINITY;
    const float scale2 = scale * ATTN_LOG2E;
    const uint32_t kquad = (uint32_t)(key >> 2), kbit = (uint32_t)(i & 3), qstride4 = (uint32_t)key_stride >> 2;
    f32x4 dka[NB], dva[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      dka[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dva[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int up = 0; up < (LQP >> 5); ++up) {
      f32x4 pd[2], ds[2];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int r0 = up * 32 + hf * 16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f}, dacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          acc = ATTN_MFMA(attn_frag_rm<HD>(sQ, r0, c, lane), kf[c], acc);
          dacc = ATTN_MFMA(attn_frag_rm<HD>(sO, r0, c, lane), vf[c], dacc);
        }
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(&sM[r0 + 4 * g]);
        const f32x4 i4 = *reinterpret_cast<const f32x4*>(&sI[r0 + 4 * g]);
        const f32x4 d4 = *reinterpret_cast<const f32x4*>(&sD[r0 + 4 * g]);
        // keep masks: the four lanes of a key quad need the masks of the same four (query, key-quad) pairs -- lane i & 3 = r
        // computes the one of query r0 + 4g + r, and the four are exchanged inside the lane quad (DPP quad_perm broadcasts)
        uint32_t kb = 15u;                             // bit r: element (query r0 + 4g + r, this lane's key) kept
        if (thresh16) {
          const int qown = r0 + 4 * g + (int)kbit;
          const int own = (int)attn_keep4(rkey, (uint32_t)qown * qstride4 + kquad, sT[qown]);
          kb = (((uint32_t)__builtin_amdgcn_update_dpp(0, own, 0x00, 0xf, 0xf, false) >> kbit) & 1u) |
               ((((uint32_t)__builtin_amdgcn_update_dpp(0, own, 0x55, 0xf, 0xf, false) >> kbit) & 1u) << 1) |
               ((((uint32_t)__builtin_amdgcn_update_dpp(0, own, 0xAA, 0xf, 0xf, false) >> kbit) & 1u) << 2) |
               ((((uint32_t)__builtin_amdgcn_update_dpp(0, own, 0xFF, 0xf, 0xf, false) >> kbit) & 1u) << 3);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = attn_prob(acc[r], scale2, ka, m4[r], i4[r]);
          const bool keep = (kb >> r) & 1u;
          const float w = keep ? dacc[r] * dscale : 0.f;     // (dscale = 1 without dropout)
          pd[hf][r] = keep ? p * dscale : 0.f;
          ds[hf][r] = p * (w - d4[r]) * scale;
        }
      }
      const bf16x8 pf = attn_pack(pd[0], pd[1]), sf = attn_pack(ds[0], ds[1]);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        dva[nb] = ATTN_MFMA(attn_frag_tr<HD>(sO, up * 32, up * 32 + 16, nb * 16, lane), pf, dva[nb]);
        dka[nb] = ATTN_MFMA(attn_frag_tr<HD>(sQ, up * 32, up * 32 + 16, nb * 16, lane), sf, dka[nb]);
      }
    }
    if (kstore) {
      bf16_t* dkd = dk + ((long long)sq.k0 + key) * lddk + h * HD + 4 * g;
      bf16_t* dvd = dv + ((long long)sq.k0 + key) * lddk + h * HD + 4 * g;
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        attn_store4(dkd + nb * 16, dka[nb]);
        attn_store4(dvd + nb * 16, dva[nb]);
      }
    }
  }
}

static inline uint32_t thresh16_of(float p) { return dropout_thresh8(p); }

// every instance, at the row attn_key gives it (attn_plan.h)
static KernelRow g_attn_kernels[ATTN_KERNELS] = {
#define ATTN_ROWS(KIND, KERN, HD) \
  KROW(attn_key(KIND, HD, 10), KERN<HD, 10>), KROW(attn_key(KIND, HD, 16), KERN<HD, 16>), KROW(attn_key(KIND, HD, 24), KERN<HD, 24>), \
  KROW(attn_key(KIND, HD, 32), KERN<HD, 32>)
    ATTN_ROWS(ATTN_FWD, attn_fwd_kernel, 16),     ATTN_ROWS(ATTN_FWD, attn_fwd_kernel, 32),     ATTN_ROWS(ATTN_FWD, attn_fwd_kernel, 64),
    ATTN_ROWS(ATTN_BWD_Q, attn_bwd_q_kernel, 16), ATTN_ROWS(ATTN_BWD_Q, attn_bwd_q_kernel, 32), ATTN_ROWS(ATTN_BWD_Q, attn_bwd_q_kernel, 64),
#undef ATTN_ROWS
    KROW(attn_key(ATTN_BWD_KV, 16, 0), attn_bwd_kv_kernel<16>), KROW(attn_key(ATTN_BWD_KV, 32, 0), attn_bwd_kv_kernel<32>),
    KROW(attn_key(ATTN_BWD_KV, 64, 0), attn_bwd_kv_kernel<64>),
};
const KernelRow* attn_kernel_table(int* n) { *n = ATTN_KERNELS; return g_attn_kernels; }

// (the LDS opt-in is raised per kernel, once per size: a process that never calls the long entry points sets what it always set)
static int attn_launch(const AttnLaunch& l, void** args, mmdti_stream_t stream) {
  KernelRow& row = g_attn_kernels[l.key];
  if (int e = ensure_dynamic_lds(row.fn, (size_t)l.lds_cap, &row.lds_have, "attn")) return e;
  (void)hipLaunchKernel(row.fn, dim3(l.grid), dim3(l.block), args, (size_t)l.lds, (hipStream_t)stream);
  return MMDTI_OK;
}

static int attn_check(const char* name, int max_len, const void* q, const void* k, const void* v, int B, int heads, int Lq, int Lk, int hd,
                      int ldq, int ldk, float drop_p) {
  MMDTI_REQUIRE(q && k && v && B > 0 && heads > 0 && Lq > 0 && Lk > 0, "%s: bad arguments", name);
  MMDTI_REQUIRE(hd == 16 || hd == 32 || hd == 64, "%s: head_dim must be 16, 32 or 64 (got %d)", name, hd);
  MMDTI_REQUIRE(Lq <= max_len && Lk <= max_len, "%s: at most %d queries / keys per head (got %d / %d)", name, max_len, Lq, Lk);
  MMDTI_REQUIRE(ldq >= heads * hd && ldk >= heads * hd && ldq % 8 == 0 && ldk % 8 == 0, "%s: row strides must cover heads*head_dim and be multiples of 8", name);
  MMDTI_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v), "%s: 16-byte alignment required", name);
  MMDTI_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "%s: dropout p out of range", name);
  return MMDTI_OK;
}

static int attn_check_varlen(const char* name, const float* key_add, const int* q_off, const int* k_off, const int* k_cnt, int q_rows) {
  const int n = (q_off ? 1 : 0) + (k_off ? 1 : 0) + (k_cnt ? 1 : 0);
  MMDTI_REQUIRE(n == 0 || n == 3, "%s: q_off, k_off and k_cnt come together (packed sequences) or not at all", name);
  MMDTI_REQUIRE(n == 0 || (q_rows > 0 && !key_add), "%s: packed sequences need q_rows > 0 and take no key_add (masked keys are left out of k_cnt)", name);
  return MMDTI_OK;
}

// What the launches and mmdti_attn_plan share: validate, plan.  Pointers are tested for null and alignment only.
// One body for mmdti_attn_fwd (max_len 256) and mmdti_attn_long_fwd (512): up to 256 keys both launch the same instantiation with
// the same arguments; the 24- and 32-tile instantiations exist for the long entry point only.
static int attn_fwd_prepare(AttnPlan& plan, const char* name, int max_len, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                            const float* key_add, const void* ctx_bf16, const float* stats, int B, int heads, int Lq, int Lk, int head_dim,
                            int ldq, int ldk, int ldo, float drop_p, const int* q_off, const int* k_off, const int* k_cnt, int q_rows) {
  if (int e = attn_check(name, max_len, q_bf16, k_bf16, v_bf16, B, heads, Lq, Lk, head_dim, ldq, ldk, drop_p)) return e;
  if (int e = attn_check_varlen(name, key_add, q_off, k_off, k_cnt, q_rows)) return e;
  MMDTI_REQUIRE(ctx_bf16 && stats && ldo >= heads * head_dim && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(ctx_bf16) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(stats) & 7) == 0, "%s: bad output arguments", name);
  plan = attn_fwd_plan(B, heads, Lq, Lk, head_dim);
  return MMDTI_OK;
}

static int attn_bwd_prepare(AttnPlan& plan, const char* name, int max_len, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                            const float* key_add, const void* dctx_bf16, const float* stats, const float* drow, const void* dq_bf16,
                            const void* dk_bf16, const void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo,
                            int lddq, int lddk, float drop_p, const int* q_off, const int* k_off, const int* k_cnt, int q_rows) {
  if (int e = attn_check(name, max_len, q_bf16, k_bf16, v_bf16, B, heads, Lq, Lk, head_dim, ldq, ldk, drop_p)) return e;
  if (int e = attn_check_varlen(name, key_add, q_off, k_off, k_cnt, q_rows)) return e;
  MMDTI_REQUIRE(dctx_bf16 && stats && drow && dq_bf16 && dk_bf16 && dv_bf16, "%s: null argument", name);
  MMDTI_REQUIRE(ldo >= heads * head_dim && ldo % 8 == 0 && aligned16(dctx_bf16), "%s: dctx stride/alignment", name);
  MMDTI_REQUIRE(lddq >= heads * head_dim && lddk >= heads * head_dim && lddq % 4 == 0 && lddk % 4 == 0 &&
                    (reinterpret_cast<uintptr_t>(dq_bf16) & 7) == 0 && (reinterpret_cast<uintptr_t>(dk_bf16) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(dv_bf16) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0,
                "%s: output stride/alignment", name);
  plan = attn_bwd_plan(B, heads, Lq, Lk, head_dim);
  return MMDTI_OK;
}

static int attn_fwd_launch(const char* name, int max_len, mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                           const float* key_add, void* ctx_bf16, float* stats, int B, int heads, int Lq, int Lk, int head_dim, int ldq,
                           int ldk, int ldo, float scale, float drop_p, unsigned long long seed, unsigned int site, const int* q_off,
                           const int* k_off, const int* k_cnt, int q_rows, int ctx_f16) {
  AttnPlan plan;
  if (int e = attn_fwd_prepare(plan, name, max_len, q_bf16, k_bf16, v_bf16, key_add, ctx_bf16, stats, B, heads, Lq, Lk, head_dim, ldq, ldk, ldo,
                               drop_p, q_off, k_off, k_cnt, q_rows))
    return e;
  AttnVarlen vl = {q_off, k_off, k_cnt, q_rows};
  uint32_t th = thresh16_of(drop_p), site32 = site;
  float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  uint64_t seed64 = seed;
  void* args[] = {&q_bf16, &k_bf16, &v_bf16, &key_add, &ctx_bf16, &stats, &heads, &Lq, &Lk, &ldq, &ldk, &ldo, &scale, &th, &sc, &seed64, &site32,
                  &vl, &ctx_f16};
  if (int e = attn_launch(plan.k[0], args, stream)) return e;
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

static int attn_bwd_launch(const char* name, int max_len, mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                           const float* key_add, const void* dctx_bf16, const float* stats, float* drow, void* dq_bf16, void* dk_bf16,
                           void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo, int lddq, int lddk,
                           float scale, float drop_p, unsigned long long seed, unsigned int site, const int* q_off, const int* k_off,
                           const int* k_cnt, int q_rows) {
  AttnPlan plan;
  if (int e = attn_bwd_prepare(plan, name, max_len, q_bf16, k_bf16, v_bf16, key_add, dctx_bf16, stats, drow, dq_bf16, dk_bf16, dv_bf16, B, heads, Lq,
                               Lk, head_dim, ldq, ldk, ldo, lddq, lddk, drop_p, q_off, k_off, k_cnt, q_rows))
    return e;
  AttnVarlen vl = {q_off, k_off, k_cnt, q_rows};
  uint32_t th = thresh16_of(drop_p), site32 = site;
  float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  uint64_t seed64 = seed;
  int kstride = plan.nt * 16;
  void* args_q[] = {&q_bf16, &k_bf16, &v_bf16, &key_add, &dctx_bf16, &stats, &dq_bf16, &drow, &heads, &Lq, &Lk, &ldq, &ldk, &ldo, &lddq, &scale,
                    &th, &sc, &seed64, &site32, &vl};
  if (int e = attn_launch(plan.k[0], args_q, stream)) return e;
  MMDTI_LAUNCH_CHECK();
  void* args_kv[] = {&q_bf16, &k_bf16, &v_bf16, &key_add, &dctx_bf16, &stats, &drow, &dk_bf16, &dv_bf16, &heads, &Lq, &Lk, &ldq, &ldk, &ldo, &lddk,
                     &scale, &th, &sc, &seed64, &site32, &kstride, &vl};
  if (int e = attn_launch(plan.k[1], args_kv, stream)) return e;
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

}  // namespace mmdti
MMDTI_DEFINE_SALT_PULL(attn)
using namespace mmdti;

extern "C" int mmdti_attn_fwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                              const float* key_add, void* ctx_bf16, float* stats, int B, int heads, int Lq, int Lk,
                              int head_dim, int ldq, int ldk, int ldo, float scale, float drop_p, unsigned long long seed,
                              unsigned int site, const int* q_off, const int* k_off, const int* k_cnt, int q_rows, int ctx_f16) {
  return attn_fwd_launch("attn_fwd", ATTN_MAX_LEN, stream, q_bf16, k_bf16, v_bf16, key_add, ctx_bf16, stats, B, heads, Lq, Lk, head_dim, ldq,
                         ldk, ldo, scale, drop_p, seed, site, q_off, k_off, k_cnt, q_rows, ctx_f16);
}

extern "C" int mmdti_attn_bwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                              const float* key_add, const void* dctx_bf16, const float* stats, float* drow, void* dq_bf16,
                              void* dk_bf16, void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk,
                              int ldo, int lddq, int lddk, float scale, float drop_p, unsigned long long seed,
                              unsigned int site, const int* q_off, const int* k_off, const int* k_cnt, int q_rows) {
  return attn_bwd_launch("attn_bwd", ATTN_MAX_LEN, stream, q_bf16, k_bf16, v_bf16, key_add, dctx_bf16, stats, drow, dq_bf16, dk_bf16, dv_bf16,
                         B, heads, Lq, Lk, head_dim, ldq, ldk, ldo, lddq, lddk, scale, drop_p, seed, site, q_off, k_off, k_cnt, q_rows);
}

extern "C" int mmdti_attn_long_fwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                                   const float* key_add, void* ctx_bf16, float* stats, int B, int heads, int Lq, int Lk,
                                   int head_dim, int ldq, int ldk, int ldo, float scale, float drop_p, unsigned long long seed,
                                   unsigned int site, const int* q_off, const int* k_off, const int* k_cnt, int q_rows, int ctx_f16) {
  return attn_fwd_launch("attn_long_fwd", ATTN_LONG_MAX_LEN, stream, q_bf16, k_bf16, v_bf16, key_add, ctx_bf16, stats, B, heads, Lq, Lk,
                         head_dim, ldq, ldk, ldo, scale, drop_p, seed, site, q_off, k_off, k_cnt, q_rows, ctx_f16);
}

extern "C" int mmdti_attn_long_bwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                                   const float* key_add, const void* dctx_bf16, const float* stats, float* drow, void* dq_bf16,
                                   void* dk_bf16, void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk,
                                   int ldo, int lddq, int lddk, float scale, float drop_p, unsigned long long seed,
                                   unsigned int site, const int* q_off, const int* k_off, const int* k_cnt, int q_rows) {
  return attn_bwd_launch("attn_long_bwd", ATTN_LONG_MAX_LEN, stream, q_bf16, k_bf16, v_bf16, key_add, dctx_bf16, stats, drow, dq_bf16,
                         dk_bf16, dv_bf16, B, heads, Lq, Lk, head_dim, ldq, ldk, ldo, lddq, lddk, scale, drop_p, seed, site, q_off, k_off,
                         k_cnt, q_rows);
}

extern "C" int mmdti_attn_plan(int backward, int long_entry, const void* q_bf16, const void* k_bf16, const void* v_bf16, const float* key_add,
                               const void* ctx_or_dctx_bf16, const float* stats, const float* drow, const void* dq_bf16, const void* dk_bf16,
                               const void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo, int lddq, int lddk,
                               float drop_p, const int* q_off, const int* k_off, const int* k_cnt, int q_rows, int* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr, "attn_plan: null plan_out");
  const int max_len = long_entry ? ATTN_LONG_MAX_LEN : ATTN_MAX_LEN;
  AttnPlan plan;
  if (backward) {
    if (int e = attn_bwd_prepare(plan, long_entry ? "attn_long_bwd" : "attn_bwd", max_len, q_bf16, k_bf16, v_bf16, key_add, ctx_or_dctx_bf16, stats,
                                 drow, dq_bf16, dk_bf16, dv_bf16, B, heads, Lq, Lk, head_dim, ldq, ldk, ldo, lddq, lddk, drop_p, q_off, k_off,
                                 k_cnt, q_rows))
      return e;
  } else {
    if (int e = attn_fwd_prepare(plan, long_entry ? "attn_long_fwd" : "attn_fwd", max_len, q_bf16, k_bf16, v_bf16, key_add, ctx_or_dctx_bf16, stats,
                                 B, heads, Lq, Lk, head_dim, ldq, ldk, ldo, drop_p, q_off, k_off, k_cnt, q_rows))
      return e;
  }
  static_assert(ATTN_PLAN_INTS == 13, "mmdti_hip.h documents 13 ints");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}
