// Pair-bias multi-head attention for the Uni-Mol tower (64 heads x head_dim 8), forward and backward.
//
// Replaces unicore SelfMultiheadAttention + softmax_dropout (fused CUDA op upstream) as reached from
// models/transformers.py:137-139 with return_attn=True, including the key-padding merge of :122-135:
//     S_l = scale * q.k^T + S_{l-1}          (S_0 = Gaussian pair bias, -inf at padded keys)
//     O   = dropout(softmax(S_l)) . v
// S_l is an OUTPUT (it is the next layer's bias and the activation saved for backward), so the score tile is
// never kept on chip only: the kernel is a stream over the [B,H,N,N] pair tensor and is HBM-bound
// (head_dim 8 => 32 flop per 8 B of pair traffic).  One workgroup per (molecule, head); lanes own KEYS
// (K/V rows live in registers for the whole tile), waves walk query rows, so every pair-tensor access is a
// fully coalesced row segment and dK/dV need no cross-lane traffic.
//
// Backward recomputes P from the saved S and carries the running pair gradient G in place:
//     G_l = G_{l+1} + softmax'(S_l)    dq = scale * G_l k,  dk = scale * G_l^T q,  dv = Pd^T dO
#include "pair_attn.h"

namespace mmdti {

template <int NCH>
__global__ __launch_bounds__(256) void pair_attn_fwd_kernel(const bf16_t* __restrict__ qkv,
                                                            const float* __restrict__ bias_in,
                                                            float* __restrict__ s_out, bf16_t* __restrict__ o,
                                                            const unsigned char* __restrict__ key_pad, int N, int H,
                                                            int ld, float scale, uint32_t thresh, float dscale,
                                                            uint64_t seed, uint32_t site) {
  __shared__ __attribute__((aligned(16))) float sq[NCH * 64][HD];
  // (the 64 heads of a token share 128-byte q / k / v lines, 8 heads per line: keep a molecule's heads on one XCD)
  const int bh = xcd_chunk(blockIdx.x, gridDim.x), b = bh / H, h = bh - b * H;
  const int D = H * HD, D3 = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* base = qkv + (long long)b * N * D3 + h * HD;
  for (int t = tid; t < N; t += 256) {
    float q[8];
    load8_bf16(base + (long long)t * D3, q);
#pragma unroll
    for (int d = 0; d < 8; ++d) sq[t][d] = q[d];
  }
  float k[NCH][8], v[NCH][8];
  bool masked[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = c * 64 + lane;
    masked[c] = true;
#pragma unroll
    for (int d = 0; d < 8; ++d) k[c][d] = v[c][d] = 0.f;
    if (j < N) {
      load8_bf16(base + (long long)j * D3 + D, k[c]);
      load8_bf16(base + (long long)j * D3 + 2 * D, v[c]);
      masked[c] = key_pad ? key_pad[b * N + j] != 0 : false;
    }
  }
  __syncthreads();
  const float NEG_INF = -INFINITY;
  // software pipeline over rows: the bias row of iteration i+4 is requested before row i is processed, so each wave keeps
  // two rows of pair traffic in flight (the stream is latency-bound otherwise: one row = 3 x 256 B per wave).
  float nb[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = c * 64 + lane;
    nb[c] = (wave < N && j < N && !masked[c]) ? bias_in[((long long)bh * N + wave) * ld + j] : 0.f;
  }
  for (int i = wave; i < N; i += 4) {
    const float4 q0 = *reinterpret_cast<const float4*>(&sq[i][0]);
    const float4 q1 = *reinterpret_cast<const float4*>(&sq[i][4]);
    const long long rowoff = ((long long)bh * N + i) * ld;
    float cb[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) cb[c] = nb[c];
    if (i + 4 < N) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = c * 64 + lane;
        nb[c] = (j < N && !masked[c]) ? bias_in[rowoff + 4LL * ld + j] : 0.f;
      }
    }
    float sv[NCH];
    float m = NEG_INF;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = c * 64 + lane;
      float s = NEG_INF;
      if (j < N) {
        float dot = q0.x * k[c][0] + q0.y * k[c][1] + q0.z * k[c][2] + q0.w * k[c][3] + q1.x * k[c][4] +
                    q1.y * k[c][5] + q1.z * k[c][6] + q1.w * k[c][7];
        s = masked[c] ? NEG_INF : scale * dot + cb[c];
        s_out[rowoff + j] = s;
      }
      sv[c] = s;
      m = fmaxf(m, s);
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      sv[c] = __expf(sv[c] - m);
      sum += sv[c];
    }
    const float inv = 1.0f / wave_sum(sum);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float p = sv[c] * inv;
      if (thresh) {
        const int j = c * 64 + lane;
        bool keep = dropout_keep(seed, site, ((uint64_t)bh * N + i) * ld + j, thresh);
        p = keep ? p * dscale : 0.f;
      }
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[d] += p * v[c][d];
    }
    const float tot = wave_sum8_scatter(acc, lane);
    if (lane < 8) o[((long long)b * N + i) * D + h * HD + lane] = f2bf(tot);
  }
}

// RAG (ragged batches): key_tiles[b] = number of 16-key tiles of molecule b that hold a real key.  The tiles past it (past
// pa_kt_effective of it) are all padding -- -inf in every S of the chain, 0 in G -- so they are neither loaded nor computed nor
// (rag_store == 0) stored; pad QUERY rows are still computed (the reference's unmasked InfoNCE mean reads the encoder output at
// padded positions).  rag_store != 0: the skipped tiles are written as -inf (the last layer, whose S is returned to the caller).
template <int NT, bool TILED, bool FULL, bool RAG, typename ST, bool F16 = false>
__global__ __launch_bounds__(256, NT > 9 ? 2 : 4) void pair_attn_fwd_mfma_kernel(const bf16_t* __restrict__ qkv, const ST* __restrict__ bias_in,
                                                                 ST* __restrict__ s_out, bf16_t* __restrict__ o,
                                                                 const unsigned char* __restrict__ key_pad, int N, int H, int ld,
                                                                 float scale, uint32_t thresh, float dscale, uint64_t seed,
                                                                 uint32_t site, const int* __restrict__ key_tiles, int rag_store,
                                                                 const int* __restrict__ row_off) {
  static_assert(TILED || sizeof(ST) == 4, "compact pair tensors exist in the tiled layout only");
  static_assert(!RAG || sizeof(ST) == 2, "key-tile skipping is built for the compact layout only");
  constexpr int NP = NT * 16;
  constexpr int KSTR = NP + 8;   // row stride (elements) of the d-major V image (see the backward kernel's sKT)
  // raw bf16 images, exactly as loaded: sQ / sK [row][8], sVT [d][key]
  __shared__ __attribute__((aligned(16))) bf16_t sQ[NP * 8];
  __shared__ __attribute__((aligned(16))) bf16_t sK[NP * 8];
  __shared__ __attribute__((aligned(16))) bf16_t sVT[8 * KSTR];
  __shared__ __attribute__((aligned(16))) float sM[NP];
  PA_WG_PROLOGUE();   // (pair_attn.h, as every PA_ piece below)
  for (int t = tid; t < NP; t += blockDim.x) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u), kk = q, vv = q;
    float msk = 1.f;
    if (t < rows) {
      q = *reinterpret_cast<const uint4*>(base + (long long)t * D3);
      kk = *reinterpret_cast<const uint4*>(base + (long long)t * D3 + D);
      vv = *reinterpret_cast<const uint4*>(base + (long long)t * D3 + 2 * D);
      msk = (key_pad && key_pad[row0 + t]) ? 1.f : 0.f;
    }
    *reinterpret_cast<uint4*>(sQ + t * 8) = q;
    *reinterpret_cast<uint4*>(sK + t * 8) = kk;
    const uint32_t vw[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int d = 0; d < 8; ++d) sVT[d * KSTR + t] = (bf16_t)((d & 1) ? (vw[d >> 1] >> 16) : (vw[d >> 1] & 0xffffu));
    sM[t] = msk;
  }
  for (int t = tid; t < 8 * 8; t += blockDim.x) sVT[(t >> 3) * KSTR + NP + (t & 7)] = 0;
  __syncthreads();
  const int g = lane >> 4, c16 = lane & 15;
  const float NEG_INF = -INFINITY;
  PA_LAST_TILE();
  auto body = [&](int qb, auto edge_c, auto kt_c) {
    constexpr bool EDGE = decltype(edge_c)::value;
    constexpr int KT = decltype(kt_c)::value;   // key tiles this molecule's sweeps cover (NT unless RAG)
    PA_QROW();
    const pa_s16x4 zero4 = {0, 0, 0, 0};
    // B of S^T = K.Q^T : Q[query c16][d = 4g..4g+3] (k = d: lane groups 2, 3 carry zeros)
    const pa_s16x4 qv = g < 2 ? *reinterpret_cast<const pa_s16x4*>(sQ + (qb * 16 + c16) * 8 + 4 * g) : zero4;
    PA_QTILE();
    // (a lane whose predicate is off reads the row's first 16 bytes -- always inside the tensor, unlike "tile 0 + 4g" when ld < 16)
    const ST* bin = bias_in + (TILED ? tbase : rowoff);
    ST* sout = s_out + (TILED ? tbase : rowoff);
    PA_TILE_STEP();
    // Phase 1: request every bias tile of this query block (the NT 16-byte loads are issued back to back and stay in
    // flight together).  Slots that are not loaded: -inf (pad keys), or 0 in a pad ROW (keeps that row's softmax finite;
    // nothing of it is stored).
    const float fillv = (TILED && qvalid) ? -INFINITY : 0.f;
    f32x4 S[KT];
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      PA_LOAD4(S[t], bin, t, fillv);
    }
    float m = NEG_INF;
    if (RAG && rag_store) {   // the all-padding tiles past KT: -inf (the last layer: its S goes back to the caller)
      const f32x4 ninf = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
#pragma unroll
      for (int t = KT; t < NT; ++t) {
        PA_STORE4(sout, t, ninf);
      }
    }
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      {
        const int kcol = t * 16 + 4 * g;
        f32x4 c = S[t];
        const pa_s16x4 ka = g < 2 ? *reinterpret_cast<const pa_s16x4*>(sK + (t * 16 + c16) * 8 + 4 * g) : zero4;
        f32x4 qk = {0.f, 0.f, 0.f, 0.f};
        qk = pa_mfma16<F16>(ka, qv, qk);   // exact products of the 16-bit operands, fp32 accumulation
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] += scale * qk[r];
        if (!TILED || key_pad) {   // (tiled tensors carry -inf in their pad keys already: only a real padding mask is left)
          const f32x4 km = *reinterpret_cast<const f32x4*>(&sM[kcol]);
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] = (km[r] != 0.f) ? NEG_INF : c[r];
        }
        typename std::conditional<sizeof(ST) == 2, pa_f16x4, f32x4>::type cs;
        c = pa_round4(cs, c);   // (compact: the fp16 value that is stored is also the one this layer's softmax sees)
        PA_STORE4(sout, t, cs);
        S[t] = c;
        m = fmaxf(fmaxf(m, c[0]), c[1]);   // (two v_max3_f32)
        m = fmaxf(fmaxf(m, c[2]), c[3]);
      }
    }
    PA_ROW_MAX(m);
    PA_ROW_EXP2(S, m);
    const float inv = dscale / lsum;   // (dropout's 1 / (1 - p) folded in: dscale == 1 without dropout)
    f32x4 oacc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      {
        f32x4 p = S[t] * inv;
        if (thresh) {
          const uint32_t kw = PA_DROP_WORD(t);
#pragma unroll
          for (int r = 0; r < 4; ++r) p[r] = rng24_kept(kw, r, t8) ? p[r] : 0.f;
        }
        // O^T += V^T . P^T : A = V[keys 16t + 4g..4g+3][d = c16 & 7] (rows d >= 8 of the result are never stored), B = P^T as it sits
        const pa_s16x4 va = *reinterpret_cast<const pa_s16x4*>(sVT + (c16 & 7) * KSTR + t * 16 + 4 * g);
        pa_s16x4 ph, pl;
        pa_split4_t<F16>(p, ph, pl);
        oacc = pa_mfma16<F16>(va, ph, oacc);
        oacc = pa_mfma16<F16>(va, pl, oacc);
      }
    }
    // O^T accumulator: column = query, rows d = 4g + r (valid for g < 2)
    if (qvalid && g < 2) {
      uint2 pk;
      if constexpr (F16) {   // (o feeds out_proj's forward GEMM: fp16 like every forward GEMM operand of this mode)
        pk.x = f2h_sat2(oacc[0], oacc[1]);
        pk.y = f2h_sat2(oacc[2], oacc[3]);
      } else {
        pk.x = (uint32_t)f2bf(oacc[0]) | ((uint32_t)f2bf(oacc[1]) << 16);
        pk.y = (uint32_t)f2bf(oacc[2]) | ((uint32_t)f2bf(oacc[3]) << 16);
      }
      *reinterpret_cast<uint2*>(o + ((long long)row0 + qi) * D + h * HD + 4 * g) = pk;
    }
  };
  PA_RUN_QUERY_BLOCKS();
}

// =====================================================================================================================
// MFMA-tiled backward, same tiling as the forward: a wave owns 16 queries and sweeps the key tiles twice.
//   sweep 1: load S^T tiles, row max / sum  ->  P^T ; dP^T = V.dO^T (MFMA) ; dropout mask (kept in the sign of P) ;
//            delta = rowsum(dP' * P)
//   sweep 2: G^T = G_in^T + P^T*(dP'^T - delta)  (16-byte load + store per lane per tile, in place) ;
//            dQ^T += K^T.G^T (MFMA, G^T is already the B operand) ;
//            dK += G.Q and dV += Pd.dO contract over QUERIES (the lane axis of the accumulator layout), so each tile is
//            transposed through a per-wave 16x16 LDS patch: written row-major, read back with ds_read_b64_tr_b16.
// Precision of sweep 2: Q, K, V, dO are bf16 in memory, so they enter the MFMAs exactly; the fp32 factors G and
// dropout(P) are split into bf16 high + bf16 low parts (x = hi + lo + O(2^-17 |x|)) and every product runs twice on
// v_mfma_f32_16x16x16_bf16 -- fp32-class products (16 mantissa bits kept of the fp32 factor, fp32 accumulation) at a
// quarter of the matrix-pipe time and a third of the LDS instructions of the fp32 16x16x4 form this replaces.
// Each (query block, key tile) contribution to dK/dV is added to an LDS image owned by the wave.

}  // namespace mmdti
MMDTI_DEFINE_SALT_PULL(pair_attn)
using namespace mmdti;


// every MFMA instance, at the row its key gives it (pair_attn_plan.h); one argument block: the instances differ in the element type of
// the two pair tensors only
#define PA_FWD_COMPACT_ROW(NT)                                                                                                    \
  KROW(pa_fwd_compact_key(NT, 0, 0), pair_attn_fwd_mfma_kernel<NT, true, true, false, _Float16>),                                 \
  KROW(pa_fwd_compact_key(NT, 0, 1), pair_attn_fwd_mfma_kernel<NT, true, true, true, _Float16>),                                  \
  KROW(pa_fwd_compact_key(NT, 1, 0), pair_attn_fwd_mfma_kernel<NT, true, true, false, _Float16, true>),                           \
  KROW(pa_fwd_compact_key(NT, 1, 1), pair_attn_fwd_mfma_kernel<NT, true, true, true, _Float16, true>)
#define PA_FWD_F32_ROW(NT)                                                                                                        \
  KROW(pa_fwd_f32_key(pa_bucket(NT), 0, 0), pair_attn_fwd_mfma_kernel<NT, false, false, false, float>),                           \
  KROW(pa_fwd_f32_key(pa_bucket(NT), 1, 0), pair_attn_fwd_mfma_kernel<NT, true, false, false, float>),                            \
  KROW(pa_fwd_f32_key(pa_bucket(NT), 1, 1), pair_attn_fwd_mfma_kernel<NT, true, true, false, float>)
static KernelRow g_pa_fwd_mfma[PA_FWD_MFMA_KERNELS] = {
    PA_FWD_COMPACT_ROW(1),  PA_FWD_COMPACT_ROW(2),  PA_FWD_COMPACT_ROW(3),  PA_FWD_COMPACT_ROW(4),  PA_FWD_COMPACT_ROW(5),  PA_FWD_COMPACT_ROW(6),
    PA_FWD_COMPACT_ROW(7),  PA_FWD_COMPACT_ROW(8),  PA_FWD_COMPACT_ROW(9),  PA_FWD_COMPACT_ROW(10), PA_FWD_COMPACT_ROW(11), PA_FWD_COMPACT_ROW(12),
    PA_FWD_COMPACT_ROW(13), PA_FWD_COMPACT_ROW(14), PA_FWD_COMPACT_ROW(15), PA_FWD_COMPACT_ROW(16), PA_FWD_COMPACT_ROW(17),
    PA_FWD_F32_ROW(5),      PA_FWD_F32_ROW(9),      PA_FWD_F32_ROW(13),     PA_FWD_F32_ROW(17),
};
#undef PA_FWD_COMPACT_ROW
#undef PA_FWD_F32_ROW
// the per-element kernels (N > 272, or rows / planes that are not 16-byte aligned): their own small family
static KernelRow g_pa_fwd_elem[PA_FWD_ELEM_KERNELS] = {
    KROW(pa_fwd_elem_key(1), pair_attn_fwd_kernel<1>), KROW(pa_fwd_elem_key(2), pair_attn_fwd_kernel<2>), KROW(pa_fwd_elem_key(3), pair_attn_fwd_kernel<3>),
    KROW(pa_fwd_elem_key(4), pair_attn_fwd_kernel<4>), KROW(pa_fwd_elem_key(5), pair_attn_fwd_kernel<5>),
};
const KernelRow* mmdti::pair_attn_fwd_table(int family, int* n) {
  *n = family == PA_FWD_MFMA ? PA_FWD_MFMA_KERNELS : PA_FWD_ELEM_KERNELS;
  return family == PA_FWD_MFMA ? g_pa_fwd_mfma : g_pa_fwd_elem;
}

// What mmdti_pair_attn_fwd and mmdti_pair_attn_plan share: validate, plan.  Pointers are tested for null and alignment only.
int mmdti::pair_attn_fwd_prepare(PairAttnPlan& plan, const void* qkv_bf16, const void* bias_in, const void* s_out, const void* o_bf16, int B, int N, int H,
                                 int ld, float drop_p, int layout, const void* key_tiles, const void* row_off, int qkv_f16) {
  const int tiled = layout & 1, compact = (layout >> 1) & 1;   // bit 0: tiled planes; bit 1: compact planes (S fp16; tiled only)
  if (int e = check_common("pair_attn_fwd", B, N, H, ld)) return e;
  MMDTI_REQUIRE((layout & ~3) == 0 && (!compact || tiled), "pair_attn_fwd: layout must be 0 (row-major fp32), 1 (tiled fp32) or 3 (tiled, fp16 logits)");
  MMDTI_REQUIRE(!key_tiles || compact, "pair_attn_fwd: key_tiles (ragged batches) needs the compact tiled pair layout (layout 3)");
  MMDTI_REQUIRE(!row_off || key_tiles, "pair_attn_fwd: packed token rows (row_off) need key_tiles");
  MMDTI_REQUIRE(!qkv_f16 || compact, "pair_attn_fwd: fp16 q | k | v (the fp16 forward-operand mode) is built for the compact tiled pair layout (layout 3)");
  MMDTI_REQUIRE(!tiled || (ld % 4 == 0 && N <= 16 * PA_MAX_NT), "pair_attn_fwd: the tiled pair layout needs ld %% 4 == 0 and N <= 272");
  MMDTI_REQUIRE(qkv_bf16 && bias_in && s_out && o_bf16, "pair_attn_fwd: null pointer");
  MMDTI_REQUIRE(aligned16(qkv_bf16), "pair_attn_fwd: qkv must be 16-byte aligned");
  MMDTI_REQUIRE(!tiled || (aligned16(bias_in) && aligned16(s_out)), "pair_attn_fwd: tiled pair tensors must be 16-byte aligned");
  MMDTI_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "pair_attn_fwd: dropout p out of range");
  plan = pair_attn_fwd_plan(B, N, H, ld, tiled, compact, aligned16(bias_in) && aligned16(s_out), key_tiles != nullptr, qkv_f16 != 0);
  return MMDTI_OK;
}

extern "C" int mmdti_pair_attn_fwd(mmdti_stream_t stream, const void* qkv_bf16, const void* bias_in, void* s_out,
                                   void* o_bf16, const unsigned char* key_pad, int B, int N, int H, int ld,
                                   float scale, float drop_p, unsigned long long seed, unsigned int site, int layout,
                                   const int* key_tiles, int rag_store, const int* row_off, int qkv_f16) {
  PairAttnPlan plan;
  if (int e = pair_attn_fwd_prepare(plan, qkv_bf16, bias_in, s_out, o_bf16, B, N, H, ld, drop_p, layout, key_tiles, row_off, qkv_f16)) return e;
  // the per-element kernel: Philox words against p * 2^32; the MFMA kernels: the shared byte generator of common.h
  uint32_t th = plan.family == PA_FWD_MFMA ? dropout_thresh8(drop_p) : dropout_thresh(drop_p), site32 = site;
  float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  uint64_t seed64 = seed;
  // (the per-element kernel's parameters are the first thirteen of the MFMA kernel's)
  void* args[] = {&qkv_bf16, &bias_in, &s_out, &o_bf16, &key_pad, &N, &H, &ld, &scale, &th, &sc, &seed64, &site32, &key_tiles, &rag_store, &row_off};
  const KernelRow& row = (plan.family == PA_FWD_MFMA ? g_pa_fwd_mfma : g_pa_fwd_elem)[plan.key];
  (void)hipLaunchKernel(row.fn, dim3(plan.grid), dim3(plan.block), args, 0, (hipStream_t)stream);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}
