// pair_attn_bwd_mfma.h -- the MFMA backward kernel of the pair-bias attention and the launcher of its hot path (compact planes:
// fp16 logits, one instantiation per tile count, dense and ragged).  A header because the hot path is compiled TWICE -- gradient
// chain G in fp32 (pair_attn_bwd.hip) and in bf16 (pair_attn_bwd_g16.hip) -- as two translation units that build in parallel
// (34 instantiations of this kernel each: two minutes of hipcc apiece).
#pragma once
#include "pair_attn.h"

namespace mmdti {

// RAG: see pair_attn_fwd_mfma_kernel (pair_attn.hip).  Skipped key tiles contribute nothing (P = 0, G = 0) and their G is NOT written: the caller
// hands in a zero-initialised G when the batch is ragged.
template <int NT, bool TILED, bool FULL, int NW, bool RAG, typename ST, typename GT>
__global__ __launch_bounds__(64 * NW, NT > 9 ? ((NT >= 16 && NW == 3) ? 2 : 1) : 3) void pair_attn_bwd_mfma_kernel(const bf16_t* __restrict__ qkv, const ST* __restrict__ s_in,
                                                                 const bf16_t* __restrict__ dO, const GT* __restrict__ gin, GT* __restrict__ gout,
                                                                 bf16_t* __restrict__ dqkv, int N, int H, int ld, float scale,
                                                                 int g_in_zero, uint32_t thresh, float dscale, uint64_t seed,
                                                                 uint32_t site, const int* __restrict__ key_tiles,
                                                                 const int* __restrict__ row_off, int qkv_f16) {
  static_assert(TILED || (sizeof(ST) == 4 && sizeof(GT) == 4), "compact pair tensors exist in the tiled layout only");
  static_assert(!RAG || sizeof(ST) == 2, "key-tile skipping is built for the compact layout only");
  constexpr int NP = NT * 16;
  constexpr int KSTR = NP + 8;   // row stride (elements) of the d-major K image: 8-byte reads of 8 rows x 2 key groups hit 16 distinct bank pairs
  // raw bf16 images, exactly as loaded.  sQ / sD / sV: [row][8]; the +16 elements are the tail that tr-reads of the last
  // rows run into (they only feed output columns d >= 8, which are never used).  sKT: [d][key].
  __shared__ __attribute__((aligned(16))) bf16_t sQ[NP * 8 + 16];
  __shared__ __attribute__((aligned(16))) bf16_t sD[NP * 8 + 16];   // dO
  __shared__ __attribute__((aligned(16))) bf16_t sV[NP * 8];
  __shared__ __attribute__((aligned(16))) bf16_t sKT[8 * KSTR];
  // per-wave dK / dV accumulators in MFMA accumulator order: [wave][tile][K|V][g][d][r] -- each lane owns one float4 per
  // (tile, K|V), read as the MFMA C input and written back, so the waves never contend (LDS float atomics cost ~57
  // cycles per wave-instruction here and were half of the kernel's time).
  __shared__ __attribute__((aligned(16))) float redw[NW * NT * 2 * 128];
  // per-wave transpose patches [P | G], each [16 queries][16 keys] bf16 (512 B), used twice per tile (high parts, then low
  // parts: with two patches instead of four the workgroup stays under 40 KB -> four per CU); the 8-byte slot s of row q
  // sits at slot s ^ (2 * (q >> 3)), which makes both the row writes and the transposing reads conflict-free
  __shared__ __attribute__((aligned(16))) bf16_t patch[NW][2][256];
  PA_WG_PROLOGUE();   // (pair_attn.h, as every PA_ piece below)
  for (int t = tid; t < NP + 2; t += blockDim.x) {
    uint4 q = make_uint4(0u, 0u, 0u, 0u), kk = q, vv = q, dd = q;
    if (t < rows) {
      q = *reinterpret_cast<const uint4*>(base + (long long)t * D3);
      kk = *reinterpret_cast<const uint4*>(base + (long long)t * D3 + D);
      vv = *reinterpret_cast<const uint4*>(base + (long long)t * D3 + 2 * D);
      dd = *reinterpret_cast<const uint4*>(dO + ((long long)row0 + t) * D + h * HD);
      // (fp16 forward operands: the forward multiplied the fp16 q | k | v; the backward's products take their bf16 rounding -- the
      //  values mmdti_cast_f16_bf16 would write -- converted here, on the way into LDS, instead of in a pass over HBM)
      if (qkv_f16) { q = h2bf8(q); kk = h2bf8(kk); vv = h2bf8(vv); }
    }
    *reinterpret_cast<uint4*>(sQ + t * 8) = q;      // (t = NP, NP + 1: the zeroed tails)
    *reinterpret_cast<uint4*>(sD + t * 8) = dd;
    if (t < NP) {
      *reinterpret_cast<uint4*>(sV + t * 8) = vv;
      const uint32_t kw[4] = {kk.x, kk.y, kk.z, kk.w};
#pragma unroll
      for (int d = 0; d < 8; ++d) sKT[d * KSTR + t] = (bf16_t)((d & 1) ? (kw[d >> 1] >> 16) : (kw[d >> 1] & 0xffffu));
    }
  }
  for (int t = tid; t < 8 * 8; t += blockDim.x) sKT[(t >> 3) * KSTR + NP + (t & 7)] = 0;
  for (int t = tid; t < NW * NT * 2 * 128; t += blockDim.x) redw[t] = 0.f;
  __syncthreads();
  const int g = lane >> 4, c16 = lane & 15;
  const bool dlane = c16 < 8;
  const float NEG_INF = -INFINITY;
  bf16_t* pw = &patch[wave][0][0];
  // patch addressing (elements): this lane WRITES row c16, logical slot g ; tr-READS address row 4g + (c16 >> 2), logical slot c16 & 3
  const int pwr = c16 * 16 + ((g ^ ((c16 >> 3) << 1)) << 2);
  const int prd = (4 * g + (c16 >> 2)) * 16 + (((c16 & 3) ^ ((g >> 1) << 1)) << 2);
  const pa_s16x4 zero4 = {0, 0, 0, 0};
  PA_LAST_TILE();   // (the pad slots of a tiled S, -inf, and of a tiled G, 0, are preserved by the stores below)
  auto body = [&](int qb, auto edge_c, auto kt_c) {
    constexpr bool EDGE = decltype(edge_c)::value;
    constexpr int KT = decltype(kt_c)::value;   // key tiles this molecule's sweeps cover (NT unless RAG)
    PA_QROW();
    PA_QTILE();
    const ST* sin_p = s_in + (TILED ? tbase : rowoff);     // (predicate-off lanes read the row's first 16 bytes: in bounds)
    const GT* gin_p = gin + (TILED ? tbase : rowoff);
    GT* gout_p = gout + (TILED ? tbase : rowoff);
    PA_TILE_STEP();
    // operands of this query block that do not depend on the key tile:
    //   dob : B of dP^T = V.dO^T          -> dO[query c16][d = 4g..4g+3]   (k = d: lane groups 2, 3 carry zeros)
    //   bD  : B of dV  += Pd^T.dO         -> dO[queries 4g..4g+3][d = c16] (transposing read; columns d >= 8 are unused)
    //   bQ  : B of dK  += G^T.Q           -> Q [queries 4g..4g+3][d = c16]
    const pa_s16x4 dob = g < 2 ? *reinterpret_cast<const pa_s16x4*>(sD + (qb * 16 + c16) * 8 + 4 * g) : zero4;
    const int trq = (qb * 16 + 4 * g + (c16 >> 2)) * 8 + 4 * (c16 & 3);
    const pa_s16x4 bD = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(sD + trq));
    const pa_s16x4 bQ = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(sQ + trq));
    // ---- sweep 1
    f32x4 P[KT];
    float m = NEG_INF;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      {
        const int kcol = t * 16 + 4 * g;
        f32x4 c;
        PA_LOAD4(c, sin_p, t, NEG_INF);
        if (!TILED) {
#pragma unroll
          for (int r = 0; r < 4; ++r) c[r] = (kcol + r < N) ? c[r] : NEG_INF;   // pad columns of the row are not data
        }
        P[t] = c;
        m = fmaxf(fmaxf(m, c[0]), c[1]);
        m = fmaxf(fmaxf(m, c[2]), c[3]);
      }
    }
    PA_ROW_MAX(m);
    if (m == NEG_INF) m = 0.f;   // rows beyond N: everything is -inf, keep the arithmetic finite
    PA_ROW_EXP2(P, m);
    const float inv = lsum > 0.f ? 1.0f / lsum : 0.f;
    // dropped elements are remembered in the SIGN of P (P >= 0): |P| feeds the softmax gradient, P > 0 selects dropout(P)
    float dl = 0.f;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      {
        // A of dP^T: V[key 16t + c16][d = 4g..4g+3] (exact bf16 products, fp32 accumulation)
        const pa_s16x4 va = g < 2 ? *reinterpret_cast<const pa_s16x4*>(sV + (t * 16 + c16) * 8 + 4 * g) : zero4;
        f32x4 dp = {0.f, 0.f, 0.f, 0.f};
        dp = PA_MFMA16(va, dob, dp);
        f32x4 pr = P[t] * inv;
        if (thresh) {
          const uint32_t kw = PA_DROP_WORD(t);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool kp = rng24_kept(kw, r, t8);
            dp[r] = kp ? dp[r] * dscale : 0.f;
            dl += dp[r] * pr[r];
            pr[r] = kp ? pr[r] : -pr[r];
          }
        } else {
          dl += dp[0] * pr[0] + dp[1] * pr[1] + dp[2] * pr[2] + dp[3] * pr[3];
        }
        P[t] = pr;
      }
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    // ---- sweep 2 (branch-free per tile;
    // dP is formed again per tile -- one 8-byte LDS read and one MFMA are cheaper than 36 more live registers)
    // G_in tiles are requested PA_LA tiles ahead of their use (a ring of PA_LA quads instead of all NT: 24 registers
    // fewer at the 168 cap -- no spills), pinned in place by scheduling barriers
    constexpr int PA_LA = 3;
    auto load_gin = [&](int t) -> f32x4 {
      f32x4 gq;
      PA_LOAD4_IF(gq, gin_p, t, 0.f, !g_in_zero);
      return gq;
    };
    f32x4 Gq[PA_LA];
#pragma unroll
    for (int t = 0; t < PA_LA && t < KT; ++t) Gq[t] = load_gin(t);
    f32x4 dq = {0.f, 0.f, 0.f, 0.f};
    const int dcol = dlane ? c16 : 0;
#pragma unroll
    for (int t = 0; t < KT; ++t) {
      const int kcol = t * 16 + 4 * g;
      const f32x4 Gin = Gq[t % PA_LA];
      if (t + PA_LA < KT) Gq[t % PA_LA] = load_gin(t + PA_LA);
      __builtin_amdgcn_sched_barrier(0);
      const pa_s16x4 va = g < 2 ? *reinterpret_cast<const pa_s16x4*>(sV + (t * 16 + c16) * 8 + 4 * g) : zero4;
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
      dp = PA_MFMA16(va, dob, dp);
      f32x4 G;
#pragma unroll
      for (int r = 0; r < 4; ++r) G[r] = fabsf(P[t][r]) * ((P[t][r] > 0.f ? dp[r] * dscale : 0.f) - dl) + Gin[r];
      if (!TILED && t * 16 + 16 > N) {   // only the last key tile has columns beyond N (uniform branch): their G must be exactly 0
#pragma unroll
        for (int r = 0; r < 4; ++r) G[r] = (kcol + r < N) ? G[r] : 0.f;
      }
      if (EDGE && !qvalid) G = f32x4{0.f, 0.f, 0.f, 0.f};
      PA_STORE4(gout_p, t, G);
      f32x4 Pd;
#pragma unroll
      for (int r = 0; r < 4; ++r) Pd[r] = P[t][r] > 0.f ? P[t][r] * dscale : 0.f;   // dscale == 1 without dropout
      if (EDGE && !qvalid) Pd = f32x4{0.f, 0.f, 0.f, 0.f};
      pa_s16x4 Gh, Gl, Ph, Pl;
      pa_split4(G, Gh, Gl);
      pa_split4(Pd, Ph, Pl);
      // transpose Pd and G through the wave's LDS patches: written [query][key], read [key][4 queries]
      *reinterpret_cast<pa_s16x4*>(pw + pwr) = Ph;
      *reinterpret_cast<pa_s16x4*>(pw + 256 + pwr) = Gh;
      // dQ^T += K^T . G^T : A = K[keys 16t + 4g..4g+3][d = c16 & 7] (rows d >= 8 of the result are never stored), B = G^T as it sits
      const pa_s16x4 ka = *reinterpret_cast<const pa_s16x4*>(sKT + (c16 & 7) * KSTR + t * 16 + 4 * g);
      dq = PA_MFMA16(ka, Gh, dq);
      dq = PA_MFMA16(ka, Gl, dq);
      pa_wave_sync();
      const pa_s16x4 aPh = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(pw + prd));
      const pa_s16x4 aGh = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(pw + 256 + prd));
      pa_wave_sync();   // (LDS operations of a wave complete in order: the low parts land after the reads above)
      *reinterpret_cast<pa_s16x4*>(pw + pwr) = Pl;
      *reinterpret_cast<pa_s16x4*>(pw + 256 + pwr) = Gl;
      pa_wave_sync();
      const pa_s16x4 aPl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(pw + prd));
      const pa_s16x4 aGl = __builtin_amdgcn_ds_read_tr16_b64_v4i16((pa_lds_s16x4*)(pw + 256 + prd));
      // dK / dV of key tile t: accumulator column = d (lanes c16 < 8), rows = keys 16t + 4g + r; the running sums of
      // this wave live in LDS and pass through the MFMA as its C operand.
      float* accK = redw + ((wave * NT + t) * 2 + 0) * 128 + (g * 8 + dcol) * 4;
      float* accV = accK + 128;
      f32x4 dKt = *reinterpret_cast<const f32x4*>(accK), dVt = *reinterpret_cast<const f32x4*>(accV);
      dVt = PA_MFMA16(aPh, bD, dVt);
      dKt = PA_MFMA16(aGh, bQ, dKt);
      dVt = PA_MFMA16(aPl, bD, dVt);
      dKt = PA_MFMA16(aGl, bQ, dKt);
      if (dlane) {
        *reinterpret_cast<f32x4*>(accK) = dKt;
        *reinterpret_cast<f32x4*>(accV) = dVt;
      }
      pa_wave_sync();   // the next tile overwrites the patches
    }
    // dQ^T accumulator: column = query, rows d = 4g + r (valid for g < 2)
    if (qvalid && g < 2) {
      uint2 pk;
      pk.x = (uint32_t)f2bf(dq[0] * scale) | ((uint32_t)f2bf(dq[1] * scale) << 16);
      pk.y = (uint32_t)f2bf(dq[2] * scale) | ((uint32_t)f2bf(dq[3] * scale) << 16);
      *reinterpret_cast<uint2*>(dqkv + ((long long)row0 + qi) * D3 + h * HD + 4 * g) = pk;
    }
  };
  PA_RUN_QUERY_BLOCKS();
  __syncthreads();
  for (int key = tid; key < rows; key += blockDim.x) {   // (packed: the representative pad row is no key -- its sums are the zeros they started as)
    const int t = key >> 4, kg = (key & 15) >> 2, r = key & 3;
    float a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, c2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int w = 0; w < nwaves; ++w) {
      const float* bk = redw + ((w * NT + t) * 2) * 128 + kg * 32 + r;
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        a[d] += bk[d * 4];
        c2[d] += bk[128 + d * 4];
      }
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) a[d] *= scale;     // dK = scale * G^T.Q  (Q sits unscaled in LDS)
    bf16_t* dst = dqkv + ((long long)row0 + key) * D3 + h * HD;
    store8_bf16(dst + D, a);
    store8_bf16(dst + 2 * D, c2);
  }
}


// compact planes (layout 3 / 7): one FULL instantiation per tile count, dense and ragged (RAG), with the wave count pa_bwd_nw gives that
// tile count -- the 34 rows a translation unit contributes to the backward's table for its gradient type GT (G16: 0 float, 1 __bf16)
#define PA_BWD_COMPACT_ROW(G16, GT, NT, NWV)                                                                              \
  KROW(pa_bwd_compact_key(G16, NT, 0), pair_attn_bwd_mfma_kernel<NT, true, true, NWV, false, _Float16, GT>),              \
  KROW(pa_bwd_compact_key(G16, NT, 1), pair_attn_bwd_mfma_kernel<NT, true, true, NWV, true, _Float16, GT>)
#define PA_BWD_COMPACT_TABLE(G16, GT)                                                                                                        \
  PA_BWD_COMPACT_ROW(G16, GT, 1, 4), PA_BWD_COMPACT_ROW(G16, GT, 2, 4), PA_BWD_COMPACT_ROW(G16, GT, 3, 3), PA_BWD_COMPACT_ROW(G16, GT, 4, 4),    \
  PA_BWD_COMPACT_ROW(G16, GT, 5, 3), PA_BWD_COMPACT_ROW(G16, GT, 6, 3), PA_BWD_COMPACT_ROW(G16, GT, 7, 4), PA_BWD_COMPACT_ROW(G16, GT, 8, 4),    \
  PA_BWD_COMPACT_ROW(G16, GT, 9, 3), PA_BWD_COMPACT_ROW(G16, GT, 10, 4), PA_BWD_COMPACT_ROW(G16, GT, 11, 4), PA_BWD_COMPACT_ROW(G16, GT, 12, 3), \
  PA_BWD_COMPACT_ROW(G16, GT, 13, 4), PA_BWD_COMPACT_ROW(G16, GT, 14, 4), PA_BWD_COMPACT_ROW(G16, GT, 15, 3), PA_BWD_COMPACT_ROW(G16, GT, 16, 3), \
  PA_BWD_COMPACT_ROW(G16, GT, 17, 3)
// the bf16-gradient rows (pair_attn_bwd_g16.hip)
extern KernelRow g_pa_bwd_compact_g16[PA_BWD_COMPACT_ROWS];

}  // namespace mmdti
