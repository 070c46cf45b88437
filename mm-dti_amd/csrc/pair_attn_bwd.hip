// pair_attn_bwd.hip -- backward of the pair-bias attention (see pair_attn.hip for the forward and the layouts).
#include "pair_attn_bwd_mfma.h"

namespace mmdti {

// DET (the deterministic mode): the four waves add their dK / dV partials one wave after the other instead of meeting in LDS atomics
template <int NCH, bool DET = false>
__global__ __launch_bounds__(256) void pair_attn_bwd_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ s,
                                                            const bf16_t* __restrict__ dO, float* __restrict__ g,
                                                            bf16_t* __restrict__ dqkv, int N, int H, int ld,
                                                            float scale, int g_in_zero, uint32_t thresh, float dscale,
                                                            uint64_t seed, uint32_t site) {
  __shared__ __attribute__((aligned(16))) float sq[NCH * 64][HD];
  __shared__ __attribute__((aligned(16))) float sdo[NCH * 64][HD];
  __shared__ __attribute__((aligned(16))) float red[NCH * 64][2 * HD];
  // (the 64 heads of a token share 128-byte q / k / v lines, 8 heads per line: keep a molecule's heads on one XCD)
  const int bh = xcd_chunk(blockIdx.x, gridDim.x), b = bh / H, h = bh - b * H;
  const int D = H * HD, D3 = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bf16_t* base = qkv + (long long)b * N * D3 + h * HD;
  for (int t = tid; t < NCH * 64; t += 256) {
    float q[8] = {0, 0, 0, 0, 0, 0, 0, 0}, d_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t < N) {
      load8_bf16(base + (long long)t * D3, q);
      load8_bf16(dO + ((long long)b * N + t) * D + h * HD, d_);
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      sq[t][d] = q[d];
      sdo[t][d] = d_[d];
      red[t][d] = 0.f;
      red[t][8 + d] = 0.f;
    }
  }
  float k[NCH][8], v[NCH][8], dk[NCH][8], dv[NCH][8];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = c * 64 + lane;
#pragma unroll
    for (int d = 0; d < 8; ++d) k[c][d] = v[c][d] = dk[c][d] = dv[c][d] = 0.f;
    if (j < N) {
      load8_bf16(base + (long long)j * D3 + D, k[c]);
      load8_bf16(base + (long long)j * D3 + 2 * D, v[c]);
    }
  }
  __syncthreads();
  const float NEG_INF = -INFINITY;
  // software pipeline over rows (see the forward kernel): S and G of row i+4 are in flight while row i is processed
  float ns[NCH], ng[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = c * 64 + lane;
    const bool ok = wave < N && j < N;
    ns[c] = ok ? s[((long long)bh * N + wave) * ld + j] : NEG_INF;
    ng[c] = (ok && !g_in_zero) ? g[((long long)bh * N + wave) * ld + j] : 0.f;
  }
  for (int i = wave; i < N; i += 4) {
    float q[8], dd[8];
    {
      const float4 a0 = *reinterpret_cast<const float4*>(&sq[i][0]), a1 = *reinterpret_cast<const float4*>(&sq[i][4]);
      const float4 b0 = *reinterpret_cast<const float4*>(&sdo[i][0]), b1 = *reinterpret_cast<const float4*>(&sdo[i][4]);
      q[0] = a0.x; q[1] = a0.y; q[2] = a0.z; q[3] = a0.w; q[4] = a1.x; q[5] = a1.y; q[6] = a1.z; q[7] = a1.w;
      dd[0] = b0.x; dd[1] = b0.y; dd[2] = b0.z; dd[3] = b0.w; dd[4] = b1.x; dd[5] = b1.y; dd[6] = b1.z; dd[7] = b1.w;
    }
    const long long rowoff = ((long long)bh * N + i) * ld;
    float p[NCH], dpp[NCH], pd[NCH], gin[NCH];
    float m = NEG_INF;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      p[c] = ns[c];
      gin[c] = ng[c];
      m = fmaxf(m, p[c]);
    }
    if (i + 4 < N) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const int j = c * 64 + lane;
        ns[c] = (j < N) ? s[rowoff + 4LL * ld + j] : NEG_INF;
        ng[c] = (j < N && !g_in_zero) ? g[rowoff + 4LL * ld + j] : 0.f;
      }
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      p[c] = __expf(p[c] - m);
      sum += p[c];
    }
    const float inv = 1.0f / wave_sum(sum);
    float dl = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      p[c] *= inv;
      float dp = 0.f;
#pragma unroll
      for (int d = 0; d < 8; ++d) dp += dd[d] * v[c][d];
      float keepscale = 1.f;
      if (thresh) {
        const int j = c * 64 + lane;
        keepscale = dropout_keep(seed, site, ((uint64_t)bh * N + i) * ld + j, thresh) ? dscale : 0.f;
      }
      dpp[c] = dp * keepscale;
      pd[c] = p[c] * keepscale;
      dl += dpp[c] * p[c];
    }
    dl = wave_sum(dl);
    float dq[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      const int j = c * 64 + lane;
      float gg = 0.f;
      if (j < N) {
        gg = p[c] * (dpp[c] - dl) + gin[c];
        g[rowoff + j] = gg;
      }
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        dq[d] += gg * k[c][d];
        dk[c][d] += gg * q[d];
        dv[c][d] += pd[c] * dd[d];
      }
    }
    const float tot = wave_sum8_scatter(dq, lane) * scale;
    if (lane < 8) dqkv[((long long)b * N + i) * D3 + h * HD + lane] = f2bf(tot);
  }
  // combine the 4 waves' dK / dV partials through LDS atomics
  if constexpr (DET) {
    for (int w = 0; w < 4; ++w) {        // (a lane owns key j of its wave's partial: plain adds, waves in order 0, 1, 2, 3)
      if (wave == w) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
          const int j = c * 64 + lane;
          if (j < N) {
#pragma unroll
            for (int d = 0; d < 8; ++d) {
              red[j][d] += dk[c][d] * scale;
              red[j][8 + d] += dv[c][d];
            }
          }
        }
      }
      __syncthreads();
    }
  } else {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int j = c * 64 + lane;
    if (j < N) {
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        atomicAdd(&red[j][d], dk[c][d] * scale);
        atomicAdd(&red[j][8 + d], dv[c][d]);
      }
    }
  }
  }
  __syncthreads();
  for (int t = tid; t < N; t += 256) {
    float a[8], c2[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      a[d] = red[t][d];
      c2[d] = red[t][8 + d];
    }
    bf16_t* dst = dqkv + ((long long)b * N + t) * D3 + h * HD;
    store8_bf16(dst + D, a);
    store8_bf16(dst + 2 * D, c2);
  }
}
}  // namespace mmdti
MMDTI_DEFINE_SALT_PULL(pair_attn_bwd)
using namespace mmdti;


// every MFMA instance of this translation unit, at the row its key gives it (pair_attn_plan.h): the compact planes with fp32 gradients
// (0..33) and the fp32 planes (68..87); rows 34..67 -- compact planes, bf16 gradients -- are pair_attn_bwd_g16.hip's
static KernelRow g_pa_bwd_compact_f32[PA_BWD_COMPACT_ROWS] = {PA_BWD_COMPACT_TABLE(0, float)};
// (per bucket: row-major on three and on four waves, tiled likewise, and the FULL form of the tile count that fills the bucket)
#define PA_BWD_F32_ROW(NT, NWFULL)                                                                                                          \
  KROW(pa_bwd_f32_key(pa_bucket(NT), 0, 0, 3), pair_attn_bwd_mfma_kernel<NT, false, false, 3, false, float, float>),                        \
  KROW(pa_bwd_f32_key(pa_bucket(NT), 0, 0, 4), pair_attn_bwd_mfma_kernel<NT, false, false, 4, false, float, float>),                        \
  KROW(pa_bwd_f32_key(pa_bucket(NT), 1, 0, 3), pair_attn_bwd_mfma_kernel<NT, true, false, 3, false, float, float>),                         \
  KROW(pa_bwd_f32_key(pa_bucket(NT), 1, 0, 4), pair_attn_bwd_mfma_kernel<NT, true, false, 4, false, float, float>),                         \
  KROW(pa_bwd_f32_key(pa_bucket(NT), 1, 1, NWFULL), pair_attn_bwd_mfma_kernel<NT, true, true, NWFULL, false, float, float>)
static KernelRow g_pa_bwd_f32[20] = {PA_BWD_F32_ROW(5, 3), PA_BWD_F32_ROW(9, 3), PA_BWD_F32_ROW(13, 4), PA_BWD_F32_ROW(17, 3)};
#undef PA_BWD_F32_ROW
static_assert(pa_bwd_nw(5) == 3 && pa_bwd_nw(9) == 3 && pa_bwd_nw(13) == 4 && pa_bwd_nw(17) == 3, "the FULL rows above carry pa_bwd_nw of their tile count");
static_assert(pa_bwd_nw(1) == 4 && pa_bwd_nw(2) == 4 && pa_bwd_nw(3) == 3 && pa_bwd_nw(4) == 4 && pa_bwd_nw(6) == 3 && pa_bwd_nw(7) == 4 && pa_bwd_nw(8) == 4 &&
                  pa_bwd_nw(10) == 4 && pa_bwd_nw(11) == 4 && pa_bwd_nw(12) == 3 && pa_bwd_nw(14) == 4 && pa_bwd_nw(15) == 3 && pa_bwd_nw(16) == 3,
              "PA_BWD_COMPACT_TABLE carries pa_bwd_nw of every tile count");
// the per-element kernels: the plain form, then the deterministic one
static KernelRow g_pa_bwd_elem[PA_BWD_ELEM_KERNELS] = {
    KROW(pa_bwd_elem_key(1, 0), pair_attn_bwd_kernel<1>),       KROW(pa_bwd_elem_key(2, 0), pair_attn_bwd_kernel<2>),       KROW(pa_bwd_elem_key(3, 0), pair_attn_bwd_kernel<3>),
    KROW(pa_bwd_elem_key(4, 0), pair_attn_bwd_kernel<4>),       KROW(pa_bwd_elem_key(5, 0), pair_attn_bwd_kernel<5>),       KROW(pa_bwd_elem_key(1, 1), pair_attn_bwd_kernel<1, true>),
    KROW(pa_bwd_elem_key(2, 1), pair_attn_bwd_kernel<2, true>), KROW(pa_bwd_elem_key(3, 1), pair_attn_bwd_kernel<3, true>), KROW(pa_bwd_elem_key(4, 1), pair_attn_bwd_kernel<4, true>),
    KROW(pa_bwd_elem_key(5, 1), pair_attn_bwd_kernel<5, true>),
};
static const KernelRow* pa_bwd_row(int family, int key) {
  if (family == PA_BWD_ELEM) return key >= 0 && key < PA_BWD_ELEM_KERNELS ? &g_pa_bwd_elem[key] : nullptr;
  if (key < 0 || key >= PA_BWD_MFMA_KERNELS) return nullptr;
  return key < PA_BWD_COMPACT_ROWS ? &g_pa_bwd_compact_f32[key] : key < 2 * PA_BWD_COMPACT_ROWS ? &g_pa_bwd_compact_g16[key - PA_BWD_COMPACT_ROWS] : &g_pa_bwd_f32[key - 2 * PA_BWD_COMPACT_ROWS];
}
// row `key` of a pair-attention table (PairAttnFamily), null past its end
const KernelRow* mmdti::pair_attn_kernel_row(int family, int key) {
  if (family == PA_BWD_MFMA || family == PA_BWD_ELEM) return pa_bwd_row(family, key);
  int n = 0;
  const KernelRow* t = (family == PA_FWD_MFMA || family == PA_FWD_ELEM) ? pair_attn_fwd_table(family, &n) : nullptr;
  return t && key >= 0 && key < n ? &t[key] : nullptr;
}

// What mmdti_pair_attn_bwd and mmdti_pair_attn_plan share: validate, plan.  Pointers are tested for null and alignment only.
static int pair_attn_bwd_prepare(PairAttnPlan& plan, const void* qkv_bf16, const void* s, const void* do_bf16, const void* g, const void* dqkv_bf16, int B,
                                 int N, int H, int ld, int layout, const void* key_tiles, const void* row_off, int qkv_f16, bool det) {
  // bit 0: tiled planes; bit 1: compact planes (s is fp16; tiled only); bit 2: g is bf16 (with bit 1 only)
  const int tiled = layout & 1, compact = (layout >> 1) & 1, g16 = (layout >> 2) & 1;
  if (int e = check_common("pair_attn_bwd", B, N, H, ld)) return e;
  MMDTI_REQUIRE((layout & ~7) == 0 && (!compact || tiled) && (!g16 || compact),
                "pair_attn_bwd: layout must be 0 (row-major fp32), 1 (tiled fp32), 3 (tiled, fp16 logits) or 7 (tiled, fp16 logits, bf16 gradients)");
  MMDTI_REQUIRE(!key_tiles || compact, "pair_attn_bwd: key_tiles (ragged batches) needs the compact planes (layout 3 or 7: tiled, fp16 logits)");
  MMDTI_REQUIRE(!row_off || key_tiles, "pair_attn_bwd: packed token rows (row_off) need key_tiles");
  MMDTI_REQUIRE(!tiled || (ld % 4 == 0 && N <= 16 * PA_MAX_NT), "pair_attn_bwd: the tiled pair layout needs ld %% 4 == 0 and N <= 272");
  MMDTI_REQUIRE(qkv_bf16 && s && do_bf16 && g && dqkv_bf16, "pair_attn_bwd: null pointer");
  MMDTI_REQUIRE(aligned16(qkv_bf16) && aligned16(do_bf16) && aligned16(dqkv_bf16), "pair_attn_bwd: alignment");
  MMDTI_REQUIRE(!tiled || (aligned16(s) && aligned16(g)), "pair_attn_bwd: tiled pair tensors must be 16-byte aligned");
  plan = pair_attn_bwd_plan(B, N, H, ld, tiled, compact, g16, aligned16(s) && aligned16(g), key_tiles != nullptr, det);
  MMDTI_REQUIRE(plan.family == PA_BWD_MFMA || !qkv_f16,
                "pair_attn_bwd: fp16 q | k | v are read by the MFMA kernels only (ld %% 4 == 0, N <= 272, 16-byte aligned pair tensors)");
  return MMDTI_OK;
}

extern "C" int mmdti_pair_attn_bwd(mmdti_stream_t stream, const void* qkv_bf16, const void* s, const void* do_bf16,
                                   void* g, void* dqkv_bf16, int B, int N, int H, int ld, float scale,
                                   int g_in_zero, float drop_p, unsigned long long seed, unsigned int site, int layout,
                                   const int* key_tiles, const int* row_off, int qkv_f16) {
  PairAttnPlan plan;
  if (int e = pair_attn_bwd_prepare(plan, qkv_bf16, s, do_bf16, g, dqkv_bf16, B, N, H, ld, layout, key_tiles, row_off, qkv_f16, det_table().on())) return e;
  // the per-element kernel: Philox words against p * 2^32; the MFMA kernel: the shared byte generator of common.h (as its forward)
  uint32_t th = plan.family == PA_BWD_MFMA ? dropout_thresh8(drop_p) : dropout_thresh(drop_p), site32 = site;
  float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
  uint64_t seed64 = seed;
  const KernelRow* row = pa_bwd_row(plan.family, plan.key);
  hipStream_t st = (hipStream_t)stream;
  if (plan.family == PA_BWD_MFMA) {
    void* args[] = {&qkv_bf16, &s, &do_bf16, &g, &g, &dqkv_bf16, &N, &H, &ld, &scale, &g_in_zero, &th, &sc, &seed64, &site32, &key_tiles, &row_off, &qkv_f16};
    (void)hipLaunchKernel(row->fn, dim3(plan.grid), dim3(plan.block), args, 0, st);
  } else {
    void* args[] = {&qkv_bf16, &s, &do_bf16, &g, &dqkv_bf16, &N, &H, &ld, &scale, &g_in_zero, &th, &sc, &seed64, &site32};
    (void)hipLaunchKernel(row->fn, dim3(plan.grid), dim3(plan.block), args, 0, st);
  }
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_pair_attn_plan(int backward, int deterministic, const void* qkv_bf16, const void* s, const void* o_or_do_bf16, const void* g,
                                    const void* dqkv_bf16, int B, int N, int H, int ld, float drop_p, int layout, const int* key_tiles,
                                    const int* row_off, int qkv_f16, int* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr, "pair_attn_plan: null plan_out");
  PairAttnPlan plan;
  if (backward) {
    if (int e = pair_attn_bwd_prepare(plan, qkv_bf16, s, o_or_do_bf16, g, dqkv_bf16, B, N, H, ld, layout, key_tiles, row_off, qkv_f16, deterministic != 0)) return e;
  } else {
    if (int e = pair_attn_fwd_prepare(plan, qkv_bf16, s, g, o_or_do_bf16, B, N, H, ld, drop_p, layout, key_tiles, row_off, qkv_f16)) return e;
  }
  static_assert(PAIR_ATTN_PLAN_INTS == 6, "mmdti_hip.h documents 6 ints");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}
