// Bandwidth-bound helpers of the fine-tune step: casts, dropout, column sums, embeddings, RoBERTa position ids,
// row softmax over materialised attention scores, masked pooling, GELU, sum of squares, Adam.
// All are simple streams; 16-byte accesses per lane wherever the layout allows (cdna guide G13).
#include "common.h"
#include <stdarg.h>
#include <stdio.h>

namespace mmdti {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---------------------------------------------------------------- casts / dropout / axpy
__device__ __forceinline__ bf16_t f2h16(float f) { return f2h_sat(f); }

// F16: the 16-bit output is fp16 (the fp16 forward-operand mode), else bf16
template <bool F16>
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y,
                                                            long long n4, long long n, uint32_t thresh, float dscale,
                                                            uint64_t seed, uint32_t site) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 v = reinterpret_cast<const float4*>(x)[i];
    float o[4] = {v.x, v.y, v.z, v.w};
    if (thresh) {
      Rand4 r = philox4(seed, site, (uint64_t)i);
      uint32_t rw[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = rw[e] >= thresh ? o[e] * dscale : 0.f;
    }
    uint2 pk;
    if (F16) {
      pk.x = (uint32_t)f2h16(o[0]) | ((uint32_t)f2h16(o[1]) << 16);
      pk.y = (uint32_t)f2h16(o[2]) | ((uint32_t)f2h16(o[3]) << 16);
    } else {
      pk.x = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
      pk.y = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
    }
    reinterpret_cast<uint2*>(y)[i] = pk;
  }
  // tail (n % 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    long long i = (n & ~3LL) + threadIdx.x;
    float o = x[i];
    if (thresh) o = dropout_keep(seed, site, (uint64_t)i, thresh) ? o * dscale : 0.f;
    y[i] = F16 ? f2h16(o) : f2bf(o);
  }
}

// fp16 -> bf16 (round to nearest even), rows of `cols` elements (cols % 8 == 0) with a source row stride: the backward GEMMs of
// the fp16 forward-operand mode take the saved forward activations as bf16
__global__ __launch_bounds__(256) void cast_f16_bf16_kernel(const bf16_t* __restrict__ x, int cols8, int ldx, bf16_t* __restrict__ y, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const long long row = i / cols8;
    const int c = (int)(i - row * cols8) * 8;
    const uint4 u = *reinterpret_cast<const uint4*>(x + row * ldx + c);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    uint32_t o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] & 0xffffu)), hi = (float)__builtin_bit_cast(_Float16, (uint16_t)(w[e] >> 16));
      o[e] = (uint32_t)f2bf(lo) | ((uint32_t)f2bf(hi) << 16);
    }
    *reinterpret_cast<uint4*>(y + row * (long long)cols8 * 8 + c) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = bf2f(x[i]);
}

__global__ __launch_bounds__(256) void dropout_f32_kernel(const float* __restrict__ x, float* __restrict__ y, long long n,
                                                          uint32_t thresh, float dscale, uint64_t seed, uint32_t site) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float o = x[i];
    if (thresh) o = dropout_keep(seed, site, (uint64_t)i, thresh) ? o * dscale : 0.f;
    y[i] = o;
  }
}

__global__ __launch_bounds__(256) void axpy_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, float a) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] += a * x[i];
}

__global__ __launch_bounds__(256) void gelu_bf16_kernel(const bf16_t* __restrict__ u, bf16_t* __restrict__ y, long long n) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
    y[i] = f2bf(gelu_erf(bf2f(u[i])));
}

// ---------------------------------------------------------------- column sum (bias gradients)
// block = 256 threads: 32 column-chunks(8 cols each, 16 B) x 8 row lanes; grid.x over column groups of 256, grid.y rows
// SLAB (the deterministic mode): row group blockIdx.y stores its sums to row blockIdx.y of `out` ([gridDim.y][cols]); det_fold_kernel adds them
template <bool SLAB>
__device__ __forceinline__ void colsum_bf16_body(const bf16_t* __restrict__ x, int rows, int cols, int ld, float* __restrict__ out) {
  __shared__ float red[8][256 + 8];
  const int cc = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 256 + cc * 8;
  float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c0 < cols) {
    const int rstep = gridDim.y * 8;
    int r = blockIdx.y * 8 + rl;
    if (c0 + 8 <= cols) {
      // 4 rows per iteration: four independent 16-byte loads in flight per lane
      for (; r + 3 * rstep < rows; r += 4 * rstep) {
        uint4 u[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = *reinterpret_cast<const uint4*>(x + (long long)(r + k * rstep) * ld + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t w[4] = {u[k].x, u[k].y, u[k].z, u[k].w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            acc[2 * i] += __uint_as_float(w[i] << 16);
            acc[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u);
          }
        }
      }
      for (; r < rows; r += rstep) {
        const uint4 u = *reinterpret_cast<const uint4*>(x + (long long)r * ld + c0);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          acc[2 * i] += __uint_as_float(w[i] << 16);
          acc[2 * i + 1] += __uint_as_float(w[i] & 0xffff0000u);
        }
      }
    } else {
      for (; r < rows; r += rstep) {
        const bf16_t* p = x + (long long)r * ld + c0;
        for (int i = 0; i < cols - c0; ++i) acc[i] += bf2f(p[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) red[rl][cc * 8 + i] = acc[i];
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < cols) {
    float s = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) s += red[r][threadIdx.x];
    if (SLAB) out[(long long)blockIdx.y * cols + c] = s;
    else atomicAdd(out + c, s);
  }
}
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ x, int rows, int cols, int ld,
                                                          float* __restrict__ out) {
  colsum_bf16_body<false>(x, rows, cols, ld, out);
}
__global__ __launch_bounds__(256) void colsum_bf16_slab_kernel(const bf16_t* __restrict__ x, int rows, int cols, int ld,
                                                               float* __restrict__ slab) {
  colsum_bf16_body<true>(x, rows, cols, ld, slab);
}

// ---------------------------------------------------------------- embeddings
__global__ __launch_bounds__(256) void embedding_fwd_kernel(const long long* __restrict__ ids, const float* __restrict__ table,
                                                            long long n, int D4, int vocab, float* __restrict__ out, int accumulate) {
  const long long total = n * D4;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long i = t / D4;
    const int c = (int)(t - i * D4);
    long long id = ids[i];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    float4 v = reinterpret_cast<const float4*>(table)[id * D4 + c];
    if (accumulate) {
      float4 o = reinterpret_cast<float4*>(out)[t];
      v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
    }
    reinterpret_cast<float4*>(out)[t] = v;
  }
}

__global__ __launch_bounds__(256) void embedding_bwd_kernel(const long long* __restrict__ ids, const float* __restrict__ dout,
                                                            long long n, int D, int vocab, long long padding_idx,
                                                            float* __restrict__ dtable) {
  const long long total = n * D;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long i = t / D;
    const int c = (int)(t - i * D);
    long long id = ids[i];
    if (id == padding_idx || id < 0 || id >= vocab) continue;
    atomicAdd(dtable + id * D + c, dout[t]);
  }
}

// The deterministic mode's form: workgroup (column chunk, part) owns the table rows with id % parts == part and walks the tokens in
// token order -- one adder per table element, a fixed order (the ids are wave-uniform loads; only matching tokens touch memory).
__global__ __launch_bounds__(256) void embedding_bwd_ordered_kernel(const long long* __restrict__ ids, const float* __restrict__ dout,
                                                                    long long n, int D, int vocab, long long padding_idx,
                                                                    float* __restrict__ dtable) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int parts = gridDim.y, part = blockIdx.y;
  if (c >= D) return;
  for (long long i = 0; i < n; ++i) {
    const long long id = ids[i];
    if (id == padding_idx || id < 0 || id >= vocab || (int)(id % parts) != part) continue;
    dtable[id * D + c] += dout[i * D + c];
  }
}

// word + position + token-type embeddings summed in one pass (HF RobertaEmbeddings.forward, modeling_roberta.py:75-122): one
// 16-byte store per element instead of a store and two read-modify-write passes.  ids_c == null: row 0 of table_c (token type 0).
__global__ __launch_bounds__(256) void embedding_fwd3_kernel(const long long* __restrict__ ids_a, const float* __restrict__ ta, int va,
                                                             const long long* __restrict__ ids_b, const float* __restrict__ tb, int vb,
                                                             const long long* __restrict__ ids_c, const float* __restrict__ tc, int vc,
                                                             long long n, int D4, float* __restrict__ out) {
  const long long total = n * D4;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long i = t / D4;
    const int c = (int)(t - i * D4);
    long long ia = ids_a[i], ib = ids_b[i], ic = ids_c ? ids_c[i] : 0;
    ia = ia < 0 ? 0 : (ia >= va ? va - 1 : ia);
    ib = ib < 0 ? 0 : (ib >= vb ? vb - 1 : ib);
    ic = ic < 0 ? 0 : (ic >= vc ? vc - 1 : ic);
    const float4 a = reinterpret_cast<const float4*>(ta)[ia * D4 + c], b = reinterpret_cast<const float4*>(tb)[ib * D4 + c],
                 d = reinterpret_cast<const float4*>(tc)[ic * D4 + c];
    reinterpret_cast<float4*>(out)[t] = make_float4(a.x + b.x + d.x, a.y + b.y + d.y, a.z + b.z + d.z, a.w + b.w + d.w);   // (a + b) + c, the reference's order
  }
}

// one-hot rows (bf16) for the embedding backward GEMM: thread per 8-column chunk
__global__ __launch_bounds__(256) void onehot_bf16_kernel(const long long* __restrict__ ids, long long n, int vocab, int ld8,
                                                          long long padding_idx, bf16_t* __restrict__ out) {
  const long long total = n * ld8;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const long long i = t / ld8;
    const int c0 = (int)(t - i * ld8) * 8;
    const long long id = ids[i];
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (id != padding_idx && id >= 0 && id < vocab && id >= c0 && id < c0 + 8) {
      const int e = (int)(id - c0);
      w[e >> 1] = (e & 1) ? 0x3F800000u : 0x00003F80u;   // bf16(1.0) = 0x3F80
    }
    reinterpret_cast<uint4*>(out)[t] = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// one wave per sequence: inclusive scan of (ids != pad) across the row in chunks of 64
__global__ __launch_bounds__(64) void roberta_posids_kernel(const long long* __restrict__ ids, int L, long long pad,
                                                            long long* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int carry = 0;
  for (int l0 = 0; l0 < L; l0 += 64) {
    const int l = l0 + lane;
    const int m = (l < L && ids[(long long)b * L + l] != pad) ? 1 : 0;
    int s = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      int t = __shfl_up(s, o, 64);
      if (lane >= o) s += t;
    }
    if (l < L) out[(long long)b * L + l] = (long long)((carry + s) * m) + pad;
    carry += __shfl(s, 63, 64);
  }
}

// ---------------------------------------------------------------- row softmax over materialised scores
// one wave per row, 4 consecutive keys per lane (16-byte score loads, 8-byte bf16 stores); ld % 8 == 0, ld <= 1024.
// Dropout element index = row*ld + key (ld-based so that a lane's 4 keys share one RNG call).
template <int NV>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* __restrict__ s, const float* __restrict__ key_add,
                                                          bf16_t* __restrict__ p_out, bf16_t* __restrict__ pd_out,
                                                          long long rows, int heads, int Lq, int Lk, int ld, uint32_t thresh,
                                                          float dscale, uint64_t seed, uint32_t site) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = (int)(row / ((long long)heads * Lq));
  const float* sr = s + row * ld;
  const float* ka = key_add ? key_add + (long long)b * Lk : nullptr;
  float v[NV][4];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int j = (c * 64 + lane) * 4;
    float4 t = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (j < ld) t = *reinterpret_cast<const float4*>(sr + j);
    const float tv[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[c][e] = (j + e < Lk) ? tv[e] + (ka ? ka[j + e] : 0.f) : -INFINITY;
      m = fmaxf(m, v[c][e]);
    }
  }
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < NV; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[c][e] = __expf(v[c][e] - m);   // exp(-inf) = 0 in the pad columns
      sum += v[c][e];
    }
  const float inv = 1.0f / wave_sum(sum);
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int j = (c * 64 + lane) * 4;
    if (j >= ld) continue;
    float p[4] = {v[c][0] * inv, v[c][1] * inv, v[c][2] * inv, v[c][3] * inv};
    uint2 pk;
    pk.x = (uint32_t)f2bf(p[0]) | ((uint32_t)f2bf(p[1]) << 16);
    pk.y = (uint32_t)f2bf(p[2]) | ((uint32_t)f2bf(p[3]) << 16);
    *reinterpret_cast<uint2*>(p_out + row * ld + j) = pk;
    if (pd_out != p_out) {
      if (thresh) {
        const Rand4 r = philox4(seed, site, (uint64_t)(row * ld + j) >> 2);
        p[0] = r.x >= thresh ? p[0] * dscale : 0.f; p[1] = r.y >= thresh ? p[1] * dscale : 0.f;
        p[2] = r.z >= thresh ? p[2] * dscale : 0.f; p[3] = r.w >= thresh ? p[3] * dscale : 0.f;
      }
      pk.x = (uint32_t)f2bf(p[0]) | ((uint32_t)f2bf(p[1]) << 16);
      pk.y = (uint32_t)f2bf(p[2]) | ((uint32_t)f2bf(p[3]) << 16);
      *reinterpret_cast<uint2*>(pd_out + row * ld + j) = pk;
    }
  }
}

template <int NV>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const bf16_t* __restrict__ p_in, const float* __restrict__ dp,
                                                          bf16_t* __restrict__ ds, long long rows, int Lk, int ld, float scale,
                                                          uint32_t thresh, float dscale, uint64_t seed, uint32_t site) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float p[NV][4], d[NV][4];
  float dl = 0.f;
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int j = (c * 64 + lane) * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) p[c][e] = d[c][e] = 0.f;
    if (j < ld) {
      const uint2 pk = *reinterpret_cast<const uint2*>(p_in + row * ld + j);
      const float4 t = *reinterpret_cast<const float4*>(dp + row * ld + j);
      p[c][0] = __uint_as_float(pk.x << 16); p[c][1] = __uint_as_float(pk.x & 0xffff0000u);
      p[c][2] = __uint_as_float(pk.y << 16); p[c][3] = __uint_as_float(pk.y & 0xffff0000u);
      d[c][0] = t.x; d[c][1] = t.y; d[c][2] = t.z; d[c][3] = t.w;
      if (thresh) {
        const Rand4 r = philox4(seed, site, (uint64_t)(row * ld + j) >> 2);
        d[c][0] = r.x >= thresh ? d[c][0] * dscale : 0.f; d[c][1] = r.y >= thresh ? d[c][1] * dscale : 0.f;
        d[c][2] = r.z >= thresh ? d[c][2] * dscale : 0.f; d[c][3] = r.w >= thresh ? d[c][3] * dscale : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (j + e >= Lk) p[c][e] = d[c][e] = 0.f;   // pad columns of dp are not data
        dl += p[c][e] * d[c][e];
      }
    }
  }
  dl = wave_sum(dl);
#pragma unroll
  for (int c = 0; c < NV; ++c) {
    const int j = (c * 64 + lane) * 4;
    if (j >= ld) continue;
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = scale * p[c][e] * (d[c][e] - dl);
    uint2 pk;
    pk.x = (uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16);
    pk.y = (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16);
    *reinterpret_cast<uint2*>(ds + row * ld + j) = pk;
  }
}

// ---------------------------------------------------------------- masked pooling (mm_model.py:572-576)
// pooled[b] = mean over the unmasked rows of [a[b]; t[b]].  grid (B, D/64): a block owns 64 columns (16 float4 lanes) and
// spreads the Na+Nt rows over 16 row groups -- 8x the workgroups of a block-per-molecule layout, 16-byte loads.
__device__ __forceinline__ int masked_pool_count(const unsigned char* ma, const unsigned char* mt, int Na, int Nt, int* cnt) {
  if (threadIdx.x == 0) *cnt = 0;
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < Na + Nt; i += 256) c += (i < Na ? ma[i] : mt[i - Na]) ? 1 : 0;
  if (c) atomicAdd(cnt, c);
  __syncthreads();
  return *cnt;
}

__global__ __launch_bounds__(256) void masked_pool_fwd_kernel(const float* __restrict__ a, const float* __restrict__ t,
                                                              const unsigned char* __restrict__ ma, const unsigned char* __restrict__ mt,
                                                              int Na, int Nt, int D, float* __restrict__ pooled) {
  const int b = blockIdx.x;
  __shared__ int cnt;
  __shared__ float4 red[16][16];
  const int n = masked_pool_count(ma + (long long)b * Na, mt + (long long)b * Nt, Na, Nt, &cnt);
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int col = blockIdx.y * 64 + cl * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < D) {
    for (int i = rg; i < Na + Nt; i += 16) {
      const bool in_a = i < Na;
      const bool on = in_a ? ma[(long long)b * Na + i] : mt[(long long)b * Nt + (i - Na)];
      if (!on) continue;
      const float* src = in_a ? a + ((long long)b * Na + i) * D : t + ((long long)b * Nt + (i - Na)) * D;
      const float4 v = *reinterpret_cast<const float4*>(src + col);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && col < D) {
#pragma unroll
    for (int r = 1; r < 16; ++r) {
      const float4 v = red[r][cl];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float inv = 1.0f / (float)n;
    *reinterpret_cast<float4*>(pooled + (long long)b * D + col) = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
  }
}

// grid (B, 8): block (b, y) writes rows y, y+8, ... of da / dt, one float4 per thread per step
__global__ __launch_bounds__(256) void masked_pool_bwd_kernel(const float* __restrict__ dp, const unsigned char* __restrict__ ma,
                                                              const unsigned char* __restrict__ mt, int Na, int Nt, int D,
                                                              float* __restrict__ da, float* __restrict__ dt) {
  const int b = blockIdx.x;
  __shared__ int cnt;
  const float inv = 1.0f / (float)masked_pool_count(ma + (long long)b * Na, mt + (long long)b * Nt, Na, Nt, &cnt);
  const int nv = D >> 2;
  for (int i = blockIdx.y; i < Na + Nt; i += gridDim.y) {
    const bool in_a = i < Na;
    const bool on = in_a ? ma[(long long)b * Na + i] : mt[(long long)b * Nt + (i - Na)];
    float* dst = in_a ? da + ((long long)b * Na + i) * D : dt + ((long long)b * Nt + (i - Na)) * D;
    for (int c = threadIdx.x; c < nv; c += 256) {
      float4 g = *reinterpret_cast<const float4*>(dp + (long long)b * D + c * 4);
      g = on ? make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(dst + c * 4) = g;
    }
  }
}

// Packed token rows (see mmdti_masked_pool_packed_fwd): only a sequence's real rows enter; no masks to read.
__global__ __launch_bounds__(256) void masked_pool_packed_fwd_kernel(const float* __restrict__ a, const float* __restrict__ t,
                                                                     const int* __restrict__ a_off, const int* __restrict__ a_cnt,
                                                                     const int* __restrict__ t_off, const int* __restrict__ t_cnt, int D,
                                                                     float* __restrict__ pooled) {
  const int b = blockIdx.x;
  __shared__ float4 red[16][16];
  const int na = a_cnt[b], nt = t_cnt[b];
  const float* pa = a + (long long)a_off[b] * D;
  const float* pt = t + (long long)t_off[b] * D;
  const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int col = blockIdx.y * 64 + cl * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < D) {
    for (int i = rg; i < na + nt; i += 16) {
      const float* src = i < na ? pa + (long long)i * D : pt + (long long)(i - na) * D;
      const float4 v = *reinterpret_cast<const float4*>(src + col);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  red[rg][cl] = s;
  __syncthreads();
  if (rg == 0 && col < D) {
#pragma unroll
    for (int r = 1; r < 16; ++r) {
      const float4 v = red[r][cl];
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    const float inv = 1.0f / (float)(na + nt);
    *reinterpret_cast<float4*>(pooled + (long long)b * D + col) = make_float4(s.x * inv, s.y * inv, s.z * inv, s.w * inv);
  }
}
// one float4 per thread: rows of da (first rows_a rows of the index space), then rows of dt
__global__ __launch_bounds__(256) void masked_pool_packed_bwd_kernel(const float* __restrict__ dp, const int* __restrict__ a_off,
                                                                     const int* __restrict__ a_cnt, const int* __restrict__ a_seq, int rows_a,
                                                                     const int* __restrict__ t_off, const int* __restrict__ t_cnt,
                                                                     const int* __restrict__ t_seq, int rows_t, int D, float* __restrict__ da,
                                                                     float* __restrict__ dt) {
  const int nv = D >> 2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = idx / nv;
  if (row >= (long long)rows_a + rows_t) return;
  const int c = (int)(idx - row * nv) * 4;
  const bool in_a = row < rows_a;
  const int r = in_a ? (int)row : (int)(row - rows_a);
  const int b = in_a ? a_seq[r] : t_seq[r];
  const bool on = in_a ? (r - a_off[b] < a_cnt[b]) : (r - t_off[b] < t_cnt[b]);
  const float inv = on ? 1.0f / (float)(a_cnt[b] + t_cnt[b]) : 0.f;
  const float4 g = *reinterpret_cast<const float4*>(dp + (long long)b * D + c);
  float* dst = (in_a ? da : dt) + (long long)r * D + c;
  *reinterpret_cast<float4*>(dst) = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
}

// ---------------------------------------------------------------- sum of squares / Adam
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long long n, float* __restrict__ out) {
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += g[i] * g[i];
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}
// The reproducible form (a workspace is given): 16-byte loads, one partial per workgroup, and the partials folded in a FIXED order by
// sumsq_fold_kernel -- the gradient norm, and with it the clip coefficient of every Adam step, is the same to the bit from run to run
// (the atomic form above differs in the last bit, and a training trajectory with it).  At most SUMSQ_WGS partials (stream_plan.h).
// CHECK: the same pass also counts the non-finite gradient elements (the found-inf test of GradScaler.unscale_) -- one per-workgroup count
// next to each partial.  Inf / NaN is told by the exponent bits, which no fast-math flag can fold away (a `x != x` test can vanish).  The
// float arithmetic is the same statement sequence in both instantiations: the sum is the same to the bit with or without the check.
__device__ __forceinline__ unsigned nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
template <bool CHECK>
__global__ __launch_bounds__(256) void sumsq_part_kernel(const float* __restrict__ g, long long n, float* __restrict__ part,
                                                         unsigned* __restrict__ cnt) {
  const long long n4 = n >> 2;
  const float4* g4 = reinterpret_cast<const float4*>(g);
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  unsigned c = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    const float4 v = g4[i];
    a.x += v.x * v.x; a.y += v.y * v.y; a.z += v.z * v.z; a.w += v.w * v.w;
    if constexpr (CHECK) c += nonfinite(v.x) + nonfinite(v.y) + nonfinite(v.z) + nonfinite(v.w);
  }
  float s = (a.x + a.y) + (a.z + a.w);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const float v = g[(n4 << 2) + threadIdx.x];
    s += v * v;
    if constexpr (CHECK) c += nonfinite(v);
  }
  s = wave_sum(s);
  __shared__ float red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  if constexpr (CHECK) {
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __shared__ unsigned cred[4];
    if ((threadIdx.x & 63) == 0) cred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = cred[0] + cred[1] + cred[2] + cred[3];
  } else {
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// Adam's bias corrections for step t: 1 - beta1^t and sqrt(1 - beta2^t) -- ONE device expression for the step state and the guard
__device__ __forceinline__ void adam_bias_dev(float b1, float b2, float t, float* bc1, float* bc2_sqrt) {
  *bc1 = 1.f - powf(b1, t);
  *bc2_sqrt = sqrtf(1.f - powf(b2, t));
}
// Non-finite guard state (device, fp32): NF_T = optimizer steps actually taken, NF_SKIPPED = steps skipped, NF_FLAG = this step is
// skipped (1) or not (0), NF_BC1 / NF_BC2 = the bias corrections 1-beta1^t, sqrt(1-beta2^t) of the taken step t.
enum { NF_T = 0, NF_SKIPPED = 1, NF_FLAG = 2, NF_BC1 = 3, NF_BC2 = 4 };
// CHECK: out[1] = the non-finite count; with a guard, out[2] = this step's skip flag and the guard advances (one thread, after the
// fold): a clean step takes t+1 and its bias corrections -- from bias_table[2(t-1) ..] (host powf, what mmdti_adam_step computes
// by value) or, without a table, from the device expression of step_state_advance_kernel.
template <bool CHECK>
__global__ __launch_bounds__(256) void sumsq_fold_kernel(const float* __restrict__ part, int np, float* __restrict__ out,
                                                         const unsigned* __restrict__ cnt, float* __restrict__ guard,
                                                         const float* __restrict__ bias_table, int table_steps, float b1, float b2) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < np; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __shared__ unsigned cred[CHECK ? 256 : 1];
  if constexpr (CHECK) {
    unsigned c = 0;
    for (int i = threadIdx.x; i < np; i += 256) c += cnt[i];
    cred[threadIdx.x] = c;
  }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      if constexpr (CHECK) cred[threadIdx.x] += cred[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    *out += red[0];
    if constexpr (CHECK) {
      out[1] = (float)cred[0];
      if (guard) {
        const bool skip = cred[0] != 0;
        out[2] = skip ? 1.f : 0.f;
        guard[NF_FLAG] = skip ? 1.f : 0.f;
        if (skip) {
          guard[NF_SKIPPED] += 1.f;
        } else {
          const float t = guard[NF_T] + 1.f;
          guard[NF_T] = t;
          if (bias_table) {
            const int i = min((int)t, table_steps) - 1;      // (the host sizes the table to every step it has enqueued)
            guard[NF_BC1] = bias_table[2 * i];
            guard[NF_BC2] = bias_table[2 * i + 1];
          } else {
            adam_bias_dev(b1, b2, t, &guard[NF_BC1], &guard[NF_BC2]);
          }
        }
      }
    }
  }
}

// Step state kept on the device so that a whole training step can be replayed from a captured HIP graph (host-side
// counters would be frozen into the graph): st[0] = optimizer steps taken, st[1] = learning rate of THIS step (HF linear
// warm-up / decay, transformers.get_linear_schedule_with_warmup as tasks/trainer.py:161-162 uses it), st[2] = 1 - beta1^t,
// st[3] = sqrt(1 - beta2^t); salt = the per-step dropout salt (mmdti_seed_salt_pull copies it into every kernel library).
__global__ void step_state_advance_kernel(float* __restrict__ st, unsigned long long* __restrict__ salt, float base_lr, int warmup, int total,
                                          float b1, float b2) {
  const int k = (int)st[0];                      // scheduler steps already taken: the schedule's lambda(k) is this step's rate
  const float lam = k < warmup ? (float)k / (float)max(1, warmup) : fmaxf(0.f, (float)(total - k) / (float)max(1, total - warmup));
  const float t = (float)(k + 1);
  st[0] = t;
  st[1] = base_lr * lam;
  adam_bias_dev(b1, b2, t, &st[2], &st[3]);
  unsigned long long x = *salt + 0x9E3779B97F4A7C15ull;       // splitmix64: a fresh, well-mixed word per step
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  *salt = x;
  salt[1] = z ^ (z >> 31);
}

// GUARD: the non-finite guard of sumsq_fold_kernel<true> decides -- a skipped step leaves before anything is read or written,
// a taken one uses the guard's bias corrections (of the steps actually taken).  The unguarded instantiation is the plain Adam pass.
// MASK: skip[i / 8] != 0 leaves element i alone (p, m, v and both shadows): parameters frozen after the arena was built.  Arena
// offsets are multiples of 8, so a group of 8 elements never straddles two parameters.  Only mmdti_adam_step_masked instantiates it.
template <bool GUARD, bool MASK = false>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, bf16_t* __restrict__ pb, bf16_t* __restrict__ ph, long long n, float lr, float b1,
                                                   float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                   const float* __restrict__ gscale, const float* __restrict__ state,
                                                   const float* __restrict__ guard, const unsigned char* __restrict__ skip = nullptr) {
  if constexpr (GUARD) {
    if (guard[NF_FLAG] != 0.f) return;
  }
  const float gs = gscale ? *gscale : 1.0f;
  if (state) {               // device-resident schedule (graph replay): this step's rate and bias corrections
    lr = state[1];
    bc1 = state[2];
    bc2_sqrt = state[3];
  }
  if constexpr (GUARD) {
    bc1 = guard[NF_BC1];
    bc2_sqrt = guard[NF_BC2];
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    if constexpr (MASK) {
      if (skip[i >> 3]) continue;
    }
    float gi = g[i] * gs;
    float pi = p[i];
    if (wd != 0.f) gi += wd * pi;
    float mi = b1 * m[i] + (1.f - b1) * gi;
    float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    pi -= (lr / bc1) * mi / denom;
    p[i] = pi;
    if (pb) pb[i] = f2bf(pi);
    if (ph) ph[i] = f2h_sat(pi);      // the fp16 shadow the forward GEMMs read (fp16 forward-operand mode)
  }
}

// One element of the grouped pass.  Every rounding point is spelt (no contraction left to the backend) as the backend forms adam_kernel's
// statements: gi = fma(wd, p, g gs); m = fma(b1, m, (1 - b1) gi); v = fma(b2, v, ((1 - b2) gi) gi); p - ((lr / bc1) m) / denom.  With
// lr_scale == 1 and one weight decay the coupled form therefore EQUALS adam_kernel to the bit (tests/test_adam_group_instances_gpu.py).
// DECOUPLED (torch.optim.AdamW): p *= 1 - lr_i wd_i first -- three roundings of their own -- and the moments see g alone.
template <bool DECOUPLED>
__device__ __forceinline__ void adam_group_elem(float& pi, float g, float& mi, float& vi, float gs, float lr_i, float wd_i, float step_size,
                                                float b1, float b2, float ob1, float ob2, float eps, float bc2_sqrt) {
#pragma clang fp contract(off)
  float gi = g * gs;
  if constexpr (DECOUPLED) {
    const float lw = lr_i * wd_i;
    const float keep = 1.f - lw;
    pi = pi * keep;
  } else {
    if (wd_i != 0.f) gi = __builtin_fmaf(wd_i, pi, gi);
  }
  const float mg = ob1 * gi;
  mi = __builtin_fmaf(b1, mi, mg);
  const float vg = ob2 * gi;
  const float vgg = vg * gi;
  vi = __builtin_fmaf(b2, vi, vgg);
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  const float num = step_size * mi;
  pi = pi - num / denom;
}

// The Adam pass with parameter groups: group[i / 8] names the group of element i (arena offsets are multiples of 8: a block of 8 never
// straddles two parameters; an id >= ngroups counts as ngroups - 1), table[2 gid] = the group's learning-rate scale, table[2 gid + 1] its
// weight decay -- coupled (added to the gradient, torch.optim.Adam) or DECOUPLED (torch.optim.AdamW).  One thread per block of 8: one byte
// and two table words (<= 2 KB, cached), then p, g, m, v as two 16-byte vectors each and each 16-bit shadow as one 16-byte store; the
// ragged last block goes element by element.  GUARD / MASK as in adam_kernel.  lr_scale == 0: m and v advance (torch with lr = 0), p and
// both shadows are not stored at all -- they keep their bits.
template <bool GUARD, bool MASK, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_group_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, bf16_t* __restrict__ pb, bf16_t* __restrict__ ph, long long n, float lr,
                                                         float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                         const float* __restrict__ gscale, const float* __restrict__ state,
                                                         const float* __restrict__ guard, const unsigned char* __restrict__ skip,
                                                         const unsigned char* __restrict__ group, const float* __restrict__ table, int ngroups) {
  if constexpr (GUARD) {
    if (guard[NF_FLAG] != 0.f) return;
  }
  const float gs = gscale ? *gscale : 1.0f;
  if (state) {
    lr = state[1];
    bc1 = state[2];
    bc2_sqrt = state[3];
  }
  if constexpr (GUARD) {
    bc1 = guard[NF_BC1];
    bc2_sqrt = guard[NF_BC2];
  }
  const float ob1 = 1.f - b1, ob2 = 1.f - b2;
  const long long nblk = (n + 7) >> 3;
  for (long long blk = (long long)blockIdx.x * 256 + threadIdx.x; blk < nblk; blk += (long long)gridDim.x * 256) {
    if constexpr (MASK) {
      if (skip[blk]) continue;
    }
    const int gid = min((int)group[blk], ngroups - 1);
    const float s = table[2 * gid], wd_i = table[2 * gid + 1];
    const float lr_i = lr * s;
    const float step_size = lr_i / bc1;
    const long long i0 = blk << 3;
    if (i0 + 8 <= n) {
      float pe[8], ge[8], me[8], ve[8];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const float4 p4 = reinterpret_cast<const float4*>(p + i0)[h], g4 = reinterpret_cast<const float4*>(g + i0)[h];
        const float4 m4 = reinterpret_cast<const float4*>(m + i0)[h], v4 = reinterpret_cast<const float4*>(v + i0)[h];
        pe[4 * h] = p4.x; pe[4 * h + 1] = p4.y; pe[4 * h + 2] = p4.z; pe[4 * h + 3] = p4.w;
        ge[4 * h] = g4.x; ge[4 * h + 1] = g4.y; ge[4 * h + 2] = g4.z; ge[4 * h + 3] = g4.w;
        me[4 * h] = m4.x; me[4 * h + 1] = m4.y; me[4 * h + 2] = m4.z; me[4 * h + 3] = m4.w;
        ve[4 * h] = v4.x; ve[4 * h + 1] = v4.y; ve[4 * h + 2] = v4.z; ve[4 * h + 3] = v4.w;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        adam_group_elem<DECOUPLED>(pe[e], ge[e], me[e], ve[e], gs, lr_i, wd_i, step_size, b1, b2, ob1, ob2, eps, bc2_sqrt);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        reinterpret_cast<float4*>(m + i0)[h] = make_float4(me[4 * h], me[4 * h + 1], me[4 * h + 2], me[4 * h + 3]);
        reinterpret_cast<float4*>(v + i0)[h] = make_float4(ve[4 * h], ve[4 * h + 1], ve[4 * h + 2], ve[4 * h + 3]);
      }
      if (s != 0.f) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
          reinterpret_cast<float4*>(p + i0)[h] = make_float4(pe[4 * h], pe[4 * h + 1], pe[4 * h + 2], pe[4 * h + 3]);
        if (pb) {
          uint32_t w[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = (uint32_t)f2bf(pe[2 * k]) | ((uint32_t)f2bf(pe[2 * k + 1]) << 16);
          *reinterpret_cast<uint4*>(pb + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (ph)
          *reinterpret_cast<uint4*>(ph + i0) =
              make_uint4(f2h_sat2(pe[0], pe[1]), f2h_sat2(pe[2], pe[3]), f2h_sat2(pe[4], pe[5]), f2h_sat2(pe[6], pe[7]));
      }
    } else {
      for (long long i = i0; i < n; ++i) {
        float pi = p[i], mi = m[i], vi = v[i];
        adam_group_elem<DECOUPLED>(pi, g[i], mi, vi, gs, lr_i, wd_i, step_size, b1, b2, ob1, ob2, eps, bc2_sqrt);
        m[i] = mi;
        v[i] = vi;
        if (s != 0.f) {
          p[i] = pi;
          if (pb) pb[i] = f2bf(pi);
          if (ph) ph[i] = f2h_sat(pi);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- weight averaging (EMA of the parameter arena)
// ema <- ema + w (p - ema), w = 1 - d, d = decay or -- warm-up -- min(decay, (1 + t) / (10 + t)); t = the optimizer steps applied so far,
// this one included.  Its ONE source: the guard (a set flag leaves before anything is read or written: a skipped step leaves the average
// alone; else NF_T, which the check kernel has already advanced), else the step state's counter, else the by-value step.  Two roundings per
// element, both spelt: the difference, then the fma.  A kernel of its own, not a fifth axis of the Adam templates (DESIGN.md "Weight
// averaging (EMA)").  One thread per 16-byte vector, grid-stride; the n % 4 tail element by element.
__global__ __launch_bounds__(256) void ema_update_kernel(const float* __restrict__ p, float* __restrict__ ema, long long n, float decay, int warmup,
                                                         float t, const float* __restrict__ guard, const float* __restrict__ state) {
  if (guard) {
    if (guard[NF_FLAG] != 0.f) return;
    t = guard[NF_T];
  } else if (state) {
    t = state[0];
  }
  const float d = warmup ? fminf(decay, (1.f + t) / (10.f + t)) : decay;
  const float w = 1.f - d;
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const long long nvec = n >> 2;
  for (long long k = tid; k < nvec; k += stride) {
    const float4 p4 = reinterpret_cast<const float4*>(p)[k];
    float4 e4 = reinterpret_cast<const float4*>(ema)[k];
    e4.x = __fmaf_rn(w, __fsub_rn(p4.x, e4.x), e4.x);
    e4.y = __fmaf_rn(w, __fsub_rn(p4.y, e4.y), e4.y);
    e4.z = __fmaf_rn(w, __fsub_rn(p4.z, e4.z), e4.z);
    e4.w = __fmaf_rn(w, __fsub_rn(p4.w, e4.w), e4.w);
    reinterpret_cast<float4*>(ema)[k] = e4;
  }
  for (long long i = (nvec << 2) + tid; i < n; i += stride) {
    const float e = ema[i];
    ema[i] = __fmaf_rn(w, __fsub_rn(p[i], e), e);
  }
}

// p <-> ema as bit patterns, and both 16-bit shadows of the NEW p with the Adam pass's own roundings (f2bf, f2h_sat): the shadows are
// valid when the kernel ends.  One thread per block of 8 elements (two 16-byte vectors of p and of ema, one 16-byte store per shadow),
// grid-stride; the n % 8 tail element by element.
__global__ __launch_bounds__(256) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema, bf16_t* __restrict__ pb,
                                                       bf16_t* __restrict__ ph, long long n) {
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
  const long long nblk = n >> 3;
  for (long long blk = tid; blk < nblk; blk += stride) {
    const long long i0 = blk << 3;
    uint4* pv = reinterpret_cast<uint4*>(p + i0);
    uint4* ev = reinterpret_cast<uint4*>(ema + i0);
    const uint4 p0 = pv[0], p1 = pv[1], e0 = ev[0], e1 = ev[1];
    pv[0] = e0; pv[1] = e1;
    ev[0] = p0; ev[1] = p1;
    const float x[8] = {__uint_as_float(e0.x), __uint_as_float(e0.y), __uint_as_float(e0.z), __uint_as_float(e0.w),
                        __uint_as_float(e1.x), __uint_as_float(e1.y), __uint_as_float(e1.z), __uint_as_float(e1.w)};
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)f2bf(x[2 * k]) | ((uint32_t)f2bf(x[2 * k + 1]) << 16);
    *reinterpret_cast<uint4*>(pb + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    if (ph)
      *reinterpret_cast<uint4*>(ph + i0) = make_uint4(f2h_sat2(x[0], x[1]), f2h_sat2(x[2], x[3]), f2h_sat2(x[4], x[5]), f2h_sat2(x[6], x[7]));
  }
  for (long long i = (nblk << 3) + tid; i < n; i += stride) {
    const uint32_t a = reinterpret_cast<uint32_t*>(p)[i], b = reinterpret_cast<uint32_t*>(ema)[i];
    reinterpret_cast<uint32_t*>(p)[i] = b;
    reinterpret_cast<uint32_t*>(ema)[i] = a;
    const float x = __uint_as_float(b);
    pb[i] = f2bf(x);
    if (ph) ph[i] = f2h_sat(x);
  }
}

// ---------------------------------------------------------------- hardware probe: ds_read_b64_tr_b16 semantics
__global__ __launch_bounds__(64) void probe_tr_kernel(int stride, unsigned short* out) {
  __shared__ __attribute__((aligned(16))) unsigned short img[64 * 64];
  for (int i = threadIdx.x; i < 64 * 64; i += 64) img[i] = (unsigned short)i;
  __syncthreads();
  const int lane = threadIdx.x;
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  // group g reads the 4x16 block starting at row 4*g, column 0: lane 4q+p supplies &img[(4g+q)*stride + 4p]
  typedef short s16x4 __attribute__((ext_vector_type(4)));
  const unsigned short* src = &img[(4 * g + q) * stride + 4 * pp];
  s16x4 r = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)src);
  for (int i = 0; i < 4; ++i) out[lane * 4 + i] = (unsigned short)r[i];
}

}  // namespace mmdti
MMDTI_DEFINE_SALT_PULL(elementwise)
using namespace mmdti;

extern "C" const char* mmdti_last_error(void) { return g_err; }
extern "C" int mmdti_abi_version(void) { return MMDTI_ABI_VERSION; }

// ---- this file's own tables: the softmax rows of MMDTI_PLAN_ROW (sm_key, row_plan.h: they follow layernorm.hip's twenty) and
// MMDTI_PLAN_STREAM (StreamKey, stream_plan.h) ----
static KernelRow g_softmax_kernels[ROW_KERNELS - ROW_LN_KERNELS] = {
    KROW(sm_key(0, 1), softmax_fwd_kernel<1>), KROW(sm_key(0, 2), softmax_fwd_kernel<2>), KROW(sm_key(0, 4), softmax_fwd_kernel<4>),
    KROW(sm_key(1, 1), softmax_bwd_kernel<1>), KROW(sm_key(1, 2), softmax_bwd_kernel<2>), KROW(sm_key(1, 4), softmax_bwd_kernel<4>),
};
static KernelRow g_stream_kernels[STREAM_KERNELS] = {
    KROW(SK_CAST_F32_BF16, cast_f32_bf16_kernel<false>), KROW(SK_CAST_F32_BF16 + 1, cast_f32_bf16_kernel<true>),
    KROW(SK_CAST_F16_BF16, cast_f16_bf16_kernel), KROW(SK_CAST_BF16_F32, cast_bf16_f32_kernel), KROW(SK_DROPOUT, dropout_f32_kernel),
    KROW(SK_AXPY, axpy_kernel), KROW(SK_GELU, gelu_bf16_kernel), KROW(SK_COLSUM, colsum_bf16_kernel), KROW(SK_COLSUM_SLAB, colsum_bf16_slab_kernel),
    KROW(SK_SUMSQ, sumsq_kernel), KROW(sumsq_part_key(0), sumsq_part_kernel<false>), KROW(sumsq_fold_key(0), sumsq_fold_kernel<false>),
    KROW(sumsq_part_key(1), sumsq_part_kernel<true>), KROW(sumsq_fold_key(1), sumsq_fold_kernel<true>),
    KROW(SK_ADAM, adam_kernel<false, false>), KROW(SK_ADAM + 1, adam_kernel<true, false>), KROW(SK_ADAM + 2, adam_kernel<false, true>),
    KROW(SK_ADAM + 3, adam_kernel<true, true>), KROW(SK_STEP_STATE, step_state_advance_kernel),
    KROW(SK_ADAM_GROUP, adam_group_kernel<false, false, false>), KROW(SK_ADAM_GROUP + 1, adam_group_kernel<false, false, true>),
    KROW(SK_ADAM_GROUP + 2, adam_group_kernel<false, true, false>), KROW(SK_ADAM_GROUP + 3, adam_group_kernel<false, true, true>),
    KROW(SK_ADAM_GROUP + 4, adam_group_kernel<true, false, false>), KROW(SK_ADAM_GROUP + 5, adam_group_kernel<true, false, true>),
    KROW(SK_ADAM_GROUP + 6, adam_group_kernel<true, true, false>), KROW(SK_ADAM_GROUP + 7, adam_group_kernel<true, true, true>),
    KROW(SK_EMA_UPDATE, ema_update_kernel), KROW(SK_EMA_SWAP, ema_swap_kernel),
};

// ---- the kernel tables of the planned families (each family's .hip file owns its table) ----
static const KernelRow* plan_row(int family, int index) {
  if (family >= MMDTI_PLAN_PAIR_ATTN_FWD && family <= MMDTI_PLAN_PAIR_ATTN_BWD_ELEM) return pair_attn_kernel_row(family - MMDTI_PLAN_PAIR_ATTN_FWD, index);
  if (family == MMDTI_PLAN_ROW && index >= ROW_LN_KERNELS) return index < ROW_KERNELS ? &g_softmax_kernels[index - ROW_LN_KERNELS] : nullptr;
  int n = 0;
  const KernelRow* t = family == MMDTI_PLAN_ATTN ? attn_kernel_table(&n) : family == MMDTI_PLAN_GBF ? gbf_kernel_table(&n)
                       : family == MMDTI_PLAN_ROW ? ln_kernel_table(&n) : family == MMDTI_PLAN_MAPS ? maps_kernel_table(&n)
                       : family == MMDTI_PLAN_LORA ? lora_kernel_table(&n) : nullptr;
  if (family == MMDTI_PLAN_STREAM) t = g_stream_kernels, n = STREAM_KERNELS;
  return t && index >= 0 && index < n ? &t[index] : nullptr;
}
extern "C" int mmdti_plan_table_size(int family, int* size_out) {
  MMDTI_REQUIRE(size_out != nullptr, "plan_table_size: null size_out");
  MMDTI_REQUIRE(plan_row(family, 0) != nullptr, "plan_table_size: unknown family %d", family);
  int n = 0;
  for (const KernelRow* r; (r = plan_row(family, n)) != nullptr; ++n)
    MMDTI_REQUIRE(r->key == n, "plan_table_size: family %d holds key %d (%s) at row %d", family, r->key, r->name, n);   // (a plan's key IS the row)
  *size_out = n;
  return MMDTI_OK;
}
extern "C" const char* mmdti_plan_kernel_name(int family, int index) {
  const KernelRow* r = plan_row(family, index);
  return r ? r->name : nullptr;
}

// ---- deterministic mode: the flag and the per-stream workspace table (det.h) ----
extern "C" int mmdti_set_deterministic(int on) {
  det_table().set_on(on != 0);
  return MMDTI_OK;
}
extern "C" int mmdti_det_workspace(mmdti_stream_t stream, void* ws, long long bytes) {
  MMDTI_REQUIRE(det_table().put(stream, ws, bytes), "det_workspace: a workspace needs bytes > 0 and 16-byte alignment");
  return MMDTI_OK;
}
extern "C" int mmdti_det_workspace_bytes(int site, long long rows, long long cols, long long* bytes_out) {
  MMDTI_REQUIRE(bytes_out != nullptr, "det_workspace_bytes: null bytes_out");
  const long long b = det_workspace_bytes(site, rows, cols);
  MMDTI_REQUIRE(b >= 0, "det_workspace_bytes: unknown site %d or bad shape (%lld x %lld)", site, rows, cols);
  *bytes_out = b;
  return MMDTI_OK;
}

// Adam's bias corrections of step t as mmdti_adam_step computes them by value (host powf): also what mmdti_adam_bias_table lists,
// so that a guarded eager step reproduces the unguarded one to the bit
static void adam_bias_host(float beta1, float beta2, int step, float* bc1, float* bc2_sqrt) {
  *bc1 = 1.f - powf(beta1, (float)step);
  *bc2_sqrt = sqrtf(1.f - powf(beta2, (float)step));
}

#define DROP_REQUIRE(name) MMDTI_REQUIRE(drop_p >= 0.f && drop_p < 1.f, name ": dropout p out of range")
#define DROP_SETUP()                           \
  const uint32_t th = dropout_thresh(drop_p);  \
  const float sc = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f
#define STREAM_ROW(plan, i) g_stream_kernels[(plan).k[i].key], (plan).k[i], (hipStream_t)stream

// ---- What each launcher and mmdti_stream_plan share: validate, plan (stream_plan.h).  Pointers are tested for null and alignment only. ----
static int cast_f32_bf16_prepare(StreamPlan& plan, const float* x, const void* y_bf16, long long n, float drop_p) {
  MMDTI_REQUIRE(x && y_bf16 && n > 0, "cast_f32_bf16: bad arguments");
  MMDTI_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(y_bf16) & 7) == 0, "cast_f32_bf16: alignment");
  DROP_REQUIRE("cast_f32_bf16");
  plan = cast_f32_16_plan(n, false);
  return MMDTI_OK;
}
static int cast_f32_f16_prepare(StreamPlan& plan, const float* x, const void* y_f16, long long n, float drop_p) {
  MMDTI_REQUIRE(x && y_f16 && n > 0, "cast_f32_f16: bad arguments");
  MMDTI_REQUIRE(aligned16(x) && (reinterpret_cast<uintptr_t>(y_f16) & 7) == 0, "cast_f32_f16: alignment");
  DROP_REQUIRE("cast_f32_f16");
  plan = cast_f32_16_plan(n, true);
  return MMDTI_OK;
}
static int cast_f16_bf16_prepare(StreamPlan& plan, const void* x_f16, int rows, int cols, int ldx, const void* y_bf16) {
  MMDTI_REQUIRE(x_f16 && y_bf16 && rows > 0 && cols > 0 && cols % 8 == 0 && ldx >= cols && ldx % 8 == 0, "cast_f16_bf16: bad arguments (cols %% 8, ldx %% 8)");
  MMDTI_REQUIRE(aligned16(x_f16) && aligned16(y_bf16), "cast_f16_bf16: 16-byte alignment required");
  plan = cast_f16_bf16_plan(rows, cols);
  return MMDTI_OK;
}
static int cast_bf16_f32_prepare(StreamPlan& plan, const void* x_bf16, const float* y, long long n) {
  MMDTI_REQUIRE(x_bf16 && y && n > 0, "cast_bf16_f32: bad arguments");
  plan = stream_plan(SK_CAST_BF16_F32, n, 256);
  return MMDTI_OK;
}
static int dropout_f32_prepare(StreamPlan& plan, const float* x, const float* y, long long n, float drop_p) {
  MMDTI_REQUIRE(x && y && n > 0, "dropout_f32: bad arguments");
  DROP_REQUIRE("dropout_f32");
  plan = stream_plan(SK_DROPOUT, n, 256);
  return MMDTI_OK;
}
static int axpy_f32_prepare(StreamPlan& plan, const float* x, const float* y, long long n) {
  MMDTI_REQUIRE(x && y && n > 0, "axpy_f32: bad arguments");
  plan = stream_plan(SK_AXPY, n, 256);
  return MMDTI_OK;
}
static int gelu_fwd_bf16_prepare(StreamPlan& plan, const void* u_bf16, const void* y_bf16, long long n) {
  MMDTI_REQUIRE(u_bf16 && y_bf16 && n > 0, "gelu_fwd_bf16: bad arguments");
  plan = stream_plan(SK_GELU, n, 256);
  return MMDTI_OK;
}
// det: the mode the launch finds (det_table().on()); the stream's workspace is looked up by the launch alone
static int colsum_bf16_prepare(StreamPlan& plan, bool det, const void* x_bf16, int rows, int cols, int ld, const float* out) {
  MMDTI_REQUIRE(x_bf16 && out && rows > 0 && cols > 0 && ld >= cols, "colsum_bf16: bad arguments");
  MMDTI_REQUIRE(ld % 8 == 0 && aligned16(x_bf16), "colsum_bf16: ld%%8 and 16-byte alignment required");
  plan = colsum_plan(rows, cols, det);
  return MMDTI_OK;
}

// (both fp32 -> 16-bit casts: one signature, the plan's key tells them apart)
static int cast_f32_16_launch(const StreamPlan& plan, mmdti_stream_t stream, const float* x, void* y16, long long n, float drop_p,
                              unsigned long long seed, unsigned int site) {
  DROP_SETUP();
  launch_row(cast_f32_bf16_kernel<false>, STREAM_ROW(plan, 0), x, (bf16_t*)y16, n / 4, n, th, sc, (uint64_t)seed, (uint32_t)site);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_cast_f32_bf16(mmdti_stream_t stream, const float* x, void* y_bf16, long long n, float drop_p,
                                   unsigned long long seed, unsigned int site) {
  StreamPlan plan;
  if (int e = cast_f32_bf16_prepare(plan, x, y_bf16, n, drop_p)) return e;
  return cast_f32_16_launch(plan, stream, x, y_bf16, n, drop_p, seed, site);
}

extern "C" int mmdti_cast_f32_f16(mmdti_stream_t stream, const float* x, void* y_f16, long long n, float drop_p,
                                  unsigned long long seed, unsigned int site) {
  StreamPlan plan;
  if (int e = cast_f32_f16_prepare(plan, x, y_f16, n, drop_p)) return e;
  return cast_f32_16_launch(plan, stream, x, y_f16, n, drop_p, seed, site);
}

extern "C" int mmdti_cast_f16_bf16(mmdti_stream_t stream, const void* x_f16, int rows, int cols, int ldx, void* y_bf16) {
  StreamPlan plan;
  if (int e = cast_f16_bf16_prepare(plan, x_f16, rows, cols, ldx, y_bf16)) return e;
  launch_row(cast_f16_bf16_kernel, STREAM_ROW(plan, 0), (const bf16_t*)x_f16, cols / 8, ldx, (bf16_t*)y_bf16, (long long)rows * (cols / 8));
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_cast_bf16_f32(mmdti_stream_t stream, const void* x_bf16, float* y, long long n) {
  StreamPlan plan;
  if (int e = cast_bf16_f32_prepare(plan, x_bf16, y, n)) return e;
  launch_row(cast_bf16_f32_kernel, STREAM_ROW(plan, 0), (const bf16_t*)x_bf16, y, n);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_dropout_f32(mmdti_stream_t stream, const float* x, float* y, long long n, float drop_p,
                                 unsigned long long seed, unsigned int site) {
  StreamPlan plan;
  if (int e = dropout_f32_prepare(plan, x, y, n, drop_p)) return e;
  DROP_SETUP();
  launch_row(dropout_f32_kernel, STREAM_ROW(plan, 0), x, y, n, th, sc, (uint64_t)seed, (uint32_t)site);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_axpy_f32(mmdti_stream_t stream, const float* x, float* y, long long n, float a) {
  StreamPlan plan;
  if (int e = axpy_f32_prepare(plan, x, y, n)) return e;
  launch_row(axpy_kernel, STREAM_ROW(plan, 0), x, y, n, a);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_gelu_fwd_bf16(mmdti_stream_t stream, const void* u_bf16, void* y_bf16, long long n) {
  StreamPlan plan;
  if (int e = gelu_fwd_bf16_prepare(plan, u_bf16, y_bf16, n)) return e;
  launch_row(gelu_bf16_kernel, STREAM_ROW(plan, 0), (const bf16_t*)u_bf16, (bf16_t*)y_bf16, n);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_colsum_bf16(mmdti_stream_t stream, const void* x_bf16, int rows, int cols, int ld, float* out) {
  StreamPlan plan;
  if (int e = colsum_bf16_prepare(plan, det_table().on(), x_bf16, rows, cols, ld, out)) return e;
  float* dst = out;
  if (plan.nlaunch == 2)   // the deterministic mode: the sums go to the stream's workspace first
    if (int e = det_workspace(stream, det_workspace_bytes(MMDTI_DET_COLSUM, rows, cols), "colsum_bf16", &dst)) return e;
  launch_row(colsum_bf16_kernel, STREAM_ROW(plan, 0), (const bf16_t*)x_bf16, rows, cols, ld, dst);
  if (plan.nlaunch == 2) det_fold<1>((hipStream_t)stream, dst, (int)plan.k[0].gy, cols, cols, DetDst<1>{{out}});
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_embedding_fwd(mmdti_stream_t stream, const long long* ids, const float* table, long long n,
                                   int D, int vocab, float* out, int accumulate) {
  MMDTI_REQUIRE(ids && table && out && n > 0 && D > 0 && D % 4 == 0 && vocab > 0, "embedding_fwd: bad arguments");
  MMDTI_REQUIRE(aligned16(table) && aligned16(out), "embedding_fwd: alignment");
  hipLaunchKernelGGL(embedding_fwd_kernel, dim3(grid_for(n * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, ids,
                     table, n, D / 4, vocab, out, accumulate);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_embedding_bwd(mmdti_stream_t stream, const long long* ids, const float* dout, long long n,
                                   int D, int vocab, long long padding_idx, float* dtable) {
  MMDTI_REQUIRE(ids && dout && dtable && n > 0 && D > 0 && vocab > 0, "embedding_bwd: bad arguments");
  if (det_table().on()) {                // (the model takes mmdti_onehot_bf16 + the split-K GEMM; this is the general entry's ordered form)
    hipLaunchKernelGGL(embedding_bwd_ordered_kernel, dim3(cdiv(D, 256), vocab < 64 ? vocab : 64), dim3(256), 0, (hipStream_t)stream, ids, dout,
                       n, D, vocab, padding_idx, dtable);
    MMDTI_LAUNCH_CHECK();
    return MMDTI_OK;
  }
  hipLaunchKernelGGL(embedding_bwd_kernel, dim3(grid_for(n * D, 256)), dim3(256), 0, (hipStream_t)stream, ids, dout,
                     n, D, vocab, padding_idx, dtable);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_embedding_fwd3(mmdti_stream_t stream, const long long* ids_a, const float* table_a, int vocab_a, const long long* ids_b,
                                    const float* table_b, int vocab_b, const long long* ids_c, const float* table_c, int vocab_c, long long n,
                                    int D, float* out) {
  MMDTI_REQUIRE(ids_a && table_a && ids_b && table_b && table_c && out && n > 0 && D > 0 && D % 4 == 0 && vocab_a > 0 && vocab_b > 0 && vocab_c > 0,
                "embedding_fwd3: bad arguments");
  MMDTI_REQUIRE(aligned16(table_a) && aligned16(table_b) && aligned16(table_c) && aligned16(out), "embedding_fwd3: alignment");
  hipLaunchKernelGGL(embedding_fwd3_kernel, dim3(grid_for(n * (D / 4), 256)), dim3(256), 0, (hipStream_t)stream, ids_a, table_a, vocab_a, ids_b,
                     table_b, vocab_b, ids_c, table_c, vocab_c, n, D / 4, out);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_onehot_bf16(mmdti_stream_t stream, const long long* ids, long long n, int vocab, int ld,
                                 long long padding_idx, void* out_bf16) {
  MMDTI_REQUIRE(ids && out_bf16 && n > 0 && vocab > 0 && ld >= vocab && ld % 8 == 0, "onehot_bf16: bad arguments");
  MMDTI_REQUIRE(aligned16(out_bf16), "onehot_bf16: output must be 16-byte aligned");
  hipLaunchKernelGGL(onehot_bf16_kernel, dim3(grid_for(n * (ld / 8), 256)), dim3(256), 0, (hipStream_t)stream, ids, n,
                     vocab, ld / 8, padding_idx, (bf16_t*)out_bf16);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_roberta_position_ids(mmdti_stream_t stream, const long long* ids, int B, int L,
                                          long long pad_idx, long long* out) {
  MMDTI_REQUIRE(ids && out && B > 0 && L > 0, "roberta_position_ids: bad arguments");
  hipLaunchKernelGGL(roberta_posids_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, ids, L, pad_idx, out);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

static int softmax_fwd_prepare(RowPlan& plan, const float* s, const void* p_bf16, const void* pd_bf16, int B, int heads, int Lq, int Lk, int ld,
                               float drop_p) {
  MMDTI_REQUIRE(s && p_bf16 && pd_bf16 && B > 0 && heads > 0 && Lq > 0 && Lk > 0, "softmax_fwd: bad arguments");
  MMDTI_REQUIRE(ld >= Lk && ld <= 1024 && ld % 8 == 0, "softmax_fwd: need Lk <= ld <= 1024, ld %% 8 == 0");
  MMDTI_REQUIRE(aligned16(s) && aligned16(p_bf16) && aligned16(pd_bf16), "softmax_fwd: 16-byte alignment required");
  DROP_REQUIRE("softmax_fwd");
  MMDTI_REQUIRE(drop_p == 0.f || pd_bf16 != p_bf16, "softmax_fwd: dropout needs a separate pd buffer");
  plan = softmax_plan(false, (long long)B * heads * Lq, ld);
  return MMDTI_OK;
}
static int softmax_bwd_prepare(RowPlan& plan, const void* p_bf16, const float* dp, const void* ds_bf16, int B, int heads, int Lq, int Lk, int ld,
                               float drop_p) {
  MMDTI_REQUIRE(p_bf16 && dp && ds_bf16 && B > 0 && heads > 0 && Lq > 0 && Lk > 0, "softmax_bwd: bad arguments");
  MMDTI_REQUIRE(ld >= Lk && ld <= 1024 && ld % 8 == 0, "softmax_bwd: need Lk <= ld <= 1024, ld %% 8 == 0");
  MMDTI_REQUIRE(aligned16(dp) && aligned16(p_bf16) && aligned16(ds_bf16), "softmax_bwd: 16-byte alignment required");
  DROP_REQUIRE("softmax_bwd");
  plan = softmax_plan(true, (long long)B * heads * Lq, ld);
  return MMDTI_OK;
}

extern "C" int mmdti_softmax_fwd(mmdti_stream_t stream, const float* s, const float* key_add, void* p_bf16,
                                 void* pd_bf16, int B, int heads, int Lq, int Lk, int ld, float drop_p,
                                 unsigned long long seed, unsigned int site) {
  RowPlan plan;
  if (int e = softmax_fwd_prepare(plan, s, p_bf16, pd_bf16, B, heads, Lq, Lk, ld, drop_p)) return e;
  DROP_SETUP();
  launch_row(softmax_fwd_kernel<1>, g_softmax_kernels[plan.k[0].key - ROW_LN_KERNELS], plan.k[0], (hipStream_t)stream, s, key_add, (bf16_t*)p_bf16,
             (bf16_t*)pd_bf16, (long long)B * heads * Lq, heads, Lq, Lk, ld, th, sc, (uint64_t)seed, (uint32_t)site);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_softmax_bwd(mmdti_stream_t stream, const void* p_bf16, const float* dp, void* ds_bf16, int B,
                                 int heads, int Lq, int Lk, int ld, float scale, float drop_p,
                                 unsigned long long seed, unsigned int site) {
  RowPlan plan;
  if (int e = softmax_bwd_prepare(plan, p_bf16, dp, ds_bf16, B, heads, Lq, Lk, ld, drop_p)) return e;
  DROP_SETUP();
  launch_row(softmax_bwd_kernel<1>, g_softmax_kernels[plan.k[0].key - ROW_LN_KERNELS], plan.k[0], (hipStream_t)stream, (const bf16_t*)p_bf16, dp,
             (bf16_t*)ds_bf16, (long long)B * heads * Lq, Lk, ld, scale, th, sc, (uint64_t)seed, (uint32_t)site);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

// The plan a LayerNorm or row-softmax entry would launch, without launching (include/mmdti_hip.h documents ptrs and plan_out)
extern "C" int mmdti_row_plan(int entry, int deterministic, const void* const* ptrs, int rows_or_B, int heads, int Lq, int Lk, int D_or_ld,
                              int dy_dtype, float drop_p, float drop2_p, long long* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr && ptrs != nullptr, "row_plan: null plan_out or ptrs");
  MMDTI_REQUIRE(entry >= MMDTI_ROW_LAYERNORM_FWD && entry <= MMDTI_ROW_SOFTMAX_BWD, "row_plan: unknown entry %d", entry);
  auto f = [&](int i) { return static_cast<const float*>(ptrs[i]); };
  RowPlan plan;
  int e;
  if (entry == MMDTI_ROW_LAYERNORM_FWD) e = ln_fwd_prepare(plan, f(0), f(1), f(2), rows_or_B, D_or_ld, f(3), ptrs[4], drop_p);
  else if (entry == MMDTI_ROW_LAYERNORM_BWD)
    e = ln_bwd_prepare(plan, deterministic != 0, ptrs[0], dy_dtype, f(1), f(2), f(3), f(4), rows_or_B, D_or_ld, f(5), f(6), f(7), drop_p, ptrs[8],
                       drop2_p, f(9));
  else if (entry == MMDTI_ROW_SOFTMAX_FWD) e = softmax_fwd_prepare(plan, f(0), ptrs[1], ptrs[2], rows_or_B, heads, Lq, Lk, D_or_ld, drop_p);
  else e = softmax_bwd_prepare(plan, ptrs[0], f(1), ptrs[2], rows_or_B, heads, Lq, Lk, D_or_ld, drop_p);
  if (e) return e;
  static_assert(ROW_PLAN_INTS == 13, "mmdti_hip.h documents 13 long long");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}

extern "C" int mmdti_masked_pool_fwd(mmdti_stream_t stream, const float* a, const float* t,
                                     const unsigned char* mask_a, const unsigned char* mask_t, int B, int Na, int Nt,
                                     int D, float* pooled) {
  MMDTI_REQUIRE(a && t && mask_a && mask_t && pooled && B > 0 && Na > 0 && Nt > 0 && D > 0, "masked_pool_fwd: bad arguments");
  MMDTI_REQUIRE(D % 4 == 0 && aligned16(a) && aligned16(t) && aligned16(pooled), "masked_pool_fwd: D%%4 and 16-byte alignment required");
  hipLaunchKernelGGL(masked_pool_fwd_kernel, dim3(B, cdiv(D, 64)), dim3(256), 0, (hipStream_t)stream, a, t, mask_a, mask_t, Na, Nt, D, pooled);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_masked_pool_bwd(mmdti_stream_t stream, const float* dpooled, const unsigned char* mask_a,
                                     const unsigned char* mask_t, int B, int Na, int Nt, int D, float* da, float* dt) {
  MMDTI_REQUIRE(dpooled && mask_a && mask_t && da && dt && B > 0 && Na > 0 && Nt > 0 && D > 0, "masked_pool_bwd: bad arguments");
  MMDTI_REQUIRE(D % 4 == 0 && aligned16(dpooled) && aligned16(da) && aligned16(dt), "masked_pool_bwd: D%%4 and 16-byte alignment required");
  hipLaunchKernelGGL(masked_pool_bwd_kernel, dim3(B, 8), dim3(256), 0, (hipStream_t)stream, dpooled, mask_a, mask_t, Na, Nt, D, da, dt);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_masked_pool_packed_fwd(mmdti_stream_t stream, const float* a, const float* t, const int* a_off, const int* a_cnt,
                                            const int* t_off, const int* t_cnt, int B, int D, float* pooled) {
  MMDTI_REQUIRE(a && t && a_off && a_cnt && t_off && t_cnt && pooled && B > 0 && D > 0, "masked_pool_packed_fwd: bad arguments");
  MMDTI_REQUIRE(D % 4 == 0 && aligned16(a) && aligned16(t) && aligned16(pooled), "masked_pool_packed_fwd: D%%4 and 16-byte alignment required");
  hipLaunchKernelGGL(masked_pool_packed_fwd_kernel, dim3(B, cdiv(D, 64)), dim3(256), 0, (hipStream_t)stream, a, t, a_off, a_cnt, t_off, t_cnt, D, pooled);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_masked_pool_packed_bwd(mmdti_stream_t stream, const float* dpooled, const int* a_off, const int* a_cnt, const int* a_seq,
                                            int rows_a, const int* t_off, const int* t_cnt, const int* t_seq, int rows_t, int D, float* da,
                                            float* dt) {
  MMDTI_REQUIRE(dpooled && a_off && a_cnt && a_seq && t_off && t_cnt && t_seq && da && dt && rows_a > 0 && rows_t > 0 && D > 0,
                "masked_pool_packed_bwd: bad arguments");
  MMDTI_REQUIRE(D % 4 == 0 && aligned16(dpooled) && aligned16(da) && aligned16(dt), "masked_pool_packed_bwd: D%%4 and 16-byte alignment required");
  const long long n = ((long long)rows_a + rows_t) * (D / 4);
  hipLaunchKernelGGL(masked_pool_packed_bwd_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, dpooled, a_off, a_cnt, a_seq,
                     rows_a, t_off, t_cnt, t_seq, rows_t, D, da, dt);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

// det: the mode the launch finds (det_table().on())
static int sumsq_f32_prepare(StreamPlan& plan, bool det, const float* g, long long n, const float* out, const float* ws, int ws_floats) {
  MMDTI_REQUIRE(g && out && n > 0, "sumsq_f32: bad arguments");
  const bool parts = ws && ws_floats >= 1 && aligned16(g);
  if (!parts)
    MMDTI_REQUIRE(!det, "sumsq_f32: deterministic mode needs the ws form (16-byte aligned g, ws_floats >= 1): without it the partials meet in an atomic");
  plan = sumsq_plan(n, parts ? ws_floats : 0, false);
  return MMDTI_OK;
}
static int sumsq_check_f32_prepare(StreamPlan& plan, const float* g, long long n, const float* out, const float* ws, int ws_floats,
                                   const float* bias_table, int table_steps) {
  MMDTI_REQUIRE(g && out && ws && n > 0 && ws_floats >= 2, "sumsq_check_f32: bad arguments");
  MMDTI_REQUIRE(aligned16(g), "sumsq_check_f32: 16-byte alignment required");
  MMDTI_REQUIRE(!bias_table || table_steps >= 1, "sumsq_check_f32: empty bias-correction table");
  plan = sumsq_plan(n, ws_floats / 2, true);   // the workgroup count of mmdti_sumsq_f32 with ws_floats / 2 partials
  return MMDTI_OK;
}
// partials, then the fixed-order fold: both instantiations, the plan's keys tell them apart
static void sumsq_parts_launch(const StreamPlan& plan, mmdti_stream_t stream, const float* g, long long n, float* ws, unsigned* cnt, float* out,
                               float* guard, const float* bias_table, int table_steps, float beta1, float beta2) {
  launch_row(sumsq_part_kernel<false>, STREAM_ROW(plan, 0), g, n, ws, cnt);
  launch_row(sumsq_fold_kernel<false>, STREAM_ROW(plan, 1), ws, (int)plan.wgs, out, cnt, guard, bias_table, table_steps, beta1, beta2);
}

extern "C" int mmdti_sumsq_f32(mmdti_stream_t stream, const float* g, long long n, float* out, float* ws, int ws_floats) {
  StreamPlan plan;
  if (int e = sumsq_f32_prepare(plan, det_table().on(), g, n, out, ws, ws_floats)) return e;
  if (plan.nlaunch == 2) sumsq_parts_launch(plan, stream, g, n, ws, nullptr, out, nullptr, nullptr, 0, 0.f, 0.f);
  else launch_row(sumsq_kernel, STREAM_ROW(plan, 0), g, n, out);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_sumsq_check_f32(mmdti_stream_t stream, const float* g, long long n, float* out, float* ws, int ws_floats, float* guard,
                                     const float* bias_table, int table_steps, float beta1, float beta2) {
  StreamPlan plan;
  if (int e = sumsq_check_f32_prepare(plan, g, n, out, ws, ws_floats, bias_table, table_steps)) return e;
  sumsq_parts_launch(plan, stream, g, n, ws, reinterpret_cast<unsigned*>(ws + plan.wgs), out, guard, bias_table, table_steps, beta1, beta2);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

// ---- the Adam pass: four entry points, each with its own argument rules, over one launcher ----
struct AdamArgs {
  float* p; const float* g; float* m; float* v; void* p_bf16; void* p_f16;
  long long n;
  float lr, beta1, beta2, eps, weight_decay;
  int step;
  const float *grad_scale_dev, *step_state_dev, *guard;
  const unsigned char* skip;
  const unsigned char* group; const float* table_dev; int ngroups;   // mmdti_adam_step_grouped alone
};
// Host bias corrections (by value, from `step`) only when no guard is given: a guarded kernel reads the guard's
static int adam_launch(const StreamPlan& plan, mmdti_stream_t stream, const AdamArgs& a) {
  if (plan.nlaunch == 0) return MMDTI_OK;
  float bc1 = 1.f, bc2s = 1.f;
  if (!a.guard) adam_bias_host(a.beta1, a.beta2, a.step, &bc1, &bc2s);
  if (a.group)
    launch_row(adam_group_kernel<false, false, false>, STREAM_ROW(plan, 0), a.p, a.g, a.m, a.v, (bf16_t*)a.p_bf16, (bf16_t*)a.p_f16, a.n, a.lr, a.beta1,
               a.beta2, a.eps, bc1, bc2s, a.grad_scale_dev, a.step_state_dev, a.guard, a.skip, a.group, a.table_dev, a.ngroups);
  else
    launch_row(adam_kernel<false, false>, STREAM_ROW(plan, 0), a.p, a.g, a.m, a.v, (bf16_t*)a.p_bf16, (bf16_t*)a.p_f16, a.n, a.lr, a.beta1, a.beta2,
               a.eps, a.weight_decay, bc1, bc2s, a.grad_scale_dev, a.step_state_dev, a.guard, a.skip);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

static int adam_step_prepare(StreamPlan& plan, const float* p, const float* g, const float* m, const float* v, long long n, int step,
                             const float* step_state_dev) {
  MMDTI_REQUIRE(p && g && m && v && n > 0 && (step >= 1 || step_state_dev), "adam_step: bad arguments");
  plan = adam_plan(ADAM_STEP, n, false, false, false);
  return MMDTI_OK;
}
static int adam_step_guarded_prepare(StreamPlan& plan, const float* p, const float* g, const float* m, const float* v, long long n,
                                     const float* guard) {
  MMDTI_REQUIRE(p && g && m && v && n > 0 && guard, "adam_step_guarded: bad arguments");
  plan = adam_plan(ADAM_STEP_GUARDED, n, true, false, false);
  return MMDTI_OK;
}
static int adam_step_masked_prepare(StreamPlan& plan, const float* p, const float* g, const float* m, const float* v, long long n, int step,
                                    const float* step_state_dev, const float* guard, const unsigned char* skip) {
  MMDTI_REQUIRE(p && g && m && v && n > 0 && skip && (guard || step >= 1 || step_state_dev), "adam_step_masked: bad arguments");
  plan = adam_plan(ADAM_STEP_MASKED, n, guard != nullptr, true, false);
  return MMDTI_OK;
}
static int adam_step_grouped_prepare(StreamPlan& plan, const float* p, const float* g, const float* m, const float* v, const void* p_bf16,
                                     long long n, int step, const float* step_state_dev, const void* p_f16, const float* guard,
                                     const unsigned char* skip, const unsigned char* group, const float* table_dev, int ngroups, int decoupled) {
  MMDTI_REQUIRE(p && g && m && v && group && table_dev, "adam_step_grouped: null pointer");
  MMDTI_REQUIRE(ngroups >= 1 && ngroups <= 256, "adam_step_grouped: ngroups must be 1 .. 256");
  MMDTI_REQUIRE(n >= 0, "adam_step_grouped: negative n");
  MMDTI_REQUIRE(guard || step >= 1 || step_state_dev, "adam_step_grouped: no source of bias corrections (guard, step >= 1 or step state)");
  MMDTI_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(p_bf16) && aligned16(p_f16),
                "adam_step_grouped: 16-byte alignment required");
  plan = adam_plan(ADAM_STEP_GROUPED, n, guard != nullptr, skip != nullptr, decoupled != 0);
  return MMDTI_OK;
}

extern "C" int mmdti_adam_step(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16,
                               long long n, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int step, const float* grad_scale_dev, const float* step_state_dev, void* p_f16) {
  StreamPlan plan;
  if (int e = adam_step_prepare(plan, p, g, m, v, n, step, step_state_dev)) return e;
  return adam_launch(plan, stream, AdamArgs{p, g, m, v, p_bf16, p_f16, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_dev, step_state_dev,
                                            nullptr, nullptr, nullptr, nullptr, 0});
}

extern "C" int mmdti_adam_step_guarded(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, const float* grad_scale_dev,
                                       const float* step_state_dev, void* p_f16, const float* guard) {
  StreamPlan plan;
  if (int e = adam_step_guarded_prepare(plan, p, g, m, v, n, guard)) return e;
  return adam_launch(plan, stream, AdamArgs{p, g, m, v, p_bf16, p_f16, n, lr, beta1, beta2, eps, weight_decay, 0, grad_scale_dev, step_state_dev,
                                            guard, nullptr, nullptr, nullptr, 0});
}

extern "C" int mmdti_adam_step_masked(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                                      float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                      const float* grad_scale_dev, const float* step_state_dev, void* p_f16, const float* guard,
                                      const unsigned char* skip) {
  StreamPlan plan;
  if (int e = adam_step_masked_prepare(plan, p, g, m, v, n, step, step_state_dev, guard, skip)) return e;
  return adam_launch(plan, stream, AdamArgs{p, g, m, v, p_bf16, p_f16, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale_dev, step_state_dev,
                                            guard, skip, nullptr, nullptr, 0});
}

extern "C" int mmdti_adam_step_grouped(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                                       float lr, float beta1, float beta2, float eps, int step, const float* grad_scale_dev,
                                       const float* step_state_dev, void* p_f16, const float* guard, const unsigned char* skip,
                                       const unsigned char* group, const float* table_dev, int ngroups, int decoupled) {
  StreamPlan plan;
  if (int e = adam_step_grouped_prepare(plan, p, g, m, v, p_bf16, n, step, step_state_dev, p_f16, guard, skip, group, table_dev, ngroups, decoupled))
    return e;
  return adam_launch(plan, stream, AdamArgs{p, g, m, v, p_bf16, p_f16, n, lr, beta1, beta2, eps, 0.f, step, grad_scale_dev, step_state_dev, guard, skip,
                                            group, table_dev, ngroups});
}

extern "C" int mmdti_adam_bias_table(float beta1, float beta2, int steps, float* table_host) {
  MMDTI_REQUIRE(table_host && steps >= 1, "adam_bias_table: bad arguments");
  for (int t = 1; t <= steps; ++t) adam_bias_host(beta1, beta2, t, &table_host[2 * (t - 1)], &table_host[2 * (t - 1) + 1]);
  return MMDTI_OK;
}

static int ema_update_prepare(StreamPlan& plan, const float* p, const float* ema, long long n, float decay, int step, const float* guard,
                              const float* step_state) {
  MMDTI_REQUIRE(p && ema && p != ema, "ema_update: p and ema are two non-null buffers");
  MMDTI_REQUIRE(n >= 0, "ema_update: negative n");
  MMDTI_REQUIRE(decay > 0.f && decay < 1.f, "ema_update: decay must lie in (0, 1)");
  MMDTI_REQUIRE(guard || step_state || step >= 1, "ema_update: no source of t (guard, step state or step >= 1)");
  MMDTI_REQUIRE(aligned16(p) && aligned16(ema), "ema_update: 16-byte alignment required");
  plan = ema_plan(false, n);
  return MMDTI_OK;
}
static int ema_swap_prepare(StreamPlan& plan, const float* p, const float* ema, const void* p_bf16, const void* p_f16, long long n) {
  MMDTI_REQUIRE(p && ema && p != ema && p_bf16, "ema_swap: p, ema (two buffers) and p_bf16 must be given");
  MMDTI_REQUIRE(n >= 0, "ema_swap: negative n");
  MMDTI_REQUIRE(aligned16(p) && aligned16(ema) && aligned16(p_bf16) && aligned16(p_f16), "ema_swap: 16-byte alignment required");
  plan = ema_plan(true, n);
  return MMDTI_OK;
}
static int step_state_advance_prepare(StreamPlan& plan, const float* state, const unsigned long long* salt, int warmup_steps, int total_steps) {
  MMDTI_REQUIRE(state && salt, "step_state_advance: null pointer");
  MMDTI_REQUIRE(total_steps > 0 && warmup_steps >= 0, "step_state_advance: bad schedule");
  plan = step_state_plan();
  return MMDTI_OK;
}

extern "C" int mmdti_ema_update(mmdti_stream_t stream, const float* p, float* ema, long long n, float decay, int warmup, int step,
                                const float* guard, const float* step_state) {
  StreamPlan plan;
  if (int e = ema_update_prepare(plan, p, ema, n, decay, step, guard, step_state)) return e;
  if (plan.nlaunch == 0) return MMDTI_OK;
  launch_row(ema_update_kernel, STREAM_ROW(plan, 0), p, ema, n, decay, warmup, (float)step, guard, step_state);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_ema_swap(mmdti_stream_t stream, float* p, float* ema, void* p_bf16, void* p_f16, long long n) {
  StreamPlan plan;
  if (int e = ema_swap_prepare(plan, p, ema, p_bf16, p_f16, n)) return e;
  if (plan.nlaunch == 0) return MMDTI_OK;
  launch_row(ema_swap_kernel, STREAM_ROW(plan, 0), p, ema, (bf16_t*)p_bf16, (bf16_t*)p_f16, n);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_step_state_advance(mmdti_stream_t stream, float* state, unsigned long long* salt, float base_lr, int warmup_steps,
                                        int total_steps, float beta1, float beta2) {
  StreamPlan plan;
  if (int e = step_state_advance_prepare(plan, state, salt, warmup_steps, total_steps)) return e;
  launch_row(step_state_advance_kernel, STREAM_ROW(plan, 0), state, salt, base_lr, warmup_steps, total_steps, beta1, beta2);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

// The plan a stream, reduction or optimizer entry would launch, without launching (include/mmdti_hip.h documents the entries, what
// each reads of ptrs, n, a, b, c and f, and plan_out)
extern "C" int mmdti_stream_plan(int entry, int deterministic, const void* const* ptrs, long long n, int a, int b, int c, float f,
                                 long long* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr && ptrs != nullptr, "stream_plan: null plan_out or ptrs");
  auto F = [&](int i) { return static_cast<const float*>(ptrs[i]); };
  auto U8 = [&](int i) { return static_cast<const unsigned char*>(ptrs[i]); };
  const bool det = deterministic != 0;
  StreamPlan plan;
  int e;
  switch (entry) {
    case MMDTI_STREAM_CAST_F32_BF16: e = cast_f32_bf16_prepare(plan, F(0), ptrs[1], n, f); break;
    case MMDTI_STREAM_CAST_F32_F16: e = cast_f32_f16_prepare(plan, F(0), ptrs[1], n, f); break;
    case MMDTI_STREAM_CAST_F16_BF16: e = cast_f16_bf16_prepare(plan, ptrs[0], a, b, c, ptrs[1]); break;
    case MMDTI_STREAM_CAST_BF16_F32: e = cast_bf16_f32_prepare(plan, ptrs[0], F(1), n); break;
    case MMDTI_STREAM_DROPOUT_F32: e = dropout_f32_prepare(plan, F(0), F(1), n, f); break;
    case MMDTI_STREAM_AXPY_F32: e = axpy_f32_prepare(plan, F(0), F(1), n); break;
    case MMDTI_STREAM_GELU_FWD_BF16: e = gelu_fwd_bf16_prepare(plan, ptrs[0], ptrs[1], n); break;
    case MMDTI_STREAM_COLSUM_BF16: e = colsum_bf16_prepare(plan, det, ptrs[0], a, b, c, F(1)); break;
    case MMDTI_STREAM_SUMSQ_F32: e = sumsq_f32_prepare(plan, det, F(0), n, F(1), F(2), a); break;
    case MMDTI_STREAM_SUMSQ_CHECK_F32: e = sumsq_check_f32_prepare(plan, F(0), n, F(1), F(2), a, F(3), b); break;
    case MMDTI_STREAM_ADAM_STEP: e = adam_step_prepare(plan, F(0), F(1), F(2), F(3), n, a, F(4)); break;
    case MMDTI_STREAM_ADAM_STEP_GUARDED: e = adam_step_guarded_prepare(plan, F(0), F(1), F(2), F(3), n, F(4)); break;
    case MMDTI_STREAM_ADAM_STEP_MASKED: e = adam_step_masked_prepare(plan, F(0), F(1), F(2), F(3), n, a, F(4), F(5), U8(6)); break;
    case MMDTI_STREAM_ADAM_STEP_GROUPED:
      e = adam_step_grouped_prepare(plan, F(0), F(1), F(2), F(3), ptrs[4], n, a, F(6), ptrs[5], F(7), U8(8), U8(9), F(10), b, c);
      break;
    case MMDTI_STREAM_EMA_UPDATE: e = ema_update_prepare(plan, F(0), F(1), n, f, a, F(2), F(3)); break;
    case MMDTI_STREAM_EMA_SWAP: e = ema_swap_prepare(plan, F(0), F(1), ptrs[2], ptrs[3], n); break;
    case MMDTI_STREAM_STEP_STATE_ADVANCE: e = step_state_advance_prepare(plan, F(0), static_cast<const unsigned long long*>(ptrs[1]), a, b); break;
    default: MMDTI_REQUIRE(false, "stream_plan: unknown entry %d", entry);
  }
  if (e) return e;
  static_assert(STREAM_PLAN_INTS == 12, "mmdti_hip.h documents 12 long long");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}

extern "C" int mmdti_seed_salt_pull(mmdti_stream_t stream, const unsigned long long* salt) {
  MMDTI_REQUIRE(salt != nullptr, "seed_salt_pull: null pointer");
  hipStream_t s = (hipStream_t)stream;
  salt_pull_gemm(s, salt);
  salt_pull_layernorm(s, salt);
  salt_pull_pair_attn(s, salt);
  salt_pull_pair_attn_bwd(s, salt);
  salt_pull_pair_attn_bwd_g16(s, salt);
  salt_pull_attn(s, salt);
  salt_pull_elementwise(s, salt);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

extern "C" int mmdti_probe_tr_read(mmdti_stream_t stream, int row_stride_elems, unsigned short* out) {
  MMDTI_REQUIRE(out && row_stride_elems >= 16 && row_stride_elems <= 64 && row_stride_elems % 4 == 0, "probe_tr_read: bad stride");
  hipLaunchKernelGGL(probe_tr_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, row_stride_elems, out);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}
