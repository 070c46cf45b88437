// lora.hip -- LoRA adapters on a Linear: the rank-r update W + s.B.A (s = alpha / r) applied next to the frozen base GEMM, never merged
// into its 16-bit weight (DESIGN.md "LoRA adapters").  x [T, in], A [r, in], B [out, r]; r is 8, 16 or 32, in and out multiples of 64.
//
//   mmdti_lora_fwd   t = bf16(x.A^T) [T, r], stored for the backward; y <- round16(float(y) + s.t.B^T) in place (y: what the base Linear
//                    wrote, possibly a column slice of a wider buffer).  One pass over x: t goes from the accumulators through LDS into
//                    the operand layout of the second product.  Two roundings are part of the contract: t to bf16, then y to its 16-bit
//                    type.  An element whose update s.(t.B^T) is zero keeps its bits (so B = 0 leaves y unchanged to the bit).
//   mmdti_lora_bwd   u = bf16(s.dy.B) [T, r], stored for mmdti_lora_dx; dB += s.dy^T.t; dA += u^T.x.  One pass over dy and x.
//   mmdti_lora_dx    dx += u.A in place, fp32 or bf16.
//
// All five products are v_mfma_f32_16x16x32 (bf16; fp16 for the forward in the fp16 forward-operand mode): lane l holds 8 consecutive k of
// row l & 15 of either operand, and 4 consecutive accumulator rows 4 (l >> 4) .. + 3 of column l & 15.  A rank below 32 fills the k (or
// row) positions past r with zeros in BOTH operands.  Which operand goes on the accumulator's row side is chosen so that a lane's
// accumulator registers are consecutive elements of the output's contiguous dimension; the rows of the small operand are permuted
// (row 16 g + 4 j + i of a 64-column block goes to tile j, row 4 g + i) so that a lane's four tiles are 16 consecutive columns.
// Launch geometry: lora_plan.h, nowhere else.
#include "common.h"
#include "lora_plan.h"

namespace mmdti {

typedef __bf16 lora_bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 lora_f16x8 __attribute__((ext_vector_type(8)));
typedef float lora_f32x4 __attribute__((ext_vector_type(4)));
typedef float lora_f32x8 __attribute__((ext_vector_type(8)));

template <bool F16>
__device__ __forceinline__ lora_f32x4 lora_mfma(const uint4& a, const uint4& b, const lora_f32x4& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(lora_f16x8, a), __builtin_bit_cast(lora_f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(lora_bf16x8, a), __builtin_bit_cast(lora_bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ uint4 lora_ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }
__device__ __forceinline__ void lora_st16(uint16_t* p, const uint4& v) { *reinterpret_cast<uint4*>(p) = v; }
__device__ __forceinline__ uint4 lora_zero16() { return make_uint4(0u, 0u, 0u, 0u); }
// eight bf16 -> eight fp16 (exact for 2^-14 <= |v| <= 65504; saturating past it, as every fp16 store of the library)
__device__ __forceinline__ uint4 lora_bf8_to_h8(const uint4& u) {
  const lora_f32x8 f = __builtin_convertvector(__builtin_bit_cast(lora_bf16x8, u), lora_f32x8);
  lora_f16x8 h = __builtin_convertvector(f, lora_f16x8);
  lora_f16x8 mx;
#pragma unroll
  for (int e = 0; e < 8; ++e) mx[e] = (_Float16)65504.f;
  h = __builtin_elementwise_max(__builtin_elementwise_min(h, mx), -mx);
  return __builtin_bit_cast(uint4, h);
}
// four fp32 -> four bf16 (8 bytes)
__device__ __forceinline__ uint2 lora_pack4(const lora_f32x4& v, float s) {
  return make_uint2((uint32_t)f2bf(s * v[0]) | ((uint32_t)f2bf(s * v[1]) << 16), (uint32_t)f2bf(s * v[2]) | ((uint32_t)f2bf(s * v[3]) << 16));
}
// rows m0 .. m0 + 7 of one column of an LDS image (base -> element [m0][col], ld elements per row): the transposed operand read
__device__ __forceinline__ uint4 lora_gather_t(const uint16_t* base, int ld) {
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) w[e] = (uint32_t)base[(2 * e) * ld] | ((uint32_t)base[(2 * e + 1) * ld] << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// one 16-bit element plus an fp32 update, rounded back to its type; a zero update keeps the bits
template <bool F16>
__device__ __forceinline__ uint32_t lora_add16(uint32_t bits, float d) {
  if (d == 0.f) return bits;
  if constexpr (F16) return (uint32_t)f2h_sat((float)__builtin_bit_cast(_Float16, (uint16_t)bits) + d);
  else return (uint32_t)f2bf(bf2f((bf16_t)bits) + d);
}
// eight 16-bit elements (one 16-byte chunk) += s * (d0 | d1)
template <bool F16>
__device__ __forceinline__ uint4 lora_add8(const uint4& o, const lora_f32x4& d0, const lora_f32x4& d1, float s) {
  const uint32_t w[4] = {o.x, o.y, o.z, o.w};
  uint32_t r[4];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    r[e] = lora_add16<F16>(w[e] & 0xffffu, s * d0[2 * e]) | (lora_add16<F16>(w[e] >> 16, s * d0[2 * e + 1]) << 16);
    r[2 + e] = lora_add16<F16>(w[2 + e] & 0xffffu, s * d1[2 * e]) | (lora_add16<F16>(w[2 + e] >> 16, s * d1[2 * e + 1]) << 16);
  }
  return make_uint4(r[0], r[1], r[2], r[3]);
}
// the row of the small operand that lane column c supplies to tile j of a 64-column block, so that accumulator (g, j, i) is column
// 16 g + 4 j + i of the block
__device__ __forceinline__ int lora_perm_row(int c, int j) { return 16 * (c >> 2) + 4 * j + (c & 3); }

extern __shared__ uint4 lora_smem[];

template <int R, bool F16, bool YF16>
__global__ __launch_bounds__(LORA_BLOCK) void lora_fwd_kernel(const uint16_t* __restrict__ x, int ldx, const uint16_t* __restrict__ A,
                                                              const uint16_t* __restrict__ B, uint16_t* __restrict__ y, int ldy,
                                                              uint16_t* __restrict__ t, int T, int n_in, int n_out, float s) {
  constexpr int NT = R > 16 ? 2 : 1, LT = R + 8;
  uint16_t* lt = reinterpret_cast<uint16_t*>(lora_smem);   // [LORA_ROWS][LT] bf16
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int wrow = w * 32;
  long long row[2];
  bool ok[2];
  const uint16_t* xp[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    row[q] = (long long)blockIdx.x * LORA_ROWS + wrow + q * 16 + c;
    ok[q] = row[q] < T;
    xp[q] = x + (ok[q] ? row[q] : 0) * ldx + 8 * g;
  }
  // t^T = A.x^T: accumulator (g, i) of tile j is t[row c][16 j + 4 g + i]
  lora_f32x4 acc[2][NT];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[q][j] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
  const uint16_t* ap[NT];
  bool aok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    aok[j] = 16 * j + c < R;
    ap[j] = A + (long long)(aok[j] ? 16 * j + c : 0) * n_in + 8 * g;
  }
  for (int k0 = 0; k0 < n_in; k0 += 32) {
    uint4 xf[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) xf[q] = ok[q] ? lora_ld16(xp[q] + k0) : lora_zero16();
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const uint4 af = aok[j] ? lora_ld16(ap[j] + k0) : lora_zero16();
#pragma unroll
      for (int q = 0; q < 2; ++q) acc[q][j] = lora_mfma<F16>(af, xf[q], acc[q][j]);
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int j = 0; j < NT; ++j)
      if (16 * j + 4 * g < R) {
        const uint2 v = lora_pack4(acc[q][j], 1.f);
        *reinterpret_cast<uint2*>(lt + (wrow + q * 16 + c) * LT + 16 * j + 4 * g) = v;
        if (ok[q]) *reinterpret_cast<uint2*>(t + row[q] * R + 16 * j + 4 * g) = v;
      }
  __syncthreads();
  // y^T += s.B.t^T: accumulator (g, i) of tile j is the update of y[row c][nb + 16 g + 4 j + i]
  uint4 tf[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    tf[q] = 8 * g < R ? lora_ld16(lt + (wrow + q * 16 + c) * LT + 8 * g) : lora_zero16();
    if constexpr (F16) tf[q] = lora_bf8_to_h8(tf[q]);
  }
  for (int nb = 0; nb < n_out; nb += 64) {
    lora_f32x4 d[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint4 bfr = 8 * g < R ? lora_ld16(B + (long long)(nb + lora_perm_row(c, j)) * R + 8 * g) : lora_zero16();
#pragma unroll
      for (int q = 0; q < 2; ++q) d[q][j] = lora_mfma<F16>(bfr, tf[q], lora_f32x4{0.f, 0.f, 0.f, 0.f});
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
      if (ok[q]) {
        uint16_t* yp = y + row[q] * ldy + nb + 16 * g;
        const uint4 o0 = lora_ld16(yp), o1 = lora_ld16(yp + 8);
        lora_st16(yp, lora_add8<YF16>(o0, d[q][0], d[q][1], s));
        lora_st16(yp + 8, lora_add8<YF16>(o1, d[q][2], d[q][3], s));
      }
  }
}

template <int R, bool DXBF>
__global__ __launch_bounds__(LORA_BLOCK) void lora_dx_kernel(const uint16_t* __restrict__ u, const uint16_t* __restrict__ A, void* __restrict__ dx,
                                                             int lddx, int T, int n_in) {
  constexpr int LT = R + 8;
  uint16_t* at = reinterpret_cast<uint16_t*>(lora_smem);   // A^T of the block: [LORA_COLS][LT] bf16
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  long long row[2];
  bool ok[2];
  uint4 uf[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    row[q] = (long long)blockIdx.x * LORA_ROWS + w * 32 + q * 16 + c;
    ok[q] = row[q] < T;
    uf[q] = ok[q] && 8 * g < R ? lora_ld16(u + row[q] * R + 8 * g) : lora_zero16();
  }
  for (int c0 = 0; c0 < n_in; c0 += LORA_COLS) {
    const int cbw = n_in - c0 < LORA_COLS ? n_in - c0 : LORA_COLS, cch = cbw / 8;
    __syncthreads();
    for (int q = threadIdx.x; q < R * cch; q += LORA_BLOCK) {
      const int rr = q / cch, cc = (q - rr * cch) * 8;
      const uint4 v = lora_ld16(A + (long long)rr * n_in + c0 + cc);
      const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int e = 0; e < 8; ++e) at[(cc + e) * LT + rr] = (uint16_t)(wv[e >> 1] >> (16 * (e & 1)));
    }
    __syncthreads();
    for (int nb = 0; nb < cbw; nb += 64) {
      lora_f32x4 d[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint4 af = 8 * g < R ? lora_ld16(at + (nb + lora_perm_row(c, j)) * LT + 8 * g) : lora_zero16();
#pragma unroll
        for (int q = 0; q < 2; ++q) d[q][j] = lora_mfma<false>(af, uf[q], lora_f32x4{0.f, 0.f, 0.f, 0.f});
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (ok[q]) {
          const long long off = row[q] * lddx + c0 + nb + 16 * g;
          if constexpr (DXBF) {
            uint16_t* p = reinterpret_cast<uint16_t*>(dx) + off;
            const uint4 o0 = lora_ld16(p), o1 = lora_ld16(p + 8);
            lora_st16(p, lora_add8<false>(o0, d[q][0], d[q][1], 1.f));
            lora_st16(p + 8, lora_add8<false>(o1, d[q][2], d[q][3], 1.f));
          } else {
            float4* p = reinterpret_cast<float4*>(reinterpret_cast<float*>(dx) + off);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              float4 o = p[j];
              o.x += d[q][j][0]; o.y += d[q][j][1]; o.z += d[q][j][2]; o.w += d[q][j][3];
              p[j] = o;
            }
          }
        }
    }
  }
}

struct LoraBwdArgs {
  const uint16_t *x, *dy, *t, *B;
  uint16_t* u;
  float *dA, *dB, *ws;
  long long slab_floats;
  int ldx, lddy, T, n_in, n_out, chunk_rows;
  float s;
};

// a partial sum into the gradient: an atomic (default), or the workgroup's own slab (SLAB: plain store for its first chunk, add after)
template <bool SLAB>
__device__ __forceinline__ void lora_flush(float* p, float v, bool first) {
  if constexpr (SLAB) *p = first ? v : *p + v;
  else atomicAdd(p, v);
}

// [LORA_SUB][cbw] of a 16-bit matrix (row stride ld, rows past T read as zero) -> the LDS tile; CVT: fp16 -> bf16 on the way
template <bool CVT>
__device__ __forceinline__ void lora_stage_tile(uint16_t* tile, const uint16_t* __restrict__ src, int ld, long long row0, int T, int c0, int cbw) {
  const int cch = cbw / 8;
  for (int q = threadIdx.x; q < LORA_SUB * cch; q += LORA_BLOCK) {
    const int r = q / cch, cc = (q - r * cch) * 8;
    uint4 v = row0 + r < T ? lora_ld16(src + (row0 + r) * ld + c0 + cc) : lora_zero16();
    if constexpr (CVT) v = h2bf8(v);
    lora_st16(tile + r * LORA_TILE_LD + cc, v);
  }
}

template <int R, bool XF16, bool SLAB>
__global__ __launch_bounds__(LORA_BLOCK) void lora_bwd_kernel(LoraBwdArgs a) {
  constexpr int NT = R > 16 ? 2 : 1, LT = R + 8, TLD = LORA_TILE_LD;
  uint16_t* tile = reinterpret_cast<uint16_t*>(lora_smem);   // [LORA_SUB][TLD]: the dy block, then the x block
  uint16_t* wt = tile + LORA_SUB * TLD;                      // B^T of the block: [R][TLD]
  uint16_t* tt = wt + R * TLD;                               // t of the tile: [LORA_SUB][LT]
  uint16_t* ut = tt + LORA_SUB * LT;                         // u of the chunk: [LORA_MAX_CHUNK][LT]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
  const int nsc = a.chunk_rows / LORA_SUB;
  const long long nchunks = ((long long)a.T + a.chunk_rows - 1) / a.chunk_rows;
  float* dBo = SLAB ? a.ws + (long long)blockIdx.x * a.slab_floats : a.dB;
  float* dAo = SLAB ? dBo + (long long)a.n_out * R : a.dA;
  bool rok[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) rok[j] = 16 * j + c < R;

  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const bool first = chunk == (long long)blockIdx.x;
    const long long crow0 = chunk * a.chunk_rows;
    // ---- dy: u^T = B^T.dy^T (accumulator (g, i) of tile j: u[row c][16 j + 4 g + i]) and dB = dy^T.t, block by block of `out` ----
    lora_f32x4 uacc[4][NT];
#pragma unroll
    for (int sc = 0; sc < 4; ++sc)
#pragma unroll
      for (int j = 0; j < NT; ++j) uacc[sc][j] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < a.n_out; c0 += LORA_COLS) {
      const int cbw = a.n_out - c0 < LORA_COLS ? a.n_out - c0 : LORA_COLS;
      __syncthreads();
      for (int q = threadIdx.x; q < cbw * (R / 8); q += LORA_BLOCK) {
        const int col = q / (R / 8), rq = (q - col * (R / 8)) * 8;
        const uint4 v = lora_ld16(a.B + (long long)(c0 + col) * R + rq);
        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) wt[(rq + e) * TLD + col] = (uint16_t)(wv[e >> 1] >> (16 * (e & 1)));
      }
      lora_f32x4 dbacc[4][NT];
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < NT; ++j) dbacc[q][j] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sc = 0; sc < 4; ++sc)
        if (sc < nsc) {
          const long long srow0 = crow0 + sc * LORA_SUB;
          __syncthreads();
          lora_stage_tile<false>(tile, a.dy, a.lddy, srow0, a.T, c0, cbw);
          for (int q = threadIdx.x; q < LORA_SUB * (R / 8); q += LORA_BLOCK) {
            const int r = q / (R / 8), rq = (q - r * (R / 8)) * 8;
            lora_st16(tt + r * LT + rq, srow0 + r < a.T ? lora_ld16(a.t + (srow0 + r) * R + rq) : lora_zero16());
          }
          __syncthreads();
          for (int k0 = 0; k0 < cbw; k0 += 32) {
            const uint4 dyf = lora_ld16(tile + (16 * w + c) * TLD + k0 + 8 * g);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
              const uint4 bfr = rok[j] ? lora_ld16(wt + (16 * j + c) * TLD + k0 + 8 * g) : lora_zero16();
              uacc[sc][j] = lora_mfma<false>(bfr, dyf, uacc[sc][j]);
            }
          }
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            uint4 tfr[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) tfr[j] = rok[j] ? lora_gather_t(tt + (32 * ks + 8 * g) * LT + 16 * j + c, LT) : lora_zero16();
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if ((4 * w + q) * 16 < cbw) {
                const uint4 dyt = lora_gather_t(tile + (32 * ks + 8 * g) * TLD + (4 * w + q) * 16 + c, TLD);
#pragma unroll
                for (int j = 0; j < NT; ++j) dbacc[q][j] = lora_mfma<false>(dyt, tfr[j], dbacc[q][j]);
              }
          }
        }
      // accumulator (g, i) of (q, j): dB[c0 + 16 (4 w + q) + 4 g + i][16 j + c]
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if ((4 * w + q) * 16 < cbw)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            if (rok[j])
#pragma unroll
              for (int i = 0; i < 4; ++i)
                lora_flush<SLAB>(dBo + (long long)(c0 + (4 * w + q) * 16 + 4 * g + i) * R + 16 * j + c, a.s * dbacc[q][j][i], first);
    }
    // ---- u = bf16(s.dy.B): to memory for mmdti_lora_dx, to LDS for dA ----
#pragma unroll
    for (int sc = 0; sc < 4; ++sc)
      if (sc < nsc)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          if (16 * j + 4 * g < R) {
            const uint2 v = lora_pack4(uacc[sc][j], a.s);
            const long long r = crow0 + sc * LORA_SUB + 16 * w + c;
            *reinterpret_cast<uint2*>(ut + (sc * LORA_SUB + 16 * w + c) * LT + 16 * j + 4 * g) = v;
            if (r < a.T) *reinterpret_cast<uint2*>(a.u + r * R + 16 * j + 4 * g) = v;
          }
    // ---- x: dA = u^T.x, block by block of `in` (accumulator (g, i) of (j, q): dA[16 j + 4 g + i][c0 + 16 (4 w + q) + c]) ----
    for (int c0 = 0; c0 < a.n_in; c0 += LORA_COLS) {
      const int cbw = a.n_in - c0 < LORA_COLS ? a.n_in - c0 : LORA_COLS;
      lora_f32x4 daacc[NT][4];
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) daacc[j][q] = lora_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int sc = 0; sc < 4; ++sc)
        if (sc < nsc) {
          __syncthreads();
          lora_stage_tile<XF16>(tile, a.x, a.ldx, crow0 + sc * LORA_SUB, a.T, c0, cbw);
          __syncthreads();
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            uint4 ufr[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j)
              ufr[j] = rok[j] ? lora_gather_t(ut + (sc * LORA_SUB + 32 * ks + 8 * g) * LT + 16 * j + c, LT) : lora_zero16();
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if ((4 * w + q) * 16 < cbw) {
                const uint4 xt = lora_gather_t(tile + (32 * ks + 8 * g) * TLD + (4 * w + q) * 16 + c, TLD);
#pragma unroll
                for (int j = 0; j < NT; ++j) daacc[j][q] = lora_mfma<false>(ufr[j], xt, daacc[j][q]);
              }
          }
        }
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if ((4 * w + q) * 16 < cbw)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (16 * j + 4 * g + i < R)
                lora_flush<SLAB>(dAo + (long long)(16 * j + 4 * g + i) * a.n_in + c0 + (4 * w + q) * 16 + c, daacc[j][q][i], first);
    }
  }
}

// every instance, at the row lora_plan.h gives it
static KernelRow g_lora_kernels[LORA_KERNELS] = {
#define LORA_ROWS_OF(R)                                                                                                          \
  KROW(lora_fwd_key(R, 0, 0), lora_fwd_kernel<R, false, false>), KROW(lora_fwd_key(R, 1, 1), lora_fwd_kernel<R, true, true>),   \
  KROW(lora_fwd_key(R, 1, 0), lora_fwd_kernel<R, true, false>)
    LORA_ROWS_OF(8), LORA_ROWS_OF(16), LORA_ROWS_OF(32),
#undef LORA_ROWS_OF
#define LORA_ROWS_OF(R)                                                                                                          \
  KROW(lora_bwd_key(R, 0, 0), lora_bwd_kernel<R, false, false>), KROW(lora_bwd_key(R, 0, 1), lora_bwd_kernel<R, false, true>),   \
  KROW(lora_bwd_key(R, 1, 0), lora_bwd_kernel<R, true, false>), KROW(lora_bwd_key(R, 1, 1), lora_bwd_kernel<R, true, true>)
    LORA_ROWS_OF(8), LORA_ROWS_OF(16), LORA_ROWS_OF(32),
#undef LORA_ROWS_OF
#define LORA_ROWS_OF(R)                                                                                                          \
  KROW(lora_dx_key(R, 0), lora_dx_kernel<R, false>), KROW(lora_dx_key(R, 1), lora_dx_kernel<R, true>)
    LORA_ROWS_OF(8), LORA_ROWS_OF(16), LORA_ROWS_OF(32),
#undef LORA_ROWS_OF
};
const KernelRow* lora_kernel_table(int* n) { *n = LORA_KERNELS; return g_lora_kernels; }

// the shape limits of the three entry points (`who` names the caller in the message)
static int lora_check_shape(const char* who, int T, int n_in, int n_out, int r) {
  MMDTI_REQUIRE(lora_rank_ok(r), "%s: the rank must be 8, 16 or 32 (got %d)", who, r);
  MMDTI_REQUIRE(T >= 1, "%s: T must be at least 1 (got %d)", who, T);
  MMDTI_REQUIRE(n_in >= 64 && n_in % 64 == 0 && n_in <= LORA_MAX_DIM, "%s: in must be a multiple of 64 in [64, %d] (got %d)", who, LORA_MAX_DIM, n_in);
  MMDTI_REQUIRE(n_out >= 64 && n_out % 64 == 0 && n_out <= LORA_MAX_DIM, "%s: out must be a multiple of 64 in [64, %d] (got %d)", who, LORA_MAX_DIM,
                n_out);
  return MMDTI_OK;
}
static int lora_launch(const LoraPlan& plan, void** args, hipStream_t s, const char* who) {
  KernelRow& row = g_lora_kernels[plan.k[0].key];
  if (int e = ensure_dynamic_lds(row.fn, (size_t)plan.k[0].lds, &row.lds_have, who)) return e;
  (void)hipLaunchKernel(row.fn, dim3((unsigned)plan.k[0].gx, (unsigned)plan.k[0].gy), dim3((unsigned)plan.k[0].block), args, (size_t)plan.k[0].lds, s);
  MMDTI_LAUNCH_CHECK();
  return MMDTI_OK;
}

}  // namespace mmdti
using namespace mmdti;

extern "C" int mmdti_lora_fwd(mmdti_stream_t stream, const void* x, int ldx, const void* A, const void* B, void* y, int ldy, void* t_bf16, int T,
                              int n_in, int n_out, int r, float scale, int f16, int y_f16) {
  MMDTI_REQUIRE(f16 || !y_f16, "lora_fwd: an fp16 y needs fp16 operands");
  if (int e = lora_check_shape("lora_fwd", T, n_in, n_out, r)) return e;
  MMDTI_REQUIRE(x && A && B && y && t_bf16, "lora_fwd: null x, A, B, y or t");
  MMDTI_REQUIRE(ldx >= n_in && ldx % 8 == 0 && ldy >= n_out && ldy % 8 == 0, "lora_fwd: row strides must cover in / out and be multiples of 8");
  MMDTI_REQUIRE(aligned16(x) && aligned16(A) && aligned16(B) && aligned16(y) && aligned16(t_bf16), "lora_fwd: x, A, B, y and t need 16-byte alignment");
  const LoraPlan plan = lora_fwd_plan(T, r, f16 != 0, y_f16 != 0);
  const uint16_t *xp = reinterpret_cast<const uint16_t*>(x), *Ap = reinterpret_cast<const uint16_t*>(A), *Bp = reinterpret_cast<const uint16_t*>(B);
  uint16_t *yp = reinterpret_cast<uint16_t*>(y), *tp = reinterpret_cast<uint16_t*>(t_bf16);
  void* args[] = {&xp, &ldx, &Ap, &Bp, &yp, &ldy, &tp, &T, &n_in, &n_out, &scale};
  return lora_launch(plan, args, (hipStream_t)stream, "lora_fwd");
}

extern "C" int mmdti_lora_bwd(mmdti_stream_t stream, const void* x, int ldx, int x_f16, const void* dy_bf16, int lddy, const void* t_bf16,
                              const void* B_bf16, void* u_bf16, float* dA, float* dB, int T, int n_in, int n_out, int r, float scale) {
  if (int e = lora_check_shape("lora_bwd", T, n_in, n_out, r)) return e;
  MMDTI_REQUIRE(x && dy_bf16 && t_bf16 && B_bf16 && u_bf16 && dA && dB, "lora_bwd: null x, dy, t, B, u, dA or dB");
  MMDTI_REQUIRE(ldx >= n_in && ldx % 8 == 0 && lddy >= n_out && lddy % 8 == 0, "lora_bwd: row strides must cover in / out and be multiples of 8");
  MMDTI_REQUIRE(aligned16(x) && aligned16(dy_bf16) && aligned16(t_bf16) && aligned16(B_bf16) && aligned16(u_bf16),
                "lora_bwd: x, dy, t, B and u need 16-byte alignment");
  MMDTI_REQUIRE((reinterpret_cast<uintptr_t>(dA) & 3) == 0 && (reinterpret_cast<uintptr_t>(dB) & 3) == 0, "lora_bwd: dA and dB need 4-byte alignment");
  const bool det = det_table().on();
  const LoraPlan plan = lora_bwd_plan(T, r, n_in, n_out, x_f16 != 0, det);
  LoraBwdArgs a = {};
  if (det) {
    if (int e = det_workspace(stream, lora_det_bytes(T, r, n_in, n_out), "lora_bwd", &a.ws)) return e;
  }
  a.x = reinterpret_cast<const uint16_t*>(x); a.dy = reinterpret_cast<const uint16_t*>(dy_bf16); a.t = reinterpret_cast<const uint16_t*>(t_bf16);
  a.B = reinterpret_cast<const uint16_t*>(B_bf16); a.u = reinterpret_cast<uint16_t*>(u_bf16);
  a.dA = dA; a.dB = dB; a.slab_floats = plan.slab_floats;
  a.ldx = ldx; a.lddy = lddy; a.T = T; a.n_in = n_in; a.n_out = n_out; a.chunk_rows = (int)plan.chunk_rows; a.s = scale;
  void* args[] = {&a};
  if (int e = lora_launch(plan, args, (hipStream_t)stream, "lora_bwd")) return e;
  if (det) {
    const int nslab = (int)plan.k[0].gx;
    det_fold<1>((hipStream_t)stream, a.ws, nslab, plan.slab_floats, n_out * r, DetDst<1>{{dB}});
    det_fold<1>((hipStream_t)stream, a.ws + (long long)n_out * r, nslab, plan.slab_floats, r * n_in, DetDst<1>{{dA}});
    MMDTI_LAUNCH_CHECK();
  }
  return MMDTI_OK;
}

extern "C" int mmdti_lora_dx(mmdti_stream_t stream, const void* u_bf16, const void* A_bf16, void* dx, int lddx, int dx_bf16, int T, int n_in, int r) {
  if (int e = lora_check_shape("lora_dx", T, n_in, 64, r)) return e;
  MMDTI_REQUIRE(u_bf16 && A_bf16 && dx, "lora_dx: null u, A or dx");
  MMDTI_REQUIRE(lddx >= n_in && lddx % 8 == 0, "lora_dx: the row stride must cover in and be a multiple of 8");
  MMDTI_REQUIRE(aligned16(u_bf16) && aligned16(A_bf16) && aligned16(dx), "lora_dx: u, A and dx need 16-byte alignment");
  const LoraPlan plan = lora_dx_plan(T, r, dx_bf16 != 0);
  const uint16_t *up = reinterpret_cast<const uint16_t*>(u_bf16), *Ap = reinterpret_cast<const uint16_t*>(A_bf16);
  void* args[] = {&up, &Ap, &dx, &lddx, &T, &n_in};
  return lora_launch(plan, args, (hipStream_t)stream, "lora_dx");
}

extern "C" int mmdti_lora_plan(int entry, int deterministic, int T, int n_in, int n_out, int r, int flag, long long* plan_out) {
  MMDTI_REQUIRE(plan_out != nullptr, "lora_plan: null plan_out");
  MMDTI_REQUIRE(entry >= 0 && entry <= 2, "lora_plan: entry must be 0 (lora_fwd), 1 (lora_bwd) or 2 (lora_dx), got %d", entry);
  static const char* const who[3] = {"lora_fwd", "lora_bwd", "lora_dx"};
  if (int e = lora_check_shape(who[entry], T, n_in, entry == 2 ? 64 : n_out, r)) return e;
  MMDTI_REQUIRE(entry != 0 || (flag >= 0 && flag <= 2), "lora_plan: the forward's flag is 0 (bf16), 1 (fp16) or 2 (fp16 operands, bf16 y), got %d", flag);
  const LoraPlan plan = entry == 0   ? lora_fwd_plan(T, r, flag != 0, flag == 1)
                        : entry == 1 ? lora_bwd_plan(T, r, n_in, n_out, flag != 0, deterministic != 0)
                                     : lora_dx_plan(T, r, flag != 0);
  static_assert(LORA_PLAN_WORDS == 18, "mmdti_hip.h documents 18 words");
  memcpy(plan_out, &plan, sizeof(plan));
  return MMDTI_OK;
}
