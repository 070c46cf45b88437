// How the three LoRA kernels (mmdti_lora_fwd, mmdti_lora_bwd, mmdti_lora_dx of lora.hip) are launched -- decided here, in plain host
// C++17 (no HIP types), and nowhere else.  The entry points validate, ask one of the plan functions below and launch what the plan names
// from one table (g_lora_kernels, indexed by the plan's key); mmdti_lora_plan returns the same plan without launching
// (tests/test_lora_cpu.py holds it to the independent statement of tests/lora_cases.py over a sweep).
//
// One adapted Linear: x [T, in], A [r, in], B [out, r], s = alpha / r.  r is 8, 16 or 32; in and out are multiples of 64.
//   forward   one workgroup of four waves per 128 token rows (two 16-row MFMA tiles per wave); t = x.A^T goes through LDS
//             ([128][r + 8] bf16) from the accumulator layout into the operand layout of the second product, which walks y in blocks of
//             64 columns.
//   dx        the same rows per workgroup; A^T is staged per block of 256 columns of `in` ([256][r + 8] bf16 of LDS), so the LDS does not
//             grow with `in`.
//   backward  a workgroup owns CHUNKS of 64, 128 or 256 token rows (the fewest rows that still give every CU a chunk: its dA / dB partial
//             is r (in + out) floats per chunk, so more rows per chunk mean fewer adds into the gradient) and walks `out`, then `in`, in
//             blocks of 256 columns through one [64][264] bf16 LDS tile that is read row-wise and transposed.  Default: one chunk per
//             workgroup, partials meet in fp32 atomics.  Deterministic: at most LORA_DET_WGS workgroups stride over the chunks, each adds
//             into its own slab [out r | r in] of the stream's workspace in chunk order, and two det_fold launches (dB, dA) sum the slabs
//             in workgroup order.
#pragma once
#include "row_plan.h"

namespace mmdti {

constexpr int LORA_KERNELS = 27;
constexpr int LORA_BLOCK = 256;            // four waves
constexpr int LORA_ROWS = 128;             // forward / dx: token rows per workgroup
constexpr int LORA_COLS = 256;             // dx / backward: columns per staged block
constexpr int LORA_TILE_LD = LORA_COLS + 8;   // bf16 elements per LDS row of a staged block (16-byte rows, 2-way on the transposed read)
constexpr int LORA_SUB = 64;               // backward: token rows per staged tile
constexpr int LORA_MAX_CHUNK = 256;        // backward: most token rows per chunk (u's accumulators stay in registers)
constexpr int LORA_DET_WGS = 64;           // backward, deterministic: most workgroups (= slabs)
constexpr int LORA_MAX_DIM = 8192;         // in, out
constexpr int LORA_CUS = 256;

constexpr bool lora_rank_ok(int r) { return r == 8 || r == 16 || r == 32; }
constexpr int lora_rank_index(int r) { return r == 8 ? 0 : r == 16 ? 1 : 2; }
// lora_fwd_kernel<R, F16, YF16> 0..8 (bf16 | fp16 | fp16 operands beside a bf16 y: tower 2 and the cross block store q, k, v as bf16
// in every mode); lora_bwd_kernel<R, XF16, SLAB> 9..20; lora_dx_kernel<R, DXBF16> 21..26
constexpr int lora_fwd_key(int r, int f16, int y_f16) { return lora_rank_index(r) * 3 + (f16 ? (y_f16 ? 1 : 2) : 0); }
constexpr int lora_bwd_key(int r, int x_f16, int slab) { return 9 + lora_rank_index(r) * 4 + x_f16 * 2 + slab; }
constexpr int lora_dx_key(int r, int dx_bf16) { return 21 + lora_rank_index(r) * 2 + dx_bf16; }

struct LoraPlan {
  long long nlaunch;       // 1; 3 for the deterministic backward (slab kernel, det_fold_kernel<1> over dB, det_fold_kernel<1> over dA)
  PlanLaunch k[3];
  long long chunk_rows;    // token rows per workgroup (forward, dx) or per chunk (backward)
  long long slab_floats;   // deterministic backward: floats per workgroup slab (else 0)
};
constexpr int LORA_PLAN_WORDS = sizeof(LoraPlan) / sizeof(long long);

static inline long long lora_fwd_lds(int r) { return (long long)LORA_ROWS * (r + 8) * 2; }
static inline long long lora_dx_lds(int r) { return (long long)LORA_COLS * (r + 8) * 2; }
// the staged tile | B^T of the block [r][264] | t of the tile [64][r + 8] | u of the chunk [256][r + 8]
static inline long long lora_bwd_lds(int r) {
  return ((long long)LORA_SUB * LORA_TILE_LD + (long long)r * LORA_TILE_LD + (long long)LORA_SUB * (r + 8) + (long long)LORA_MAX_CHUNK * (r + 8)) * 2;
}
static inline int lora_bwd_chunk_rows(long long T) {
  const long long per = (T + LORA_CUS - 1) / LORA_CUS;
  return per <= 64 ? 64 : per <= 128 ? 128 : LORA_MAX_CHUNK;
}
static inline long long lora_slab_floats(int r, int n_in, int n_out) { return (long long)r * ((long long)n_in + n_out); }
// bytes of the stream's reduction workspace the deterministic backward needs
static inline long long lora_det_bytes(long long T, int r, int n_in, int n_out) {
  const long long chunks = (T + lora_bwd_chunk_rows(T) - 1) / lora_bwd_chunk_rows(T);
  return (chunks < LORA_DET_WGS ? chunks : LORA_DET_WGS) * lora_slab_floats(r, n_in, n_out) * 4;
}

// (arguments already validated by the entry point)
static inline LoraPlan lora_fwd_plan(long long T, int r, bool f16, bool y_f16) {
  LoraPlan p = {};
  p.nlaunch = 1; p.chunk_rows = LORA_ROWS;
  p.k[0] = {lora_fwd_key(r, f16, y_f16), (T + LORA_ROWS - 1) / LORA_ROWS, 1, LORA_BLOCK, lora_fwd_lds(r)};
  return p;
}
static inline LoraPlan lora_dx_plan(long long T, int r, bool dx_bf16) {
  LoraPlan p = {};
  p.nlaunch = 1; p.chunk_rows = LORA_ROWS;
  p.k[0] = {lora_dx_key(r, dx_bf16), (T + LORA_ROWS - 1) / LORA_ROWS, 1, LORA_BLOCK, lora_dx_lds(r)};
  return p;
}
static inline LoraPlan lora_bwd_plan(long long T, int r, int n_in, int n_out, bool x_f16, bool slab) {
  LoraPlan p = {};
  p.chunk_rows = lora_bwd_chunk_rows(T);
  const long long chunks = (T + p.chunk_rows - 1) / p.chunk_rows;
  p.nlaunch = slab ? 3 : 1;
  p.k[0] = {lora_bwd_key(r, x_f16, slab), slab && chunks > LORA_DET_WGS ? LORA_DET_WGS : chunks, 1, LORA_BLOCK, lora_bwd_lds(r)};
  if (slab) {
    p.slab_floats = lora_slab_floats(r, n_in, n_out);
    p.k[1] = det_fold_launch(n_out * r, 1);
    p.k[2] = det_fold_launch(r * n_in, 1);
  }
  return p;
}

}  // namespace mmdti
