// Which kernel a streaming, reduction or optimizer call of elementwise.hip runs, and with which grid -- decided here, in plain host
// C++17 (no HIP types), and nowhere else.  The entry points validate, ask one of the plan functions below, and launch what the plan
// names from one table (g_stream_kernels, indexed by the plan's key); mmdti_stream_plan returns the same plan without launching
// (tests/test_stream_cases_cpu.py, test_adam_group_cases_cpu.py and test_ema_cpu.py ask it for every case and sweep the sizes past them).
// det.h sizes the deterministic column sum's workspace from colsum_grid_y.
#pragma once
#include "row_plan.h"

namespace mmdti {

// ---- geometry ----
// grid-stride streams: at most 16 workgroups of 256 per CU's worth of 256 CUs, at least one
constexpr int STREAM_GRID_CAP = 256 * 16;
static inline int grid_for(long long n, int per_block) {
  long long b = (n + per_block - 1) / per_block;
  if (b > STREAM_GRID_CAP) b = STREAM_GRID_CAP;
  if (b < 1) b = 1;
  return (int)b;
}
// elements a workgroup of 256 takes per round: the sum of squares' atomic form, the Adam pass and the EMA update, the grouped Adam
// pass and the EMA swap (one thread per block of 8)
constexpr int SUMSQ_PER_WG = 256 * 8, ADAM_PER_WG = 256 * 4, ADAM_GROUP_PER_WG = 256 * 8, EMA_UPDATE_PER_WG = 256 * 4, EMA_SWAP_PER_WG = 256 * 8;
// column sum: 8 rows per thread (two rounds of four 16-byte loads): enough workgroups to fill 256 CUs several times over -- the
// reduction is latency-bound at one workgroup per CU.  Row groups (grid.y):
static inline int colsum_grid_y(int rows) {
  const int gy = (int)(((long long)rows + 8 * 8 - 1) / (8 * 8));
  return gy > 1024 ? 1024 : gy;
}
// The reproducible sum of squares: one partial per workgroup, at most SUMSQ_WGS and at most `parts` (the partials the caller's workspace
// holds: ws_floats, or ws_floats / 2 next to the non-finite counts -- the same partials, so the same sum to the bit)
constexpr int SUMSQ_WGS = 2048;
static inline int sumsq_wgs(long long n, int parts) {
  const long long want = (n / 4 + 255) / 256 + 1, have = parts < SUMSQ_WGS ? parts : SUMSQ_WGS;
  return (int)(have < want ? have : want);
}

// ---- the instance key: a dense index into g_stream_kernels ----
constexpr int STREAM_KERNELS = 29;
enum StreamKey {
  SK_CAST_F32_BF16 = 0,   // cast_f32_bf16_kernel<F16>: + F16
  SK_CAST_F16_BF16 = 2, SK_CAST_BF16_F32 = 3, SK_DROPOUT = 4, SK_AXPY = 5, SK_GELU = 6, SK_COLSUM = 7, SK_COLSUM_SLAB = 8, SK_SUMSQ = 9,
  SK_SUMSQ_PART = 10,     // sumsq_part_kernel<CHECK>, sumsq_fold_kernel<CHECK>: 10, 11 | 12, 13
  SK_ADAM = 14,           // adam_kernel<GUARD, MASK>: + GUARD + 2 MASK
  SK_STEP_STATE = 18,
  SK_ADAM_GROUP = 19,     // adam_group_kernel<GUARD, MASK, DECOUPLED>: + 4 GUARD + 2 MASK + DECOUPLED
  SK_EMA_UPDATE = 27, SK_EMA_SWAP = 28
};
constexpr int sumsq_part_key(int check) { return SK_SUMSQ_PART + 2 * check; }
constexpr int sumsq_fold_key(int check) { return SK_SUMSQ_PART + 2 * check + 1; }
// The Adam instance is a function of the entry point and of which optional pointers are given:
// mmdti_adam_step <false, false>; _guarded <true, false>; _masked <guard given, true>; _grouped <guard given, skip given, decoupled>
enum AdamEntry { ADAM_STEP = 0, ADAM_STEP_GUARDED = 1, ADAM_STEP_MASKED = 2, ADAM_STEP_GROUPED = 3 };
constexpr int adam_key(int entry, bool guard, bool skip, bool decoupled) {
  return entry == ADAM_STEP           ? SK_ADAM
         : entry == ADAM_STEP_GUARDED ? SK_ADAM + 1
         : entry == ADAM_STEP_MASKED  ? SK_ADAM + (guard ? 1 : 0) + 2
                                      : SK_ADAM_GROUP + 4 * (guard ? 1 : 0) + 2 * (skip ? 1 : 0) + (decoupled ? 1 : 0);
}

struct StreamPlan {
  long long nlaunch;   // 0 (an empty arena where the entry admits one), 1, or 2 (slab kernel + det_fold_kernel<1>; partials + fold)
  PlanLaunch k[2];
  long long wgs;       // sum of squares with a workspace: workgroups = partials (else 0)
};
constexpr int STREAM_PLAN_INTS = sizeof(StreamPlan) / sizeof(long long);

// (arguments already validated by the entry point)
// one grid-stride launch of workgroups of 256 over `items` work items, `per_block` of them per workgroup and round
static inline StreamPlan stream_plan(int key, long long items, int per_block) {
  StreamPlan p = {};
  p.nlaunch = 1;
  p.k[0] = {key, grid_for(items, per_block), 1, 256, 0};
  return p;
}
// fp32 -> bf16 / fp16: one float4 per thread; the n % 4 tail rides on workgroup 0 (hence the + 1)
static inline StreamPlan cast_f32_16_plan(long long n, bool f16) { return stream_plan(SK_CAST_F32_BF16 + (f16 ? 1 : 0), n / 4 + 1, 256); }
// fp16 -> bf16: 8 elements per thread
static inline StreamPlan cast_f16_bf16_plan(int rows, int cols) { return stream_plan(SK_CAST_F16_BF16, (long long)rows * (cols / 8), 256); }
// slab (the deterministic mode): one row of the stream's workspace per row group, folded in row-group order (never atomics)
static inline StreamPlan colsum_plan(int rows, int cols, bool slab) {
  StreamPlan p = {};
  p.nlaunch = slab ? 2 : 1;
  p.k[0] = {slab ? SK_COLSUM_SLAB : SK_COLSUM, ((long long)cols + 255) / 256, colsum_grid_y(rows), 256, 0};
  if (slab) p.k[1] = det_fold_launch(cols, 1);
  return p;
}
// parts == 0: the atomic form
static inline StreamPlan sumsq_plan(long long n, int parts, bool check) {
  if (parts == 0) return stream_plan(SK_SUMSQ, n, SUMSQ_PER_WG);
  StreamPlan p = {};
  p.nlaunch = 2; p.wgs = sumsq_wgs(n, parts);
  p.k[0] = {sumsq_part_key(check), p.wgs, 1, 256, 0};
  p.k[1] = {sumsq_fold_key(check), 1, 1, 256, 0};
  return p;
}
static inline StreamPlan adam_plan(int entry, long long n, bool guard, bool skip, bool decoupled) {
  if (n == 0) return StreamPlan{};   // no launch (only mmdti_adam_step_grouped admits an empty arena)
  return stream_plan(adam_key(entry, guard, skip, decoupled), n, entry == ADAM_STEP_GROUPED ? ADAM_GROUP_PER_WG : ADAM_PER_WG);
}
static inline StreamPlan ema_plan(bool swap, long long n) {
  if (n == 0) return StreamPlan{};   // no launch
  return swap ? stream_plan(SK_EMA_SWAP, n, EMA_SWAP_PER_WG) : stream_plan(SK_EMA_UPDATE, n, EMA_UPDATE_PER_WG);
}
static inline StreamPlan step_state_plan() {
  StreamPlan p = {};
  p.nlaunch = 1;
  p.k[0] = {SK_STEP_STATE, 1, 1, 1, 0};
  return p;
}

}  // namespace mmdti
