// Which kernel a LayerNorm or row-softmax call runs, with which grid, LDS and follow-up pass -- decided here, in plain host C++17 (no HIP
// types), and nowhere else.  The entry points of layernorm.hip and the softmax pair of elementwise.hip validate, ask one of the plan
// functions below, and launch what the plan names from the MMDTI_PLAN_ROW table (rows 0..19 in layernorm.hip, 20..25 next to the softmax
// kernels); mmdti_row_plan returns the same plan without launching (tests/test_row_cases_cpu.py asks it for every case and sweeps the
// shapes past them).  det.h sizes the deterministic mode's workspace from the same functions.
#pragma once

namespace mmdti {

// ---- geometry: one wave per row, four rows per workgroup of 256 ----
// LayerNorm: float4 columns per lane (D <= 2048: 1..8); the instance that serves them is <1>, <2>, <4> (3, 4) or <8> (5..8)
static inline int ln_nv(int D) { return (D / 4 + 63) / 64; }
static inline int ln_inst_nv(int D) { return ln_nv(D) <= 2 ? ln_nv(D) : ln_nv(D) <= 4 ? 4 : 8; }
// LayerNorm backward, rows per wave: enough that the whole grid is resident at once (3 workgroups of 4 waves per CU at this kernel's
// register count, 2 for the wide-row variants) -- no second, partly filled round, and fewer dgamma / dbeta atomics
constexpr int LN_BWD_MIN_ROWS_PER_WAVE = 4;
static inline int ln_bwd_rows_per_wave(int rows, int D) {
  const int per = 4 * (ln_nv(D) <= 2 ? 3 : 2) * 256, r = (int)(((long long)rows + per - 1) / per);
  return r > LN_BWD_MIN_ROWS_PER_WAVE ? r : LN_BWD_MIN_ROWS_PER_WAVE;
}
static inline int ln_bwd_grid(int rows, int D) {
  const int per = 4 * ln_bwd_rows_per_wave(rows, D);
  return (int)(((long long)rows + per - 1) / per);
}
// row softmax: 4 consecutive keys per lane and chunk of 256 (ld <= 1024); the instance is <1>, <2> or <4> (3, 4)
static inline int sm_inst_nv(int ld) { return (ld + 255) / 256 <= 2 ? (ld + 255) / 256 : 4; }

// ---- the instance key: a dense index into the MMDTI_PLAN_ROW table ----
constexpr int ROW_KERNELS = 26, ROW_LN_KERNELS = 20;
constexpr int row_nv_index(int nv) { return nv == 1 ? 0 : nv == 2 ? 1 : nv == 4 ? 2 : 3; }
// ln_fwd_kernel<NV> 0..3; ln_bwd_kernel<NV, DY_BF16> 4..11 and ln_bwd_slab_kernel<NV, DY_BF16> 12..19 by (NV, DY_BF16);
// softmax_fwd_kernel<NV> 20..22; softmax_bwd_kernel<NV> 23..25
constexpr int ln_fwd_key(int nv) { return row_nv_index(nv); }
constexpr int ln_bwd_key(int slab, int nv, int dy_bf16) { return 4 + slab * 8 + row_nv_index(nv) * 2 + dy_bf16; }
constexpr int sm_key(int backward, int nv) { return ROW_LN_KERNELS + backward * 3 + row_nv_index(nv); }
// the launch queued behind a slab kernel is det_fold_kernel<NDST> (common.h), which no family's table lists
constexpr int PLAN_KEY_DET_FOLD = -1;

struct PlanLaunch {
  long long key;      // the row of the family's table (PLAN_KEY_DET_FOLD: the fixed-order fold)
  long long gx, gy;   // grid
  long long block;
  long long lds;      // dynamic LDS bytes
};
struct RowPlan {
  long long nlaunch;   // 1; 2 for the deterministic LayerNorm backward (slab kernel, then det_fold_kernel<3>)
  PlanLaunch k[2];
  long long nv;        // the instance's NV
  long long rpw;       // LayerNorm backward: rows per wave (else 0)
};
constexpr int ROW_PLAN_INTS = sizeof(RowPlan) / sizeof(long long);

// det_fold<NDST> over n elements per destination (common.h launches exactly this)
static inline PlanLaunch det_fold_launch(int n, int ndst) { return {PLAN_KEY_DET_FOLD, ((long long)n + 63) / 64, ndst, 1024, 0}; }

// (arguments already validated by the entry point)
static inline RowPlan ln_fwd_plan(int rows, int D) {
  RowPlan p = {};
  p.nlaunch = 1; p.nv = ln_inst_nv(D);
  p.k[0] = {ln_fwd_key((int)p.nv), ((long long)rows + 3) / 4, 1, 256, 0};
  return p;
}
// slab: the deterministic mode is on and at least one of dgamma, dbeta, dx_colsum is given -- per-workgroup slabs [3][D] in the stream's
// workspace, folded in workgroup order (never atomics)
static inline RowPlan ln_bwd_plan(int rows, int D, bool dy_bf16, bool slab) {
  RowPlan p = {};
  p.nlaunch = slab ? 2 : 1; p.nv = ln_inst_nv(D); p.rpw = ln_bwd_rows_per_wave(rows, D);
  p.k[0] = {ln_bwd_key(slab, (int)p.nv, dy_bf16), ln_bwd_grid(rows, D), 1, 256, 12ll * D * 4};   // LDS: [3][4 waves][D] floats
  if (slab) p.k[1] = det_fold_launch(D, 3);
  return p;
}
static inline RowPlan softmax_plan(bool backward, long long rows, int ld) {
  RowPlan p = {};
  p.nlaunch = 1; p.nv = sm_inst_nv(ld);
  p.k[0] = {sm_key(backward, (int)p.nv), (rows + 3) / 4, 1, 256, 0};
  return p;
}

}  // namespace mmdti
