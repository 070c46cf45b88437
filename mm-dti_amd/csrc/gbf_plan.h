// Which kernel a pair-bias (GBF) call runs, with which grid, LDS and follow-up pass -- decided here, in plain host C++17 (no HIP types),
// and nowhere else.  gbf.hip's entry points validate, ask one of the plan functions below, and launch what the plan names from one
// table (g_gbf_kernels, indexed by the plan's key); mmdti_gbf_plan returns the same plan without launching
// (tests/test_gbf_cases_cpu.py asks it for every case and sweeps the shapes past them).
#pragma once
#include "det.h"

namespace mmdti {

// ---- geometry of the fused kernels (the kernels in gbf.hip are written against these) ----
constexpr int GBF_K = 128, GBF_F = 128, GBF_H = 64;
constexpr int GBF_WS = 136;  // LDS row stride (elements) of the weight images: 272-B rows, conflict-free ds_read_b128 fragments
constexpr int GBF_W2S = 72;   // LDS row stride of W2^T [128 f][64 h]: 144-B rows, conflict-free ds_read_b128 fragments
constexpr int GBF_LW = 144;       // LDS row stride (elements) of W1 [128 f][144] and of the two pair tiles [128 pairs][144]
constexpr int GBF_MAXE = 4096;        // per-pair backwards: the mul / bias histograms over edge types sit in LDS up to here
constexpr int GBF_FWD_MAXE = 4096;    // forward: the per-edge-type tables sit in LDS up to here (ltab)
constexpr int GBF_FULL_MAXE = 1536;   // 4 per-edge-type fp32 tables next to 126 KB of tiles in the CU's 160 KB
// per-workgroup slab of partial gradients (fp32 elements): dW1 [F][K] | dW2 [H][F] | db1 [F] | db2 [H] | dmeans [K] | dstds [K] | dmul [E] | dbias [E]
constexpr int GBF_SLAB_B1 = GBF_F * GBF_K + GBF_H * GBF_F, GBF_SLAB_B2 = GBF_SLAB_B1 + GBF_F, GBF_SLAB_MU = GBF_SLAB_B2 + GBF_H,
              GBF_SLAB_SG = GBF_SLAB_MU + GBF_K, GBF_SLAB = GBF_SLAB_SG + GBF_K;
constexpr size_t gbf_full_smem(int E) {
  return (size_t)(GBF_F * GBF_LW + GBF_F * GBF_W2S + 2 * 128 * GBF_LW) * 2 + (size_t)(4 * GBF_K + GBF_F + 2 * 128 + 4 * E) * 4;
}
// the deterministic form's staging rows (gbf_bias_bwd_full_kernel<.., DET = true>)
constexpr size_t GBF_DET_SMEM = (size_t)(8 * 128 + 3 * 128) * 4;

// ---- the instance key: a dense index into g_gbf_kernels ----
enum GbfEntry { GBF_FEATURES_FWD = 0, GBF_FEATURES_BWD = 1, GBF_BIAS_FWD = 2, GBF_BIAS_BWD = 3, GBF_BIAS_BWD_FULL = 4 };
constexpr int GBF_KERNELS = 27;
// layout: 0 row-major planes, 1 tiled, 2 compact (tiled, 16-bit planes)
constexpr int gbf_layout(int tiled, int compact) { return compact ? 2 : tiled ? 1 : 0; }
// forward 0..8: (plain | saving | from coordinates) x layout; per-pair backward 9..11: layout; complete backward 12..23:
// (det, coords) x layout; 24 gbf_fwd_kernel, 25 gbf_bwd_kernel, 26 gbf_bwd_det_kernel
constexpr int gbf_fwd_key(int save, int coords, int layout) { return (coords ? 2 : save ? 1 : 0) * 3 + layout; }
constexpr int gbf_bwd_key(int layout) { return 9 + layout; }
constexpr int gbf_full_key(int det, int coords, int layout) { return 12 + (det * 2 + coords) * 3 + layout; }
constexpr int GBF_KEY_FEATURES_FWD = 24, GBF_KEY_FEATURES_BWD = 25, GBF_KEY_FEATURES_BWD_DET = 26;

struct GbfPlan {
  long long key;          // the row of g_gbf_kernels
  long long grid, block;
  long long lds;          // dynamic LDS bytes of this launch
  long long lds_cap;      // what the kernel's MaxDynamicSharedMemorySize is raised to before its first launch (0: never above 64 KiB)
  long long tpm;          // 16-pair tiles per molecule (fused kernels; 0 for the feature kernels)
  long long ntiles;       // tiles the host counts: B * tpm (feature kernels: 16-pair blocks)
  long long ltab;         // forward: the per-edge-type tables sit in LDS
  long long slab;         // partial sums go to per-workgroup slabs (complete backward: of the caller's workspace; feature backward in the
                          // deterministic mode: of the stream's) and a fixed-order pass adds them; 0: fp32 atomics
  long long reduce_grid;  // complete backward with slabs: workgroups of the gbf_slab_reduce_kernel launch that follows (else 0)
};
constexpr int GBF_PLAN_INTS = sizeof(GbfPlan) / sizeof(long long);

// tiled planes: the 4x4 blocks that hold a real pair; row-major planes: 16 consecutive slots of the [N][ld] plane
static inline int gbf_tpm(int tiled, int N, int ld) {
  const int nb4 = (N + 3) / 4;
  return tiled ? nb4 * nb4 : det_cdiv((long long)N * ld, 16);
}

static inline GbfPlan gbf_features_fwd_plan(long long P) {
  GbfPlan p = {};
  long long blocks = (P + 15) / 16;
  p.ntiles = blocks;
  if (blocks > 256 * 32) blocks = 256 * 32;
  p.key = GBF_KEY_FEATURES_FWD; p.grid = blocks; p.block = 256;
  return p;
}
static inline GbfPlan gbf_features_bwd_plan(long long P, int E, bool det) {
  GbfPlan p = {};
  long long blocks = (P + 15) / 16;
  p.ntiles = blocks; p.block = 256;
  if (det) {
    // the deterministic mode: per-workgroup slabs [mul | bias | means | stds] in the stream's workspace, folded in workgroup order
    p.key = GBF_KEY_FEATURES_BWD_DET; p.grid = gbf_features_bwd_grid(P); p.lds = 2 * (long long)E * 4; p.slab = 1;
    return p;
  }
  if (blocks > 256 * 8) blocks = 256 * 8;
  p.key = GBF_KEY_FEATURES_BWD; p.grid = blocks; p.lds = E <= GBF_MAXE ? 2 * (long long)E * 4 : 0;
  return p;
}

static inline GbfPlan gbf_bias_fwd_plan(int B, int N, int ld, int E, int tiled, int compact, bool save, bool coords) {
  GbfPlan p = {};
  p.tpm = gbf_tpm(tiled, N, ld);
  const long long ntiles = (long long)B * p.tpm;
  p.ntiles = ntiles;
  p.grid = (ntiles + 7) / 8 < 512 ? (ntiles + 7) / 8 : 512;     // two resident workgroups per CU
  p.block = 512;
  p.ltab = E <= GBF_FWD_MAXE ? 1 : 0;
  p.lds = (long long)((size_t)(GBF_F + GBF_H) * GBF_WS * 2 + (size_t)(3 * GBF_K + GBF_F + GBF_H + (p.ltab ? 2 * E : 0)) * 4);
  p.lds_cap = (long long)((size_t)(GBF_F + GBF_H) * GBF_WS * 2 + (size_t)(3 * GBF_K + GBF_F + GBF_H + 2 * GBF_FWD_MAXE) * 4);
  // (the coords form saves nothing: it exists for the configurations of the complete backward kernel)
  p.key = gbf_fwd_key(save, coords, gbf_layout(tiled, compact));
  return p;
}

static inline GbfPlan gbf_bias_bwd_plan(int B, int N, int ld, int E, int tiled, int compact) {
  GbfPlan p = {};
  p.tpm = gbf_tpm(tiled, N, ld);
  const long long ntiles = (long long)B * p.tpm;
  p.ntiles = ntiles;
  p.grid = ntiles / 4 + 1 < 1024 ? ntiles / 4 + 1 : 1024;
  p.block = 256;
  p.lds = (long long)((size_t)GBF_K * GBF_WS * 2 + (size_t)GBF_F * GBF_W2S * 2 + (size_t)(3 * GBF_K + 4 * (long long)E) * 4);
  p.lds_cap = 96 * 1024;
  p.key = gbf_bwd_key(gbf_layout(tiled, compact));
  return p;
}

// ws_ok: a non-null, 16-byte aligned workspace was given
static inline GbfPlan gbf_bias_bwd_full_plan(int B, int N, int ld, int E, int tiled, int compact, bool coords, bool det, bool ws_ok,
                                             long long ws_bytes) {
  GbfPlan p = {};
  p.tpm = gbf_tpm(tiled, N, ld);
  const long long ntiles = (long long)B * p.tpm;
  p.ntiles = ntiles;
  p.grid = (ntiles + 7) / 8 < 256 ? (ntiles + 7) / 8 : 256;
  p.block = 512;
  p.lds = (long long)(gbf_full_smem(E) + (det ? GBF_DET_SMEM : 0));
  p.lds_cap = det ? 160 * 1024 : (long long)gbf_full_smem(GBF_FULL_MAXE);
  const long long SL = GBF_SLAB + 2 * (long long)E;
  // (a workspace of at least grid slots: partial sums in per-workgroup slabs + a fixed-order reduce; else fp32 atomics)
  p.slab = ws_ok && ws_bytes >= p.grid * SL * 4 ? 1 : 0;
  p.reduce_grid = p.slab ? det_cdiv(SL, 64) : 0;
  p.key = gbf_full_key(det, coords, gbf_layout(tiled, compact));
  return p;
}

}  // namespace mmdti
