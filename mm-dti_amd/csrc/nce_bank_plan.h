// How a banked InfoNCE direction (mmdti_infonce_bank_dir) is launched -- decided here, in plain host C++17 (no HIP types), and nowhere
// else.  The entry point in losses.hip validates, asks nce_bank_plan and launches what it says; mmdti_infonce_bank_plan returns the same
// plan without launching (tests/test_infonce_bank_cpu.py holds it to an independent statement over a sweep).
//
// Key tiles: the Bg live keys make ceil(Bg / 16) tiles, the cap bank slots ceil(cap / 16) more (slot s sits in tile live_tiles + s / 16,
// so no tile mixes live keys and slots).  A workgroup is ONE wave: it owns 16 anchors and the contiguous tile range
// [split * tiles / splits, (split + 1) * tiles / splits) -- no cross-wave fold, and a split can be as small as two tiles.
//
// The split rule depends on Bl, Bg and cap only:
//   want  = enough splits that anchor blocks x splits reaches one wave per SIMD of the chip (256 CUs x 4);
//   bound = bank tiles / 2: the bank is what makes the key set long -- without one (or with a tiny one) the call is one split, and a
//           split never holds fewer than two tiles;
//   splits = clamp(want, 1, bound).
// B = 32, cap = 4096: 2 anchor blocks, 258 tiles -> 128 splits of 2-3 tiles, 256 workgroups.  Bl >= 16369: one split.
#pragma once

namespace mmdti {

constexpr int NCE_BANK_BLOCK = 64;          // one wave
constexpr int NCE_BANK_WAVE_SLOTS = 1024;   // 256 CUs x 4 SIMDs
constexpr int NCE_BANK_MIN_TILES = 2;       // bank tiles per split, at least
constexpr int NCE_BANK_SLAB_W = 64;         // floats per anchor of a dQ slab (the widest D)

struct NceBankPlan {
  int grid, block;       // rows launches (statistics, gradient): anchor blocks x splits workgroups of one wave
  int splits;
  int tiles;             // key tiles in all: live + bank
  int live_tiles;
  int anchor_blocks;
  int fold_grid;         // the dQ fold: one thread per (anchor, feature of the slab), 256 per workgroup
  int cols_grid;         // infonce_cols_mfma_kernel over the live keys
  long long off_terms;   // scratch, in floats: gl [Bl, Bg] at 0 | the Bl loss terms | (max, sum) [splits, 16 anchor_blocks] | dQ slabs
  long long off_stats;
  long long off_slabs;   //   [splits, 16 anchor_blocks, 64]
  long long scratch_floats;
};
constexpr int NCE_BANK_PLAN_WORDS = 12;     // what mmdti_infonce_bank_plan writes (long long each, in the order above)

static inline int nce_bank_splits(int Bl, int Bg, int cap) {
  (void)Bg;
#ifdef MMDTI_NCE_BANK_ONE_SPLIT             // (measurement build: the same kernels, never split -- profiles/infonce_bank.txt)
  (void)Bl; (void)cap;
  return 1;
#else
  const int ab = (Bl + 15) / 16, bank_tiles = (cap + 15) / 16;
  const int want = (NCE_BANK_WAVE_SLOTS + ab - 1) / ab, bound = bank_tiles / NCE_BANK_MIN_TILES;
  const int s = want < bound ? want : bound;
  return s < 1 ? 1 : s;
#endif
}

// (arguments already validated by the entry point)
static inline NceBankPlan nce_bank_plan(int Bg, int Bl, int cap) {
  NceBankPlan p = {};
  p.anchor_blocks = (Bl + 15) / 16;
  p.live_tiles = (Bg + 15) / 16;
  p.tiles = p.live_tiles + (cap + 15) / 16;
  p.splits = nce_bank_splits(Bl, Bg, cap);
  p.grid = p.anchor_blocks * p.splits;
  p.block = NCE_BANK_BLOCK;
  const long long rows = 16LL * p.anchor_blocks;
  p.fold_grid = (int)((rows * NCE_BANK_SLAB_W + 255) / 256);
  p.cols_grid = p.live_tiles;
  p.off_terms = (long long)Bl * Bg;
  p.off_stats = p.off_terms + Bl;
  p.off_slabs = p.off_stats + 2LL * p.splits * rows;
  p.scratch_floats = p.off_slabs + (long long)p.splits * rows * NCE_BANK_SLAB_W;
  return p;
}

}  // namespace mmdti
