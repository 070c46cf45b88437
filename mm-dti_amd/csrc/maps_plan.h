// Which kernel an attention-map call runs, with which grid, workgroup size and LDS -- decided here, in plain host C++17 (no HIP types),
// and nowhere else.  attn_maps.hip's two entry points validate, ask attn_map_plan / pair_attn_map_plan, and launch what the plan names
// from one table (g_maps_kernels, indexed by the plan's key); mmdti_maps_plan returns the same plan without launching
// (tests/test_maps_cases_cpu.py asks it for every case and sweeps every length).
//
// Size classes: the fused map has none (one instance per head_dim; the tile counts are run-time loop bounds).  The tiled pair map keeps a
// row of 16-key tiles in registers, so it is unrolled for 5, 9, 13 or 17 tiles (N <= 80, 144, 208, 272: the buckets the fp32 pair-attention
// kernels use) and a call runs the smallest instance that holds its row.
#pragma once

namespace mmdti {

constexpr int MAPS_ATTN_MAX_LEN = 512;    // mmdti_attn_map: what mmdti_attn_long_fwd takes
constexpr int MAPS_PAIR_MAX_N = 320;      // mmdti_pair_attn_map, row-major planes: what mmdti_pair_attn_fwd takes
constexpr int MAPS_PAIR_MAX_TILED = 272;  // ... tiled planes (17 key tiles of 16)
constexpr int MAPS_PAIR_MAX_NT = 17;

// ---- the instance key: a dense index into g_maps_kernels (table MMDTI_PLAN_MAPS) ----
// 0..2 attn_map_kernel<16 | 32 | 64>; 3 pair_attn_map_rows_kernel (layout 0); 4..7 pair_attn_map_tiled_kernel<float, 5 | 9 | 13 | 17> (layout 1);
// 8..11 pair_attn_map_tiled_kernel<_Float16, 5 | 9 | 13 | 17> (layout 3)
constexpr int MAPS_KERNELS = 12;
constexpr int maps_attn_key(int hd) { return hd == 16 ? 0 : hd == 32 ? 1 : 2; }
constexpr int maps_pair_bucket(int N) { return N <= 80 ? 0 : N <= 144 ? 1 : N <= 208 ? 2 : 3; }
constexpr int maps_pair_bucket_nt(int bucket) { return 5 + 4 * bucket; }
constexpr int maps_pair_key(int layout, int N) { return layout == 0 ? 3 : (layout == 1 ? 4 : 8) + maps_pair_bucket(N); }

constexpr int MAPS_BLOCK = 256;           // four waves, every instance

struct MapsPlan {
  int key;       // the row of g_maps_kernels
  int grid, block;
  int lds;       // dynamic LDS bytes (the tiled pair map's fold; else 0)
  int inst;      // what the instance is keyed by: head_dim (fused map); the tiles it is unrolled for (tiled pair map; row-major: 0)
  int tiles;     // 16-key tiles a workgroup walks: of an output row (fused map), of a plane row (pair map)
};
constexpr int MAPS_PLAN_INTS = sizeof(MapsPlan) / sizeof(int);

// (arguments already validated by the entry point)
// fused map: one workgroup per (sequence, block of 16 output rows); its four waves split the 16-column tiles of the output row
static inline MapsPlan attn_map_plan(int B, int Lq_out, int ld_out, int head_dim) {
  MapsPlan p = {};
  p.key = maps_attn_key(head_dim);
  p.grid = B * ((Lq_out + 15) / 16);
  p.block = MAPS_BLOCK;
  p.lds = 0;
  p.inst = head_dim;
  p.tiles = (ld_out + 15) / 16;
  return p;
}
// pair map: one workgroup per (molecule, block of 16 queries).  Tiled planes: the waves split the heads, each keeps the sum of its heads
// in registers, and waves 1..3 hand theirs to wave 0 through LDS (64 lanes x tiles x 16 bytes each).  Row-major planes: a wave per
// query row, no LDS.
static inline MapsPlan pair_attn_map_plan(int B, int N, int layout) {
  MapsPlan p = {};
  const int nt = (N + 15) / 16;
  p.key = maps_pair_key(layout, N);
  p.grid = B * nt;
  p.block = MAPS_BLOCK;
  p.lds = layout == 0 ? 0 : 3 * 64 * nt * 16;
  p.inst = layout == 0 ? 0 : maps_pair_bucket_nt(maps_pair_bucket(N));
  p.tiles = nt;
  return p;
}

}  // namespace mmdti
