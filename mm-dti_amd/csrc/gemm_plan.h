// Which kernel a GEMM call runs, with which grid, LDS and split -- decided here, in plain host C++17 (no HIP types), and
// nowhere else.  gemm.hip's entry points validate, ask one of the three plan functions below, and launch what the plan names
// from one table; mmdti_gemm_plan / mmdti_linear_dw_grouped_plan / mmdti_gemm_ln_rows return the same plans without launching
// (tests/test_gemm_plan_cpu.py holds the truth table).
#pragma once
#include <limits.h>
#include <stdlib.h>

namespace mmdti {

// ---- tile geometry of the kernel families (the kernels in gemm.hip are written against these) ----
constexpr int BM = 128, BN = 128, BK = 64;
constexpr int LDT = BK;      // [row][k] image: unpadded 128-B rows, 16-B chunks XOR-swizzled by (row & 7) -> conflict-free ds_read_b128
constexpr int LDC_S = BN + 4;  // fp32 row stride of the epilogue's staging image (528 B)
constexpr int DEEP_STAGES = 4;
constexpr int SBM = 64, SBN = 64, SM_STAGES = 4;
constexpr int SM_TILE = SBM * BK;      // elements of one operand tile (8 KB)
constexpr int BMT = 144;
constexpr int BBM = 256, BBN = 256;
constexpr int BIG_PIECE = 128 * BK;          // elements of one 16 KB piece
constexpr int BIG_BUF = 4 * BIG_PIECE;       // A0 | A1 | B0 | B1
constexpr int GROUP_MAX = 8;
constexpr int LN_BN = 512;
constexpr int LDC_LN = LN_BN + 4;

static inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

// ---- every GEMM tuning switch (README "Environment switches"; mmdti_set_option writes the same fields) ----
// big / small / deep are read from the environment when the library is loaded; the others once, at the first call (or plan
// query) of the entry point that uses them: until then they hold UNREAD.
struct GemmOptions {
  static constexpr int UNREAD = INT_MIN;
  int big;                          // MMDTI_GEMM_BIG: 256 x 256 tiles -- 0 off, 1 (default) where the shape fills the chip, 2 every eligible shape
  int small;                        // MMDTI_GEMM_SMALL: 64 x 64 tiles for small launches
  int deep;                         // MMDTI_GEMM_DEEP: four-stage ring at <= 1 workgroup per CU
  int dbg = 0;                      // measurement only: 1 = gemm_big_kernel returns after its K loop (no epilogue, no slab pass)
  int glds = UNREAD;                // MMDTI_GEMM_GLDS: LDS-DMA tile fetch (0 off, 3 double-buffered everywhere)
  int tall = UNREAD;                // MMDTI_GEMM_TALL: tall tiles when they save a whole round
  int small_max_tiles = UNREAD;     // MMDTI_GEMM_SMALL_TILES: most 128 x 128 tiles a launch may have to take the 64 x 64 kernel
  int stream_mb = UNREAD;           // MMDTI_GEMM_STREAM_MB: streaming stores for outputs of at least this size (0 = always, negative = never)
  int ln_rows = UNREAD;             // MMDTI_GEMM_LN_ROWS: 64 / 80 forces the fused Linear + LayerNorm tile height
  int grouped_small_rows = UNREAD;  // MMDTI_GROUPED_SMALL_ROWS: most token rows for the 64 x 64 grouped weight-gradient kernel
};
static inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}
static inline void read_once(int& field, const char* name, int dflt) {
  if (field == GemmOptions::UNREAD) field = env_int(name, dflt);
}
static inline GemmOptions& gemm_options_raw() {
  static GemmOptions o{env_int("MMDTI_GEMM_BIG", 1), env_int("MMDTI_GEMM_SMALL", 1), env_int("MMDTI_GEMM_DEEP", 1)};
  return o;
}
enum GemmEntry { ENTRY_GEMM, ENTRY_GEMM_LN, ENTRY_GROUPED_DW };
static inline const GemmOptions& gemm_options(GemmEntry entry) {
  GemmOptions& o = gemm_options_raw();
  if (entry == ENTRY_GEMM) {
    read_once(o.stream_mb, "MMDTI_GEMM_STREAM_MB", 96);
    read_once(o.glds, "MMDTI_GEMM_GLDS", 1);
    read_once(o.tall, "MMDTI_GEMM_TALL", 1);
    read_once(o.small_max_tiles, "MMDTI_GEMM_SMALL_TILES", 128);
  } else if (entry == ENTRY_GEMM_LN) {
    read_once(o.ln_rows, "MMDTI_GEMM_LN_ROWS", 0);
  } else {
    read_once(o.grouped_small_rows, "MMDTI_GROUPED_SMALL_ROWS", 4096);
  }
  return o;
}

// ---- mmdti_gemm_bf16 ----
enum GemmFamily {
  GEMM_REG = 0,    // gemm_bf16_kernel: register-staged 128 x 128
  GEMM_GLDS = 1,   // gemm_glds_kernel<DBUF = 0>: LDS-DMA, single-buffered
  GEMM_DBUF = 2,   // gemm_glds_kernel<DBUF = 1>: double-buffered
  GEMM_DEEP = 3,   // gemm_glds_kernel<DBUF = 2>: four-stage ring
  GEMM_TALL = 4,   // gemm_glds_tall_kernel: up to 144 x 128
  GEMM_SMALL = 5,  // gemm_small_kernel: 64 x 64
  GEMM_BIG = 6,    // gemm_big_kernel: 256 x 256
};
enum GemmArowsum { AROWSUM_NONE = 0, AROWSUM_IN_KERNEL = 1, AROWSUM_COLSUM_PASS = 2 };

struct GemmShape {
  int M, N, K, lda, ldb;
  bool transA, transB;
  int batch;             // batch_outer * batch_inner
  int splitk;            // as requested
  bool c_bf16, c_atomic; // output type (after MMDTI_DT_F16 is folded into bf16): 16-bit / fp32 atomic / neither = fp32
  bool ab16, bcvt;       // MMDTI_DT_AB_F16 / MMDTI_DT_B_F16
  bool vec_ok;           // the vector epilogue's alignment rules hold
  bool has_aux_in, has_colsum, has_arowsum;
  bool beta_zero;
  bool ws_ok;            // a 16-byte aligned workspace was given
  long long ws_bytes;
  bool slab_epilogue_ok; // what the slab form needs of the epilogue: alpha == 1, no bias / residual / act, C 16-byte aligned, ldc % 4 == 0
};
struct GemmPlan {
  int family;                            // GemmFamily
  int ta, tb, fast, f16, bcvt;           // template key of the instance (a parameter the family does not have stays 0)
  int grid_x, grid_z, block;
  int lds;                               // dynamic LDS bytes
  int splitk;                            // effective K split (GemmArgs::splitk)
  int mstep;                             // rows per tile of the tall kernel, else 0
  int slabs;                             // 1: partial tiles go to workspace slabs and splitk_reduce_kernel adds them into C
  int stream_c;                          // streaming stores for C
  int arowsum;                           // GemmArowsum
};
constexpr int GEMM_PLAN_INTS = sizeof(GemmPlan) / sizeof(int);

// K split of the slab / grouped forms: about one workgroup per CU (floor: all of them resident in ONE round -- a 257th would cost a
// whole second round), at least 4 K-tiles per split, and no empty split (the slab pass sums EVERY slab)
static inline int slab_splits(int ktiles, int tiles) {
  int sk = 256 / (tiles > 1 ? tiles : 1);
  if (ktiles / 4 < sk) sk = ktiles / 4;
  if (sk < 1) sk = 1;
  return ceil_div(ktiles, ceil_div(ktiles, sk));
}

// bare-load fast path: no K tail, no ragged 8-row chunk on a k-major operand, offsets fit 32 bits
static inline bool gemm_fast(const GemmShape& s) {
  return (s.K % BK == 0) && (!s.transA || s.M % 8 == 0) && (!s.transB || s.N % 8 == 0) && s.M >= 8 && s.N >= 8 &&
         ((long long)(s.transA ? BK : s.M) * s.lda * 2 < 0x7fffffffLL) && ((long long)(s.transB ? BK : s.N) * s.ldb * 2 < 0x7fffffffLL);
}

// split-K weight gradients: double-buffered DMA from 48 output tiles up (-5...-13 %), register staging below (+13 %)
// arowsum rides on the kernel that has register room for it (double-buffered DMA: the large weight gradients); on
// the other paths it is the plain column-sum pass over A's memory image ([K][M] row-major)
// (a small split-K weight gradient that also carries its bias gradient takes the double-buffered kernel too: +6 us
//  there against a 35-50 us column-sum pass over dy)
static inline bool gemm_dbuf_path(const GemmShape& s, const GemmOptions& o, bool fast, int tiles) {
  return fast && o.glds && ((s.splitk > 1 && (tiles >= 48 || (s.has_arowsum && s.transA))) || o.glds == 3);
}

// 256 x 256 tiles with the DMA in flight across barriers (gemm_big_kernel): MMDTI_GEMM_BIG=0 off, 1 (default) where
// the shape fills the chip, 2 every eligible shape
static inline bool gemm_big_ok(const GemmShape& s, const GemmOptions& o, bool fast) {
  return fast && o.big && s.batch == 1 && !s.has_colsum && s.M >= 256 && s.N >= 256 && (s.c_atomic || s.vec_ok) && s.M % 256 == 0 &&
         s.N % 256 == 0;
}

// Shapes on which the 256 x 256 kernel (one workgroup per CU) beats the 128 x 128 ones (four per CU): enough tiles to fill
// the 256 CUs with little waste in the last round (measured table: DESIGN.md section 4 "GEMM").
static inline bool big_shape_pays(int M, int N, int K, int splitk, int transA, int transB, bool reads_aux) {
  // Measured on MI355X against the 128 x 128 kernels (scratch/gemm_big_test.py, profiles/r02_gemm_big_ab.json).  The K loop
  // of this kernel runs at 900-1300 TF/s, but with ONE workgroup per CU nothing overlaps a tile's epilogue (an HBM / VALU
  // burst of 15-20 us for a 256 x 256 fp32 / GELU tile) with another tile's loop, and 33 280-row outputs quantise badly on
  // 256 CUs (130 row tiles).  It pays where the loop dominates and the tile count divides the chip:
  const long long tiles = (long long)ceil_div(M, 256) * ceil_div(N, 256);
  if (splitk > 1) return K >= 16384 && 256 % tiles == 0 && tiles >= 4;     // long-K weight gradients: 4 or 16 output tiles (x1.02...1.25)
  // tower-2 shapes in whole rounds: forward x1.03...1.10; input gradients (k-major B) x1.09...1.10 when the epilogue reads nothing
  // (with the saved-activation multiply the 128 x 128 kernels win, 266 vs 304 us); 512 x 512 x 512 stays with them too (72 vs 77 us)
  return tiles % 256 == 0 && K >= 512 && N <= 2048 && M >= 65536 && (long long)N * K >= 512 * 1024 && !(transB && reads_aux);
}

// tall tiles when they save a whole round of the 1024 resident workgroups (see gemm_glds_tall_kernel): rows per tile, or 0
static inline int gemm_tall_mstep(const GemmShape& s, const GemmOptions& o, int tiles, int grid_z) {
  if (!(o.tall && !s.transA && s.vec_ok && grid_z == 1 && s.M >= 1024)) return 0;
  const int slots = 1024, tn = ceil_div(s.N, BN);
  const int r128 = ceil_div(tiles, slots);
  if (r128 >= 2 && (r128 - 1) * slots >= tn) {
    const int rows_fit = ((r128 - 1) * slots) / tn;           // row-tiles that fit in one round fewer
    const int sneed = ceil_div(s.M, rows_fit);
    // (measured: 2 -> 1 rounds is -12...-16 %; 4 -> 3 and 5 -> 4 rounds lose to the taller tile's own cost)
    if (sneed > 128 && sneed <= BMT && 1.125 * (r128 - 1) < 0.75 * r128) return sneed;
  }
  return 0;
}

// `o` from gemm_options(ENTRY_GEMM); `s` already validated by the entry point (grid_z <= 65535 included)
static inline GemmPlan gemm_plan(const GemmShape& s, const GemmOptions& o) {
  GemmPlan p = {};
  const int tiles = ceil_div(s.M, BM) * ceil_div(s.N, BN);
  const bool fast = gemm_fast(s);
  p.grid_x = tiles; p.grid_z = s.batch * s.splitk; p.block = 256;
  p.splitk = s.splitk;
  p.ta = s.transA; p.tb = s.transB; p.f16 = s.ab16; p.bcvt = s.bcvt;
  // streaming stores for outputs of at least MMDTI_GEMM_STREAM_MB (default 96 MB; 0 = always, negative = never)
  const long long cbytes = (long long)s.M * s.N * (s.c_bf16 ? 2 : 4) * s.batch;
  p.stream_c = (o.stream_mb >= 0 && cbytes >= o.stream_mb * 1000000LL && s.beta_zero) ? 1 : 0;
  // the 128 x 128 staging image: one (A|B) tile pair (32,768 B), re-used by the epilogue's [64][132] fp32 image (33,792 B)
  const int lds_128 = 64 * LDC_S * (int)sizeof(float);
  const int lds_dbuf = 4 * BM * LDT * 2;

  if (gemm_big_ok(s, o, fast) && (o.big == 2 || big_shape_pays(s.M, s.N, s.K, s.splitk, s.transA, s.transB, s.has_aux_in))) {
    p.family = GEMM_BIG;
    p.block = 512; p.lds = 2 * BIG_BUF * 2;
    const int btiles = ceil_div(s.M, BBM) * ceil_div(s.N, BBN);
    if (s.splitk > 1) p.splitk = slab_splits(s.K / BK, btiles);   // weight gradients
    p.grid_x = btiles; p.grid_z = p.splitk;
    const long long slab = (long long)s.M * s.N;
    p.slabs = p.splitk > 1 && s.ws_ok && s.ws_bytes >= (long long)p.splitk * slab * 4 && s.N % 8 == 0 && s.slab_epilogue_ok && slab % 4 == 0 &&
              !(o.dbg & 1);
    if (p.slabs) p.stream_c = 0;
    p.arowsum = s.has_arowsum ? AROWSUM_IN_KERNEL : AROWSUM_NONE;
    return p;
  }
  const bool dbuf_path = gemm_dbuf_path(s, o, fast, tiles);
  if (s.has_arowsum) p.arowsum = (dbuf_path || (s.bcvt && fast && o.glds)) ? AROWSUM_IN_KERNEL : AROWSUM_COLSUM_PASS;
  if (s.bcvt) {
    // weight gradient with an fp16 activation operand: the double-buffered LDS-DMA kernel on bare-load shapes (whatever the split), the
    // register-staged one otherwise
    if (fast && o.glds) { p.family = GEMM_DBUF; p.lds = lds_dbuf; }
    else { p.family = GEMM_REG; p.fast = fast; p.lds = lds_128; }
  } else if (dbuf_path) {
    p.family = GEMM_DBUF; p.f16 = 0; p.lds = lds_dbuf;
  } else if (fast && o.glds && s.splitk == 1) {
    // LDS-DMA tile fetch for every bare-load shape except the split-K weight gradients (measured: -15...-20 % on the
    // N >= 1536 / K >= 1536 shapes, equal at 512x512, +9 % on the atomic split-K ones); MMDTI_GEMM_GLDS=0 turns it off
    const int deep_max_wgs = 256;                     // (one workgroup per CU)
    p.mstep = gemm_tall_mstep(s, o, tiles, p.grid_z);
    if (p.mstep) {
      p.family = GEMM_TALL;
      p.grid_x = ceil_div(s.M, p.mstep) * ceil_div(s.N, BN);
      p.lds = (BMT + BN) * LDT * 2;
    } else if (o.small && !s.transA && s.vec_ok && !s.c_atomic && !s.has_colsum && p.grid_z == 1 && tiles <= o.small_max_tiles) {
      // small launches: a quarter of the tile per workgroup, four times the CUs (see gemm_small_kernel)
      p.family = GEMM_SMALL;
      p.grid_x = ceil_div(s.M, SBM) * ceil_div(s.N, SBN); p.grid_z = 1;
      p.lds = SM_STAGES * 2 * SM_TILE * 2;
    } else if (o.deep && tiles * p.grid_z <= deep_max_wgs && s.K >= 4 * BK) {
      // at most one workgroup per CU: the four-stage ring hides the fetch latency nothing else would (small batches)
      p.family = GEMM_DEEP; p.lds = DEEP_STAGES * 2 * BM * LDT * 2;
    } else {
      p.family = GEMM_GLDS; p.lds = lds_128;
    }
  } else {
    p.family = GEMM_REG; p.fast = fast; p.lds = lds_128;
  }
  return p;
}

// ---- mmdti_gemm_ln_bf16: rows per tile, 64 or 80 -- whichever needs less (rounds of the 512 resident workgroups) x (rows per tile) ----
static inline int gemm_ln_rows(int M, const GemmOptions& o) {
  const long long cost4 = (long long)ceil_div(ceil_div(M, 64), 512) * 4, cost5 = (long long)ceil_div(ceil_div(M, 80), 512) * 5;
  return o.ln_rows == 64 ? 64 : (o.ln_rows == 80 ? 80 : (cost5 < cost4 ? 80 : 64));
}
static inline int gemm_ln_lds(int rows) {
  const int a = (rows + LN_BN) * LDT * 2, b = (16 * LDC_LN + 3 * LN_BN) * (int)sizeof(float);
  return a > b ? a : b;
}

// ---- mmdti_linear_dw_grouped ----
struct GroupedDwPlan {
  int small;              // 1: gemm_small_dw_grouped_kernel (64 x 64 tiles, no K split, plain +=); 0: gemm_big_grouped_kernel
  int grid_x, grid_z, block, lds;
  int splitk;
  int ktail;              // template TAIL of the big form: rows % 64 != 0
  int atomic;             // big form: the K splits add into dW with fp32 atomics (no slab pass)
  int bcvt;               // template BCVT of either form: every x holds fp16, converted between LDS and the matrix pipe
  long long ws_bytes;     // workspace the launch needs (0 for the small form)
};
// tiles256 / tiles64: 256 x 256 / 64 x 64 output tiles over all problems; elems: sum of n_out * n_in
static inline GroupedDwPlan grouped_dw_plan(int tiles256, int tiles64, long long elems, int rows, bool x_f16, const GemmOptions& o) {
  GroupedDwPlan p = {};
  p.bcvt = x_f16;
  // small token counts: 64 x 64 tiles, no K split, plain += (gemm_small_dw_grouped_kernel)
  if (rows <= o.grouped_small_rows && o.small) {
    // (three stages = 48 KB: three workgroups per CU; measured -2 % on the step against a four-stage ring at two per CU)
    p.small = 1; p.grid_x = tiles64; p.grid_z = 1; p.block = 256; p.lds = 3 * 2 * SM_TILE * 2; p.splitk = 1;
    return p;
  }
  p.splitk = slab_splits(ceil_div(rows, BK), tiles256);
  p.grid_x = tiles256; p.grid_z = p.splitk; p.block = 512; p.lds = 2 * BIG_BUF * 2;
  p.ktail = rows % BK != 0;
  // Small token counts (the reference's real batch sizes, 16-32 molecules): the step is a chain of ~20 us kernels, and the slab
  // pass is one more of them per layer -- the K-splits add into dW with fp32 atomics instead (a few MB of them: cheaper than a launch)
  // (reached only with the 64 x 64 kernel switched off: gemm_small = 0)
  p.atomic = rows <= 4096 ? 1 : 0;
  p.ws_bytes = (long long)p.splitk * elems * 4;
  return p;
}

}  // namespace mmdti
