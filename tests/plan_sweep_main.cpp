// Stand-alone host program over mm-dti_amd/csrc/row_plan.h and stream_plan.h (which kernel a LayerNorm, softmax, stream, reduction or
// optimizer call runs, and with which grid).  No GPU, no HIP: tests/test_row_cases_cpu.py builds it with -fsanitize=address,undefined
// and runs it.  It sweeps every width and sizes up to the largest an int or a 2^40-element arena can name and checks what every plan
// must satisfy: a key inside its table and of the right instance, a grid that covers the work and respects its cap, no overflow on the way.
// Prints "ok" and exits 0, or prints the failed check and exits 1.
#include <climits>
#include <cstdio>
#include <initializer_list>

#include "../mm-dti_amd/csrc/stream_plan.h"

using namespace mmdti;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      if (++fails <= 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                              \
  } while (0)

static const int ROWS[] = {1, 3, 4, 5, 17, 3071, 3072, 3073, 8197, 12293, 65536, 1 << 24, INT_MAX - 3, INT_MAX};
static const long long NS[] = {1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 22) - 1, 1 << 22,
                               (1 << 22) + 1, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1ll << 24) + 5, (1ll << 31) - 1, 1ll << 31, (1ll << 31) + 1, 1ll << 40};

static void one_launch(const PlanLaunch& k, int key, long long gx, long long gy, long long block, long long lds) {
  CHECK(k.key == key && k.gx == gx && k.gy == gy && k.block == block && k.lds == lds);
}
static void no_second(const PlanLaunch& k) { CHECK(k.key == 0 && k.gx == 0 && k.gy == 0 && k.block == 0 && k.lds == 0); }

static void sweep_rows() {
  for (int D = 4; D <= 2048; D += 4) {
    const int nv = ln_inst_nv(D);
    CHECK(nv == 1 || nv == 2 || nv == 4 || nv == 8);
    CHECK(nv >= ln_nv(D) && ln_nv(D) >= 1 && ln_nv(D) * 256 >= D && (ln_nv(D) - 1) * 256 < D);
    CHECK(nv == 1 || nv / 2 < ln_nv(D));                 // the smallest instance that holds the row
    for (int rows : ROWS) {
      const RowPlan f = ln_fwd_plan(rows, D);
      CHECK(f.nlaunch == 1 && f.nv == nv && f.rpw == 0 && f.k[0].key == ln_fwd_key(nv) && f.k[0].key >= 0 && f.k[0].key < 4);
      CHECK(f.k[0].gx * 4 >= rows && (f.k[0].gx - 1) * 4 < rows && f.k[0].gy == 1 && f.k[0].block == 256 && f.k[0].lds == 0);
      no_second(f.k[1]);
      const int rpw = ln_bwd_rows_per_wave(rows, D), grid = ln_bwd_grid(rows, D);
      CHECK(rpw >= LN_BWD_MIN_ROWS_PER_WAVE && grid >= 1);
      CHECK((long long)grid * 4 * rpw >= rows && ((long long)grid - 1) * 4 * rpw < rows);          // covers the rows, no idle workgroup
      CHECK(rpw == LN_BWD_MIN_ROWS_PER_WAVE || grid <= (nv <= 2 ? 3 : 2) * 256);                   // past the floor: one resident round
      for (int bf = 0; bf < 2; ++bf)
        for (int slab = 0; slab < 2; ++slab) {
          const RowPlan b = ln_bwd_plan(rows, D, bf, slab);
          CHECK(b.nlaunch == 1 + slab && b.nv == nv && b.rpw == rpw);
          CHECK(b.k[0].key == ln_bwd_key(slab, nv, bf) && b.k[0].key >= 4 + 8 * slab && b.k[0].key < 12 + 8 * slab && (b.k[0].key & 1) == bf);
          one_launch(b.k[0], ln_bwd_key(slab, nv, bf), grid, 1, 256, 12ll * D * 4);
          CHECK(b.k[0].lds <= 64 * 1024 * 2);                                                     // 96 KiB at D = 2048: inside the CU's LDS
          if (slab) one_launch(b.k[1], PLAN_KEY_DET_FOLD, (D + 63) / 64, 3, 1024, 0);
          else no_second(b.k[1]);
        }
    }
  }
  for (int ld = 8; ld <= 1024; ld += 8) {
    const int nv = sm_inst_nv(ld);
    CHECK((nv == 1 || nv == 2 || nv == 4) && nv * 256 >= ld && (nv == 1 || nv * 128 < ld || (nv == 4 && ld > 512)));
    for (long long rows : NS)
      for (int bwd = 0; bwd < 2; ++bwd) {
        if (rows > (1ll << 32)) continue;                 // (B heads Lq of three ints' worth of rows: the grid stays an int)
        const RowPlan p = softmax_plan(bwd, rows, ld);
        CHECK(p.nlaunch == 1 && p.nv == nv && p.rpw == 0 && p.k[0].key == sm_key(bwd, nv) && p.k[0].key >= ROW_LN_KERNELS + 3 * bwd && p.k[0].key < ROW_LN_KERNELS + 3 * bwd + 3);
        CHECK(p.k[0].gx * 4 >= rows && (p.k[0].gx - 1) * 4 < rows && p.k[0].gy == 1 && p.k[0].block == 256 && p.k[0].lds == 0);
        no_second(p.k[1]);
      }
  }
  // every row of the table is named by exactly one (entry, NV, flags)
  int seen[ROW_KERNELS] = {};
  for (int nv : {1, 2, 4, 8}) {
    ++seen[ln_fwd_key(nv)];
    for (int bf = 0; bf < 2; ++bf)
      for (int slab = 0; slab < 2; ++slab) ++seen[ln_bwd_key(slab, nv, bf)];
    if (nv < 8) ++seen[sm_key(0, nv)], ++seen[sm_key(1, nv)];
  }
  for (int s : seen) CHECK(s == 1);
}

static void flat(const StreamPlan& p, int key, long long items, int per) {
  CHECK(p.nlaunch == 1 && p.wgs == 0 && p.k[0].key == key && p.k[0].gy == 1 && p.k[0].block == 256 && p.k[0].lds == 0);
  CHECK(p.k[0].gx >= 1 && p.k[0].gx <= STREAM_GRID_CAP);
  CHECK(p.k[0].gx == STREAM_GRID_CAP || p.k[0].gx * per >= items);                  // below the cap one round covers the work
  CHECK(p.k[0].gx == 1 || (p.k[0].gx - 1) * per < items);                           // ... and no workgroup is idle
  no_second(p.k[1]);
}

static void sweep_streams() {
  for (long long n : NS) {
    flat(cast_f32_16_plan(n, false), SK_CAST_F32_BF16, n / 4 + 1, 256);
    flat(cast_f32_16_plan(n, true), SK_CAST_F32_BF16 + 1, n / 4 + 1, 256);
    for (int key : {(int)SK_CAST_BF16_F32, (int)SK_DROPOUT, (int)SK_AXPY, (int)SK_GELU}) flat(stream_plan(key, n, 256), key, n, 256);
    flat(sumsq_plan(n, 0, false), SK_SUMSQ, n, SUMSQ_PER_WG);
    flat(ema_plan(false, n), SK_EMA_UPDATE, n, EMA_UPDATE_PER_WG);
    flat(ema_plan(true, n), SK_EMA_SWAP, n, EMA_SWAP_PER_WG);
    for (int g = 0; g < 2; ++g)
      for (int m = 0; m < 2; ++m) {
        flat(adam_plan(ADAM_STEP_MASKED, n, g, true, false), SK_ADAM + g + 2, n, ADAM_PER_WG);
        for (int d = 0; d < 2; ++d) flat(adam_plan(ADAM_STEP_GROUPED, n, g, m, d), SK_ADAM_GROUP + 4 * g + 2 * m + d, n, ADAM_GROUP_PER_WG);
      }
    flat(adam_plan(ADAM_STEP, n, false, false, false), SK_ADAM, n, ADAM_PER_WG);
    flat(adam_plan(ADAM_STEP_GUARDED, n, true, false, false), SK_ADAM + 1, n, ADAM_PER_WG);
    for (int parts : {1, 2, 3, 6, 2047, 2048, 2049, 4096, 8192, INT_MAX})
      for (int check = 0; check < 2; ++check) {
        const StreamPlan p = sumsq_plan(n, parts, check);
        CHECK(p.nlaunch == 2 && p.wgs >= 1 && p.wgs <= parts && p.wgs <= SUMSQ_WGS && p.wgs <= (n / 4 + 255) / 256 + 1);
        CHECK(p.wgs == parts || p.wgs == SUMSQ_WGS || p.wgs == (n / 4 + 255) / 256 + 1);
        one_launch(p.k[0], SK_SUMSQ_PART + 2 * check, p.wgs, 1, 256, 0);
        one_launch(p.k[1], SK_SUMSQ_PART + 2 * check + 1, 1, 1, 256, 0);
      }
  }
  // an empty arena: no launch at all, where the entry admits one
  for (const StreamPlan& p : {adam_plan(ADAM_STEP_GROUPED, 0, true, true, true), ema_plan(false, 0), ema_plan(true, 0)}) {
    CHECK(p.nlaunch == 0 && p.wgs == 0);
    no_second(p.k[0]);
    no_second(p.k[1]);
  }
  for (int rows : ROWS) {
    const int gy = colsum_grid_y(rows);
    CHECK(gy >= 1 && gy <= 1024 && (gy == 1024 || ((long long)gy * 64 >= rows && ((long long)gy - 1) * 64 < rows)));
    for (int cols : {1, 8, 255, 256, 257, 4096, 1 << 20, INT_MAX - 255})
      for (int slab = 0; slab < 2; ++slab) {
        const StreamPlan p = colsum_plan(rows, cols, slab);
        CHECK(p.nlaunch == 1 + slab && p.wgs == 0);
        one_launch(p.k[0], slab ? SK_COLSUM_SLAB : SK_COLSUM, ((long long)cols + 255) / 256, gy, 256, 0);
        if (slab) one_launch(p.k[1], PLAN_KEY_DET_FOLD, ((long long)cols + 63) / 64, 1, 1024, 0);
        else no_second(p.k[1]);
      }
    for (int cols : {8, 4096, 1 << 20})
      flat(cast_f16_bf16_plan(rows, cols), SK_CAST_F16_BF16, (long long)rows * (cols / 8), 256);
  }
  const StreamPlan st = step_state_plan();
  CHECK(st.nlaunch == 1 && st.wgs == 0);
  one_launch(st.k[0], SK_STEP_STATE, 1, 1, 1, 0);
  // every row of the table is named by exactly one key
  int seen[STREAM_KERNELS] = {};
  for (int k : {(int)SK_CAST_F32_BF16, SK_CAST_F32_BF16 + 1, (int)SK_CAST_F16_BF16, (int)SK_CAST_BF16_F32, (int)SK_DROPOUT, (int)SK_AXPY, (int)SK_GELU, (int)SK_COLSUM,
                (int)SK_COLSUM_SLAB, (int)SK_SUMSQ, sumsq_part_key(0), sumsq_fold_key(0), sumsq_part_key(1), sumsq_fold_key(1), (int)SK_STEP_STATE,
                (int)SK_EMA_UPDATE, (int)SK_EMA_SWAP, adam_key(ADAM_STEP, false, false, false), adam_key(ADAM_STEP_GUARDED, true, false, false),
                adam_key(ADAM_STEP_MASKED, false, true, false), adam_key(ADAM_STEP_MASKED, true, true, false)})
    ++seen[k];
  for (int g = 0; g < 2; ++g)
    for (int m = 0; m < 2; ++m)
      for (int d = 0; d < 2; ++d) ++seen[adam_key(ADAM_STEP_GROUPED, g, m, d)];
  for (int s : seen) CHECK(s == 1);
}

int main() {
  static_assert(ROW_PLAN_INTS == 13 && STREAM_PLAN_INTS == 12, "the word counts include/mmdti_hip.h documents");
  sweep_rows();
  sweep_streams();
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
