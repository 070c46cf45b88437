// Which kernels a fused-attention call runs, with which grid, workgroup size and LDS -- decided here, in plain host C++17 (no HIP
// types), and nowhere else.  attn.hip's entry points validate, ask attn_fwd_plan / attn_bwd_plan, and launch what the plan names from
// one table (g_attn_kernels, indexed by attn_key); mmdti_attn_plan returns the same plan without launching
// (tests/test_attn_cases_cpu.py asks it for every case and sweeps every length).
#pragma once

namespace mmdti {

constexpr int ATTN_MAX_LEN = 256, ATTN_LONG_MAX_LEN = 512;
// largest dynamic LDS any launch of mmdti_attn_* asks for: 2 x 256 rows x (64+16) bf16 + 3 x 256 floats
constexpr int ATTN_SMEM_MAX = 2 * 256 * 80 * 2 + 4 * 256 * 4;
// ... and of mmdti_attn_long_*: the dK/dV kernel's Q + dO images of 512 rows x (64+8) bf16 + four 512-float row vectors = 155 648 B
// (forward / dQ: K + V images + 512 floats of key mask = 149 504 B) of the CU's 160 KiB
constexpr int ATTN_SMEM_MAX_LONG = 2 * 512 * 72 * 2 + 4 * 512 * 4;

// 16-key tiles of a score row (the forward / dQ kernels' NT; times 16, the key stride of the dropout counter).  Up to 256 keys: the
// two sizes of mmdti_attn_*; 24 and 32 tiles are reached through mmdti_attn_long_* only.
static inline int attn_nt(int Lk) { return Lk <= 160 ? 10 : Lk <= 256 ? 16 : Lk <= 384 ? 24 : 32; }
// workgroup size of the forward (its __launch_bounds__ too)
constexpr int attn_fwd_threads(int hd, int nt) { return hd == 16 && nt == 32 ? 256 : 512; }

// ---- the instance key: a dense index into g_attn_kernels ----
enum AttnKind { ATTN_FWD = 0, ATTN_BWD_Q = 1, ATTN_BWD_KV = 2 };
constexpr int ATTN_KERNELS = 27;
constexpr int attn_hd_index(int hd) { return hd == 16 ? 0 : hd == 32 ? 1 : 2; }
constexpr int attn_nt_index(int nt) { return nt == 10 ? 0 : nt == 16 ? 1 : nt == 24 ? 2 : 3; }
// forward 0..11 and dQ 12..23 by (head_dim, tiles); dK/dV 24..26 by head_dim (its nt is 0)
constexpr int attn_key(int kind, int hd, int nt) {
  return kind == ATTN_BWD_KV ? 24 + attn_hd_index(hd) : kind * 12 + attn_hd_index(hd) * 4 + attn_nt_index(nt);
}

struct AttnLaunch {
  int key;       // attn_key: the row of g_attn_kernels
  int grid, block;
  int lds;       // dynamic LDS bytes of this launch
  int lds_cap;   // what the kernel's MaxDynamicSharedMemorySize is raised to before its first launch at this size class
};
struct AttnPlan {
  int nt;        // attn_nt(Lk)
  int lqp;       // queries rounded up to 32: the rows of the dK/dV kernel's LDS images
  int nlaunch;   // 1 forward; 2 backward (dQ, then dK/dV)
  AttnLaunch k[2];
};
constexpr int ATTN_PLAN_INTS = sizeof(AttnPlan) / sizeof(int);

// (arguments already validated by the entry point)
static inline AttnPlan attn_fwd_plan(int B, int heads, int Lq, int Lk, int head_dim) {
  AttnPlan p = {};
  const int nt = attn_nt(Lk);
  p.nt = nt; p.lqp = ((Lq + 31) / 32) * 32; p.nlaunch = 1;
  p.k[0] = {attn_key(ATTN_FWD, head_dim, nt), B * heads, attn_fwd_threads(head_dim, nt), 2 * nt * 16 * (head_dim + 8) * 2 + nt * 16 * 4,
            nt > 16 ? ATTN_SMEM_MAX_LONG : ATTN_SMEM_MAX};
  return p;
}
static inline AttnPlan attn_bwd_plan(int B, int heads, int Lq, int Lk, int head_dim) {
  AttnPlan p = {};
  const int nt = attn_nt(Lk);
  const int smem_q = 2 * nt * 16 * (head_dim + 8) * 2 + nt * 16 * 4;
  const int lqp = ((Lq + 31) / 32) * 32;
  const int smem_kv = 2 * lqp * (head_dim + 8) * 2 + 4 * lqp * 4;
  p.nt = nt; p.lqp = lqp; p.nlaunch = 2;
  // (dQ: 4 waves up to 16 tiles; with 24 / 32 tiles the image pair leaves room for one workgroup per CU, which then brings 16 --
  //  that form keeps no probability row and needs about 100 registers)
  p.k[0] = {attn_key(ATTN_BWD_Q, head_dim, nt), B * heads, nt > 16 ? 1024 : 256, smem_q, nt > 16 ? ATTN_SMEM_MAX_LONG : ATTN_SMEM_MAX};
  p.k[1] = {attn_key(ATTN_BWD_KV, head_dim, 0), B * heads, 512, smem_kv, smem_kv > ATTN_SMEM_MAX ? ATTN_SMEM_MAX_LONG : ATTN_SMEM_MAX};
  return p;
}

}  // namespace mmdti
