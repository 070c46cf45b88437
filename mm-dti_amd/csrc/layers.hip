// layers.hip -- launch sequencing of one transformer layer behind ONE call.
// At the reference's default batch sizes (16-32 molecules) a step is ~500 launches of 5-30 us kernels and the Python side of
// each (wrapper, allocations, autograd bookkeeping: 13-17 us) sets the pace, not the GPU (DESIGN.md "small batches").  The
// functions here issue the launches of a whole layer from C++: the same kernels, arguments and order as the op-by-op host path
// (functional.py), which stays as the general path -- every variant this file does not cover falls back to it -- and as the
// reference the tests hold this path bit-identical to.  No kernels of its own: it only calls the entry points of mmdti_hip.h.
#include "common.h"

using namespace mmdti;

namespace {
// dx[M, n_out] = dy[M, n_in] . w[n_in, n_out] (bf16), optionally x saved gelu' / recomputed gelu'   (ops.linear_bwd_input)
inline int dx_gemm(mmdti_stream_t s, const void* dy, int ldy, const void* w, int ldw, void* out, int M, int n_out, int n_in, int act,
                   const void* aux_in, int ld_aux) {
  return mmdti_gemm_bf16(s, dy, w, out, M, n_out, n_in, ldy, ldw, n_out, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1.f, 0.f, nullptr, nullptr, n_out, act, aux_in,
                         nullptr, aux_in ? ld_aux : n_out, MMDTI_DT_BF16, 0.f, 0ull, 0u, nullptr, nullptr, nullptr, 0);
}
// y[M, n_out] = epi(x[M, n_in] . w[n_out, n_in]^T + bias)   (ops.linear_fwd)
inline int fwd_gemm(mmdti_stream_t s, const void* x, int ldx, const void* w, int ldw, const float* bias, void* out, int M, int n_out, int n_in,
                    int act, void* aux_out, const float* residual, int c_dtype, float drop_p, unsigned long long seed, unsigned int site) {
  return mmdti_gemm_bf16(s, x, w, out, M, n_out, n_in, ldx, ldw, n_out, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1.f, 0.f, bias, residual, n_out, act, nullptr,
                         aux_out, n_out, c_dtype, drop_p, seed, site, nullptr, nullptr, nullptr, 0);
}
// the Linear that closes a residual branch + the LayerNorm behind it (ops.linear_ln_fwd): one kernel for 512-wide outputs up to
// ln_max_k deep, else the GEMM and the LayerNorm kernels back to back.  ln_f32 / ln_bf16: either may be null.
inline int closer(mmdti_stream_t s, const void* x, const void* w, const float* bias, const float* residual, int M, int n_out, int n_in, float drop_p,
                  unsigned long long seed, unsigned int site, float* y, const float* gamma, const float* beta, float eps, float* ln_f32,
                  void* ln_bf16, float* mean, float* rstd, int ln_max_k, int f16) {
  // f16: the fp16 forward-operand mode -- x and w hold fp16, the 16-bit LayerNorm output is fp16
  if (n_out == 512 && n_in % 64 == 0 && n_in <= ln_max_k)
    return mmdti_gemm_ln_bf16(s, x, w, bias, residual, M, n_out, n_in, n_in, n_in, n_out, drop_p, seed, site, y, gamma, beta, eps, ln_f32, ln_bf16, mean,
                              rstd, f16 ? 3 : 0);
  if (int e = fwd_gemm(s, x, n_in, w, n_in, bias, y, M, n_out, n_in, MMDTI_ACT_NONE, nullptr, residual, MMDTI_DT_F32 | (f16 ? MMDTI_DT_AB_F16 : 0), drop_p, seed,
                       site))
    return e;
  return mmdti_layernorm_fwd(s, y, gamma, beta, eps, M, n_out, ln_f32, ln_bf16, mean, rstd, nullptr, 0.f, 0ull, 0u, f16 ? 1 : 0);
}
}  // namespace

// ---------------------------------------------------------------------------------------------------------------- tower 1
namespace {
inline long long up256(long long b) { return (b + 255) / 256 * 256; }
inline long long up16(long long b) { return (b + 15) / 16 * 16; }
// bytes of ONE layer's backward temporaries, the grouped weight-gradient slabs aside (the layout: unimol_layer_bwd_core)
inline long long unimol_layer_tmp_bytes(long long M, long long D, long long F) { return (M * F + 7 * M * D) * 2 + M * D * 4; }
// what a call needs of a layer's parameter block (the stack calls ask for every layer before the first launch)
inline bool unimol_fwd_params(const mmdti_unimol_layer_t& P) { return P.w_in && P.w_out && P.w_fc1 && P.w_fc2 && P.g_ln2 && P.bt_ln2; }
// frozen: the base of an adapted layer -- no weight gradient is launched, so none is asked for
inline bool unimol_bwd_params(const mmdti_unimol_layer_t& P, bool frozen = false) {
  return P.wb_fc2 && P.wb_fc1 && P.wb_out && P.wb_in && P.g_ln2 && P.g_ln1 && (frozen || (P.dw_fc2 && P.dw_fc1 && P.dw_out && P.dw_in));
}

// ---- LoRA adapters in a sequenced layer (mmdti_lora_adapter_t; the *_lora_* entry points further down)
inline bool lora_on(const mmdti_lora_adapter_t* a) { return a && a->r != 0; }
inline long long lora_row(long long rows) { return MMDTI_LORA_ROW_BYTES(rows); }
// what a call needs of an adapter before its first launch (bwd: the backward's fields)
inline bool lora_ok(const mmdti_lora_adapter_t* a, bool bwd) {
  if (!lora_on(a)) return true;
  if (a->r != 8 && a->r != 16 && a->r != 32) return false;
  return bwd ? a->A_bf16 && a->B_bf16 && a->dA && a->dB : a->A && a->B;
}
#define MMDTI_REQUIRE_LORA(who, a, bwd, rows)                                                                                         \
  MMDTI_REQUIRE(lora_ok(a, bwd), "%s: an adapter needs rank 8, 16 or 32 (got %d) and its %s", who, (a)->r,                        \
                (bwd) ? "bf16 shadows and gradient buffers" : "forward shadows");                                                     \
  MMDTI_REQUIRE(!lora_on(a) || (rows), "%s: an adapter needs its t%s", who, (bwd) ? " and u rows" : " row")
inline int lora_fwd(mmdti_stream_t s, const mmdti_lora_adapter_t& a, const void* x, void* y, int ldy, void* t, int T, int n_in, int n_out, int f16, int y_f16) {
  return mmdti_lora_fwd(s, x, n_in, a.A, a.B, y, ldy, t, T, n_in, n_out, a.r, a.scale, f16, y_f16);
}
inline int lora_bwd(mmdti_stream_t s, const mmdti_lora_adapter_t& a, const void* x, int x_f16, const void* dy, int lddy, const void* t, void* u, int T, int n_in,
                    int n_out) {
  return mmdti_lora_bwd(s, x, n_in, x_f16, dy, lddy, t, a.B_bf16, u, a.dA, a.dB, T, n_in, n_out, a.r, a.scale);
}
}  // namespace

/* Forward of one Uni-Mol encoder layer behind one call: replaces the per-layer body of PairEncoderFn.forward (functional.py) with
 * the same launches -- in_proj, pair attention, out_proj + residual + dropout + LayerNorm-2, fc1 + GELU (saving gelu' or u as
 * act_fwd says), fc2 + residual + dropout and the LayerNorm that reads its output (next_mode 1: the next layer's LayerNorm-1 -> bf16;
 * 2: the encoder's final LayerNorm -> fp32; 0: none).  The arguments: mmdti_hip.h.
 * lora / t (mmdti_unimol_lora_layer_fwd; null: no adapter): mmdti_lora_fwd on q | k | v right behind the in_proj GEMM, t saved. */
static int unimol_layer_fwd_core(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                                 const mmdti_unimol_saved_t* saved, const mmdti_lora_adapter_t* lora, void* t, unsigned int site_att,
                                 unsigned int site_o, unsigned int site_f, const void* s_in, const unsigned char* key_pad, int rag_store,
                                 int next_mode, const float* g_next, const float* bt_next, float eps_next, float* x_out, void* ln_out, float* mn,
                                 float* rn) {
  MMDTI_REQUIRE(run && layer && saved, "unimol_layer_fwd: null block");
  MMDTI_REQUIRE_LORA("unimol_layer_fwd", lora, false, t);
  const mmdti_unimol_run_t& R = *run;
  const mmdti_unimol_layer_t& P = *layer;
  const mmdti_unimol_saved_t& S = *saved;
  const int M = R.M, D = R.D, F = R.F, fwd_f16 = R.fwd_f16;
  MMDTI_REQUIRE(M > 0 && D > 0 && F > 0 && D % 8 == 0 && F % 8 == 0 && next_mode >= 0 && next_mode <= 2, "unimol_layer_fwd: bad shape / mode");
  MMDTI_REQUIRE(S.x && S.h1 && s_in && unimol_fwd_params(P) && S.qkv && S.s && S.o && S.x1 && S.h2 && S.m2 && S.r2 && S.u && S.a && x_out,
                "unimol_layer_fwd: null argument");
  MMDTI_REQUIRE(next_mode == 0 || (g_next && bt_next && ln_out && mn && rn), "unimol_layer_fwd: the next LayerNorm needs its parameters and outputs");
  // fwd_f16 (the fp16 forward-operand mode; compact pair planes only): h1, the four weights, q | k | v, o, h2, a and a 16-bit
  // ln_out hold fp16; u (the saved gelu', read by the backward) stays bf16
  MMDTI_REQUIRE(!fwd_f16 || R.pair_layout == 3, "unimol_layer_fwd: fp16 forward operands need the compact pair planes (layout 3)");
  const int ab = fwd_f16 ? MMDTI_DT_AB_F16 : 0, o16 = (fwd_f16 ? MMDTI_DT_F16 : MMDTI_DT_BF16) | ab;
  if (int e = fwd_gemm(stream, S.h1, D, P.w_in, D, P.b_in, S.qkv, M, 3 * D, D, MMDTI_ACT_NONE, nullptr, nullptr, o16, 0.f, 0ull, 0u)) return e;
  if (lora_on(lora))
    if (int e = lora_fwd(stream, *lora, S.h1, S.qkv, 3 * D, t, M, D, 3 * D, fwd_f16 ? 1 : 0, fwd_f16 ? 1 : 0)) return e;
  if (int e = mmdti_pair_attn_fwd(stream, S.qkv, s_in, S.s, S.o, key_pad, R.B, R.N, R.H, R.ld, R.scale, R.p_att, R.seed, site_att, R.pair_layout, R.key_tiles,
                                  rag_store, R.row_off, fwd_f16 ? 1 : 0))
    return e;
  if (int e = closer(stream, S.o, P.w_out, P.b_out, S.x, M, D, D, R.p_res, R.seed, site_o, S.x1, P.g_ln2, P.bt_ln2, P.eps_ln2, nullptr, S.h2, S.m2, S.r2,
                     R.ln_max_k, fwd_f16))
    return e;
  if (int e = fwd_gemm(stream, S.h2, D, P.w_fc1, D, P.b_fc1, S.a, M, F, D, R.act_fwd, S.u, nullptr, o16, 0.f, 0ull, 0u)) return e;
  if (next_mode == 0)
    return fwd_gemm(stream, S.a, F, P.w_fc2, F, P.b_fc2, x_out, M, D, F, MMDTI_ACT_NONE, nullptr, S.x1, MMDTI_DT_F32 | ab, R.p_res, R.seed, site_f);
  return closer(stream, S.a, P.w_fc2, P.b_fc2, S.x1, M, D, F, R.p_res, R.seed, site_f, x_out, g_next, bt_next, eps_next, next_mode == 2 ? (float*)ln_out : nullptr,
                next_mode == 1 ? ln_out : nullptr, mn, rn, R.ln_max_k, fwd_f16);
}

extern "C" int mmdti_unimol_layer_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                                      const mmdti_unimol_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                                      const void* s_in, const unsigned char* key_pad, int rag_store, int next_mode, const float* g_next,
                                      const float* bt_next, float eps_next, float* x_out, void* ln_out, float* mn, float* rn) {
  return unimol_layer_fwd_core(stream, run, layer, saved, nullptr, nullptr, site_att, site_o, site_f, s_in, key_pad, rag_store, next_mode, g_next, bt_next,
                               eps_next, x_out, ln_out, mn, rn);
}
extern "C" int mmdti_unimol_lora_layer_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                                           const mmdti_unimol_saved_t* saved, const mmdti_lora_adapter_t* lora, void* t, unsigned int site_att,
                                           unsigned int site_o, unsigned int site_f, const void* s_in, const unsigned char* key_pad, int rag_store,
                                           int next_mode, const float* g_next, const float* bt_next, float eps_next, float* x_out, void* ln_out,
                                           float* mn, float* rn) {
  return unimol_layer_fwd_core(stream, run, layer, saved, lora, t, site_att, site_o, site_f, s_in, key_pad, rag_store, next_mode, g_next, bt_next, eps_next,
                               x_out, ln_out, mn, rn);
}

/* Backward of one Uni-Mol encoder layer (pre-LN: x1 = x + drop(out_proj(attn(LN1(x)))), x2 = x1 + drop(fc2(gelu(fc1(LN2(x1))))));
 * replaces the per-layer body of PairEncoderFn.backward (functional.py) -- transformers.py:136-139 through unicore's
 * TransformerEncoderLayer.  Eight launches: fc2 input gradient (x gelu'), fc1 input gradient, LayerNorm-2 backward, out_proj
 * input gradient, pair-attention backward, in_proj input gradient, LayerNorm-1 backward, the four weight gradients (grouped).
 *   ws: du [M,F] | dh2 [M,D] | dy1 [M,D] | do [M,D] | dqkv [M,3D] | dh1 [M,D] (bf16) | dx_mid [M,D] fp32 | grouped-dW slabs.
 *   dw_stream (the stack call at small batches; null: everything on `stream`): the weight gradients -- leaves of the backward graph --
 *   leave on their own stream behind ev_fork and run under the layer below; ev_done marks them finished.
 *   frozen (mmdti_unimol_lora_layer_bwd): an adapted layer on a frozen base -- no weight gradients; mmdti_lora_bwd on dqkv (lora / t; the
 *   u row sits behind the temporaries, 256-byte aligned) and mmdti_lora_dx on dh1; dx_out null: the lowest layer that runs, whose in_proj
 *   input gradient, adapter dx and LayerNorm-1 backward nobody reads. */
static int unimol_layer_bwd_core(mmdti_stream_t stream, const mmdti_unimol_run_t& R, const mmdti_unimol_layer_t& P, const mmdti_unimol_saved_t& S,
                                 unsigned int site_f_below, unsigned int site_o, unsigned int site_att, const float* dx_in, const void* dy2,
                                 float* dx_out, void* dx16_out, float* db_below, void* G, int g_in_zero, void* ws, long long ws_bytes,
                                 mmdti_stream_t dw_stream, hipEvent_t ev_fork, hipEvent_t ev_done, bool frozen = false,
                                 const mmdti_lora_adapter_t* lora = nullptr, const void* t = nullptr) {
  const int M = R.M, D = R.D, F = R.F, fwd_f16 = R.fwd_f16;
  MMDTI_REQUIRE(M > 0 && D > 0 && F > 0 && D % 8 == 0 && F % 8 == 0, "unimol_layer_bwd: bad shape");
  MMDTI_REQUIRE(dx_in && dy2 && (dx_out || frozen) && S.a && S.u && S.h2 && S.x1 && S.m2 && S.r2 && S.o && S.qkv && S.s && S.h1 && S.x && S.m1 && S.r1 &&
                    unimol_bwd_params(P, frozen) && G && ws,
                "unimol_layer_bwd: null argument");
  MMDTI_REQUIRE_LORA("unimol_layer_bwd", lora, true, t);
  const long long MD = (long long)M * D, MF = (long long)M * F;
  // bf16 temporaries + the fp32 mid-layer gradient (+ the adapter's u row)
  const long long fixed = frozen ? up256(unimol_layer_tmp_bytes(M, D, F)) + lora_row(M) : unimol_layer_tmp_bytes(M, D, F);
  MMDTI_REQUIRE(ws_bytes >= fixed && aligned16(ws), "unimol_layer_bwd: workspace too small (%lld bytes for the temporaries alone)", fixed);
  char* wp = reinterpret_cast<char*>(ws);
  void* du = wp;                 wp += MF * 2;
  void* dh2 = wp;                wp += MD * 2;
  void* dy1 = wp;                wp += MD * 2;
  void* dob = wp;                wp += MD * 2;
  void* dqkv = wp;               wp += 3 * MD * 2;
  void* dh1 = wp;                wp += MD * 2;
  float* dx_mid = reinterpret_cast<float*>(wp); wp += MD * 4;
  void* slabs = wp;
  const long long slab_bytes = ws_bytes - fixed;
  // ---- FFN
  if (int e = dx_gemm(stream, dy2, D, P.wb_fc2, F, du, M, F, D, R.act_dx, S.u, F)) return e;
  if (int e = dx_gemm(stream, du, F, P.wb_fc1, D, dh2, M, D, F, MMDTI_ACT_NONE, nullptr, 0)) return e;
  if (int e = mmdti_layernorm_bwd(stream, dh2, MMDTI_DT_BF16, nullptr, S.x1, P.g_ln2, S.m2, S.r2, M, D, dx_in, dx_mid, P.dg_ln2, P.dbt_ln2, nullptr, 0.f, 0ull, 0u,
                                  dy1, R.p_res, site_o, P.db_out))
    return e;
  // ---- attention
  if (int e = dx_gemm(stream, dy1, D, P.wb_out, D, dob, M, D, D, MMDTI_ACT_NONE, nullptr, 0)) return e;
  // (fwd_f16: the saved a, h2, o, h1 and q | k | v hold fp16 -- converted inside the kernels that read them)
  if (int e = mmdti_pair_attn_bwd(stream, S.qkv, S.s, dob, G, dqkv, R.B, R.N, R.H, R.ld, R.scale, g_in_zero, R.p_att, R.seed, site_att, R.pair_layout, R.key_tiles,
                                  R.row_off, fwd_f16 ? 1 : 0))
    return e;
  void* u = frozen ? reinterpret_cast<char*>(ws) + fixed - lora_row(M) : nullptr;
  if (lora_on(lora))
    if (int e = lora_bwd(stream, *lora, S.h1, fwd_f16 ? 1 : 0, dqkv, 3 * D, t, u, M, D, 3 * D)) return e;
  if (frozen && !dx_out) return MMDTI_OK;
  if (int e = dx_gemm(stream, dqkv, 3 * D, P.wb_in, D, dh1, M, D, 3 * D, MMDTI_ACT_NONE, nullptr, 0)) return e;
  if (lora_on(lora))
    if (int e = mmdti_lora_dx(stream, u, lora->A_bf16, dh1, D, 1, M, D, lora->r)) return e;
  if (int e = mmdti_layernorm_bwd(stream, dh1, MMDTI_DT_BF16, nullptr, S.x, P.g_ln1, S.m1, S.r1, M, D, dx_mid, dx_out, P.dg_ln1, P.dbt_ln1, nullptr, 0.f, 0ull, 0u,
                                  dx16_out, dx16_out ? R.p_res : 0.f, dx16_out ? site_f_below : 0u, dx16_out ? db_below : nullptr))
    return e;
  if (frozen) return MMDTI_OK;
  // ---- the four weight gradients over the same M rows: one grouped launch (bias gradients of fc1 / in_proj ride on it; those of
  //      fc2 / out_proj came from the LayerNorm backward that produced their dy)
  const void* dys[4] = {dy2, du, dy1, dqkv};
  const void* xs[4] = {S.a, S.h2, S.o, S.h1};
  float* dws[4] = {P.dw_fc2, P.dw_fc1, P.dw_out, P.dw_in};
  float* dbs[4] = {nullptr, P.db_fc1, nullptr, P.db_in};
  const int n_out[4] = {D, F, D, 3 * D}, n_in[4] = {F, D, D, D};
  const int ldy[4] = {D, F, D, 3 * D}, ldx[4] = {F, D, D, D}, lddw[4] = {F, D, D, D};
  if (!dw_stream) return mmdti_linear_dw_grouped(stream, 4, dys, xs, dws, dbs, n_out, n_in, ldy, ldx, lddw, M, slabs, slab_bytes, fwd_f16 ? 1 : 0);
  if (hipEventRecord(ev_fork, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent((hipStream_t)dw_stream, ev_fork, 0) != hipSuccess) {
    set_error("unimol_layer_bwd: event fork failed");
    return MMDTI_ERR_LAUNCH;
  }
  if (int e = mmdti_linear_dw_grouped(dw_stream, 4, dys, xs, dws, dbs, n_out, n_in, ldy, ldx, lddw, M, slabs, slab_bytes, fwd_f16 ? 1 : 0)) return e;
  if (hipEventRecord(ev_done, (hipStream_t)dw_stream) != hipSuccess) {
    set_error("unimol_layer_bwd: hipEventRecord failed");
    return MMDTI_ERR_LAUNCH;
  }
  return MMDTI_OK;
}

extern "C" int mmdti_unimol_layer_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                                      const mmdti_unimol_saved_t* saved, unsigned int site_f_below, unsigned int site_o, unsigned int site_att,
                                      const float* dx_in, const void* dy2, float* dx_out, void* dx16_out, float* db_below, void* G,
                                      int g_in_zero, void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(run && layer && saved, "unimol_layer_bwd: null block");
  return unimol_layer_bwd_core(stream, *run, *layer, *saved, site_f_below, site_o, site_att, dx_in, dy2, dx_out, dx16_out, db_below, G, g_in_zero, ws,
                               ws_bytes, nullptr, nullptr, nullptr);
}
extern "C" int mmdti_unimol_lora_layer_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                                           const mmdti_unimol_saved_t* saved, const mmdti_lora_adapter_t* lora, const void* t,
                                           unsigned int site_f_below, unsigned int site_o, unsigned int site_att, const float* dx_in,
                                           const void* dy2, float* dx_out, void* dx16_out, float* db_below, void* G, int g_in_zero, void* ws,
                                           long long ws_bytes) {
  MMDTI_REQUIRE(run && layer && saved, "unimol_lora_layer_bwd: null block");
  return unimol_layer_bwd_core(stream, *run, *layer, *saved, site_f_below, site_o, site_att, dx_in, dy2, dx_out, dx16_out, db_below, G, g_in_zero, ws,
                               ws_bytes, nullptr, nullptr, nullptr, true, lora, t);
}

// ---------------------------------------------------------------------------------------------------------------- tower 1's stack
// At the reference's batch size the per-layer calls above still leave ~90 us of Python per layer and direction (17 allocations and
// the marshalling): the stack calls issue ALL layers of a tower from one call.  The saved tensors of a layer live at fixed offsets
// of one caller-owned arena (mmdti_unimol_stack_layout), the parameters come as an array of the layers' blocks.
namespace {
struct UniArena {      // byte offsets inside one layer's slice
  long long qkv, o, s, x1, h2, m2, r2, u, a, x_out, ln_out, mn, rn, t, stride;
  UniArena(long long M, long long D, long long F, long long s_bytes, bool lora = false) {      // lora: an adapter's t row behind the slice
    long long at = 0;
    auto take = [&](long long b) { const long long r = at; at += up256(b); return r; };
    qkv = take(M * 3 * D * 2); o = take(M * D * 2); s = take(s_bytes); x1 = take(M * D * 4); h2 = take(M * D * 2); m2 = take(M * 4); r2 = take(M * 4);
    u = take(M * F * 2); a = take(M * F * 2); x_out = take(M * D * 4); ln_out = take(M * D * 2); mn = take(M * 4); rn = take(M * 4);
    t = lora ? take(lora_row(M)) : 0;
    stride = at;
  }
  // the saved block of slice l: a layer's inputs are what the slice below holds of its output stream (layer 0: the caller's)
  mmdti_unimol_saved_t saved(const void* arena, int l, const float* x0, const void* h1_0, const float* m1_0, const float* r1_0) const {
    char* a_ = const_cast<char*>(static_cast<const char*>(arena)) + stride * l;
    const char* prev = a_ - stride;
    auto f = [](const char* p) { return reinterpret_cast<float*>(const_cast<char*>(p)); };
    mmdti_unimol_saved_t S;
    S.x = l ? f(prev + x_out) : x0;        S.h1 = l ? static_cast<const void*>(prev + ln_out) : h1_0;
    S.m1 = l ? f(prev + mn) : m1_0;        S.r1 = l ? f(prev + rn) : r1_0;
    S.qkv = a_ + qkv; S.s = a_ + s; S.o = a_ + o; S.x1 = f(a_ + x1); S.h2 = a_ + h2; S.m2 = f(a_ + m2); S.r2 = f(a_ + r2); S.u = a_ + u; S.a = a_ + a;
    return S;
  }
};
// backward workspace of the stack: two layer workspaces (the side-stream weight gradients of layer l read slot l & 1 while layer
// l - 1 fills the other), a ring of three bf16 gradient copies, two fp32 gradients
struct UniBwdWs {
  long long layer_ws, lws[2], dx16[3], dx32[2], total;
  UniBwdWs(long long M, long long D, long long F, long long slab_bytes, bool lora = false) {     // lora: one u row behind each layer workspace
    layer_ws = up256(unimol_layer_tmp_bytes(M, D, F) + slab_bytes) + (lora ? lora_row(M) : 0);
    long long at = 0;
    for (int i = 0; i < 2; ++i) { lws[i] = at; at += layer_ws; }
    for (int i = 0; i < 3; ++i) { dx16[i] = at; at += up256(M * D * 2); }
    for (int i = 0; i < 2; ++i) { dx32[i] = at; at += up256(M * D * 4); }
    total = at;
  }
};
}  // namespace

/* out[0] = bytes of one layer's slice of the activation arena, out[1] = bytes of the stack backward's workspace, out[2] = bytes of
 * mmdti_unimol_layer_bwd's (given the bytes of the grouped weight-gradient slabs of ONE layer: mmdti_linear_dw_grouped_splits) */
extern "C" int mmdti_unimol_stack_layout(int M, int D, int F, long long s_bytes, long long dw_slab_bytes, long long* out) {
  MMDTI_REQUIRE(M > 0 && D > 0 && F > 0 && s_bytes >= 0 && dw_slab_bytes >= 0 && out, "unimol_stack_layout: bad arguments");
  out[0] = UniArena(M, D, F, s_bytes).stride;
  out[1] = UniBwdWs(M, D, F, dw_slab_bytes).total;
  out[2] = unimol_layer_tmp_bytes(M, D, F) + dw_slab_bytes;
  return MMDTI_OK;
}
/* the same three for the adapted calls: each arena slice ends in the layer's t row, each layer workspace in a u row; no slabs */
extern "C" int mmdti_unimol_lora_stack_layout(int M, int D, int F, long long s_bytes, long long* out) {
  MMDTI_REQUIRE(M > 0 && D > 0 && F > 0 && s_bytes >= 0 && out, "unimol_lora_stack_layout: bad arguments");
  out[0] = UniArena(M, D, F, s_bytes, true).stride;
  out[1] = UniBwdWs(M, D, F, 0, true).total;
  out[2] = up256(unimol_layer_tmp_bytes(M, D, F)) + lora_row(M);
  return MMDTI_OK;
}

/* Forward of ALL layers of the Uni-Mol encoder (models/transformers.py:136-139 looped by :96-183) behind one call: nl x
 * mmdti_unimol_layer_fwd with the tensors a layer hands the next taken from the arena.  The last layer writes the tensors the caller
 * returns: s_last, x_last and -- with a final LayerNorm (g_final non-null) -- out_final [M,D] fp32 with its statistics.
 * lora (mmdti_unimol_lora_stack_fwd; null: the plain stack): nl adapter blocks, layer l's t row at the end of its slice. */
static int unimol_stack_fwd_core(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers,
                                 const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* x0, const void* h1_0, const void* s_in,
                                 const unsigned char* key_pad, int rag_store_last, const float* g_final, const float* bt_final, float eps_final,
                                 void* arena, long long arena_bytes, long long s_bytes, float* x_last, void* s_last, float* out_final,
                                 float* mean_final, float* rstd_final) {
  MMDTI_REQUIRE(run && nl > 0 && layers && arena && aligned16(arena) && x0 && h1_0 && s_in && x_last && s_last, "unimol_stack_fwd: null argument");
  MMDTI_REQUIRE(!g_final || (bt_final && out_final && mean_final && rstd_final), "unimol_stack_fwd: the final LayerNorm needs its outputs");
  for (int l = 0; l < nl; ++l)
    MMDTI_REQUIRE(unimol_fwd_params(layers[l]) && (l == 0 || (layers[l].g_ln1 && layers[l].bt_ln1)), "unimol_stack_fwd: null parameter in layer %d", l);
  const UniArena A(run->M, run->D, run->F, s_bytes, lora != nullptr);
  MMDTI_REQUIRE(arena_bytes >= A.stride * nl, "unimol_stack_fwd: arena too small (%lld bytes per layer)", A.stride);
  for (int l = 0; lora && l < nl; ++l) { MMDTI_REQUIRE_LORA("unimol_stack_fwd", lora + l, false, arena); }
  const void* sp = s_in;
  for (int l = 0; l < nl; ++l) {
    char* a = reinterpret_cast<char*>(arena) + A.stride * l;
    const bool last = l == nl - 1;
    mmdti_unimol_saved_t S = A.saved(arena, l, x0, h1_0, nullptr, nullptr);
    if (last) S.s = s_last;
    const mmdti_unimol_layer_t* nx = last ? nullptr : layers + l + 1;
    if (int e = unimol_layer_fwd_core(stream, run, layers + l, &S, lora ? lora + l : nullptr, a + A.t, site0 + 3 * l, site0 + 3 * l + 1, site0 + 3 * l + 2, sp,
                                      l ? nullptr : key_pad, last ? rag_store_last : 0, last ? (g_final ? 2 : 0) : 1, last ? g_final : nx->g_ln1,
                                      last ? bt_final : nx->bt_ln1, last ? eps_final : nx->eps_ln1, last ? x_last : reinterpret_cast<float*>(a + A.x_out),
                                      last ? static_cast<void*>(out_final) : static_cast<void*>(a + A.ln_out),
                                      last ? mean_final : reinterpret_cast<float*>(a + A.mn), last ? rstd_final : reinterpret_cast<float*>(a + A.rn)))
      return e;
    sp = S.s;
  }
  return MMDTI_OK;
}
extern "C" int mmdti_unimol_stack_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers, int nl,
                                      unsigned int site0, const float* x0, const void* h1_0, const void* s_in, const unsigned char* key_pad,
                                      int rag_store_last, const float* g_final, const float* bt_final, float eps_final, void* arena,
                                      long long arena_bytes, long long s_bytes, float* x_last, void* s_last, float* out_final,
                                      float* mean_final, float* rstd_final) {
  return unimol_stack_fwd_core(stream, run, layers, nullptr, nl, site0, x0, h1_0, s_in, key_pad, rag_store_last, g_final, bt_final, eps_final, arena,
                               arena_bytes, s_bytes, x_last, s_last, out_final, mean_final, rstd_final);
}
extern "C" int mmdti_unimol_lora_stack_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers,
                                           const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* x0, const void* h1_0,
                                           const void* s_in, const unsigned char* key_pad, int rag_store_last, const float* g_final,
                                           const float* bt_final, float eps_final, void* arena, long long arena_bytes, long long s_bytes,
                                           float* x_last, void* s_last, float* out_final, float* mean_final, float* rstd_final) {
  MMDTI_REQUIRE(lora, "unimol_lora_stack_fwd: null adapter blocks (a layer without an adapter has r 0)");
  return unimol_stack_fwd_core(stream, run, layers, lora, nl, site0, x0, h1_0, s_in, key_pad, rag_store_last, g_final, bt_final, eps_final, arena, arena_bytes,
                               s_bytes, x_last, s_last, out_final, mean_final, rstd_final);
}

/* Backward of the same stack, top layer first: nl x mmdti_unimol_layer_bwd.  dx_in [M,D] fp32 / dy2_in [M,D] bf16: the gradient of
 * the top layer's output and its dropout-backward bf16 copy (from the final LayerNorm's backward); dx_final [M,D] fp32: the gradient
 * of x0.  m1_0 / r1_0: LayerNorm-1 statistics of the first layer (the caller's, like x0 / h1_0); s_last: the top layer's logits.
 * G: the pair-gradient chain (g_first_zero: not yet written).  dw_stream + events (hipEvent_t [3], nullable together): the weight
 * gradients run on dw_stream under the layer below; `stream` has joined dw_stream when the call returns.
 * lora (mmdti_unimol_lora_stack_bwd; null: the plain stack): adapted layers on a frozen base, as unimol_layer_bwd_core's `frozen`; dx_final
 * may then be null (nothing under layer 0 reads its input gradient). */
static int unimol_stack_bwd_core(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers,
                                 const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* dx_in, const void* dy2_in, float* dx_final,
                                 const float* x0, const void* h1_0, const float* m1_0, const float* r1_0, const void* s_last, void* G, int g_first_zero,
                                 const void* arena, long long arena_bytes, long long s_bytes, void* ws, long long ws_bytes, long long dw_slab_bytes,
                                 mmdti_stream_t dw_stream, void* const* events) {
  const bool frozen = lora != nullptr;
  MMDTI_REQUIRE(run && nl > 0 && layers && arena && ws && aligned16(ws) && dx_in && dy2_in && (dx_final || frozen) && x0 && h1_0 && m1_0 && r1_0 && s_last && G,
                "unimol_stack_bwd: null argument");
  MMDTI_REQUIRE(!dw_stream || (events && events[0] && events[1] && events[2]), "unimol_stack_bwd: a weight-gradient stream needs three events");
  for (int l = 0; l < nl; ++l) MMDTI_REQUIRE(unimol_bwd_params(layers[l], frozen), "unimol_stack_bwd: null parameter in layer %d", l);
  for (int l = 0; frozen && l < nl; ++l) { MMDTI_REQUIRE_LORA("unimol_stack_bwd", lora + l, true, arena); }
  const UniArena A(run->M, run->D, run->F, s_bytes, frozen);
  const UniBwdWs W(run->M, run->D, run->F, dw_slab_bytes, frozen);
  MMDTI_REQUIRE(arena_bytes >= A.stride * nl && ws_bytes >= W.total, "unimol_stack_bwd: arena / workspace too small (%lld / %lld bytes)", A.stride * nl, W.total);
  char* wb = reinterpret_cast<char*>(ws);
  hipEvent_t fork = dw_stream ? (hipEvent_t)events[0] : nullptr;
  const float* dx = dx_in;
  const void* dy2 = dy2_in;
  for (int l = nl - 1, it = 0; l >= 0; --l, ++it) {
    hipEvent_t done = dw_stream ? (hipEvent_t)events[1 + (it & 1)] : nullptr;
    // (the weight gradients issued two layers ago read this layer workspace and the ring slot about to be written)
    if (dw_stream && it >= 2 && hipStreamWaitEvent((hipStream_t)stream, done, 0) != hipSuccess) {
      set_error("unimol_stack_bwd: hipStreamWaitEvent failed");
      return MMDTI_ERR_LAUNCH;
    }
    float* dx_out = l ? reinterpret_cast<float*>(wb + W.dx32[it & 1]) : dx_final;
    void* dx16_out = l ? static_cast<void*>(wb + W.dx16[it % 3]) : nullptr;
    mmdti_unimol_saved_t S = A.saved(arena, l, x0, h1_0, m1_0, r1_0);
    if (l == nl - 1) S.s = const_cast<void*>(s_last);
    if (int e = unimol_layer_bwd_core(stream, *run, layers[l], S, l ? site0 + 3 * (l - 1) + 2 : 0u, site0 + 3 * l + 1, site0 + 3 * l, dx, dy2, dx_out, dx16_out,
                                      l ? layers[l - 1].db_fc2 : nullptr, G, it == 0 ? g_first_zero : 0, wb + W.lws[it & 1], W.layer_ws, dw_stream, fork, done,
                                      frozen, frozen ? lora + l : nullptr, static_cast<const char*>(arena) + A.stride * l + A.t))
      return e;
    dx = dx_out;
    dy2 = dx16_out;
  }
  if (dw_stream) {
    for (int i = 0; i < 2 && i < nl; ++i)
      if (hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)events[1 + i], 0) != hipSuccess) {
        set_error("unimol_stack_bwd: join failed");
        return MMDTI_ERR_LAUNCH;
      }
  }
  return MMDTI_OK;
}
extern "C" int mmdti_unimol_stack_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers, int nl,
                                      unsigned int site0, const float* dx_in, const void* dy2_in, float* dx_final, const float* x0,
                                      const void* h1_0, const float* m1_0, const float* r1_0, const void* s_last, void* G, int g_first_zero,
                                      const void* arena, long long arena_bytes, long long s_bytes, void* ws, long long ws_bytes,
                                      long long dw_slab_bytes, mmdti_stream_t dw_stream, void* const* events) {
  return unimol_stack_bwd_core(stream, run, layers, nullptr, nl, site0, dx_in, dy2_in, dx_final, x0, h1_0, m1_0, r1_0, s_last, G, g_first_zero, arena,
                               arena_bytes, s_bytes, ws, ws_bytes, dw_slab_bytes, dw_stream, events);
}
extern "C" int mmdti_unimol_lora_stack_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers,
                                           const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* dx_in, const void* dy2_in,
                                           float* dx_final, const float* x0, const void* h1_0, const float* m1_0, const float* r1_0,
                                           const void* s_last, void* G, int g_first_zero, const void* arena, long long arena_bytes,
                                           long long s_bytes, void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(lora, "unimol_lora_stack_bwd: null adapter blocks (a layer without an adapter has r 0)");
  return unimol_stack_bwd_core(stream, run, layers, lora, nl, site0, dx_in, dy2_in, dx_final, x0, h1_0, m1_0, r1_0, s_last, G, g_first_zero, arena, arena_bytes,
                               s_bytes, ws, ws_bytes, 0, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- tower 2 and the cross block
/* The fused attention of the BERT-style sequencers below: mmdti_attn_* up to 256 queries x 256 keys, mmdti_attn_long_* beyond (the rule of
 * the host's ops.attn_dispatch, so that a sequenced layer launches what the op-by-op path launches).  Forward and backward of a layer
 * see the same Lq / Lk, hence the same pair -- and the same dropout mask. */
static inline bool attn_is_long(int Lq, int Lk) { return (Lq > Lk ? Lq : Lk) > 256; }
template <typename... A>
static int attn_pair_fwd(mmdti_stream_t stream, const void* q, const void* k, const void* v, const float* key_add, void* ctx, float* stats, int B,
                         int heads, int Lq, int Lk, A... rest) {
  return (attn_is_long(Lq, Lk) ? mmdti_attn_long_fwd : mmdti_attn_fwd)(stream, q, k, v, key_add, ctx, stats, B, heads, Lq, Lk, rest...);
}
template <typename... A>
static int attn_pair_bwd(mmdti_stream_t stream, const void* q, const void* k, const void* v, const float* key_add, const void* dctx,
                         const float* stats, float* drow, void* dq, void* dk, void* dv, int B, int heads, int Lq, int Lk, A... rest) {
  return (attn_is_long(Lq, Lk) ? mmdti_attn_long_bwd : mmdti_attn_bwd)(stream, q, k, v, key_add, dctx, stats, drow, dq, dk, dv, B, heads, Lq, Lk, rest...);
}

namespace {
// rows of the attention backward's row term
inline long long bert_nrow(const mmdti_bert_run_t& R) { return R.q_off ? (long long)R.heads * R.q_rows : (long long)R.B * R.heads * R.Lq; }
// bytes of ONE layer's backward temporaries, weight-gradient slabs aside (the layouts: mmdti_bert_layer_bwd / mmdti_bert_cross_layer_bwd;
// the cross layer's five activation gradients are its caller's)
inline long long bert_layer_tmp_bytes(long long M, long long D, long long F, long long nrow, bool cross) {
  return (cross ? 2 * M * D : M * F + 7 * M * D) * 2 + M * D * 4 + up16(nrow * 4);
}
// split: the three separate projections of a frozen base (mmdti_bert_split_t) stand in for the fused one
// the same for an adapted layer on a frozen base, self-attention (Mk = Mq: the count above) or cross: dzb, da, dyb, dctx, dq [Mq,D], du [Mq,F],
// dk, dv [Mk,D] (bf16), dz [Mq,D] fp32, drow
inline long long bert_lora_tmp_bytes(long long Mq, long long Mk, long long D, long long F, long long nrow) {
  return (Mq * F + 5 * Mq * D + 2 * Mk * D) * 2 + Mq * D * 4 + up16(nrow * 4);
}
inline bool bert_fwd_params(const mmdti_bert_layer_t& P, bool cross, const mmdti_bert_split_t* split = nullptr) {
  return (split ? split->w_q && split->w_k && split->w_v : P.w_qkv && (!cross || P.w_q)) && P.w_o && P.g_ln1 && P.bt_ln1 && P.w_i && P.w_o2 && P.g_ln2 &&
         P.bt_ln2;
}
inline bool bert_lora_bwd_params(const mmdti_bert_layer_t& P, const mmdti_bert_split_t& T) {
  return T.wb_q && T.wb_k && T.wb_v && P.wb_o && P.wb_i && P.wb_o2 && P.g_ln1 && P.g_ln2;
}
inline bool bert_bwd_params(const mmdti_bert_layer_t& P, bool cross) {
  return P.wb_qkv && P.wb_o && P.wb_i && P.wb_o2 && P.g_ln1 && P.g_ln2 && (cross ? P.wb_q != nullptr : P.dw_qkv && P.dw_o && P.dw_i && P.dw_o2);
}
// q, k, v of a layer inside its saved projections (self-attention: one [Mq,3D] matrix; cross: q [Mq,D] beside k | v [Mk,2D]; the
// separate projections of a frozen base, planes > 0: q [Mq,D], k [Mk,D], v [Mk,D] back to back, planes = Mq and Mk the rows) -- and, by
// the same rule, dq, dk, dv inside the gradients
struct Qkv { char *q, *k, *v; int ldq, ldkv; };
inline Qkv split_qkv(void* qkv, void* q, int D, bool cross, long long planes = 0, long long Mk = 0) {
  char* p = static_cast<char*>(qkv);
  if (planes) return {p, p + planes * D * 2, p + (planes + Mk) * D * 2, D, D};
  if (cross) return {static_cast<char*>(q), p, p + (size_t)D * 2, D, 2 * D};
  return {p, p + (size_t)D * 2, p + (size_t)2 * D * 2, 3 * D, 3 * D};
}

/* Forward of one post-LN BERT layer on the fused attention kernels.  Self-attention (HF RobertaLayer reached from
 * models/mm_model.py:562; the variant functional._bert_layer_fwd takes on the hot path): the q | k | v projection as one GEMM.  Cross
 * (BertCrossAttentionLayer, mm_module.py:615-626 through :663-677): the queries come from s1, keys and values from s2 through the
 * fused key | value projection.  Then, for both: fused attention (packed: q_off / k_off / k_cnt as mmdti_attn_fwd), output.dense +
 * residual + LayerNorm, intermediate + GELU, output + residual + LayerNorm.
 * split (the *_lora_* entry points; null otherwise): a frozen base -- three separate projection GEMMs into the planes of S.qkv, then
 * mmdti_lora_fwd of every adapted one (lora[0..2]: query, key, value; its t row j of `t`), in the order of functional._bert_layer_fwd. */
int bert_layer_fwd(const char* who, bool cross, mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                   const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f, float* out32, void* out16,
                   const mmdti_bert_split_t* split = nullptr, const mmdti_lora_adapter_t* lora = nullptr, void* t = nullptr) {
  MMDTI_REQUIRE(run && layer && saved, "%s: null block", who);
  const mmdti_bert_run_t& R = *run;
  const mmdti_bert_layer_t& P = *layer;
  const mmdti_bert_saved_t& S = *saved;
  const int Mq = R.Mq, Mk = cross ? R.Mk : R.Mq, Lk = cross ? R.Lk : R.Lq, D = R.D, F = R.F, heads = R.heads, fwd_f16 = R.fwd_f16;
  MMDTI_REQUIRE(Mq > 0 && Mk > 0 && D > 0 && F > 0 && heads > 0 && D % heads == 0, "%s: bad shape", who);
  MMDTI_REQUIRE(S.s1_32 && S.s1_16 && (!cross || (S.s2_16 && (split || S.q))) && bert_fwd_params(P, cross, split) && S.qkv && S.ctx && S.stats && S.y &&
                    S.a32 && S.a16 && S.am && S.ar && S.u && S.i && S.z && out32 && out16 && S.zm && S.zr, "%s: null argument", who);
  for (int j = 0; lora && j < 3; ++j) { MMDTI_REQUIRE_LORA(who, lora + j, false, t); }
  // fwd_f16 (the fp16 forward-operand mode): s1_16 / s2_16, the weights, ctx, a16, i and out16 hold fp16; q | k | v stay bf16 (the
  // attention kernels' operand type in every mode), u too
  const int ab = fwd_f16 ? MMDTI_DT_AB_F16 : 0;
  const Qkv T = split_qkv(S.qkv, S.q, D, cross, split ? Mq : 0, Mk);
  if (split) {
    const void* x[3] = {S.s1_16, cross ? S.s2_16 : S.s1_16, cross ? S.s2_16 : S.s1_16};
    void* y[3] = {T.q, T.k, T.v};
    const void* w[3] = {split->w_q, split->w_k, split->w_v};
    const float* b[3] = {split->b_q, split->b_k, split->b_v};
    const int rows[3] = {Mq, Mk, Mk};
    for (int j = 0; j < 3; ++j)
      if (int e = fwd_gemm(stream, x[j], D, w[j], D, b[j], y[j], rows[j], D, D, MMDTI_ACT_NONE, nullptr, nullptr, MMDTI_DT_BF16 | ab, 0.f, 0ull, 0u)) return e;
    for (int j = 0; lora && j < 3; ++j)
      if (lora_on(lora + j))
        if (int e = lora_fwd(stream, lora[j], x[j], y[j], D, static_cast<char*>(t) + j * lora_row(Mq > Mk ? Mq : Mk), rows[j], D, D, fwd_f16 ? 1 : 0, 0)) return e;
  } else if (cross) {
    if (int e = fwd_gemm(stream, S.s1_16, D, P.w_q, D, P.b_q, S.q, Mq, D, D, MMDTI_ACT_NONE, nullptr, nullptr, MMDTI_DT_BF16 | ab, 0.f, 0ull, 0u)) return e;
    if (int e = fwd_gemm(stream, S.s2_16, D, P.w_qkv, D, P.b_qkv, S.qkv, Mk, 2 * D, D, MMDTI_ACT_NONE, nullptr, nullptr, MMDTI_DT_BF16 | ab, 0.f, 0ull, 0u)) return e;
  } else if (int e = fwd_gemm(stream, S.s1_16, D, P.w_qkv, D, P.b_qkv, S.qkv, Mq, 3 * D, D, MMDTI_ACT_NONE, nullptr, nullptr, MMDTI_DT_BF16 | ab, 0.f, 0ull, 0u)) {
    return e;
  }
  if (int e = attn_pair_fwd(stream, T.q, T.k, T.v, R.key_add, S.ctx, S.stats, R.B, heads, R.Lq, Lk, D / heads, T.ldq, T.ldkv, D, R.scale, R.p_att, R.seed,
                             site_att, R.q_off, R.k_off, R.k_cnt, R.q_rows, fwd_f16 ? 1 : 0))
    return e;
  if (int e = closer(stream, S.ctx, P.w_o, P.b_o, S.s1_32, Mq, D, D, R.p_hid, R.seed, site_o, S.y, P.g_ln1, P.bt_ln1, R.eps, S.a32, S.a16, S.am, S.ar, R.ln_max_k,
                     fwd_f16))
    return e;
  if (int e = fwd_gemm(stream, S.a16, D, P.w_i, D, P.b_i, S.i, Mq, F, D, R.act_fwd, S.u, nullptr, (fwd_f16 ? MMDTI_DT_F16 : MMDTI_DT_BF16) | ab, 0.f, 0ull, 0u))
    return e;
  return closer(stream, S.i, P.w_o2, P.b_o2, S.a32, Mq, D, F, R.p_hid, R.seed, site_f, S.z, P.g_ln2, P.bt_ln2, R.eps, out32, out16, S.zm, S.zr, R.ln_max_k,
                fwd_f16);
}

/* What the two backwards share, six launches: LayerNorm-2 backward, the FFN's two input gradients, LayerNorm-1 backward (its output
 * fed the FFN and the residual: dy_add; ds1 receives its residual gradient), the output projection's input gradient, the fused
 * attention backward (dq | dk | dv written straight into dqkv -- cross: dq beside dk | dv).  The bf16 temporaries dzb [Mq,D], du [Mq,F],
 * da, dyb, dctx [Mq,D] and the fp32 dz [Mq,D], drow are the caller's. */
int bert_bwd_shared(mmdti_stream_t stream, const mmdti_bert_run_t& R, const mmdti_bert_layer_t& P, const mmdti_bert_saved_t& S, bool cross,
                    unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout, float* ds1, void* dzb, void* du, void* da,
                    void* dyb, void* dctx, float* dz, float* drow, void* dqkv, void* dq, bool planes = false) {
  // planes: S.qkv and dqkv hold q, k, v (dq, dk, dv) as three planes (a frozen base: split_qkv)
  const int Mq = R.Mq, Mk = cross ? R.Mk : R.Mq, Lk = cross ? R.Lk : R.Lq, D = R.D, F = R.F;
  if (int e = mmdti_layernorm_bwd(stream, dout, MMDTI_DT_F32, nullptr, S.z, P.g_ln2, S.zm, S.zr, Mq, D, nullptr, dz, P.dg_ln2, P.dbt_ln2, nullptr, 0.f, 0ull, 0u,
                                  dzb, R.p_hid, site_f, P.db_o2))
    return e;
  if (int e = dx_gemm(stream, dzb, D, P.wb_o2, F, du, Mq, F, D, R.act_dx, S.u, F)) return e;
  if (int e = dx_gemm(stream, du, F, P.wb_i, D, da, Mq, D, F, MMDTI_ACT_NONE, nullptr, 0)) return e;
  if (int e = mmdti_layernorm_bwd(stream, da, MMDTI_DT_BF16, dz, S.y, P.g_ln1, S.am, S.ar, Mq, D, nullptr, ds1, P.dg_ln1, P.dbt_ln1, nullptr, 0.f, 0ull, 0u, dyb,
                                  R.p_hid, site_o, P.db_o))
    return e;
  if (int e = dx_gemm(stream, dyb, D, P.wb_o, D, dctx, Mq, D, D, MMDTI_ACT_NONE, nullptr, 0)) return e;
  const Qkv T = split_qkv(S.qkv, S.q, D, cross, planes ? Mq : 0, Mk), dT = split_qkv(dqkv, dq, D, cross, planes ? Mq : 0, Mk);
  return attn_pair_bwd(stream, T.q, T.k, T.v, R.key_add, dctx, S.stats, drow, dT.q, dT.k, dT.v, R.B, R.heads, R.Lq, Lk, D / R.heads, T.ldq, T.ldkv, D, dT.ldq,
                       dT.ldkv, R.scale, R.p_att, R.seed, site_att, R.q_off, R.k_off, R.k_cnt, R.q_rows);
}
// out[M, D] (fp32) = beta * out + dy[M, n_in] . w[n_in, D]: the input gradient of a projection, straight into the fp32 stream gradient
inline int dx_gemm_f32(mmdti_stream_t s, const void* dy, const void* w, float* out, int M, int D, int n_in, float beta) {
  return mmdti_gemm_bf16(s, dy, w, out, M, D, n_in, n_in, D, D, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1.f, beta, nullptr, nullptr, D, MMDTI_ACT_NONE, nullptr, nullptr, D,
                         MMDTI_DT_F32, 0.f, 0ull, 0u, nullptr, nullptr, nullptr, 0);
}
}  // namespace

extern "C" int mmdti_bert_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                    const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                                    float* out32, void* out16) {
  return bert_layer_fwd("bert_layer_fwd", false, stream, run, layer, saved, site_att, site_o, site_f, out32, out16);
}
extern "C" int mmdti_bert_cross_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                          const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                                          float* out32, void* out16) {
  return bert_layer_fwd("bert_cross_layer_fwd", true, stream, run, layer, saved, site_att, site_o, site_f, out32, out16);
}

extern "C" int mmdti_bert_lora_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                         const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved, void* t,
                                         unsigned int site_att, unsigned int site_o, unsigned int site_f, float* out32, void* out16) {
  MMDTI_REQUIRE(split, "bert_lora_layer_fwd: null block");
  return bert_layer_fwd("bert_lora_layer_fwd", false, stream, run, layer, saved, site_att, site_o, site_f, out32, out16, split, lora, t);
}
extern "C" int mmdti_bert_lora_cross_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                               const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                                               void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, float* out32,
                                               void* out16) {
  MMDTI_REQUIRE(split, "bert_lora_cross_layer_fwd: null block");
  return bert_layer_fwd("bert_lora_cross_layer_fwd", true, stream, run, layer, saved, site_att, site_o, site_f, out32, out16, split, lora, t);
}

/* Backward of the self-attention layer: the shared launches, the fused projection's input gradient accumulated into ds1, and the four
 * weight gradients as one grouped launch.  dout [Mq,D] fp32 -> ds1 [Mq,D] fp32 (written).
 *   ws: dzb [Mq,D] | du [Mq,F] | da [Mq,D] | dyb [Mq,D] | dctx [Mq,D] | dqkv [Mq,3D] (bf16) | dz [Mq,D] f32 | drow [heads*rows] f32 | slabs. */
extern "C" int mmdti_bert_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                    const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                                    const float* dout, float* ds1, void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(run && layer && saved, "bert_layer_bwd: null block");
  const mmdti_bert_run_t& R = *run;
  const mmdti_bert_layer_t& P = *layer;
  const mmdti_bert_saved_t& S = *saved;
  const int Mq = R.Mq, D = R.D, F = R.F;
  MMDTI_REQUIRE(Mq > 0 && D > 0 && F > 0 && R.heads > 0 && D % R.heads == 0, "bert_layer_bwd: bad shape");
  MMDTI_REQUIRE(dout && ds1 && S.s1_16 && S.qkv && S.ctx && S.stats && S.y && S.a16 && S.am && S.ar && S.u && S.i && S.z && S.zm && S.zr &&
                    bert_bwd_params(P, false) && ws, "bert_layer_bwd: null argument");
  const long long MD = (long long)Mq * D, MF = (long long)Mq * F, nrow = bert_nrow(R);
  const long long fixed = bert_layer_tmp_bytes(Mq, D, F, nrow, false);
  MMDTI_REQUIRE(ws_bytes >= fixed && aligned16(ws), "bert_layer_bwd: workspace too small (%lld bytes for the temporaries alone)", fixed);
  char* wp = reinterpret_cast<char*>(ws);
  void* dzb = wp;  wp += MD * 2;
  void* du = wp;   wp += MF * 2;
  void* da = wp;   wp += MD * 2;
  void* dyb = wp;  wp += MD * 2;
  void* dctx = wp; wp += MD * 2;
  void* dqkv = wp; wp += 3 * MD * 2;
  float* dz = reinterpret_cast<float*>(wp); wp += MD * 4;
  float* drow = reinterpret_cast<float*>(wp); wp += up16(nrow * 4);
  void* slabs = wp;
  const long long slab_bytes = ws_bytes - fixed;
  if (int e = bert_bwd_shared(stream, R, P, S, false, site_att, site_o, site_f, dout, ds1, dzb, du, da, dyb, dctx, dz, drow, dqkv, nullptr)) return e;
  if (int e = dx_gemm_f32(stream, dqkv, P.wb_qkv, ds1, Mq, D, 3 * D, 1.f)) return e;      // ds1 += dqkv . W_qkv
  const void* dys[4] = {dqkv, dzb, du, dyb};
  const void* xs[4] = {S.s1_16, S.i, S.a16, S.ctx};
  float* dws[4] = {P.dw_qkv, P.dw_o2, P.dw_i, P.dw_o};
  float* dbs[4] = {P.db_qkv, nullptr, P.db_i, nullptr};
  const int n_out[4] = {3 * D, D, F, D}, n_in[4] = {D, F, D, D};
  const int ldy[4] = {3 * D, D, F, D}, ldx[4] = {D, F, D, D}, lddw[4] = {P.lddw_qkv, F, D, D};
  // (fwd_f16: the saved s1_16, i, a16 and ctx hold fp16 -- converted between LDS and the matrix pipe)
  return mmdti_linear_dw_grouped(stream, 4, dys, xs, dws, dbs, n_out, n_in, ldy, ldx, lddw, Mq, slabs, slab_bytes, R.fwd_f16 ? 1 : 0);
}

/* Backward of the cross layer up to the weight gradients: the shared launches (dq [Mq,D]; dk | dv straight into dkv [Mk,2D]), ds1 += dq .
 * W_q, ds2 = dkv . W_kv ([Mk,D] fp32, written; null: s2 needs no gradient).  The caller owns the five activation gradients (dzb, du,
 * dyb, dq, dkv: bf16) -- they are the A operands of the layer's weight gradients, which it launches itself (two token-row counts:
 * mmdti_linear_dw_grouped takes one per launch).  ws: da [Mq,D] | dctx [Mq,D] bf16 | dz [Mq,D] f32 | drow. */
extern "C" int mmdti_bert_cross_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                          const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                                          const float* dout, float* ds1, float* ds2, void* dzb, void* du, void* dyb, void* dq, void* dkv,
                                          void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(run && layer && saved, "bert_cross_layer_bwd: null block");
  const mmdti_bert_run_t& R = *run;
  const mmdti_bert_layer_t& P = *layer;
  const mmdti_bert_saved_t& S = *saved;
  const int Mq = R.Mq, D = R.D;
  MMDTI_REQUIRE(Mq > 0 && R.Mk > 0 && D > 0 && R.F > 0 && R.heads > 0 && D % R.heads == 0, "bert_cross_layer_bwd: bad shape");
  MMDTI_REQUIRE(dout && ds1 && S.q && S.qkv && S.stats && S.y && S.am && S.ar && S.u && S.z && S.zm && S.zr && bert_bwd_params(P, true) && dzb && du && dyb &&
                    dq && dkv && ws, "bert_cross_layer_bwd: null argument");
  const long long MD = (long long)Mq * D, need = bert_layer_tmp_bytes(Mq, D, R.F, bert_nrow(R), true);
  MMDTI_REQUIRE(ws_bytes >= need && aligned16(ws), "bert_cross_layer_bwd: workspace too small (%lld bytes)", need);
  char* wp = reinterpret_cast<char*>(ws);
  void* da = wp;   wp += MD * 2;
  void* dctx = wp; wp += MD * 2;
  float* dz = reinterpret_cast<float*>(wp); wp += MD * 4;
  float* drow = reinterpret_cast<float*>(wp);
  if (int e = bert_bwd_shared(stream, R, P, S, true, site_att, site_o, site_f, dout, ds1, dzb, du, da, dyb, dctx, dz, drow, dkv, dq)) return e;
  if (int e = dx_gemm_f32(stream, dq, P.wb_q, ds1, Mq, D, D, 1.f)) return e;               // ds1 += dq . W_q
  if (!ds2) return MMDTI_OK;          // (s2 needs no gradient)
  return dx_gemm_f32(stream, dkv, P.wb_qkv, ds2, R.Mk, D, 2 * D, 0.f);                    // ds2 = dkv . W_kv
}

/* Backward of an adapted layer on a frozen base, self-attention or cross (functional._bert_layer_bwd, the branch without a fused
 * projection): the shared launches (dq, dk, dv as three planes), mmdti_lora_bwd of every adapted projection (query, key, value), then
 * the input gradients with each adapter's dx behind the GEMMs of its stream gradient: ds1 += dq . W_q; self-attention: ds1 += dk . W_k,
 * ds1 += dv . W_v; cross: ds2 = dk . W_k, ds2 += dv . W_v.  No weight gradient: the base has none.
 *   ws: dzb [Mq,D] | du [Mq,F] | da | dyb | dctx | dq [Mq,D] | dk | dv [Mk,D] (bf16) | dz [Mq,D] f32 | drow -> rounded up to 256 | three u rows. */
static int bert_lora_layer_bwd(const char* who, bool cross, mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                               const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved, const void* t,
                               unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout, float* ds1, int want_ds1,
                               float* ds2, int want_ds2, void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(run && layer && saved && split, "%s: null block", who);
  const mmdti_bert_run_t& R = *run;
  const mmdti_bert_layer_t& P = *layer;
  const mmdti_bert_saved_t& S = *saved;
  const int Mq = R.Mq, Mk = cross ? R.Mk : R.Mq, D = R.D, F = R.F;
  MMDTI_REQUIRE(Mq > 0 && Mk > 0 && D > 0 && F > 0 && R.heads > 0 && D % R.heads == 0 && D % 8 == 0, "%s: bad shape", who);
  MMDTI_REQUIRE(dout && ds1 && (!want_ds2 || (cross && ds2)) && S.s1_16 && (!cross || S.s2_16) && S.qkv && S.stats && S.y && S.am && S.ar && S.u && S.z &&
                    S.zm && S.zr && bert_lora_bwd_params(P, *split) && ws, "%s: null argument", who);
  for (int j = 0; lora && j < 3; ++j) { MMDTI_REQUIRE_LORA(who, lora + j, true, t); }
  const long long MD = (long long)Mq * D, KD = (long long)Mk * D, row = lora_row(Mq > Mk ? Mq : Mk);
  const long long tmp = up256(bert_lora_tmp_bytes(Mq, Mk, D, F, bert_nrow(R))), need = tmp + 3 * row;
  MMDTI_REQUIRE(ws_bytes >= need && aligned16(ws), "%s: workspace too small (%lld bytes)", who, need);
  char* wp = reinterpret_cast<char*>(ws);
  void* dzb = wp;  wp += MD * 2;
  void* du = wp;   wp += (long long)Mq * F * 2;
  void* da = wp;   wp += MD * 2;
  void* dyb = wp;  wp += MD * 2;
  void* dctx = wp; wp += MD * 2;
  void* dqkv = wp; wp += (MD + 2 * KD) * 2;
  float* dz = reinterpret_cast<float*>(wp); wp += MD * 4;
  float* drow = reinterpret_cast<float*>(wp);
  char* u = reinterpret_cast<char*>(ws) + tmp;
  if (int e = bert_bwd_shared(stream, R, P, S, cross, site_att, site_o, site_f, dout, ds1, dzb, du, da, dyb, dctx, dz, drow, dqkv, nullptr, true)) return e;
  const Qkv dT = split_qkv(dqkv, nullptr, D, cross, Mq, Mk);
  const void* x[3] = {S.s1_16, cross ? S.s2_16 : S.s1_16, cross ? S.s2_16 : S.s1_16};
  const void* dy[3] = {dT.q, dT.k, dT.v};
  const int rows[3] = {Mq, Mk, Mk};
  for (int j = 0; lora && j < 3; ++j)
    if (lora_on(lora + j))
      if (int e = lora_bwd(stream, lora[j], x[j], R.fwd_f16 ? 1 : 0, dy[j], D, static_cast<const char*>(t) + j * row, u + j * row, rows[j], D, D)) return e;
  auto dx = [&](int j, float* ds) {       // ds += u_j . A_j
    return lora && lora_on(lora + j) ? mmdti_lora_dx(stream, u + j * row, lora[j].A_bf16, ds, D, 0, rows[j], D, lora[j].r) : MMDTI_OK;
  };
  if (want_ds1) {
    if (int e = dx_gemm_f32(stream, dT.q, split->wb_q, ds1, Mq, D, D, 1.f)) return e;
    if (int e = dx(0, ds1)) return e;
  }
  float* dkv = cross ? ds2 : ds1;
  if (!(cross ? want_ds2 : want_ds1)) return MMDTI_OK;
  if (int e = dx_gemm_f32(stream, dT.k, split->wb_k, dkv, Mk, D, D, cross ? 0.f : 1.f)) return e;
  if (int e = dx_gemm_f32(stream, dT.v, split->wb_v, dkv, Mk, D, D, 1.f)) return e;
  if (int e = dx(1, dkv)) return e;
  return dx(2, dkv);
}
extern "C" int mmdti_bert_lora_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                         const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                                         const void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout,
                                         float* ds1, int want_ds1, void* ws, long long ws_bytes) {
  return bert_lora_layer_bwd("bert_lora_layer_bwd", false, stream, run, layer, split, lora, saved, t, site_att, site_o, site_f, dout, ds1, want_ds1, nullptr, 0, ws,
                             ws_bytes);
}
extern "C" int mmdti_bert_lora_cross_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                                               const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                                               const void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout,
                                               float* ds1, int want_ds1, float* ds2, int want_ds2, void* ws, long long ws_bytes) {
  return bert_lora_layer_bwd("bert_lora_cross_layer_bwd", true, stream, run, layer, split, lora, saved, t, site_att, site_o, site_f, dout, ds1, want_ds1, ds2,
                             want_ds2, ws, ws_bytes);
}

// ---------------------------------------------------------------------------------------------------------------- tower 2's stack
namespace {
struct BertArena {     // byte offsets inside one layer's slice
  long long qkv, ctx, stats, y, a32, a16, am, ar, u, i, z, out32, out16, zm, zr, t, stride;
  BertArena(long long M, long long D, long long F, long long stats_bytes, bool lora = false) {       // lora: three t rows behind the slice
    long long at = 0;
    auto take = [&](long long b) { const long long r = at; at += up256(b); return r; };
    qkv = take(M * 3 * D * 2); ctx = take(M * D * 2); stats = take(stats_bytes); y = take(M * D * 4); a32 = take(M * D * 4); a16 = take(M * D * 2);
    am = take(M * 4); ar = take(M * 4); u = take(M * F * 2); i = take(M * F * 2); z = take(M * D * 4); out32 = take(M * D * 4); out16 = take(M * D * 2);
    zm = take(M * 4); zr = take(M * 4);
    t = lora ? take(3 * lora_row(M)) : 0;
    stride = at;
  }
  // the saved block of slice l: a layer's input is the output of the slice below (layer 0: the caller's)
  mmdti_bert_saved_t saved(const void* arena, int l, const float* s1_32_0, const void* s1_16_0) const {
    char* a_ = const_cast<char*>(static_cast<const char*>(arena)) + stride * l;
    const char* prev = a_ - stride;
    auto f = [](const char* p) { return reinterpret_cast<float*>(const_cast<char*>(p)); };
    mmdti_bert_saved_t S;
    S.s1_32 = l ? f(prev + out32) : s1_32_0;   S.s1_16 = l ? static_cast<const void*>(prev + out16) : s1_16_0;   S.s2_16 = nullptr;   S.q = nullptr;
    S.qkv = a_ + qkv; S.ctx = a_ + ctx; S.stats = f(a_ + stats); S.y = f(a_ + y); S.a32 = f(a_ + a32); S.a16 = a_ + a16; S.am = f(a_ + am); S.ar = f(a_ + ar);
    S.u = a_ + u; S.i = a_ + i; S.z = f(a_ + z); S.zm = f(a_ + zm); S.zr = f(a_ + zr);
    return S;
  }
};
struct BertBwdWs {     // one layer workspace (mmdti_bert_layer_bwd's) + two fp32 gradients handed from layer to layer
  long long layer_ws, lws, ds[2], total;
  BertBwdWs(long long M, long long D, long long F, long long nrow, long long slab_bytes, bool lora = false) {       // lora: three u rows
    layer_ws = up256(bert_layer_tmp_bytes(M, D, F, nrow, false) + slab_bytes) + (lora ? 3 * lora_row(M) : 0);
    lws = 0;
    long long at = layer_ws;
    for (int k = 0; k < 2; ++k) { ds[k] = at; at += up256(M * D * 4); }
    total = at;
  }
};
}  // namespace

/* out[0] = arena bytes per layer, out[1] = the stack backward's workspace bytes, out[2] / out[3] = mmdti_bert_layer_bwd's /
 * mmdti_bert_cross_layer_bwd's (stats_bytes: one layer's softmax statistics; nrow: rows of the attention backward's row term -- heads *
 * q_rows packed, B * heads * Lq dense; dw_slab_bytes: see mmdti_unimol_stack_layout -- the cross layer takes no slab) */
extern "C" int mmdti_bert_stack_layout(int Mq, int D, int F, long long stats_bytes, long long nrow, long long dw_slab_bytes, long long* out) {
  MMDTI_REQUIRE(Mq > 0 && D > 0 && F > 0 && stats_bytes >= 0 && nrow >= 0 && dw_slab_bytes >= 0 && out, "bert_stack_layout: bad arguments");
  out[0] = BertArena(Mq, D, F, stats_bytes).stride;
  out[1] = BertBwdWs(Mq, D, F, nrow, dw_slab_bytes).total;
  out[2] = bert_layer_tmp_bytes(Mq, D, F, nrow, false) + dw_slab_bytes;
  out[3] = bert_layer_tmp_bytes(Mq, D, F, nrow, true);
  return MMDTI_OK;
}
/* the same for the adapted calls (mmdti_hip.h): t rows behind each arena slice, u rows behind each layer workspace, no slabs */
extern "C" int mmdti_bert_lora_stack_layout(int Mq, int Mk, int D, int F, long long stats_bytes, long long nrow, long long* out) {
  MMDTI_REQUIRE(Mq > 0 && Mk > 0 && D > 0 && F > 0 && stats_bytes >= 0 && nrow >= 0 && out, "bert_lora_stack_layout: bad arguments");
  const long long rows3 = 3 * lora_row(Mq > Mk ? Mq : Mk);
  out[0] = BertArena(Mq, D, F, stats_bytes, true).stride;
  out[1] = BertBwdWs(Mq, D, F, nrow, 0, true).total;
  out[2] = up256(bert_lora_tmp_bytes(Mq, Mq, D, F, nrow)) + 3 * lora_row(Mq);
  out[3] = up256(bert_lora_tmp_bytes(Mq, Mk, D, F, nrow)) + rows3;
  out[4] = rows3;
  return MMDTI_OK;
}

/* Forward of ALL layers of tower 2 (HF RobertaEncoder's layer loop, reached from models/mm_model.py:562) behind one call: nl x
 * mmdti_bert_layer_fwd, a layer's out32 / out16 being the next one's input.  s1_32_0 / s1_16_0: the embeddings' LayerNorm output (the
 * caller's).  The last layer's fp32 output goes to out32_last (the caller's).
 * split / lora (mmdti_bert_lora_stack_fwd; null: the plain stack): nl blocks of separate projections, 3 nl adapter blocks. */
static int bert_stack_fwd_core(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, const mmdti_bert_split_t* split,
                               const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* s1_32_0, const void* s1_16_0, void* arena,
                               long long arena_bytes, long long stats_bytes, float* out32_last) {
  MMDTI_REQUIRE(run && nl > 0 && layers && arena && aligned16(arena) && s1_32_0 && s1_16_0 && out32_last, "bert_stack_fwd: null argument");
  for (int l = 0; l < nl; ++l) MMDTI_REQUIRE(bert_fwd_params(layers[l], false, split ? split + l : nullptr), "bert_stack_fwd: null parameter in layer %d", l);
  for (int j = 0; split && j < 3 * nl; ++j) { MMDTI_REQUIRE_LORA("bert_stack_fwd", lora + j, false, arena); }
  const BertArena A(run->Mq, run->D, run->F, stats_bytes, split != nullptr);
  MMDTI_REQUIRE(arena_bytes >= A.stride * nl, "bert_stack_fwd: arena too small (%lld bytes per layer)", A.stride);
  for (int l = 0; l < nl; ++l) {
    char* a = reinterpret_cast<char*>(arena) + A.stride * l;
    const mmdti_bert_saved_t S = A.saved(arena, l, s1_32_0, s1_16_0);
    if (int e = bert_layer_fwd(split ? "bert_lora_layer_fwd" : "bert_layer_fwd", false, stream, run, layers + l, &S, site0 + 3 * l, site0 + 3 * l + 1, site0 + 3 * l + 2,
                               l == nl - 1 ? out32_last : reinterpret_cast<float*>(a + A.out32), a + A.out16, split ? split + l : nullptr,
                               split ? lora + 3 * l : nullptr, a + A.t))
      return e;
  }
  return MMDTI_OK;
}
extern "C" int mmdti_bert_stack_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, int nl,
                                    unsigned int site0, const float* s1_32_0, const void* s1_16_0, void* arena, long long arena_bytes,
                                    long long stats_bytes, float* out32_last) {
  return bert_stack_fwd_core(stream, run, layers, nullptr, nullptr, nl, site0, s1_32_0, s1_16_0, arena, arena_bytes, stats_bytes, out32_last);
}
extern "C" int mmdti_bert_lora_stack_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers,
                                         const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, int nl, unsigned int site0,
                                         const float* s1_32_0, const void* s1_16_0, void* arena, long long arena_bytes, long long stats_bytes,
                                         float* out32_last) {
  MMDTI_REQUIRE(split && lora, "bert_lora_stack_fwd: null block (a projection without an adapter has r 0)");
  return bert_stack_fwd_core(stream, run, layers, split, lora, nl, site0, s1_32_0, s1_16_0, arena, arena_bytes, stats_bytes, out32_last);
}

/* Backward of the same stack, top layer first: nl x mmdti_bert_layer_bwd.  dout [Mq,D] fp32: the gradient of the tower's output;
 * ds1_final [Mq,D] fp32: the gradient of s1_32_0.
 * split / lora (mmdti_bert_lora_stack_bwd; null: the plain stack): nl x mmdti_bert_lora_layer_bwd on the arena and workspace with the t / u
 * rows; want_final 0: nothing reads the gradient of s1_32_0. */
static int bert_stack_bwd_core(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, const mmdti_bert_split_t* split,
                               const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* dout, float* ds1_final, int want_final,
                               const void* s1_16_0, const void* arena, long long arena_bytes, long long stats_bytes, void* ws, long long ws_bytes,
                               long long dw_slab_bytes) {
  MMDTI_REQUIRE(run && nl > 0 && layers && arena && ws && aligned16(ws) && dout && ds1_final && s1_16_0, "bert_stack_bwd: null argument");
  for (int l = 0; l < nl; ++l)
    MMDTI_REQUIRE(split ? bert_lora_bwd_params(layers[l], split[l]) : bert_bwd_params(layers[l], false), "bert_stack_bwd: null parameter in layer %d", l);
  for (int j = 0; split && j < 3 * nl; ++j) { MMDTI_REQUIRE_LORA("bert_stack_bwd", lora + j, true, arena); }
  const BertArena A(run->Mq, run->D, run->F, stats_bytes, split != nullptr);
  const BertBwdWs W(run->Mq, run->D, run->F, bert_nrow(*run), dw_slab_bytes, split != nullptr);
  MMDTI_REQUIRE(arena_bytes >= A.stride * nl && ws_bytes >= W.total, "bert_stack_bwd: arena / workspace too small (%lld / %lld bytes)", A.stride * nl, W.total);
  char* wb = reinterpret_cast<char*>(ws);
  const float* d = dout;
  for (int l = nl - 1, it = 0; l >= 0; --l, ++it) {
    float* ds1 = l ? reinterpret_cast<float*>(wb + W.ds[it & 1]) : ds1_final;
    // (a backward does not read s1_32: layer 0 goes without)
    const mmdti_bert_saved_t S = A.saved(arena, l, nullptr, s1_16_0);
    const unsigned int s0 = site0 + 3 * l;
    if (int e = split ? bert_lora_layer_bwd("bert_lora_layer_bwd", false, stream, run, layers + l, split + l, lora + 3 * l, &S,
                                            static_cast<const char*>(arena) + A.stride * l + A.t, s0, s0 + 1, s0 + 2, d, ds1, l ? 1 : want_final, nullptr, 0,
                                            wb + W.lws, W.layer_ws)
                      : mmdti_bert_layer_bwd(stream, run, layers + l, &S, s0, s0 + 1, s0 + 2, d, ds1, wb + W.lws, W.layer_ws))
      return e;
    d = ds1;
  }
  return MMDTI_OK;
}
extern "C" int mmdti_bert_stack_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, int nl,
                                    unsigned int site0, const float* dout, float* ds1_final, const void* s1_16_0, const void* arena,
                                    long long arena_bytes, long long stats_bytes, void* ws, long long ws_bytes, long long dw_slab_bytes) {
  return bert_stack_bwd_core(stream, run, layers, nullptr, nullptr, nl, site0, dout, ds1_final, 1, s1_16_0, arena, arena_bytes, stats_bytes, ws, ws_bytes,
                             dw_slab_bytes);
}
extern "C" int mmdti_bert_lora_stack_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers,
                                         const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, int nl, unsigned int site0,
                                         const float* dout, float* ds1_final, int want_ds1_final, const void* s1_16_0, const void* arena,
                                         long long arena_bytes, long long stats_bytes, void* ws, long long ws_bytes) {
  MMDTI_REQUIRE(split && lora, "bert_lora_stack_bwd: null block (a projection without an adapter has r 0)");
  return bert_stack_bwd_core(stream, run, layers, split, lora, nl, site0, dout, ds1_final, want_ds1_final, s1_16_0, arena, arena_bytes, stats_bytes, ws,
                             ws_bytes, 0);
}
