/* mmdti_hip.h -- C ABI of libmmdti_hip.so: the MI355X (gfx950) kernels behind the
 * MM-DTI dual-encoder contrastive fine-tune step.
 *
 * The reference (ndlongvn/MM-DTI) has no native layer: its hot path is Python
 * calling torch / Uni-Core / HuggingFace ops.  Each entry point below replaces
 * the ATen / Uni-Core-CUDA kernels that one reference call site reaches; the
 * call site is cited per function as file:line relative to the reference root.
 * The host-side mirror of the reference's module interface (same class names,
 * ctor/forward signatures, parameter names) lives in mm-dti_amd/mmdti_hip/models
 * and binds these symbols through ctypes.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is DEVICE memory unless noted.
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on
 *     it (no host sync, no allocation, graph-capture safe).
 *   - bf16 tensors are raw uint16 bit patterns (`void*` in the signature).
 *   - return value: MMDTI_OK or an error code; mmdti_last_error() gives the text
 *     (thread-local).  Argument validation happens on the host BEFORE any launch.
 *   - "atomic accumulate" outputs must be zeroed by the caller (gradient arena).
 *   - dropout: p in [0,1); mask = counter-based hash RNG(seed, site, element index); the
 *     backward entry regenerates the same mask from (seed, site).
 */
#ifndef MMDTI_HIP_H
#define MMDTI_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mmdti_stream_t;

/* What mmdti_abi_version() of a library built from this header returns.  It changes with every incompatible change of a signature, a
 * struct or a layout below; a binding compares the two before its first call (the host package does: _abi.py). */
#define MMDTI_ABI_VERSION 2

#define MMDTI_OK 0
#define MMDTI_ERR_INVALID 1
#define MMDTI_ERR_LAUNCH 2

#define MMDTI_ACT_NONE 0
#define MMDTI_ACT_GELU 1      /* erf GELU; optional aux_out = pre-activation (bf16) */
#define MMDTI_ACT_GELU_BWD 2  /* multiply by gelu'(aux_in) */
#define MMDTI_ACT_GELU_G 4    /* erf GELU; aux_out (required) = gelu'(pre-activation) as bf16: the forward has the erf and
                                 the Gaussian in hand, so the backward (MUL_AUX) is one multiply per element */
#define MMDTI_ACT_MUL_AUX 5   /* multiply by aux_in (bf16) */

#define MMDTI_DT_F32 0
#define MMDTI_DT_BF16 1
#define MMDTI_DT_F32_ATOMIC 2 /* atomicAdd into fp32 C (split-K / gradient accumulation) */
/* fp16 forward operands (the default precision mode since round 4; the reference's own AMP dtype, tasks/trainer.py:181-182 -- three
 * more mantissa bits than bf16 at the same matrix-pipe rate; profiles/r03_rounding_sites_fp16.json): */
#define MMDTI_DT_F16 3        /* the 16-bit output is fp16 instead of bf16 */
#define MMDTI_DT_AB_F16 16    /* OR-ed into mmdti_gemm_bf16's c_dtype: A and B hold fp16 (forward Linear shapes only: row-major A,
                                 weight-layout B, no split-K, no batch) */
#define MMDTI_DT_B_F16 32     /* OR-ed into mmdti_gemm_bf16's c_dtype: B holds fp16 beside a bf16 A -- the weight gradient dW += dy^T.x
                                 (transA = transB = 1, MMDTI_DT_F32_ATOMIC) whose x is a forward activation saved as fp16.  The tile is
                                 fetched as it lies in memory and converted to bf16 (round to nearest even: the values
                                 mmdti_cast_f16_bf16 would write) between LDS and the matrix pipe; no pass over HBM */

#define MMDTI_CT_REGRESS 0
#define MMDTI_CT_SINGLE 1
#define MMDTI_CT_MULTI 2

const char* mmdti_last_error(void);
int mmdti_abi_version(void);
/* The kernel tables the launch plans index (mmdti_attn_plan, mmdti_gbf_plan, mmdti_pair_attn_plan, mmdti_row_plan, mmdti_stream_plan): every instance a family can launch has one row, and a
 * plan names a kernel by its row.  size_out receives the number of rows; the name of row `index` is the kernel's template-id as the
 * source spells it ("attn_fwd_kernel<16, 10>"), null for an unknown family or a row past the end.  No GPU needed. */
#define MMDTI_PLAN_ATTN 0
#define MMDTI_PLAN_GBF 1
#define MMDTI_PLAN_PAIR_ATTN_FWD 2       /* pair_attn_fwd_mfma_kernel */
#define MMDTI_PLAN_PAIR_ATTN_BWD 3       /* pair_attn_bwd_mfma_kernel */
#define MMDTI_PLAN_PAIR_ATTN_FWD_ELEM 4  /* pair_attn_fwd_kernel: the per-element form (N > 272, or unaligned rows / planes) */
#define MMDTI_PLAN_PAIR_ATTN_BWD_ELEM 5  /* pair_attn_bwd_kernel */
#define MMDTI_PLAN_ROW 6                 /* LayerNorm and row softmax (mmdti_row_plan): 26 rows */
#define MMDTI_PLAN_STREAM 7              /* casts, dropout, axpy, GELU, column sum, sum of squares, Adam, EMA, step state (mmdti_stream_plan): 29 rows */
#define MMDTI_PLAN_MAPS 8                /* attention maps (mmdti_maps_plan): 12 rows -- attn_map_kernel<16 | 32 | 64>, the pair map by plane layout and tile bucket */
#define MMDTI_PLAN_LORA 9                /* LoRA adapters (mmdti_lora_plan): 27 rows -- lora_fwd_kernel<R, F16, YF16>, lora_bwd_kernel<R, XF16, SLAB>, lora_dx_kernel<R, DXBF16> */
int mmdti_plan_table_size(int family, int* size_out);
const char* mmdti_plan_kernel_name(int family, int index);
/* Run-time tuning switches (A/B measurements inside one process; defaults come from the environment variable of the same
 * upper-cased name, e.g. MMDTI_GEMM_BIG).  Known names: "gemm_big" (0 off, 1 where the shape fills the chip, 2 every
 * eligible shape); "gemm_dbg" (measurement only: 1 = the large-tile GEMM skips its epilogue); "gemm_small" (1: 64 x 64 tiles for launches of
 * few tiles -- small batches; 0: 128 x 128 everywhere) and "gemm_deep" (1: four-stage LDS-DMA ring for launches of at most one
 * workgroup per CU); all paths give bit-identical results.  The switches that are otherwise read from the environment once, at the first
 * call of their entry point, can be written too: "gemm_glds" (MMDTI_GEMM_GLDS), "gemm_tall" (MMDTI_GEMM_TALL), "gemm_small_tiles"
 * (MMDTI_GEMM_SMALL_TILES), "gemm_stream_mb" (MMDTI_GEMM_STREAM_MB), "gemm_ln_rows" (MMDTI_GEMM_LN_ROWS) and "grouped_small_rows"
 * (MMDTI_GROUPED_SMALL_ROWS).  Returns MMDTI_ERR_INVALID for an unknown name.  Not part of any reference interface. */
int mmdti_set_option(const char* name, int value);

/* ---- Deterministic mode: bit-identical parameter gradients run to run (DESIGN.md "Deterministic mode") ----
 * Off by default; with it off no launch changes.  mmdti_set_deterministic(1) sets a process-wide flag.  While it is on, every launcher whose
 * default form lets workgroups (or K splits) meet in fp32 atomics -- mmdti_layernorm_bwd, mmdti_colsum_bf16, the bias gradients and the
 * split-K output of mmdti_gemm_bf16 / mmdti_linear_dw_grouped, mmdti_gbf_features_bwd -- stores per-workgroup partials into the workspace registered for ITS
 * launch stream and folds them in a fixed order with a kernel queued directly behind on the same stream.  A launch whose stream has no
 * workspace, or too small a one, returns MMDTI_ERR_INVALID before anything is launched (mmdti_last_error names the site): the mode never
 * falls back to atomics.  (A split-K GEMM lowers its split count until its slabs fit instead; one split is always deterministic.)  Sites
 * that have no fixed-order form refuse in the mode the same way: mmdti_gbf_bias_bwd (the fused per-pair half of the round-1 pair-bias
 * chain), mmdti_gbf_bias_bwd_full without its workspace, mmdti_sumsq_f32 without ws and mmdti_ct_loss_fwd without row_ws.
 * mmdti_gbf_bias_bwd_full (its waves then meet in wave / pair order in LDS), the general mmdti_pair_attn_bwd kernel (waves add in
 * wave order) and mmdti_embedding_bwd (one adder per table element, in token order) take fixed-order forms that need no workspace.
 * mmdti_det_workspace registers `ws` (16-byte aligned device memory, `bytes` long, owned by the caller and kept alive while registered)
 * for `stream`; ws == NULL forgets the stream.  The table is mutex-guarded and read on the host only.
 * mmdti_det_workspace_bytes: what ONE launch of `site` needs -- MMDTI_DET_LAYERNORM_BWD (rows, cols = D), MMDTI_DET_COLSUM (rows, cols),
 * MMDTI_DET_GEMM_SLAB (rows, cols = the output's M, N: one split's slab; a launch wants one per K split), MMDTI_DET_GBF_FEATURES_BWD
 * (rows = pairs P, cols = 2 E + 2 K).  Not part of any reference interface. */
#define MMDTI_DET_LAYERNORM_BWD 1
#define MMDTI_DET_COLSUM 2
#define MMDTI_DET_GEMM_SLAB 3
#define MMDTI_DET_GBF_FEATURES_BWD 4
int mmdti_set_deterministic(int on);
int mmdti_det_workspace(mmdti_stream_t stream, void* ws, long long bytes);
int mmdti_det_workspace_bytes(int site, long long rows, long long cols, long long* bytes_out);

/* ---- GEMM: C = epi(alpha * A.B^T) ----------------------------------------------------------
 * Replaces nn.Linear / torch.bmm fwd+bwd: unicore in_proj/out_proj/fc1/fc2 (models/transformers.py:137-139),
 * gbf_proj (models/mm_model.py:554), RobertaModel linears (mm_model.py:562), InfoNCE projections
 * (models/infonce.py:28-29), BertCrossEncoder linears (models/mm_module.py:486-488,527,545,581).
 * A: transA=0 -> [M,K] row-major (lda), transA=1 -> stored [K,M].  B: transB=0 -> [N,K] ("weight" layout),
 * transB=1 -> stored [K,N].  lda/ldb multiples of 8, 16-byte aligned bases.  If K%8 != 0 the k-contiguous
 * operand must hold zeros in its padded tail.  Batch index z = outer*batch_inner + inner.
 * colsum_out (nullable, [N] fp32, +=): column sums of the stored C -- the bias gradient of the Linear whose output
 * gradient C is -- accumulated by the epilogue (aligned, unbatched, unsplit outputs only).
 * arowsum_out (nullable, [M] fp32, +=, transA only, unbatched): sum over k of op(A)[m][k].  For a weight gradient
 * dW = dy^T.x (A = dy stored [tokens, out]) that is the Linear's bias gradient, taken inside the same pass over dy.
 * workspace (nullable, workspace_bytes): device scratch for split-K.  With it, a split-K product of a large-tile shape
 * writes one fp32 partial per split with plain stores and a second pass adds their sum into C -- global float atomics
 * run at a fifth of the store rate on this chip -- instead of atomicAdd-ing every partial into C.  Without it (or when
 * it is too small: splits * M * N * 4 bytes) the atomic form runs.  Contents on return are unspecified. */
int mmdti_gemm_bf16(mmdti_stream_t stream, const void* A, const void* B, void* C, int M, int N, int K, int lda,
                    int ldb, int ldc, int transA, int transB, int batch_outer, int batch_inner, long long sAo,
                    long long sAi, long long sBo, long long sBi, long long sCo, long long sCi, int splitk,
                    float alpha, float beta, const float* bias, const float* residual, int ldr, int act,
                    const void* aux_in, void* aux_out, int ld_aux, int c_dtype, float drop_p,
                    unsigned long long seed, unsigned int site, float* colsum_out, float* arowsum_out, void* workspace,
                    long long workspace_bytes);

/* What mmdti_gemm_bf16 would launch for the same arguments, without launching: the same validation and the same plan
 * (csrc/gemm_plan.h), pointers tested for null and alignment only -- it runs on a machine without a GPU.  plan_out receives 15 ints:
 * family (0 register-staged 128 x 128, 1 LDS-DMA single-buffered, 2 double-buffered, 3 four-stage "deep", 4 tall, 5 small 64 x 64,
 * 6 big 256 x 256), the instance's template key TA, TB, FAST, F16, BCVT (0 where the family has no such parameter), grid x,
 * grid z, workgroup size, dynamic LDS bytes, effective K split, rows per tile of the tall kernel (else 0), slabs (1: partials go
 * through the workspace and a second pass adds them into C), streaming stores for C, and who computes arowsum (0 nobody, 1 the
 * kernel, 2 a separate column-sum pass over A). */
int mmdti_gemm_plan(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, int transA, int transB,
                    int batch_outer, int batch_inner, long long sAo, long long sAi, long long sBo, long long sBi, long long sCo,
                    long long sCi, int splitk, float alpha, float beta, const float* bias, const float* residual, int ldr, int act,
                    const void* aux_in, void* aux_out, int ld_aux, int c_dtype, float drop_p, unsigned long long seed,
                    unsigned int site, float* colsum_out, float* arowsum_out, void* workspace, long long workspace_bytes,
                    int* plan_out);

/* ---- Linear + residual + LayerNorm in one kernel ------------------------------------------------
 * The Linear that closes a residual branch and the LayerNorm that follows it: unicore out_proj -> final_layer_norm and fc2 -> the
 * next layer's self_attn_layer_norm / the encoder's final_layer_norm (pre-LN, models/transformers.py:137-139,160-161); HF / BertCross
 * attention.output.dense -> LayerNorm and output.dense -> LayerNorm (post-LN, mm_model.py:562, mm_module.py:523-534,561-587):
 *   x_out[M,N] (fp32) = residual + dropout(A.W^T + bias);   h = (x - mean) * rstd * gamma + beta  -> ln_f32 and / or ln_bf16
 * (either may be null); mean, rstd: [M] fp32 (row mean and 1/sqrt(biased var + eps), what mmdti_layernorm_bwd takes).
 * A: [M,K] bf16 (lda), W: [N,K] bf16 (ldb); N == 512 (a workgroup owns whole rows), K % 64 == 0.  Dropout counters are those of
 * mmdti_gemm_bf16's epilogue (element row*N + col), so the fused and the unfused path draw the same mask. */
int mmdti_gemm_ln_bf16(mmdti_stream_t stream, const void* A_bf16, const void* W_bf16, const float* bias, const float* residual, int M,
                       int N, int K, int lda, int ldb, int ldr, float drop_p, unsigned long long seed, unsigned int site, float* x_out,
                       const float* gamma, const float* beta, float eps, float* ln_f32, void* ln_bf16, float* mean, float* rstd,
                       int f16 /* bit 0: A and W hold fp16; bit 1: ln_bf16 receives fp16 */);
/* rows per tile (64 or 80) mmdti_gemm_ln_bf16 uses for M rows: its grid is ceil(M / rows) workgroups of 512 threads */
int mmdti_gemm_ln_rows(int M);

/* ---- Grouped weight gradients of one transformer layer -----------------------------------------
 * The weight half of nn.Linear's backward for up to 8 Linears that saw the SAME token rows (unicore in_proj / out_proj /
 * fc1 / fc2 of one encoder layer, models/transformers.py:137-139; query|key|value / dense / intermediate / output of one
 * RoBERTa or BertCrossAttention layer, mm_model.py:562, mm_module.py:470-587):
 *   dw[i] [n_out[i], lddw[i]] fp32 += dy[i]^T . x[i],   db[i] [n_out[i]] fp32 += column sums of dy[i]   (db or db[i] may be null)
 * dy[i]: [rows, ldy[i]] bf16, x[i]: [rows, ldx[i]] bf16; n_out, n_in multiples of 256; rows a multiple of 64.
 * One launch over all output tiles with a K split chosen to fill the chip; partial sums go through `workspace`
 * (mmdti_linear_dw_grouped_splits(total 256x256 tiles, rows) * sum_i n_out[i]*n_in[i] * 4 bytes) and a second pass adds
 * them into dw.  The argument tables are HOST arrays of nprob entries. */
int mmdti_linear_dw_grouped(mmdti_stream_t stream, int nprob, const void* const* dy_bf16, const void* const* x_bf16,
                            float* const* dw, float* const* db, const int* n_out, const int* n_in, const int* ldy,
                            const int* ldx, const int* lddw, int rows, void* workspace, long long workspace_bytes,
                            int x_f16 /* 1: every x[i] holds fp16 (saved forward activations of the fp16 forward-operand mode),
                                         converted to bf16 between LDS and the matrix pipe -- see MMDTI_DT_B_F16 */);
int mmdti_linear_dw_grouped_splits(int tiles, int rows);
/* What mmdti_linear_dw_grouped would launch for these problems, without launching.  plan_out receives 9 ints: small (1: the 64 x 64
 * kernel without a K split, plain +=; 0: the 256 x 256 kernel), grid x, grid z, workgroup size, dynamic LDS bytes, K splits, K-tail
 * instance (rows % 64 != 0), atomic (1: the splits add into dw with fp32 atomics, no second pass), BCVT
 * (the fp16-x instance: x_f16 != 0); *workspace_bytes_out: the workspace
 * the launch demands (0 for the small form). */
int mmdti_linear_dw_grouped_plan(int nprob, const int* n_out, const int* n_in, int rows, int x_f16, int* plan_out,
                                 long long* workspace_bytes_out);

/* ---- Sequenced layers: a whole layer's launches, or a whole tower's, behind ONE call (launch sequencing in the library: at 16-32
 * molecules the Python side of ~500 launches per step sets the pace).  The SAME kernels, arguments and order as the op-by-op host
 * path: bit-identical results.  What a call takes is grouped by role into the structs below -- a run block (the same for every layer
 * of one call), one parameter block per layer, one saved-tensor block per layer -- so that a host names every pointer it hands over.
 * Only pointers, int / unsigned int / float / (unsigned) long long and mmdti_stream_t fields, widest first: a binding reproduces the
 * layout from the field list alone.  A field a call does not use may stay null; every call refuses a null it needs before its
 * first launch.  Shapes and the workspace layouts: layers.hip. */

/* Tower 1 (Uni-Mol encoder; unicore TransformerEncoderLayer as driven by models/transformers.py:136-139). */
typedef struct {
  const int *key_tiles, *row_off;      /* ragged batches / packed rows, as mmdti_pair_attn_fwd (nullable) */
  unsigned long long seed;
  int M, B, N, H, D, F, ld;            /* M token rows; pair planes [B,H,N,ld] */
  int pair_layout;                     /* as mmdti_pair_attn_fwd (forward) / mmdti_pair_attn_bwd (backward) */
  int act_fwd, act_dx;                 /* MMDTI_ACT_* of fc1's epilogue (forward) and of fc2's input gradient (backward) */
  int ln_max_k;                        /* deepest Linear + LayerNorm that runs as one kernel (0: never) */
  int fwd_f16;                         /* 1: the fp16 forward-operand mode -- every 16-bit operand of a forward GEMM (h1, weights, q | k | v,
                                          o, h2, a, a 16-bit ln_out) holds fp16; pair_layout 3 only.  The saved gelu' (u) stays bf16 */
  float scale, p_res, p_att;
} mmdti_unimol_run_t;

typedef struct {
  const void *w_in, *w_out, *w_fc1, *w_fc2;          /* forward: the 16-bit shadows (bf16, or fp16 under fwd_f16) */
  const float *b_in, *b_out, *b_fc1, *b_fc2;         /* (nullable) */
  const void *wb_in, *wb_out, *wb_fc1, *wb_fc2;      /* backward: the bf16 shadows */
  const float *g_ln1, *bt_ln1, *g_ln2, *bt_ln2;      /* self_attn_layer_norm, final_layer_norm */
  float *dw_in, *dw_out, *dw_fc1, *dw_fc2;           /* gradients: fp32, accumulated.  A forward-only caller leaves them null */
  float *db_in, *db_out, *db_fc1, *db_fc2;
  float *dg_ln1, *dbt_ln1, *dg_ln2, *dbt_ln2;
  float eps_ln1, eps_ln2;
} mmdti_unimol_layer_t;

/* What the forward of one layer writes for its backward, behind the layer's inputs (which the backward reads again): x [M,D] fp32 the
 * residual stream, h1 [M,D] its LayerNorm-1 output with m1 / r1 [M] (backward only).  qkv [M,3D], s (pair logits, layout as the input
 * logits), o [M,D], x1 [M,D] f32, h2 [M,D], m2 / r2 [M], u (gelu' or pre-activation, as act_fwd says) / a [M,F]. */
typedef struct {
  const float* x;
  const void* h1;
  const float *m1, *r1;
  void *qkv, *s, *o;
  float* x1;
  void* h2;
  float *m2, *r2;
  void *u, *a;
} mmdti_unimol_saved_t;

/* One layer.  Forward: in_proj, pair attention (s_in -> saved s), out_proj + residual + dropout + LayerNorm-2, fc1 + GELU, fc2 + residual +
 * dropout -> x_out [M,D] fp32 and the LayerNorm that reads it (next_mode 1: the next layer's LayerNorm-1 -> 16-bit ln_out; 2: the
 * encoder's final LayerNorm -> fp32 ln_out; 0: none) with its statistics mn / rn.
 * Backward, eight launches: fc2 / fc1 input gradients, LayerNorm-2 backward, out_proj input gradient, pair-attention backward (G: the
 * pair-gradient chain; g_in_zero: not yet written), in_proj input gradient, LayerNorm-1 backward, grouped weight gradients.  dx_in
 * [M,D] fp32 / dy2 [M,D] bf16: the gradient of x_out and its dropout-backward copy; dx_out / dx16_out (nullable: the lowest layer):
 * the same two for the layer below, whose fc2 bias gradient db_below (nullable) receives the column sums of dx16_out.
 * ws: mmdti_unimol_stack_layout's out[2] bytes, 16-byte aligned. */
int mmdti_unimol_layer_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                           const mmdti_unimol_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                           const void* s_in, const unsigned char* key_pad, int rag_store, int next_mode, const float* g_next,
                           const float* bt_next, float eps_next, float* x_out, void* ln_out, float* mn, float* rn);
int mmdti_unimol_layer_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layer,
                           const mmdti_unimol_saved_t* saved, unsigned int site_f_below, unsigned int site_o, unsigned int site_att,
                           const float* dx_in, const void* dy2, float* dx_out, void* dx16_out, float* db_below, void* G,
                           int g_in_zero, void* ws, long long ws_bytes);

/* ALL nl layers of the encoder (the loop of models/transformers.py:136-139 in :96-183): nl x the calls above, the saved blocks being
 * slices of ONE caller-owned arena.  mmdti_unimol_stack_layout (launch-free): out[0] = arena bytes per layer, out[1] = bytes of the stack
 * backward's workspace, out[2] = bytes of ONE layer's backward workspace (s_bytes: one layer's pair logits; dw_slab_bytes: split-K
 * slabs of one layer's grouped weight gradients, see mmdti_linear_dw_grouped_splits).
 *   x0 / h1_0 / m1_0 / r1_0: the stream entering layer 0 and its LayerNorm-1 output + statistics (the caller's); the last layer writes
 *   x_last, s_last and (g_final non-null) the final LayerNorm out_final / mean_final / rstd_final.  Dropout sites: site0 + 3 l + {0, 1, 2}.
 *   dw_stream + events (hipEvent_t [3]; both null: everything on `stream`): the grouped weight gradients of a layer run on dw_stream
 *   under the layer below; `stream` has joined dw_stream when mmdti_unimol_stack_bwd returns. */
int mmdti_unimol_stack_layout(int M, int D, int F, long long s_bytes, long long dw_slab_bytes, long long* out);
int mmdti_unimol_stack_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers, int nl,
                           unsigned int site0, const float* x0, const void* h1_0, const void* s_in, const unsigned char* key_pad,
                           int rag_store_last, const float* g_final, const float* bt_final, float eps_final, void* arena,
                           long long arena_bytes, long long s_bytes, float* x_last, void* s_last, float* out_final,
                           float* mean_final, float* rstd_final);
int mmdti_unimol_stack_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run, const mmdti_unimol_layer_t* layers, int nl,
                           unsigned int site0, const float* dx_in, const void* dy2_in, float* dx_final, const float* x0,
                           const void* h1_0, const float* m1_0, const float* r1_0, const void* s_last, void* G, int g_first_zero,
                           const void* arena, long long arena_bytes, long long s_bytes, void* ws, long long ws_bytes,
                           long long dw_slab_bytes, mmdti_stream_t dw_stream, void* const* events);

/* Tower 2 and the cross block: one post-LN BERT layer on the fused attention kernels (HF RobertaLayer reached from
 * models/mm_model.py:562; BertCrossAttentionLayer, mm_module.py:615-626 through :663-677).  Self-attention: Mk = Mq, Lk = Lq. */
typedef struct {
  const float* key_add;                        /* [B,Lk] additive key mask (nullable) */
  const int *q_off, *k_off, *k_cnt;            /* packed sequences, as mmdti_attn_fwd (null / q_rows 0: dense) */
  unsigned long long seed;
  int Mq, Mk, B, Lq, Lk, heads, D, F;          /* token rows of the query / key side; the longest sequences */
  int q_rows;
  int act_fwd, act_dx, ln_max_k;               /* as mmdti_unimol_run_t */
  int fwd_f16;                                 /* 1: s1_16 / s2_16, the weights, ctx, a16, i, out16 hold fp16 (q | k | v and u stay bf16) */
  float scale, p_hid, p_att, eps;
} mmdti_bert_run_t;

/* w_qkv [3D,D] / b_qkv [3D]: the fused query | key | value projection; in the cross layer the fused key | value one ([2D,D]) beside the
 * separate query projection w_q / b_q.  The cross backward leaves the weight gradients to its caller: only db_o, db_o2 and the
 * LayerNorm gradients are read there. */
typedef struct {
  const void *w_qkv, *w_q, *w_o, *w_i, *w_o2;
  const float *b_qkv, *b_q, *b_o, *b_i, *b_o2;
  const void *wb_qkv, *wb_q, *wb_o, *wb_i, *wb_o2;
  const float *g_ln1, *bt_ln1, *g_ln2, *bt_ln2;      /* attention.output.LayerNorm, output.LayerNorm */
  float *dw_qkv, *dw_q, *dw_o, *dw_i, *dw_o2;        /* gradients: fp32, accumulated.  A forward-only caller leaves them null */
  float *db_qkv, *db_q, *db_o, *db_i, *db_o2;
  float *dg_ln1, *dbt_ln1, *dg_ln2, *dbt_ln2;
  int lddw_qkv;                                      /* row stride of dw_qkv */
} mmdti_bert_layer_t;

/* s1_32 / s1_16 [Mq,D]: the layer input (fp32 residual stream and its 16-bit copy); s2_16 [Mk,D]: the key / value side (cross only).
 * qkv [Mq,3D] (cross: k | v [Mk,2D] beside q [Mq,D]), ctx [Mq,D], stats, y [Mq,D] f32 (pre-LN1), a32 / a16 (LN1 output), am / ar,
 * u / i [Mq,F] (gelu' / the intermediate activation), z [Mq,D] f32 (pre-LN2), zm / zr. */
typedef struct {
  const float* s1_32;
  const void *s1_16, *s2_16;
  void *qkv, *q, *ctx;
  float *stats, *y, *a32;
  void* a16;
  float *am, *ar;
  void *u, *i;
  float *z, *zm, *zr;
} mmdti_bert_saved_t;

/* Forward: the projection(s), fused attention, output.dense + residual + LayerNorm, intermediate + GELU,
 * output + residual + LayerNorm -> out32 / out16 [Mq,D].  Backward of the self-attention layer: LayerNorm-2 backward, the FFN's two
 * input gradients, LayerNorm-1 backward, the output projection's input gradient, the fused attention backward, the fused projection's
 * input gradient accumulated into ds1, the four weight gradients as one grouped launch.  dout [Mq,D] fp32 -> ds1 [Mq,D] fp32.
 * ws: mmdti_bert_stack_layout's out[2] bytes.
 * The cross backward stops before the weight gradients (ten launches): its five bf16 activation gradients (dzb [Mq,D], du [Mq,F], dyb
 * [Mq,D], dq [Mq,D], dkv [Mk,2D]) are the caller's -- the A operands of the weight gradients it launches itself (mmdti_linear_dw_grouped
 * takes one token-row count per launch, this layer has two).  ds2 [Mk,D] may be null (s2 needs no gradient): its GEMM is then not
 * launched; dkv is still written.  ws: out[3] bytes. */
int mmdti_bert_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                         const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                         float* out32, void* out16);
int mmdti_bert_cross_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                               const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                               float* out32, void* out16);
int mmdti_bert_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                         const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                         const float* dout, float* ds1, void* ws, long long ws_bytes);
int mmdti_bert_cross_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layer,
                               const mmdti_bert_saved_t* saved, unsigned int site_att, unsigned int site_o, unsigned int site_f,
                               const float* dout, float* ds1, float* ds2, void* dzb, void* du, void* dyb, void* dq, void* dkv,
                               void* ws, long long ws_bytes);

/* ALL nl layers of tower 2 (HF RobertaEncoder's layer loop): as the Uni-Mol stack above.  mmdti_bert_stack_layout (launch-free): out[0] =
 * arena bytes per layer, out[1] = the stack backward's workspace bytes, out[2] / out[3] = ONE self-attention / cross layer's backward
 * workspace bytes (stats_bytes: one layer's softmax statistics; nrow: heads * q_rows packed, B * heads * Lq dense; dw_slab_bytes:
 * split-K slabs of one layer's weight gradients -- the cross layer has none).  s1_32_0 / s1_16_0: the embeddings' LayerNorm output; the
 * last layer's fp32 output goes to out32_last.  Dropout sites: site0 + 3 l + {0: attention, 1: output.dense, 2: FFN}. */
int mmdti_bert_stack_layout(int Mq, int D, int F, long long stats_bytes, long long nrow, long long dw_slab_bytes, long long* out);
int mmdti_bert_stack_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, int nl,
                         unsigned int site0, const float* s1_32_0, const void* s1_16_0, void* arena, long long arena_bytes,
                         long long stats_bytes, float* out32_last);
int mmdti_bert_stack_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run, const mmdti_bert_layer_t* layers, int nl,
                         unsigned int site0, const float* dout, float* ds1_final, const void* s1_16_0, const void* arena,
                         long long arena_bytes, long long stats_bytes, void* ws, long long ws_bytes, long long dw_slab_bytes);

/* ---- Sequenced layers that carry LoRA adapters next to a FROZEN base (csrc/layers.hip; DESIGN.md "LoRA adapters").  What the
 * op-by-op host path launches for such a layer -- the same kernels, arguments and order, bit-identical results -- behind one call per
 * layer or per tower: the sequences above with mmdti_lora_fwd / _bwd / _dx in them and without the weight gradients, which a frozen
 * base has none of.  The gradient fields of the layer blocks (dw_*, db_*, dg_*, dbt_*) may all be null here.  The calls allocate
 * nothing: the saved t = bf16(x.A^T) of every adapter and the backward's u = bf16(s.dy.B) are the caller's, as rows of
 * MMDTI_LORA_ROW_BYTES(rows) bytes (room for the widest rank, rounded up to 256 bytes).  Not part of any reference interface.
 * Purely additive: MMDTI_ABI_VERSION does not move. */

/* One adapter: A [r, in], B [out, r] (mmdti_lora_fwd).  A null block, or r == 0, means "this projection carries no adapter"; any
 * other rank than 8, 16 or 32 is refused before a launch.  (The two blocks of this section follow the field rules of the sequencers'
 * blocks above.  They carry a struct tag so that the six blocks above stay what an untagged scan of this header finds -- callers
 * that enumerate the sequencers' blocks, such as the layout check of tests/test_layer_structs_cpu.py, go on seeing exactly those; a
 * binding gets all eight with _abi.parse_structs(tagged=True), which is what mmdti_hip loads.) */
typedef struct mmdti_lora_adapter {
  const void *A, *B;               /* forward: the 16-bit shadows (bf16, or fp16 under fwd_f16) */
  const void *A_bf16, *B_bf16;     /* backward: the bf16 shadows */
  float *dA, *dB;                  /* gradients: fp32, accumulated.  A forward-only caller leaves them null */
  int r;
  float scale;                     /* alpha / r */
} mmdti_lora_adapter_t;

/* The separate query, key and value projections of a BERT-style layer whose base is frozen (a frozen base has no fused [3D, D] view:
 * w_qkv / w_q of its mmdti_bert_layer_t stay null). */
typedef struct mmdti_bert_split {
  const void *w_q, *w_k, *w_v;     /* forward: the 16-bit shadows, each [D, D] */
  const float *b_q, *b_k, *b_v;    /* (nullable) */
  const void *wb_q, *wb_k, *wb_v;  /* backward: the bf16 shadows */
} mmdti_bert_split_t;

#define MMDTI_LORA_MAX_RANK 32
#define MMDTI_LORA_ROW_BYTES(rows) (((long long)(rows) * MMDTI_LORA_MAX_RANK * 2 + 255) / 256 * 256)

/* Tower 1, one layer.  Forward: mmdti_unimol_layer_fwd's sequence with mmdti_lora_fwd on q | k | v right behind the in_proj GEMM (one
 * adapter on the fused [3D, D] projection; lora null or r 0: none); t [M, r] bf16 is written for the backward.
 * Backward: mmdti_unimol_layer_bwd's sequence without the grouped weight gradients, mmdti_lora_bwd on dqkv behind the pair-attention
 * backward and mmdti_lora_dx on the bf16 dh1 behind the in_proj input gradient.  dx_out null: the lowest layer that runs -- the in_proj
 * input gradient, the adapter's dx and the LayerNorm-1 backward are skipped (mmdti_lora_bwd still runs).
 * ws: mmdti_unimol_lora_stack_layout's out[2] bytes, 16-byte aligned. */
int mmdti_unimol_lora_layer_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run_block, const mmdti_unimol_layer_t* layer,
                                const mmdti_unimol_saved_t* saved, const mmdti_lora_adapter_t* lora, void* t, unsigned int site_att,
                                unsigned int site_o, unsigned int site_f, const void* s_in, const unsigned char* key_pad, int rag_store,
                                int next_mode, const float* g_next, const float* bt_next, float eps_next, float* x_out, void* ln_out,
                                float* mn, float* rn);
int mmdti_unimol_lora_layer_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run_block, const mmdti_unimol_layer_t* layer,
                                const mmdti_unimol_saved_t* saved, const mmdti_lora_adapter_t* lora, const void* t,
                                unsigned int site_f_below, unsigned int site_o, unsigned int site_att, const float* dx_in, const void* dy2,
                                float* dx_out, void* dx16_out, float* db_below, void* G, int g_in_zero, void* ws, long long ws_bytes);

/* ALL nl layers of tower 1: nl x the calls above, as mmdti_unimol_stack_fwd / _bwd.  lora: nl adapter blocks, one per layer (r 0: that
 * layer has none).  mmdti_unimol_lora_stack_layout (launch-free): out[0] = arena bytes per layer (mmdti_unimol_stack_layout's slice
 * and the layer's t row behind it), out[1] = the stack backward's workspace bytes (mmdti_unimol_stack_layout's without slabs, and a u
 * row behind each of its two layer workspaces), out[2] = ONE layer's backward workspace bytes (its temporaries rounded up to 256, and one u row).  dx_final null: nothing under
 * layer 0 reads its input gradient (see dx_out above). */
int mmdti_unimol_lora_stack_layout(int M, int D, int F, long long s_bytes, long long* out);
int mmdti_unimol_lora_stack_fwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run_block, const mmdti_unimol_layer_t* layers,
                                const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* x0, const void* h1_0,
                                const void* s_in, const unsigned char* key_pad, int rag_store_last, const float* g_final,
                                const float* bt_final, float eps_final, void* arena, long long arena_bytes, long long s_bytes,
                                float* x_last, void* s_last, float* out_final, float* mean_final, float* rstd_final);
int mmdti_unimol_lora_stack_bwd(mmdti_stream_t stream, const mmdti_unimol_run_t* run_block, const mmdti_unimol_layer_t* layers,
                                const mmdti_lora_adapter_t* lora, int nl, unsigned int site0, const float* dx_in, const void* dy2_in,
                                float* dx_final, const float* x0, const void* h1_0, const float* m1_0, const float* r1_0,
                                const void* s_last, void* G, int g_first_zero, const void* arena, long long arena_bytes,
                                long long s_bytes, void* ws, long long ws_bytes);

/* Tower 2's self-attention layer and the cross layer.  lora: three adapter blocks -- query, key, value -- of which any subset has r 0
 * (lora null: none is adapted).  saved->qkv holds q [Mq, D], k [Mk, D] and v [Mk, D] as three planes back to back (saved->q is not
 * read); t: three rows of MMDTI_LORA_ROW_BYTES(max(Mq, Mk)) bytes -- query, key, value -- each [rows, r] bf16.
 * Forward: the three projection GEMMs, mmdti_lora_fwd of every adapted one (query, key, value order), then the fused attention and the
 * rest of mmdti_bert_layer_fwd.
 * Backward: the six launches the two backwards above share, mmdti_lora_bwd of every adapted projection, then the input gradients:
 * ds1 += dq . W_q, the query adapter's dx; self-attention: ds1 += dk . W_k, ds1 += dv . W_v, the key and the value adapter's dx; cross:
 * ds2 = dk . W_k, ds2 += dv . W_v, the two dx into ds2.  want_ds1 / want_ds2 0: that gradient's products are not launched (ds1 is still
 * written by the LayerNorm-1 backward and must be there; ds2 may then be null).  ws: mmdti_bert_lora_stack_layout's out[2] (cross: out[3]). */
int mmdti_bert_lora_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layer,
                              const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved, void* t,
                              unsigned int site_att, unsigned int site_o, unsigned int site_f, float* out32, void* out16);
int mmdti_bert_lora_cross_layer_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layer,
                                    const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                                    void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, float* out32, void* out16);
int mmdti_bert_lora_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layer,
                              const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                              const void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout, float* ds1,
                              int want_ds1, void* ws, long long ws_bytes);
int mmdti_bert_lora_cross_layer_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layer,
                                    const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, const mmdti_bert_saved_t* saved,
                                    const void* t, unsigned int site_att, unsigned int site_o, unsigned int site_f, const float* dout,
                                    float* ds1, int want_ds1, float* ds2, int want_ds2, void* ws, long long ws_bytes);

/* ALL nl layers of tower 2: nl x mmdti_bert_lora_layer_fwd / _bwd, as mmdti_bert_stack_fwd / _bwd (the cross block has no stack).
 * split: nl blocks; lora: 3 nl adapter blocks (layer l: 3 l + {0: query, 1: key, 2: value}).  mmdti_bert_lora_stack_layout
 * (launch-free): out[0] = arena bytes per layer (mmdti_bert_stack_layout's slice and three t rows of Mq), out[1] = the stack backward's
 * workspace bytes (mmdti_bert_stack_layout's without slabs, and three u rows), out[2] / out[3] = ONE self-attention / cross layer's
 * backward workspace bytes (the temporaries rounded up to 256 -- the cross layer's activation gradients, its caller's in
 * mmdti_bert_cross_layer_bwd, are temporaries here -- and three u rows of max(Mq, Mk)), out[4] = bytes of one layer call's t (three rows of max(Mq, Mk)).  Self-attention: Mk = Mq.
 * want_ds1_final 0: nothing reads the gradient of s1_32_0 (ds1_final is still the LayerNorm-1 backward's output buffer). */
int mmdti_bert_lora_stack_layout(int Mq, int Mk, int D, int F, long long stats_bytes, long long nrow, long long* out);
int mmdti_bert_lora_stack_fwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layers,
                              const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, int nl, unsigned int site0,
                              const float* s1_32_0, const void* s1_16_0, void* arena, long long arena_bytes, long long stats_bytes,
                              float* out32_last);
int mmdti_bert_lora_stack_bwd(mmdti_stream_t stream, const mmdti_bert_run_t* run_block, const mmdti_bert_layer_t* layers,
                              const mmdti_bert_split_t* split, const mmdti_lora_adapter_t* lora, int nl, unsigned int site0,
                              const float* dout, float* ds1_final, int want_ds1_final, const void* s1_16_0, const void* arena,
                              long long arena_bytes, long long stats_bytes, void* ws, long long ws_bytes);


/* ---- LayerNorm (unicore LayerNorm eps 1e-5: transformers.py:69,71,114,161; BertLayerNorm eps 1e-12:
 * mm_module.py:320-333; HF nn.LayerNorm) -------------------------------------------------------
 * y = LN(x)*gamma+beta, then optional dropout, then rows with row_zero[r]!=0 forced to 0
 * (transformers.py:115-118).  Writes y_f32 and/or y_bf16 (either may be null). */
int mmdti_layernorm_fwd(mmdti_stream_t stream, const float* x, const float* gamma, const float* beta, float eps,
                        int rows, int D, float* y_f32, void* y_bf16, float* mean, float* rstd,
                        const unsigned char* row_zero, float drop_p, unsigned long long seed, unsigned int site,
                        int y16_f16 /* != 0: y_bf16 receives fp16 (the fp16 forward-operand mode) */);
/* dx = dres + LN'(dy + dy_add) ; dgamma/dbeta atomic accumulate.  dy is fp32 (dy_dtype=MMDTI_DT_F32) or bf16;
 * dy_add (fp32, nullable) is a second upstream gradient of the LN OUTPUT (post-LN residual: a = LN(y) feeds both the FFN
 * and the next residual add); dres (fp32, nullable) is a gradient of the LN INPUT that bypasses the LN (pre-LN residual). */
/* dx_bf16 (nullable): a second copy of dx for the next backward GEMM, with the dropout-backward of site2 (probability
 * drop2_p, same seed) applied and rounded to bf16 -- saves the separate cast pass over dx.  dx_colsum (nullable, [D] fp32,
 * +=): column sums of that bf16 copy = the bias gradient of the Linear whose output gradient it is. */
int mmdti_layernorm_bwd(mmdti_stream_t stream, const void* dy, int dy_dtype, const float* dy_add, const float* x, const float* gamma,
                        const float* mean, const float* rstd, int rows, int D, const float* dres, float* dx,
                        float* dgamma, float* dbeta, const unsigned char* row_zero, float drop_p,
                        unsigned long long seed, unsigned int site, void* dx_bf16, float drop2_p, unsigned int site2,
                        float* dx_colsum);

/* ---- small utilities ------------------------------------------------------------------------ */
/* out[c] += sum_r x[r,c]  (bias gradients of every Linear) */
int mmdti_colsum_bf16(mmdti_stream_t stream, const void* x_bf16, int rows, int cols, int ld, float* out);
/* y = bf16(dropout(x)) elementwise; dropout site indexes elements 0..n-1 */
int mmdti_cast_f32_bf16(mmdti_stream_t stream, const float* x, void* y_bf16, long long n, float drop_p,
                        unsigned long long seed, unsigned int site);
int mmdti_cast_bf16_f32(mmdti_stream_t stream, const void* x_bf16, float* y, long long n);
/* fp16 forward-operand mode: y = fp16(dropout(x)) (as mmdti_cast_f32_bf16), and fp16 -> bf16 (round to nearest even) for the
 * backward GEMMs, which keep bf16 operands (gradients need bf16's range) */
int mmdti_cast_f32_f16(mmdti_stream_t stream, const float* x, void* y_f16, long long n, float drop_p, unsigned long long seed,
                       unsigned int site);
int mmdti_cast_f16_bf16(mmdti_stream_t stream, const void* x_f16, int rows, int cols, int ldx, void* y_bf16);
/* y = dropout(x) in fp32 (F.dropout on fp32 activations: infonce.py:24, mm_model.py:390-391,79,82) */
int mmdti_dropout_f32(mmdti_stream_t stream, const float* x, float* y, long long n, float drop_p,
                      unsigned long long seed, unsigned int site);
/* y += a*x (fp32) */
int mmdti_axpy_f32(mmdti_stream_t stream, const float* x, float* y, long long n, float a);

/* ---- Embedding (nn.Embedding: mm_model.py:552; HF roberta embeddings) ---------------------- */
int mmdti_embedding_fwd(mmdti_stream_t stream, const long long* ids, const float* table, long long n, int D,
                        int vocab, float* out, int accumulate);
/* dtable[ids[i]] += dout[i] (atomic), rows with ids==padding_idx skipped (padding_idx<0: none) */
int mmdti_embedding_bwd(mmdti_stream_t stream, const long long* ids, const float* dout, long long n, int D,
                        int vocab, long long padding_idx, float* dtable);
/* out[i] = table_a[ids_a[i]] + table_b[ids_b[i]] + table_c[ids_c[i]] in one pass (HF RobertaEmbeddings.forward,
 * modeling_roberta.py:75-122: word + position + token-type, summed in that order); ids_c == NULL: row 0 of table_c. */
int mmdti_embedding_fwd3(mmdti_stream_t stream, const long long* ids_a, const float* table_a, int vocab_a, const long long* ids_b,
                         const float* table_b, int vocab_b, const long long* ids_c, const float* table_c, int vocab_c, long long n, int D,
                         float* out);
/* One-hot rows for the embedding backward: out[i, ids[i]] = 1 (bf16), everything else 0; rows with ids == padding_idx or
 * out of range are all-zero.  out is [n, ld] with ld >= vocab, ld % 8 == 0.  dtable = onehot^T . dout is then ONE split-K
 * MFMA GEMM (mmdti_gemm_bf16, both operands k-major) instead of n*D contended atomics on a few hundred table rows. */
int mmdti_onehot_bf16(mmdti_stream_t stream, const long long* ids, long long n, int vocab, int ld, long long padding_idx,
                      void* out_bf16);
/* RoBERTa position ids: cumsum(ids!=pad)*(ids!=pad)+pad, int64, bit-exact (modeling_roberta.py:142-155) */
int mmdti_roberta_position_ids(mmdti_stream_t stream, const long long* ids, int B, int L, long long pad_idx,
                               long long* out);

/* ---- Gaussian pair-distance basis (GaussianLayer.forward, mm_model.py:254-269; gaussian :211-224) */
int mmdti_gbf_features_fwd(mmdti_stream_t stream, const float* dist, const long long* edge_type, const float* mul,
                           const float* bias, const float* means, const float* stds, long long P, int K, int E,
                           void* feat_bf16);
int mmdti_gbf_features_bwd(mmdti_stream_t stream, const float* dist, const long long* edge_type, const float* mul,
                           const float* bias, const float* means, const float* stds, long long P, int K, int E,
                           const void* dfeat_bf16, float* dmul, float* dbias, float* dmeans, float* dstds);
/* gbf -> gbf_proj (Linear+GELU+Linear, NonLinearHead mm_model.py:190-208) -> permute (mm_model.py:553-556) in one kernel:
 * out[b,h,i,j] (fp32, [B,H,N,ld], pad columns j >= N written 0).  w1: [F,K] bf16, w2: [H,F] bf16; built for K=128, F=128,
 * H=64.  feat/u/h (nullable, together): the [B*N*N, 128] bf16 basis / pre-activation / hidden rows for the backward.
 * tiled != 0: out is [B,H,plane] in the blocked-row tile layout the pair-attention kernels stream (see mmdti_pair_attn_fwd, layout 1)
 * and the pad keys N .. N4-1 of every query are written -inf. */
int mmdti_gbf_bias_fwd(mmdti_stream_t stream, const float* dist, const void* edge_type,
                       int edge_bytes /* 8, 4 or 2: int64 as the reference collates (mm_model.py:657-660), or narrowed */, const float* mul,
                       const float* bias, const float* means, const float* stds, const void* w1_bf16, const float* b1,
                       const void* w2_bf16, const float* b2, int B, int N, int ld, int K, int F, int H, int E, void* out,
                       void* feat_bf16, void* u_bf16, void* h_bf16, int flags /* bit 0: tiled pair layout; bit 1: u_bf16 receives
                       gelu'(pre-activation) instead of the pre-activation (then pass the same bit to mmdti_gbf_bias_bwd); bit 2 (with
                       bit 0): the pair tensor of the call is a 16-bit plane -- out is fp16 here (layout 3 of mmdti_pair_attn_fwd,
                       which explains the type); g of the two backward entry points is bf16 (layout 7 of mmdti_pair_attn_bwd).
                       Without bit 2 out and g are fp32 */,
                       const int* tile_prefix /* nullable, tiled layout only: ragged batches.  [B+1] int32 on the device,
                       tile_prefix[b+1] - tile_prefix[b] = 16-pair tiles (4x4 blocks, column block slowest) of molecule b to produce:
                       4*k_b*4*nt for its first k_b key tiles (nt = ceil(N/16); k_b as mmdti_pair_attn_fwd's key_tiles, rounded up to a
                       count its sweeps are built for).  The blocks of the all-padding key tiles behind them are not written: the ragged
                       pair-attention kernels never read them */,
                       const int* row_blocks /* nullable, with tile_prefix: PACKED token rows (mmdti_pair_attn_fwd, row_off).  [B] int32 on the
                       device: molecule b's tiles cover only its first row_blocks[b] 4-row query blocks (up to its representative pad
                       row) -- tile_prefix[b+1] - tile_prefix[b] = 4*k_b * row_blocks[b]; no query row past it is read downstream */);
/* Per-pair half of the backward of mmdti_gbf_bias_fwd, one pass over g = dL/d(out) (same layout flag): writes
 * do_bf16 [B*N*N, 64] = bf16(g re-laid out) and du_bf16 [B*N*N, 128] = bf16((do.W2) * gelu'(u)) -- the A operands of the two
 * weight-gradient GEMMs (dW2 = do^T.h, dW1 = du^T.feat; bias gradients are their column sums) -- and accumulates the
 * Gaussian-layer gradients dmul/dbias [E] and dmeans/dstds [128] (fp32, +=).  E <= 4096. */
int mmdti_gbf_bias_bwd(mmdti_stream_t stream, const void* g, const float* dist, const void* edge_type, int edge_bytes,
                       const float* mul, const float* bias, const float* means, const float* stds, const void* w1_bf16,
                       const void* w2_bf16, const void* u_bf16, int B, int N, int ld, int K, int F, int H, int E, int flags,
                       void* do_bf16, void* du_bf16, float* dmul, float* dbias, float* dmeans, float* dstds);
/* The WHOLE backward of mmdti_gbf_bias_fwd in one persistent kernel (autograd of mm_model.py:553-556 through gbf_proj
 * :190-208 and GaussianLayer :211-236): the forward saves nothing -- each 128-pair block recomputes basis / pre-activation /
 * hidden from dist and edge_type, forms do and du, and accumulates ALL parameter gradients on chip (MFMA, contraction over the
 * pairs staged transposed in LDS), flushing once per workgroup: dw1 [128,128], db1 [128], dw2 [64,128], db2 [64], dmul/dbias [E],
 * dmeans/dstds [128] (fp32, +=).  g: dL/d(out) in the layout of flags bits 0 and 2.  K=128, F=128, H=64, E <= 1536.  An fp32 g
 * enters its products as a bf16 high + a bf16 low part: the rows of g sum to zero and padded query rows repeat one basis vector, so
 * a g rounded to bf16 leaves coherent residues where the exact sums cancel. */
int mmdti_gbf_bias_bwd_full(mmdti_stream_t stream, const void* g, const float* dist, const void* edge_type, int edge_bytes,
                            const float* mul, const float* bias, const float* means, const float* stds, const void* w1_bf16,
                            const float* b1, const void* w2_bf16, int B, int N, int ld, int K, int F, int H, int E, int flags,
                            float* dw1, float* db1, float* dw2, float* db2, float* dmul, float* dbias, float* dmeans, float* dstds,
                            const int* tile_prefix /* nullable, tiled layout only: as in mmdti_gbf_bias_fwd, in this kernel's tile
                            units: tile_prefix[b+1] - tile_prefix[b] = nb * min(nb, 4*k_b) blocks of real pairs, nb = ceil(N/4) */,
                            const int* row_blocks /* nullable, with tile_prefix: packed token rows, as in the forward: the count is then
                            row_blocks[b] * min(nb, 4*k_b) -- the gradient of the query rows past the representative pad row is zero */,
                            void* workspace /* nullable; mmdti_gbf_bias_bwd_full_workspace(E) bytes, 16-byte aligned: every workgroup stores
                            its partial sums to its own slab and a second kernel folds the slabs in a fixed order -- the eight gradients
                            are then bitwise reproducible from run to run; without it the partials meet in fp32 atomics */,
                            long long workspace_bytes);
/* bytes of workspace for mmdti_gbf_bias_bwd_full with E edge types (a value, not a status code) */
int mmdti_gbf_bias_bwd_full_workspace(int E);
/* What a pair-bias entry point would launch, without launching: the same validation, message for message, and the same plan
 * (csrc/gbf_plan.h) -- it runs on a machine without a GPU.  entry: 0 mmdti_gbf_features_fwd, 1 mmdti_gbf_features_bwd, 2
 * mmdti_gbf_bias_fwd, 3 mmdti_gbf_bias_bwd, 4 mmdti_gbf_bias_bwd_full; with `records` non-null, 2 and 4 are the _coords forms.
 * deterministic: the mode the launch would find (mmdti_set_deterministic); the query does not read the process flag.  Pointers are
 * tested for null and alignment only, and stand for groups: `operands` for every operand that needs no 16-byte alignment (null: one of
 * them is null), `aligned` for every operand that does (feat / dfeat; w1, w2, out; u, do, du), `saved` for the forward's three saved
 * intermediates, `records`, `tile_prefix`, `row_blocks`, `workspace` for themselves.  P is read by entries 0 and 1; B, N, ld, F, H, V,
 * pad_idx, edge_bytes and flags by the others.  The stream's reduction workspace, which entry 1 needs in the deterministic mode, is not
 * looked up.  plan_out receives 10 long long: the kernel's row in the MMDTI_PLAN_GBF table (mmdti_plan_kernel_name), grid x, workgroup
 * size, dynamic LDS bytes, the MaxDynamicSharedMemorySize the kernel is raised to before its first launch (0: it never asks for more
 * than 64 KiB), tpm (16-pair tiles per molecule; 0 for entries 0 and 1), ntiles (B * tpm; 16-pair blocks for entries 0 and 1), ltab
 * (forward: per-edge-type tables in LDS), slab (1: partial sums go to per-workgroup slabs and a fixed-order pass adds them; 0: fp32
 * atomics), and the grid of the gbf_slab_reduce_kernel launch that follows entry 4 with slabs (else 0). */
int mmdti_gbf_plan(int entry, int deterministic, const void* operands, const void* aligned, const void* saved, const void* records,
                   const int* tile_prefix, const int* row_blocks, const void* workspace, long long workspace_bytes, long long P, int B,
                   int N, int ld, int K, int F, int H, int E, int V, int pad_idx, int edge_bytes, int flags, long long* plan_out);
/* ---- Pair inputs from coordinates.  The two [B,N,N] planes above are functions of the atoms: the reference builds them per
 * molecule as distance_matrix(coord, coord) and tok_i * len(dictionary) + tok_j (data/conformer.py:204-212), right-pads them with 0.0
 * and the pad index, and mm_model.py:553-556 consumes them.  These entry points take the atoms instead: one 16-byte record per atom,
 * [B,N] { fp32 x, y, z, int32 token }, 16-byte aligned.  THE PAIR RULE (one device function, used by all four): either token equal to
 * pad_idx -> (edge type, distance) = (pad_idx, 0.0f), whatever the slot's coordinates hold; otherwise edge type = tok_i * V + tok_j and
 * distance = |c_i - c_j| in fp32 -- three subtractions, dx * dx, two fused multiply-adds, one correctly rounded square root; i == j
 * gives exactly 0.  Every coords entry point checks, before any launch: records non-null and 16-byte aligned, N * N < 2^30 (the limit of
 * the planes forms), V * V == E with V <= 181, 0 <= pad_idx < V.  Purely additive: MMDTI_ABI_VERSION does not move. */
/* coord [B,N,3] fp32 + tokens [B,N] (token_bytes 8: int64 as the reference collates, or 4) -> records [B,N]
 * (data/conformer.py:204-212, mm_model.py:553-556) */
int mmdti_pair_records_pack(mmdti_stream_t stream, const float* coord, const void* tokens, int token_bytes, int B, int N, void* records);
/* records -> dist [B,N,N] fp32 and edge_type [B,N,N] (edge_bytes 8 or 2), by the pair rule: the planes of data/conformer.py:204-212 as
 * mm_model.py:553-556 reads them.  What a configuration without a fused coords kernel runs on. */
int mmdti_pair_inputs_from_coords(mmdti_stream_t stream, const void* records, int B, int N, int V, int pad_idx, float* dist, void* edge_type,
                                  int edge_bytes);
/* mmdti_gbf_bias_fwd with the pair rule in place of the two plane loads (data/conformer.py:204-212 folded into mm_model.py:553-556):
 * bit-identical to mmdti_pair_inputs_from_coords followed by mmdti_gbf_bias_fwd.  Saves no intermediates (it serves the configurations
 * of mmdti_gbf_bias_bwd_full_coords); flags, tile_prefix and row_blocks as in mmdti_gbf_bias_fwd. */
int mmdti_gbf_bias_fwd_coords(mmdti_stream_t stream, const void* records, int V, int pad_idx, const float* mul, const float* bias,
                              const float* means, const float* stds, const void* w1_bf16, const float* b1, const void* w2_bf16,
                              const float* b2, int B, int N, int ld, int K, int F, int H, int E, void* out, int flags,
                              const int* tile_prefix, const int* row_blocks);
/* mmdti_gbf_bias_bwd_full from the records (data/conformer.py:204-212, mm_model.py:553-556 backward): the same kernel body, the same
 * deterministic form, bit-identical in that mode to the planes form run on mmdti_pair_inputs_from_coords' output. */
int mmdti_gbf_bias_bwd_full_coords(mmdti_stream_t stream, const void* g, const void* records, int V, int pad_idx, const float* mul,
                                   const float* bias, const float* means, const float* stds, const void* w1_bf16, const float* b1,
                                   const void* w2_bf16, int B, int N, int ld, int K, int F, int H, int E, int flags, float* dw1,
                                   float* db1, float* dw2, float* db2, float* dmul, float* dbias, float* dmeans, float* dstds,
                                   const int* tile_prefix, const int* row_blocks, void* workspace, long long workspace_bytes);
/* [B,N,N,H] fp32 -> [B,H,N,ld] fp32 (mm_model.py:555-556 permute(0,3,1,2).contiguous()) and its gradient
 * [B,H,N,ld] fp32 (or, tiled != 0, the blocked-row tile layout of mmdti_gbf_bias_fwd) -> [B,N,N,H] bf16 */
int mmdti_pair_permute_fwd(mmdti_stream_t stream, const float* x, float* out, int B, int N, int H, int ld);
int mmdti_pair_permute_bwd(mmdti_stream_t stream, const float* g, void* out_bf16, int B, int N, int H, int ld, int tiled);

/* ---- Pair-bias attention, head_dim 8 (unicore SelfMultiheadAttention + softmax_dropout with
 * return_attn=True, reached from transformers.py:137-139; key-padding merge :122-135) ------------
 * S = scale*q.k^T + bias_in (+ -inf at padded keys); s_out = S (next layer's bias AND the saved activation);
 * O = dropout(softmax(S)).v.   qkv: [B,N,3*H*8] bf16 (q|k|v).
 * layout (of bias_in / s_out, and of s / g in the backward):
 *   0  row-major planes [B,H,N,ld] fp32;
 *   1  tiled planes [B,H,plane] fp32, N <= 272, "blocked rows": per block of 16 queries the 4-key groups follow each other, each
 *      holding its vr query rows x 4 keys (vr = 16, or N - 16 qb in the last block) --
 *          off(query i, key j) = 16 qb N4 + vr (j - j % 4) + 4 (i % 16) + j % 4,   qb = i / 16, N4 = N rounded up to 4,
 *          plane = N * N4 rounded up to 8 elements
 *      -- so a 16x16 tile of a complete block is 256 contiguous elements in MFMA accumulator order (one contiguous KiB per wave
 *      access) and nothing is stored for queries or 4-key groups past N.  Pad keys N .. N4-1 hold -inf in S, 0 in G;
 *   3  COMPACT tiled planes: same element order, the logits chain as fp16 -- half the bytes of the forward's dominant traffic,
 *      a sixth less in the backward.  The reference carries these logits as fp16 itself when it runs under AMP (autocast makes
 *      attn_weights fp16; tasks/trainer.py:266-282).  Each layer rounds S once (to nearest even, saturating at 65504) and its own
 *      softmax runs on the rounded value, so forward and backward see the same logits.  The gradient chain g stays fp32;
 *   7  (backward only, opt-in) as 3 with g as bf16: another third less traffic, at a cost in gradient fidelity wherever sums
 *      over pairs cancel (measured: DESIGN.md); dense and ragged (key_tiles / row_off) forms like layout 3. */
int mmdti_pair_attn_fwd(mmdti_stream_t stream, const void* qkv_bf16, const void* bias_in, void* s_out,
                        void* o_bf16, const unsigned char* key_pad, int B, int N, int H, int ld, float scale,
                        float drop_p, unsigned long long seed, unsigned int site, int layout,
                        const int* key_tiles /* nullable, layout 3 only: [B] int32, number of 16-key tiles of each molecule that
                        hold a real key (ragged batches, right-padded by mm_model.py:645-682).  The key tiles past it (past the next count the
                        sweeps are built for: every count up to 9 tiles, every 2nd up to 13, every 4th beyond) are all padding:
                        they are not loaded, not computed, and not stored unless rag_store != 0 (then written as -inf: pass it for the
                        last layer, whose S goes back to the caller).  Pad QUERY rows are computed as ever. */,
                        int rag_store,
                        const int* row_off /* nullable, with key_tiles only: PACKED token rows.  [B+1] int32 on the device: molecule b owns
                        rows [row_off[b], row_off[b+1]) of qkv, o_bf16 and key_pad (then indexed by packed row) -- its n_b real tokens
                        followed by at most ONE representative pad row -- instead of rows [b*N, (b+1)*N).  Why one row is enough: the
                        reference zeroes padded rows before the first layer (transformers.py:114-118) and pads src_distance with 0 and
                        src_edge_type with the pad index (mm_model.py:657-661), so at dropout 0 every pad row of a molecule has the same
                        input, the same bias row and the same keys in every layer; the unmasked InfoNCE mean (infonce.py:32-33) then
                        weights the one row by the number of pad positions (mmdti_seq_mean_packed_fwd).  Pair planes (bias_in, s_out) stay
                        indexed by POSITION: query position i of molecule b is packed row row_off[b] + i; query rows past the
                        representative one are neither computed nor stored. */,
                        int qkv_f16 /* != 0 (layout 3 only): qkv holds fp16 and o_bf16 receives fp16 -- the fp16 forward-operand
                        mode (MMDTI_DT_AB_F16); the backward converts q | k | v on its way into LDS */);
/* g (in/out, same layout as s; fp32, or bf16 for layout 7): on entry dL/dS_l from the layers above (ignored if g_in_zero), on
 * exit dL/dS_l total = dL/d(bias_in).  dqkv: [B,N,3*H*8] bf16.  key_tiles: as in the forward; the skipped tiles of g are neither
 * read nor written (hand in a zero-initialised g for a ragged batch). */
int mmdti_pair_attn_bwd(mmdti_stream_t stream, const void* qkv_bf16, const void* s, const void* do_bf16, void* g,
                        void* dqkv_bf16, int B, int N, int H, int ld, float scale, int g_in_zero, float drop_p,
                        unsigned long long seed, unsigned int site, int layout, const int* key_tiles,
                        const int* row_off /* nullable: packed token rows of qkv / do_bf16 / dqkv_bf16, as in the forward */,
                        int qkv_f16 /* != 0 (tiled layouts): qkv holds the fp16 q | k | v the forward multiplied; the kernel rounds them to
                        bf16 (to nearest even: the values mmdti_cast_f16_bf16 would write) on their way into LDS -- the backward's
                        products keep bf16 operands, whose range activation gradients need.  do_bf16 / dqkv_bf16 stay bf16 */);
/* What mmdti_pair_attn_fwd (backward 0) or mmdti_pair_attn_bwd (1) would launch for the same arguments, without launching: the same
 * validation, message for message, and the same plan (csrc/pair_attn_plan.h).  Pointers are tested for null and alignment only -- it
 * runs on a machine without a GPU.  For the forward, s stands for bias_in, g for s_out and o_or_do_bf16 for o_bf16; dqkv_bf16 and
 * deterministic are read for the backward only, drop_p for the forward only.  deterministic: the mode the launch would find
 * (mmdti_set_deterministic); the query does not read the process flag.  plan_out receives 6 ints: the family (0 forward MFMA, 1
 * backward MFMA, 2 forward per-element, 3 backward per-element: MMDTI_PLAN_PAIR_ATTN_FWD + family is its table for
 * mmdti_plan_kernel_name), the kernel's row in that table, grid x, workgroup size, nqb (query blocks of 16; 0 for the per-element
 * kernels) and NW (the backward MFMA kernel's wave count; else 0). */
int mmdti_pair_attn_plan(int backward, int deterministic, const void* qkv_bf16, const void* s, const void* o_or_do_bf16, const void* g,
                         const void* dqkv_bf16, int B, int N, int H, int ld, float drop_p, int layout, const int* key_tiles,
                         const int* row_off, int qkv_f16, int* plan_out);

/* ---- Row softmax over materialised scores (HF eager_attention_forward :158-183; BertCoAttention
 * mm_module.py:497-514) ------------------------------------------------------------------------
 * s: [B*heads*Lq, ld] fp32 (already scaled); key_add: [B,Lk] fp32 additive mask or null.
 * p_bf16 = softmax (saved), pd_bf16 = dropout(p) (may equal p_bf16 when drop_p==0); pad columns [Lk,ld) = 0. */
int mmdti_softmax_fwd(mmdti_stream_t stream, const float* s, const float* key_add, void* p_bf16, void* pd_bf16,
                      int B, int heads, int Lq, int Lk, int ld, float drop_p, unsigned long long seed,
                      unsigned int site);
/* ds = scale * p*(dp' - sum(dp'*p)),  dp' = dropout-backward(dp) */
int mmdti_softmax_bwd(mmdti_stream_t stream, const void* p_bf16, const float* dp, void* ds_bf16, int B, int heads,
                      int Lq, int Lk, int ld, float scale, float drop_p, unsigned long long seed,
                      unsigned int site);

/* ---- Fused multi-head attention (HF eager_attention_forward modeling_roberta.py:158-183 via mm_model.py:562;
 * BertCoAttention mm_module.py:470-514): softmax(q.k^T * scale + key_add) -> dropout -> . v without materialising the
 * [B,heads,Lq,Lk] scores.  q: rows b*Lq+i, head h at columns [h*head_dim, (h+1)*head_dim), row stride ldq (elements);
 * k, v: rows b*Lk+j, stride ldk; ctx: [B*Lq, ldo] bf16; key_add: [B,Lk] fp32 additive mask or null.
 * stats: [B,heads,Lq,2] fp32 (row max of the logits in base-2 units, i.e. times log2 e; 1/row sum) saved for the backward -- opaque
 * to the caller.  head_dim 16, 32 or 64; Lq, Lk <= 256. */
int mmdti_attn_fwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                   const float* key_add, void* ctx_bf16, float* stats, int B, int heads, int Lq, int Lk, int head_dim,
                   int ldq, int ldk, int ldo, float scale, float drop_p, unsigned long long seed, unsigned int site,
                   const int* q_off, const int* k_off, const int* k_cnt, int q_rows /* all nullable / 0 together: PACKED sequences
                   (right-padded batches, mm_model.py:645-682 / HF tokenizer padding=True).  q_off, k_off: [B+1] int32 on the device,
                   sequence b owns rows [off[b], off[b+1]) of the query-side (q, ctx) / key-side (k, v) row arrays -- its real tokens,
                   then at most one representative pad row; k_cnt: [B] int32, REAL keys of sequence b (its first k_cnt[b] key-side
                   rows).  Padded keys get probability exactly 0 in the reference (finfo.min / -10000 additive masks underflow), so
                   leaving them out of the key range is the same arithmetic; key_add must be null.  Lq, Lk: the longest sequence
                   (rows) of each side, <= 256.  stats (and drow in the backward) are then [heads, q_rows] with q_rows = q_off[B]. */,
                   int ctx_f16 /* != 0: ctx_bf16 receives fp16 (it feeds the output projection's GEMM: fp16 forward-operand mode) */);
/* dq/dk/dv (bf16, strides lddq / lddk / lddk) from dctx (stride ldo); drow: [B,heads,Lq] fp32 scratch that receives
 * sum_j dP'_ij p_ij.  Same (seed, site) as the forward call regenerates the dropout mask. */
int mmdti_attn_bwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                   const float* key_add, const void* dctx_bf16, const float* stats, float* drow, void* dq_bf16,
                   void* dk_bf16, void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo,
                   int lddq, int lddk, float scale, float drop_p, unsigned long long seed, unsigned int site,
                   const int* q_off, const int* k_off, const int* k_cnt, int q_rows /* packed sequences, as in the forward; the
                   key-side rows past k_cnt[b] (the representative pad row) receive dk = dv = 0 */);
/* The same attention for 1 <= Lq, Lk <= 512 (SMILES up to the tokenizer's 512 tokens, mm_model.py:671; 258 atoms x more than 256
 * tokens in the cross-modal block): arguments, layouts (stats, drow, packed sequences) and numerics of mmdti_attn_fwd / _bwd --
 * the softmax still runs over the whole row in registers, a row of 24 (Lk <= 384) or 32 sixteen-key tiles, against 384- / 512-row
 * LDS images (one workgroup per CU).  With Lq, Lk <= 256 they launch what mmdti_attn_fwd / _bwd launch; longer rows add exact
 * zeros, so without dropout the results on a shared shape are bit-identical.  The dropout counter strides by the padded key
 * count (16 x tiles): the mask of a (seed, site) is one and the same in the three kernels of this pair, and differs from the
 * short pair's above 256 keys.  The forward and the backward of one attention must come from the same pair. */
int mmdti_attn_long_fwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                        const float* key_add, void* ctx_bf16, float* stats, int B, int heads, int Lq, int Lk, int head_dim,
                        int ldq, int ldk, int ldo, float scale, float drop_p, unsigned long long seed, unsigned int site,
                        const int* q_off, const int* k_off, const int* k_cnt, int q_rows, int ctx_f16);
int mmdti_attn_long_bwd(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const void* v_bf16,
                        const float* key_add, const void* dctx_bf16, const float* stats, float* drow, void* dq_bf16,
                        void* dk_bf16, void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo,
                        int lddq, int lddk, float scale, float drop_p, unsigned long long seed, unsigned int site,
                        const int* q_off, const int* k_off, const int* k_cnt, int q_rows);

/* What mmdti_attn_fwd / _bwd (long_entry 0) or mmdti_attn_long_fwd / _bwd (1) would launch for the same arguments, without
 * launching: the same validation, message for message, and the same plan (csrc/attn_plan.h).  Pointers are tested for null and
 * alignment only (pass any address with the alignment in question) -- it runs on a machine without a GPU.  ctx_or_dctx_bf16 is the
 * forward's ctx_bf16 or the backward's dctx_bf16; drow, dq, dk, dv, lddq and lddk are read for the backward only.  The fused attention
 * has no atomics, so the deterministic mode does not enter.  plan_out receives 13 ints: nt (16-key tiles of a score row: 10, 16, 24 or
 * 32), lqp (queries rounded up to 32), the number of launches (1 forward; 2 backward: dQ, then dK/dV), and per launch -- the second
 * is zero for the forward -- the kernel's row in the MMDTI_PLAN_ATTN table (mmdti_plan_kernel_name), grid x, workgroup size, dynamic
 * LDS bytes, and the MaxDynamicSharedMemorySize the kernel is raised to before its first launch in this size class. */
int mmdti_attn_plan(int backward, int long_entry, const void* q_bf16, const void* k_bf16, const void* v_bf16, const float* key_add,
                    const void* ctx_or_dctx_bf16, const float* stats, const float* drow, const void* dq_bf16, const void* dk_bf16,
                    const void* dv_bf16, int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int ldo, int lddq, int lddk,
                    float drop_p, const int* q_off, const int* k_off, const int* k_cnt, int q_rows, int* plan_out);

/* ---- Attention maps: the probabilities of an attention, reduced over heads, as [B, Lq, Lk] fp32 -- without the [B, heads, Lq, Lk]
 * tensor (BertCoAttention's attention_probs mm_module.py:497-514; HF eager_attention_forward's attn_weights
 * modeling_roberta.py:158-183; the pair attention's softmax, transformers.py:137-139).  Read-outs: nothing in a training step calls them.
 * Every element of `out` is written exactly once (pass uninitialised memory), each from a sum in a fixed order: no atomics, two calls
 * give the same bits.  Purely additive: MMDTI_ABI_VERSION does not move.
 *
 * mmdti_attn_map: the map of ONE fused attention, from what mmdti_attn_fwd / mmdti_attn_long_fwd read (q, k, key_add, scale, the packed
 * arguments -- same meaning, same layouts) and wrote: stats, required, [B,heads,Lq,2] dense or [heads,q_rows,2] packed (q_rows = 0: dense).
 * p_ij = exp2(s2_ij - m_i) * inv_i with s2 = fma(q.k, scale * log2 e, max(key_add * log2 e, -FLT_MAX)): the expression the backward
 * kernels recompute.  head = -1: the mean over heads (summed in ascending head order, then times fp32(1 / heads)); head = h: that head.
 * out: [B, Lq_out, ld_out] fp32, POSITIONAL -- query position i of sequence b is row q_off[b] + i of the packed side -- with
 * Lq_out >= Lq, ld_out >= Lk; 1 <= Lq, Lk <= 512; head_dim 16, 32 or 64.  q_cnt: nullable [B] int32, the REAL queries of each sequence
 * (dense or packed; null: every row of the sequence -- under packing that includes its representative pad row).  Zeros are written
 * wherever the query position is not a real query or the key not a real key (packed: >= k_cnt[b]; dense keys are masked by key_add
 * alone); such rows of q, k and stats are never read. */
int mmdti_attn_map(mmdti_stream_t stream, const void* q_bf16, const void* k_bf16, const float* key_add, const float* stats, float* out,
                   int B, int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int Lq_out, int ld_out, float scale, int head,
                   const int* q_off, const int* k_off, const int* k_cnt, int q_rows, const int* q_cnt);
/* mmdti_pair_attn_map: the same from ONE layer's stored pair logits s (mmdti_pair_attn_fwd's s_out; the -inf of padded keys is in it):
 * fp32 softmax over the stored value, widened exactly.  layout 0 (row-major fp32, stride ld, N <= 320), 1 (tiled fp32) or 3 (compact
 * fp16), the tiled ones N <= 272 (ld is not read).  out: [B, N, ld_out] fp32, ld_out >= N.  head as above; the mean adds the heads of
 * each of four runs of ceil(H / 4) consecutive heads in ascending order and the four runs in order (layout 0: all heads in order).
 * Two rules keep it off memory the forward never stored -- key_tiles: nullable [B] int32, layout 3 (as mmdti_pair_attn_fwd): the key
 * tiles past the covered count of molecule b are never loaded and count as probability 0; n_real: nullable [B] int32, mandatory with
 * key_tiles: query rows i >= n_real[b] are written as zeros without reading s (under packed rows the rows past the representative pad
 * row are never stored). */
int mmdti_pair_attn_map(mmdti_stream_t stream, const void* s, float* out, int B, int N, int H, int ld, int ld_out, int head, int layout,
                        const int* key_tiles, const int* n_real);
/* What mmdti_attn_map (pair 0) or mmdti_pair_attn_map (pair != 0) would launch for the same arguments, without launching: the same
 * validation, message for message, and the same plan (csrc/maps_plan.h).  Pointers are tested for null and alignment only -- it runs on
 * a machine without a GPU.  pair != 0 reads q_or_s as s, heads as H, Lq as N, ldq as ld, and out, B, ld_out, head, layout, key_tiles,
 * n_real; pair 0 reads everything but the last three.  plan_out receives 6 ints: the kernel's row in the MMDTI_PLAN_MAPS table
 * (mmdti_plan_kernel_name), grid x, workgroup size, dynamic LDS bytes, what the instance is keyed by (head_dim; the 5, 9, 13 or 17 tiles a
 * tiled pair map is unrolled for -- N <= 80, 144, 208, 272; 0 for row-major planes) and the 16-key tiles a workgroup walks. */
int mmdti_maps_plan(int pair, const void* q_or_s, const void* k_bf16, const float* key_add, const float* stats, const float* out, int B,
                    int heads, int Lq, int Lk, int head_dim, int ldq, int ldk, int Lq_out, int ld_out, int head, const int* q_off,
                    const int* k_off, const int* k_cnt, int q_rows, const int* q_cnt, int layout, const int* key_tiles,
                    const int* n_real, int* plan_out);

/* ---- GELU on bf16 (kept for un-fused call sites) ------------------------------------------- */
int mmdti_gelu_fwd_bf16(mmdti_stream_t stream, const void* u_bf16, void* y_bf16, long long n);

/* ---- InfoNCE head (models/infonce.py) ------------------------------------------------------- */
/* unmasked mean over dim 1 (infonce.py:32-33): x [B,S,ld] bf16 -> out [B,D] fp32 */
int mmdti_seq_mean_fwd(mmdti_stream_t stream, const void* x_bf16, int B, int S, int D, int ld, float* out);
/* dx[b,s,:] = dout[b,:]/S  (bf16, [B,S,ld]; pad columns zeroed) */
/* dx[b*S+s, d] = bf16(dout[b, d] / S * f(aux[b*S+s, d])): f = 1 (aux_mode 0), aux (1: a saved gelu') or gelu'(aux) (2) -- the
 * backward of "pool the GELU outputs, then project" (mean_t(W2 h_t + b2) = W2 mean_t(h_t) + b2, infonce.py:28-33) */
int mmdti_seq_mean_bwd(mmdti_stream_t stream, const float* dout, int B, int S, int D, int ld, void* dx_bf16, const void* aux_bf16,
                       int ld_aux, int aux_mode);
/* The same unmasked mean over a PACKED token layout (mmdti_pair_attn_fwd, row_off): sequence b owns rows [row_off[b], row_off[b+1])
 * of x -- n_real[b] real tokens, then (if n_real[b] < S) ONE representative pad row that stands for all S - n_real[b] padded
 * positions:  out[b] = (sum_real x + (S - n_real[b]) * x_pad) / S   -- infonce.py:32-33 over the padded [B,S,*] tensor, whose pad rows
 * are identical at dropout 0.  x: [rows, ld] bf16, D % 8 == 0, ld % 8 == 0. */
int mmdti_seq_mean_packed_fwd(mmdti_stream_t stream, const void* x_bf16, int B, int S, int D, int ld, const int* row_off,
                              const int* n_real, float* out);
/* dx[r] = bf16(dout[b(r)] * w(r) / S * f(aux[r])), w = 1 for a real row, S - n_real[b] for the representative pad row; row_seq:
 * [rows] int32, the sequence each packed row belongs to; f / aux_mode as in mmdti_seq_mean_bwd. */
int mmdti_seq_mean_packed_bwd(mmdti_stream_t stream, const float* dout, int rows, int S, int D, int ld, const int* row_off,
                              const int* n_real, const int* row_seq, void* dx_bf16, const void* aux_bf16, int ld_aux, int aux_mode);
/* The mean over the REAL positions of every sequence -- where models/infonce.py:32-33 averages over all positions, padding included,
 * this divides the sum over the real positions by their number (InfoNCE(pool="real")): no padded row is read.  One entry point for
 * both layouts; exactly one of mask / row_off is non-null, anything else is MMDTI_ERR_INVALID before a launch.
 *   mask    [B,S] uint8, non-zero = real (any pattern, not only prefixes): x is [B*S, ld] bf16, masked rows may hold anything;
 *   row_off [B+1] int32: x is packed rows without pad rows, sequence b owns rows [row_off[b], row_off[b+1]), all of them real.
 * out [B,D] fp32.  A sequence with no real position gives a zero row.  D % 8 == 0, ld % 8 == 0 and a 16-byte aligned x take 16-byte
 * loads (D <= 4096), anything else a scalar kernel.  Both forms walk a sequence's positions in the same order and skip a masked row by
 * predicate, so a right-padded batch pools to the same bits in either layout.  No atomics: the sum has one order. */
int mmdti_seq_mean_real_fwd(mmdti_stream_t stream, const void* x_bf16, int B, int S, int D, int ld, const unsigned char* mask,
                            const int* row_off, float* out);
/* Its backward (the adjoint of the mean over real positions, not of infonce.py:32-33's mean over all S):
 *   dx[row] = bf16(dout[b] / count_b * f(aux[row]))   for a real row, f / aux_mode as in mmdti_seq_mean_bwd;
 *   dx[row] = 0 exactly                               for a masked row (its aux is not read), and in the pad columns D..ld.
 * rows: B*S with mask; the packed row count with row_off, and then row_seq [rows] int32 names each row's sequence (unread with mask).
 * An aux factor needs ld % 8 == 0, ld_aux % 8 == 0, ld_aux >= ld and 16-byte aligned dx / aux (MMDTI_ERR_INVALID otherwise); without
 * one, rows that are not 8-column aligned take a scalar kernel.  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_seq_mean_real_bwd(mmdti_stream_t stream, const float* dout, int rows, int B, int S, int D, int ld, const unsigned char* mask,
                            const int* row_off, const int* row_seq, void* dx_bf16, const void* aux_bf16, int ld_aux, int aux_mode);
/* F.normalize(x, dim=-1) (infonce.py:104-105; contrastive.py:22-23) */
int mmdti_l2norm_fwd(mmdti_stream_t stream, const float* x, int B, int D, int ldx, float* xhat, float* inv_norm);
int mmdti_l2norm_bwd(mmdti_stream_t stream, const float* dxhat, const float* xhat, const float* inv_norm, int B,
                     int D, int ldx, float* dx);
/* One direction of the symmetric CE (infonce.py:93-98) for anchors rows [row0,row0+Bl) of qh_all against all
 * Bg keys kh_all (global negatives under DDP).  loss_sum += sum_i CE_i (the rows' terms added in row order by one thread of the
 * column pass: reproducible to the bit); dq_all rows [row0,row0+Bl) and all
 * Bg rows of dk_all are accumulated (+=, caller zero-initialises).  Gradients are of (1/(2*Bg)) * sum_i CE_i.
 * scratch: Bl*(Bg+1) floats (the logit-gradient matrix handed from the row pass to the column pass + the Bl per-row loss terms).
 * Feature width D <= 64 (the reference's 50): the Bl x Bg similarity matrix and both gradient products run as fp32 MFMAs
 * (v_mfma_f32_16x16x4_f32 -- fp32 products and accumulation, the loss keeps fp32 precision); wider D takes scalar kernels. */
int mmdti_infonce_dir(mmdti_stream_t stream, const float* qh_all, const float* kh_all, int Bg, int D, int row0,
                      int Bl, float temperature, float* loss_sum, float* dq_all, float* dk_all, float* scratch);
/* ---- Memory bank of InfoNCE negatives: a ring of the last `cap` L2-normalised embeddings of one side, used as extra keys that receive
 * no gradient (XBM, Wang et al. 2020; the MoCo queue).  bank [cap, D] fp32, bank_valid [cap] bytes, bank_ids [cap] int64, head one
 * device int.  D <= 64.  Purely additive: MMDTI_ABI_VERSION does not move.
 *
 * mmdti_infonce_bank_dir: mmdti_infonce_dir with the key set extended -- the Bg live keys followed by the slots whose bank_valid byte is
 * non-zero; when bank_ids and ids_all ([Bg] int64) are both non-null, slot s is also skipped for anchor i if bank_ids[s] ==
 * ids_all[row0 + i] (a molecule's own stale embedding is not its negative).  A skipped slot adds nothing to the log-sum-exp and
 * nothing to dq.  The label of anchor i stays live key row0 + i.  dq_all rows [row0, row0 + Bl) accumulate over live and bank keys,
 * dk_all over the live keys only (the bank gets no gradient); scale and normalisation as mmdti_infonce_dir (0.5 / Bg; the caller
 * divides the loss by 2 Bg).  The rows pass spans anchors x key splits; every sum has a fixed order (no atomics): same inputs, same bits.
 * scratch: plan word 11 floats.  The bank buffers are only read. */
int mmdti_infonce_bank_dir(mmdti_stream_t stream, const float* qh_all, const float* kh_all, int Bg, int D, int row0, int Bl,
                           const float* bank, const unsigned char* bank_valid, const long long* bank_ids /* nullable */,
                           const long long* ids_all /* nullable */, int cap, float temperature, float* loss_sum, float* dq_all,
                           float* dk_all, float* scratch);
/* Its launch plan without launching (csrc/nce_bank_plan.h; a function of Bl, Bg and cap only), 12 words: 0 grid and 1 block of the two
 * rows launches (grid = anchor blocks x splits), 2 splits, 3 key tiles in all, 4 live key tiles, 5 anchor blocks of 16, 6 grid of the dQ
 * fold (256 threads), 7 grid of the column pass, 8-10 scratch offsets in floats of the loss terms, the (max, sum) pairs and the dQ
 * slabs (the logit gradients [Bl, Bg] sit at 0), 11 scratch floats in all. */
int mmdti_infonce_bank_plan(int Bg, int Bl, int cap, int D, long long* plan_out);
/* rows [n, D] -> slots (head + i) % cap, i < n <= cap; a slot's valid byte is 1 only if every element of its row is finite (a
 * non-finite row is stored as zeros), its id is ids[i] or -1 when ids is null; then head = (head + n) % cap in a launch of its own.
 * No host read, no synchronisation: a captured graph replays it. */
int mmdti_infonce_bank_push(mmdti_stream_t stream, float* bank, unsigned char* bank_valid, long long* bank_ids, int* head,
                            const float* rows, const long long* ids /* nullable */, int n, int D, int cap);

/* ---- ConR / SupCon (models/contrastive.py:3-59, 62-112, 114-169) --------------------------- */
/* fhat: L2-normalised features [B,D].  labels_f: [B] fp32 (regress: mean target; single: class id as float);
 * labels_i: [B,C] int64 (multi).  pred: [B] fp32 (regress).  weights: [B] fp32 or null.
 * Outputs: loss (scalar, overwritten), G [B,B] = dL/dprod. */
int mmdti_ct_loss_fwd(mmdti_stream_t stream, int mode, const float* fhat, int B, int D, const float* labels_f,
                      const long long* labels_i, int C, const float* pred, const float* weights, float w, float t,
                      float e, float coef, float* loss, float* G,
                      float* row_ws /* nullable, [B] floats: the per-row loss terms, summed in row order (bitwise reproducible loss);
                                       null: fp32 atomics */);
/* dfhat[i] = (1/t) * sum_j (G[i,j]+G[j,i]) fhat[j] */
int mmdti_ct_loss_bwd(mmdti_stream_t stream, const float* fhat, const float* G, int B, int D, float t, float* dfhat);
/* Row-block form (global ConR / SupCon negatives under data parallelism): the ranks' local batches concatenated in rank order are
 * one batch of Bg rows; this rank's anchors are rows [row0, row0 + rows) and their keys are all Bg rows.  fhat_all [Bg,D],
 * labels_f_all [Bg] / labels_i_all [Bg,C] / pred_all [Bg] / weights_all [Bg] (nullable) are the GATHERED arrays, indexed by global
 * row.  Per-anchor terms are those of mmdti_ct_loss_fwd on the Bg-row batch (same kernel body, same summation orders):
 *   loss   (scalar, overwritten) = (1/Bg) sum over this block's anchors: the block's share, the shares of a partition add up to
 *          the loss of the whole batch;
 *   G      [rows, Bg] = d(share)/d prod for the block's anchors; row_ws [rows] (nullable as above): the per-anchor terms / Bg.
 * row0 = 0, rows = Bg is mmdti_ct_loss_fwd bit for bit.  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_ct_loss_rows_fwd(mmdti_stream_t stream, int mode, const float* fhat_all, int Bg, int D, int row0, int rows,
                           const float* labels_f_all, const long long* labels_i_all, int C, const float* pred_all,
                           const float* weights_all, float w, float t, float e, float coef, float* loss, float* G, float* row_ws);
/* The block's contribution to EVERY row of the feature gradient (all Bg rows written, one writer per element, no atomics):
 *   dfhat_all[k] = (1/t) sum_j ([j in block] G[j-row0,k] + [k in block] G[k-row0,j]) fhat_all[j].
 * Summed over the blocks of a partition it is mmdti_ct_loss_bwd's dfhat; with row0 = 0, rows = Bg it is that, bit for bit. */
int mmdti_ct_loss_rows_bwd(mmdti_stream_t stream, const float* fhat_all, const float* G, int Bg, int D, int row0, int rows, float t,
                           float* dfhat_all);

/* ---- FDS (models/fds.py; utils/util.py:159-169) --------------------------------------------- */
/* bins[i] = int((label_i - min_value)//bin_width) in fp32 floor-division arithmetic (fds.py:125,164), int32;
 * flags[0] = any(bin==bucket_start), flags[1] = any(bin==bucket_num-1) (flags must be zeroed by the caller). */
int mmdti_fds_bins(mmdti_stream_t stream, const float* labels, int n, float min_value, float bin_width,
                   int bucket_start, int bucket_num, int* bins, int* flags);
/* FDS.smooth (fds.py:157-190): y = calibrate_mean_var(x, m1[b], v1[b], m2[b], v2[b]) per row bucket; scale_out[r,c]
 * = d y/d x (for backward).  Stats arrays are [bucket_num-bucket_start, D]. */
int mmdti_fds_smooth(mmdti_stream_t stream, const float* x, const int* bins, const int* flags, int n, int D,
                     int bucket_start, int bucket_num, const float* m1, const float* v1, const float* m2,
                     const float* v2, float* y, float* scale_out);
/* FDS.update_running_stats (fds.py:116-155) for all buckets: per-bucket mean / unbiased var of features, EMA into
 * running_mean/var with `factor`, num_samples_tracked += count. */
int mmdti_fds_update_stats(mmdti_stream_t stream, const float* feats, const int* bins, const int* flags, int n,
                           int D, int bucket_start, int bucket_num, float factor, float* running_mean,
                           float* running_var, float* num_samples_tracked);
/* FDS._update_last_epoch_stats smoothing (fds.py:86-99): reflect-pad + conv1d across buckets */
int mmdti_fds_smooth_stats(mmdti_stream_t stream, const float* stat, int nb, int D, const float* window, int ks,
                           float* out);
/* Streaming statistics: the training steps feed per-bucket running moments, the epoch's end is one small kernel -- in place of the
 * second forward over the training set that feeds mmdti_fds_update_stats (models/fds.py:116-155, tasks/trainer.py:288-306).  The
 * accumulator `acc` is (nb + 2) slots of (1 + 2 D) 32-bit words, nb = bucket_num - bucket_start, 4-byte aligned, zeroed by the caller
 * at the start of an epoch: { int32 rows | fp32 mean[D] | fp32 M2[D] } (Welford).  Slot s < nb: rows whose bin is exactly
 * bucket_start + s; slot nb: bins < bucket_start; slot nb + 1: bins > bucket_num - 1 -- whether those fold into the end buckets is
 * only known once the whole epoch has been seen (mmdti_fds_bins' flags).  One owner per (slot, column), no cross-workgroup float sum:
 * the results are fixed by the row order.  Purely additive: MMDTI_ABI_VERSION does not move. */
/* continues every (slot, column) recurrence over feats [n, D] in row order, with mmdti_fds_update_stats' update expression: one call
 * or any split of the same rows into calls leaves bit-identical accumulators.  A slot without a row in the batch is not written;
 * n == 0 is a no-op (models/fds.py:116-155, tasks/trainer.py:288-306). */
int mmdti_fds_stream_accumulate(mmdti_stream_t stream, const float* feats, const int* bins, int n, int D, int bucket_start,
                                int bucket_num, void* acc);
/* acc_dst <- acc_dst (+) acc_src slot by slot (Chan: n = na + nb, d = mb - ma, mean = ma + d nb / n, M2 = M2a + M2b + d^2 na nb / n):
 * the ranks' accumulators under data parallelism.  An empty side leaves the other unchanged to the bit; equal constant columns keep
 * M2 exactly 0 (models/fds.py:116-155, tasks/trainer.py:288-306). */
int mmdti_fds_stream_merge(mmdti_stream_t stream, void* acc_dst, const void* acc_src, int nb, int D);
/* the epoch's end (models/fds.py:116-155, tasks/trainer.py:288-306): the below slot merges into the first bucket iff that bucket's
 * exact count is > 0, the above slot into the last iff its exact count is > 0 and bucket_start != bucket_num - 1 (rows of a slot
 * that does not merge are dropped); a bucket with exact count 0 is untouched; variance M2 / (cnt - 1), M2 / cnt for cnt == 1; then
 * mmdti_fds_update_stats' EMA with `factor` and num_samples_tracked += cnt.  Does not clear acc. */
int mmdti_fds_stream_finish(mmdti_stream_t stream, const void* acc, int D, int bucket_start, int bucket_num, float factor,
                            float* running_mean, float* running_var, float* num_samples_tracked);

/* ---- masked pooling (mm_model.py:572-576) --------------------------------------------------- */
/* pooled[b] = (sum_{valid n} a[b,n] + sum_{valid l} t[b,l]) / (n_valid_a + n_valid_t);  a:[B,Na,D], t:[B,Nt,D] fp32,
 * masks uint8 (1 = valid). */
int mmdti_masked_pool_fwd(mmdti_stream_t stream, const float* a, const float* t, const unsigned char* mask_a,
                          const unsigned char* mask_t, int B, int Na, int Nt, int D, float* pooled);
int mmdti_masked_pool_bwd(mmdti_stream_t stream, const float* dpooled, const unsigned char* mask_a,
                          const unsigned char* mask_t, int B, int Na, int Nt, int D, float* da, float* dt);

/* The same pooling over PACKED token layouts: a: [rows_a, D], t: [rows_t, D] fp32; sequence b owns rows [a_off[b], a_off[b+1]) of a,
 * the first a_cnt[b] of them real (likewise t): pooled[b] = (sum of its real rows of a and t) / (a_cnt[b] + t_cnt[b]).  The
 * representative pad rows do not enter (mm_model.py:572-573 zeroes padded rows before the sum) and get a zero gradient.
 * a_seq / t_seq: [rows] int32, the sequence of each packed row (backward only). */
int mmdti_masked_pool_packed_fwd(mmdti_stream_t stream, const float* a, const float* t, const int* a_off, const int* a_cnt,
                                 const int* t_off, const int* t_cnt, int B, int D, float* pooled);
int mmdti_masked_pool_packed_bwd(mmdti_stream_t stream, const float* dpooled, const int* a_off, const int* a_cnt, const int* a_seq,
                                 int rows_a, const int* t_off, const int* t_cnt, const int* t_seq, int rows_t, int D, float* da,
                                 float* dt);

/* ---- small fp32 linear for the classification head (mm_model.py:44-84) ---------------------- */
/* y = act(x.W^T + b); act: 0 none, 3 tanh */
int mmdti_linear_f32_fwd(mmdti_stream_t stream, const float* x, const float* W, const float* b, int rows, int in_f,
                         int out_f, int act, float* y);
/* given dy (wrt post-activation y) and y: dx (overwrite), dW/db atomic accumulate */
int mmdti_linear_f32_bwd(mmdti_stream_t stream, const float* x, const float* W, const float* y, const float* dy,
                         int rows, int in_f, int out_f, int act, float* dx, float* dW, float* db);
/* task losses (models/nnmodel.py:24-34): mean-reduced MSE / cross-entropy, loss + dlogits in one pass */
int mmdti_mse_loss(mmdti_stream_t stream, const float* pred, const float* target, int n, float* loss, float* dpred);
int mmdti_ce_loss(mmdti_stream_t stream, const float* logits, const long long* target, int B, int C, float* loss,
                  float* dlogits);
/* nn.BCEWithLogitsLoss() -- the 'bce' entry of the multilabel_classification loss table (models/nnmodel.py:28-29) -- over n = B * C
 * logits against 0 / 1 targets given as fp32: mean-reduced loss + dlogits in one pass. */
int mmdti_bce_logits_loss(mmdti_stream_t stream, const float* logits, const float* target, int n, float* loss, float* dlogits);
/* FocalLossWithLogits -- the 'focal' entry of that table and the default of a multilabel_classification model (models/nnmodel.py:31,
 * 90-93; models/loss.py:233-276) -- over n = B * C logits against targets given as fp32.  An entry is valid iff its target is exactly
 * 0 or 1; NaN and every other value (-1) mark a missing label.  Per valid entry p = sigmoid(x), q = clamp(y ? p : 1 - p, 1e-5, 1),
 * l = -alpha (1 - q)^gamma log q (the clamped q in the modulating factor, one alpha for both classes: loss.py:253-254); loss = sum of
 * l / valid count.  dlogits in closed form in the same pass: / valid count, exactly 0 at missing entries and where the clamp holds q at
 * 1e-5.  gamma: any positive value (2 takes a path without powf).  No valid entry at all gives what the reference gives: a NaN loss
 * (the mean of an empty tensor) and dlogits = 0 everywhere.  Such a step is NOT skipped by skip_nonfinite: its gradients are finite.
 * One workgroup, fixed summation order, no floating-point atomics. */
int mmdti_focal_logits_loss(mmdti_stream_t stream, const float* logits, const float* target, int n, float alpha, float gamma,
                            float* loss, float* dlogits);
/* GHMC_Loss(bins, alpha) -- the 'ghm' entry (models/nnmodel.py:30; models/loss.py:63-132) -- in one launch: the histogram of
 * g = |sigmoid(x) - y| over bins floor(g (bins - 1e-4)) (integer counters), count = alpha * last + (1 - alpha) * count when the state
 * has history, beta_b = N / max(count_b * #{count > 0}, 1e-4) with N = n, loss = mean over N of beta_bin * bce_with_logits,
 * dlogits = beta_bin (sigmoid(x) - y) / N (the weights carry no gradient).  state: [bins + 1] fp32 on the device, zero-initialised =
 * no history; [0, bins) the counts this call leaves for the next, [bins] the "has history" flag.  EVERY call updates it, training and
 * validation alike (the reference's single loss object sees both).  bins <= 256.  Entries whose target is not exactly 0 or 1 -- where
 * the reference raises IndexError -- stay out of the histogram and get zero weight and gradient; N stays n.  Same reproducibility as
 * above. */
int mmdti_ghmc_logits_loss(mmdti_stream_t stream, const float* logits, const float* target, int n, int bins, float alpha,
                           float* state, float* loss, float* dlogits);

/* ---- optimizer step on the flat arenas (tasks/trainer.py:160,270-282) ---------------------- */
/* out[0] += sum of squares of g (zero first).  ws (nullable, ws_floats >= 1; 2048 used at most): one partial per workgroup folded in a
 * fixed order -- the gradient norm is then the same to the bit from run to run; null: fp32 atomics */
int mmdti_sumsq_f32(mmdti_stream_t stream, const float* g, long long n, float* out, float* ws, int ws_floats);
/* Adam (torch.optim.Adam semantics, eps outside sqrt of bias-corrected v): p,m,v updated in place; also refreshes the
 * bf16 shadow copy of p (the backward GEMMs' weights) and, when p_f16 is given, the fp16 one (the forward GEMMs' weights in the fp16
 * forward-operand mode; saturating).  grad is multiplied by *grad_scale_dev (device scalar, e.g. clip coefficient) if non-null.
 * step_state_dev (nullable): the device-resident schedule of mmdti_step_state_advance -- when given, lr and the bias
 * corrections are read from it and the by-value lr / step are ignored (a captured HIP graph replays with fresh values). */
int mmdti_adam_step(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    const float* grad_scale_dev, const float* step_state_dev, void* p_f16 /* nullable */);
/* Device-resident step state, so that a whole fine-tune step (tasks/trainer.py:177-283) can be captured in ONE HIP graph
 * and replayed: state[4] fp32 = {optimizer steps taken, this step's learning rate (HF linear warm-up / decay,
 * tasks/trainer.py:161-162), 1-beta1^t, sqrt(1-beta2^t)}; salt[2] u64 = {counter, mixed word}.  Call once at the top of
 * every step (inside the captured region): advances both. */
int mmdti_step_state_advance(mmdti_stream_t stream, float* state, unsigned long long* salt, float base_lr, int warmup_steps,
                             int total_steps, float beta1, float beta2);
/* Copies *salt into the dropout generators of every kernel library: all dropout sites launched after it on the stream XOR
 * their (seed, site) streams with it -- masks change from replay to replay although seed and site are frozen in the graph.
 * 0 (the initial value) leaves the generators exactly as the by-value seeds define them. */
int mmdti_seed_salt_pull(mmdti_stream_t stream, const unsigned long long* salt);

/* ---- skipping optimizer steps on non-finite gradients (GradScaler.step, tasks/trainer.py:268-282) ---- */
/* The reproducible mmdti_sumsq_f32 pass (same workgroup count, so out[0] is the same to the bit) that also counts the elements of g
 * that are inf or NaN (exponent bits all ones): out[0] += sum of squares (zero first), out[1] = non-finite count (as fp32).
 * ws: ws_floats >= 2, 4096 used at most (per-workgroup partials | per-workgroup counts).
 * guard (nullable): the device guard state, fp32 {steps taken t, steps skipped, this step's skip flag, 1-beta1^t, sqrt(1-beta2^t)}
 * (zero-initialised).  When given, the pass decides the step after its fixed-order fold, on the device: a non-finite count sets the
 * flag, out[2] = 1 and counts a skip; otherwise the flag clears, out[2] = 0, t advances and the bias corrections of the new t are
 * taken from bias_table (pairs for t = 1 .. table_steps, mmdti_adam_bias_table; the caller keeps table_steps >= every t it enqueues)
 * or, if bias_table is null, computed on the device as mmdti_step_state_advance does. */
int mmdti_sumsq_check_f32(mmdti_stream_t stream, const float* g, long long n, float* out, float* ws, int ws_floats, float* guard,
                          const float* bias_table, int table_steps, float beta1, float beta2);
/* mmdti_adam_step under the guard of mmdti_sumsq_check_f32: when the guard's flag is set nothing is read or written (p, m, v and both
 * shadows keep their values); otherwise the same update, with the bias corrections read from the guard (lr: by value, or from
 * step_state_dev when given).  With the flag clear it reproduces mmdti_adam_step to the bit for the same t and the same source of
 * bias corrections (bias_table: the by-value step; no table: the step state). */
int mmdti_adam_step_guarded(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                            float lr, float beta1, float beta2, float eps, float weight_decay, const float* grad_scale_dev,
                            const float* step_state_dev, void* p_f16 /* nullable */, const float* guard);
/* mmdti_adam_step (guard null) or mmdti_adam_step_guarded (guard given; step ignored) that leaves alone every element i with
 * skip[i / 8] != 0: p, m, v and both shadows keep their bits (parameters frozen after the arena was built, the reference's
 * requires_grad = False: torch.optim.Adam skips a parameter whose grad is None).  skip: one byte per 8 elements, (n + 7) / 8 bytes;
 * the arena's parameters start at multiples of 8 elements.  The other elements get exactly the unmasked update. */
int mmdti_adam_step_masked(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_scale_dev,
                           const float* step_state_dev, void* p_f16 /* nullable */, const float* guard /* nullable */,
                           const unsigned char* skip);
/* Parameter groups in the fused pass (tasks/trainer.py:160,270-282: the reference's one Adam(lr, eps) with its clip, extended by what
 * torch.optim's parameter groups give): mmdti_adam_step_masked (guard and skip nullable, same meaning, same sources of lr and of the
 * bias corrections) where element i belongs to group gid = group[i / 8] and is updated with the learning rate lr * table_dev[2 gid]
 * and the weight decay wd = table_dev[2 gid + 1]; there is no by-value weight decay.  Two decay forms:
 *   decoupled == 0 (torch.optim.Adam):   g' = g * scale + wd * p; the moments and the update see g'
 *   decoupled != 0 (torch.optim.AdamW):  p *= 1 - lr_i * wd before the update; the moments see g * scale alone
 * group: one byte per 8 elements, (n + 7) / 8 bytes (the arena's parameters start at multiples of 8 elements); table_dev: fp32
 * [ngroups][2] on the device, 1 <= ngroups <= 256.  Group ids are NOT checked on the host: the kernel clamps an id >= ngroups to
 * ngroups - 1.  A scale of 0 is legal: the group's m and v advance (torch with lr = 0) while p and both shadows are not written and
 * keep their bits.  With a scale of 1 and one weight decay the coupled form reproduces the three entry points above to the bit.
 * p, g, m, v and the shadows are 16-byte aligned; n == 0 launches nothing.  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_adam_step_grouped(mmdti_stream_t stream, float* p, const float* g, float* m, float* v, void* p_bf16, long long n,
                            float lr, float beta1, float beta2, float eps, int step, const float* grad_scale_dev,
                            const float* step_state_dev, void* p_f16 /* nullable */, const float* guard /* nullable */,
                            const unsigned char* skip /* nullable */, const unsigned char* group, const float* table_dev, int ngroups,
                            int decoupled);
/* HOST function: table_host[2(t-1)], [2(t-1)+1] = 1-beta1^t, sqrt(1-beta2^t) for t = 1 .. steps, exactly as mmdti_adam_step computes
 * them from its by-value step. */
int mmdti_adam_bias_table(float beta1, float beta2, int steps, float* table_host);

/* ---- weight averaging: an exponential moving average of the parameter arena (an engine feature; the reference has none) ---- */
/* ema[i] <- fma(w, p[i] - ema[i], ema[i]) for i < n: two roundings, the difference and the fma.  w = 1 - d in fp32 with d = decay, or,
 * warmup != 0, d = min(decay, (1 + t) / (10 + t)).  t = the optimizer steps applied so far, this one included, from exactly one source:
 *   guard non-null (the state of mmdti_sumsq_check_f32, already advanced by this step's check): a set skip flag returns before anything is
 *     read or written -- a skipped step leaves the average alone -- else t = the guard's count of steps taken;
 *   else step_state non-null (mmdti_step_state_advance): t = state[0];
 *   else t = step by value, >= 1.
 * Launch it right after the Adam pass of the step, on the same stream.  0 < decay < 1; p and ema are two buffers, 16-byte aligned;
 * n == 0 launches nothing.  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_ema_update(mmdti_stream_t stream, const float* p, float* ema, long long n, float decay, int warmup, int step,
                     const float* guard /* nullable */, const float* step_state /* nullable */);
/* One pass that exchanges p[i] and ema[i] bit for bit and writes the bf16 shadow -- and the fp16 one when given -- of the new p[i] with the
 * roundings of the Adam pass: both shadows are valid when the kernel ends, without a temporary and without cast passes.  Twice is the
 * identity.  p, ema and the shadows are 16-byte aligned; n == 0 launches nothing.  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_ema_swap(mmdti_stream_t stream, float* p, float* ema, void* p_bf16, void* p_f16 /* nullable */, long long n);

/* ---- Launch plans of the row kernels and of the streaming, reduction and optimizer kernels, without launching.  Each query runs the
 * validation of the entry point it stands for, message for message, and returns the plan that entry would launch (csrc/row_plan.h,
 * csrc/stream_plan.h).  No GPU needed.  ptrs is a HOST array of the entry's addresses in the order listed below; they are tested for
 * null and alignment only (pass any address with the alignment in question).  deterministic: the mode the launch would find
 * (mmdti_set_deterministic); the queries do not read the process flag, and the stream's reduction workspace is not looked up.
 * plan_out receives long long words: the number of launches (0: the entry returns without one, n == 0 where it admits that), then for
 * each of two launches -- the second is zero when there is one -- the kernel's row in the family's table (mmdti_plan_kernel_name;
 * -1: det_fold_kernel, the fixed-order fold queued behind a slab kernel), grid x, grid y, workgroup size, dynamic LDS bytes; then the
 * family's derived numbers.
 *
 * mmdti_row_plan, table MMDTI_PLAN_ROW, 13 words: ... nv (the instance's NV), rows per wave (LayerNorm backward; else 0).
 *   MMDTI_ROW_LAYERNORM_FWD  ptrs = x, gamma, beta, y_f32, y_bf16;  rows, D, drop_p
 *   MMDTI_ROW_LAYERNORM_BWD  ptrs = dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dx_bf16, dx_colsum;  rows, D, dy_dtype, drop_p, drop2_p,
 *                            deterministic (two launches: ln_bwd_slab_kernel, then the fold)
 *   MMDTI_ROW_SOFTMAX_FWD    ptrs = s, p_bf16, pd_bf16;  B, heads, Lq, Lk, ld, drop_p
 *   MMDTI_ROW_SOFTMAX_BWD    ptrs = p_bf16, dp, ds_bf16;  B, heads, Lq, Lk, ld, drop_p */
#define MMDTI_ROW_LAYERNORM_FWD 0
#define MMDTI_ROW_LAYERNORM_BWD 1
#define MMDTI_ROW_SOFTMAX_FWD 2
#define MMDTI_ROW_SOFTMAX_BWD 3
int mmdti_row_plan(int entry, int deterministic, const void* const* ptrs, int rows_or_B, int heads, int Lq, int Lk, int D_or_ld, int dy_dtype,
                   float drop_p, float drop2_p, long long* plan_out);
/* mmdti_stream_plan, table MMDTI_PLAN_STREAM, 12 words: ... the sum of squares' workgroups = partials (0 in its atomic form and elsewhere).
 *   MMDTI_STREAM_CAST_F32_BF16, _CAST_F32_F16   ptrs = x, y;  n, f = drop_p
 *   MMDTI_STREAM_CAST_F16_BF16                  ptrs = x_f16, y_bf16;  a = rows, b = cols, c = ldx
 *   MMDTI_STREAM_CAST_BF16_F32, _AXPY_F32, _GELU_FWD_BF16   ptrs = x (u), y;  n
 *   MMDTI_STREAM_DROPOUT_F32                    ptrs = x, y;  n, f = drop_p
 *   MMDTI_STREAM_COLSUM_BF16                    ptrs = x_bf16, out;  a = rows, b = cols, c = ld, deterministic (two launches: slab kernel, fold)
 *   MMDTI_STREAM_SUMSQ_F32                      ptrs = g, out, ws;  n, a = ws_floats, deterministic (refused without the ws form)
 *   MMDTI_STREAM_SUMSQ_CHECK_F32                ptrs = g, out, ws, bias_table;  n, a = ws_floats, b = table_steps
 *   MMDTI_STREAM_ADAM_STEP                      ptrs = p, g, m, v, step_state_dev;  n, a = step
 *   MMDTI_STREAM_ADAM_STEP_GUARDED              ptrs = p, g, m, v, guard;  n
 *   MMDTI_STREAM_ADAM_STEP_MASKED               ptrs = p, g, m, v, step_state_dev, guard, skip;  n, a = step
 *   MMDTI_STREAM_ADAM_STEP_GROUPED              ptrs = p, g, m, v, p_bf16, p_f16, step_state_dev, guard, skip, group, table_dev;  n, a = step,
 *                                               b = ngroups, c = decoupled
 *   MMDTI_STREAM_EMA_UPDATE                     ptrs = p, ema, guard, step_state;  n, a = step, f = decay
 *   MMDTI_STREAM_EMA_SWAP                       ptrs = p, ema, p_bf16, p_f16;  n
 *   MMDTI_STREAM_STEP_STATE_ADVANCE             ptrs = state, salt;  a = warmup_steps, b = total_steps */
#define MMDTI_STREAM_CAST_F32_BF16 0
#define MMDTI_STREAM_CAST_F32_F16 1
#define MMDTI_STREAM_CAST_F16_BF16 2
#define MMDTI_STREAM_CAST_BF16_F32 3
#define MMDTI_STREAM_DROPOUT_F32 4
#define MMDTI_STREAM_AXPY_F32 5
#define MMDTI_STREAM_GELU_FWD_BF16 6
#define MMDTI_STREAM_COLSUM_BF16 7
#define MMDTI_STREAM_SUMSQ_F32 8
#define MMDTI_STREAM_SUMSQ_CHECK_F32 9
#define MMDTI_STREAM_ADAM_STEP 10
#define MMDTI_STREAM_ADAM_STEP_GUARDED 11
#define MMDTI_STREAM_ADAM_STEP_MASKED 12
#define MMDTI_STREAM_ADAM_STEP_GROUPED 13
#define MMDTI_STREAM_EMA_UPDATE 14
#define MMDTI_STREAM_EMA_SWAP 15
#define MMDTI_STREAM_STEP_STATE_ADVANCE 16
int mmdti_stream_plan(int entry, int deterministic, const void* const* ptrs, long long n, int a, int b, int c, float f, long long* plan_out);

/* ---- LoRA adapters on a Linear (csrc/lora.hip; DESIGN.md "LoRA adapters") -----------------------------------------
 * Not part of any reference interface: the reference has no adapters.  One adapted Linear y = x.W^T (+ bias) trains the rank-r update
 * W + s.B.A with s = alpha / r: x is [T, in] (row stride ldx), A [r, in], B [out, r], all row-major.  r is 8, 16 or 32; in and out are
 * multiples of 64 (at most 8192); T >= 1 is arbitrary; row strides are multiples of 8 elements and every 16-bit base is 16-byte
 * aligned.  Anything else is MMDTI_ERR_INVALID before a launch.  All products are 16-bit MFMAs with fp32 accumulation.
 *
 * mmdti_lora_fwd: t = bf16(x.A^T), stored to t_bf16 [T, r] for the backward; then, in place, y <- round16(float(y) + s.t.B^T) where y
 * [T, out] (row stride ldy; it may be a column slice of a fused q | k | v buffer) is what the base Linear wrote.  x, A and B are
 * bf16 (f16 = 0) or fp16 (f16 = 1, the fp16 forward-operand mode; t stays bf16 and enters the second product converted to fp16, which
 * is exact for 2^-14 <= |t| <= 65504); y is bf16 (y_f16 = 0) or, beside fp16 operands only, fp16 (y_f16 = 1; the store saturates).  BOTH roundings -- t to bf16, then y to its 16-bit type -- are part
 * of the contract.  An element whose update s.(t.B^T) is zero keeps its bits: with B = 0, y is unchanged to the bit.
 *
 * mmdti_lora_bwd: u = bf16(s.dy.B), stored to u_bf16 [T, r] for mmdti_lora_dx; dB [out, r] += s.dy^T.t and dA [r, in] += u^T.x, both
 * fp32 (the arena's gradient buffers).  x is bf16, or (x_f16 = 1) a saved fp16 activation converted to bf16 inside the kernel as the
 * weight-gradient GEMM does; dy (row stride lddy), t and B are bf16 (A is not an input: no product of the backward reads it).  One
 * pass over x and dy.  Partial sums of workgroups meet in fp32 atomics; in the deterministic mode they go to per-workgroup slabs of the
 * stream's reduction workspace, folded in workgroup order -- never atomics, and a missing or too small workspace is MMDTI_ERR_INVALID.
 *
 * mmdti_lora_dx: dx [T, in] (row stride lddx) += u.A in place; dx is fp32 (dx_bf16 = 0) or bf16 (1, rounded to nearest even).
 *
 * mmdti_lora_plan: what entry 0 (mmdti_lora_fwd), 1 (mmdti_lora_bwd) or 2 (mmdti_lora_dx; n_out is ignored) would launch, without
 * launching (csrc/lora_plan.h; the same shape validation, message for message); no GPU needed.  flag: x_f16 | dx_bf16 of the
 * entry; for the forward 0 (bf16), 1 (fp16 operands and y) or 2 (fp16 operands, bf16 y).  plan_out receives 18 long long: the number of launches (1; 3 for the deterministic backward: the slab kernel, then the
 * fixed-order fold of dB and of dA), three launches of (the kernel's row in the MMDTI_PLAN_LORA table, or -1 for the fold; grid x;
 * grid y; workgroup size; dynamic LDS bytes), token rows per workgroup (forward, dx) or per chunk (backward), and the floats of one
 * workgroup's slab (deterministic backward; else 0).  Purely additive: MMDTI_ABI_VERSION does not move. */
int mmdti_lora_fwd(mmdti_stream_t stream, const void* x, int ldx, const void* A, const void* B, void* y, int ldy, void* t_bf16, int T,
                   int n_in, int n_out, int r, float scale, int f16, int y_f16);
int mmdti_lora_bwd(mmdti_stream_t stream, const void* x, int ldx, int x_f16, const void* dy_bf16, int lddy, const void* t_bf16,
                   const void* B_bf16, void* u_bf16, float* dA, float* dB, int T, int n_in, int n_out, int r, float scale);
int mmdti_lora_dx(mmdti_stream_t stream, const void* u_bf16, const void* A_bf16, void* dx, int lddx, int dx_bf16, int T, int n_in, int r);
int mmdti_lora_plan(int entry, int deterministic, int T, int n_in, int n_out, int r, int flag, long long* plan_out);

/* ---- hardware probes used by the test-suite ------------------------------------------------- */
/* out[64*4] <- what ds_read_b64_tr_b16 returns to each lane for an LDS image holding element index == value */
int mmdti_probe_tr_read(mmdti_stream_t stream, int row_stride_elems, unsigned short* out);

#ifdef __cplusplus
}
#endif
#endif /* MMDTI_HIP_H */
