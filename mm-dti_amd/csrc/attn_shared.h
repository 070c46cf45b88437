// attn_shared.h -- what the fused attention kernels (attn.hip) and the attention-map kernels (attn_maps.hip) share, one definition each:
// the maps recompute the forward's probabilities, so the mask clamp, the probability expression and the operand fragment are the
// forward's own.  Every kernel of both files is held to the instruction stream it had before the pieces were
// shared (profiles/attn_head_shared_isa.txt).
#pragma once
#include "common.h"

namespace mmdti {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Logits are carried in base-2 units (scale * log2 e folded into the scale and the additive key mask), so that the softmax
// exponential is a bare v_exp_f32.  A finite "minus infinity" mask (finfo.min) stays finite: a fully masked row then softmaxes
// to uniform, as it does in the unfused path.
constexpr float ATTN_LOG2E = 1.4426950408889634f;
__device__ __forceinline__ float attn_mask2(float ka) { return fmaxf(ka * ATTN_LOG2E, -3.4028234663852886e38f); }

// 16 rows x 8 consecutive k of a [rows, ld] bf16 matrix in global memory as an MFMA 16x16x32 operand (lane & 15 = row, lane >> 4 = k
// group); head_dim 16: the upper two k groups are zeros
template <int HD>
__device__ __forceinline__ bf16x8 attn_frag_global(const bf16_t* base, bool valid, int c, int lane) {
  bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (valid && (HD >= 32 || 8 * (lane >> 4) < HD)) z = *reinterpret_cast<const bf16x8*>(base + 32 * c + 8 * (lane >> 4));
  return z;
}
// One probability from the saved row statistics (max in base-2 units, 1 / sum): THE expression of the dQ kernel's sweeps (both forms),
// of the dK/dV kernel and of the attention maps -- their bit-identity rests on it being one.
__device__ __forceinline__ float attn_prob(float s, float scale2, float ka, float m, float inv) {
  return __builtin_amdgcn_exp2f(s * scale2 + ka - m) * inv;
}

}  // namespace mmdti
