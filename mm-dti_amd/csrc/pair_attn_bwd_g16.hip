// pair_attn_bwd_g16.hip -- the pair-attention backward's hot path with the gradient chain G stored as bf16 (layout 7): the same kernel as
// pair_attn_bwd.hip (pair_attn_bwd_mfma.h), compiled as its own translation unit so that the two builds run in parallel.  It contributes
// rows 34..67 of the backward's kernel table.
#include "pair_attn_bwd_mfma.h"

MMDTI_DEFINE_SALT_PULL(pair_attn_bwd_g16)

namespace mmdti {
KernelRow g_pa_bwd_compact_g16[PA_BWD_COMPACT_ROWS] = {PA_BWD_COMPACT_TABLE(1, __bf16)};
}  // namespace mmdti
