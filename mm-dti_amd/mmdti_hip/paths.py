"""Which way a transformer layer runs.  Every layer of the two towers and of the cross block has three execution paths:

  STACK  all layers of a tower behind one library call per direction (mmdti_unimol_stack_*, mmdti_bert_stack_*);
  LAYER  one library call per layer and direction (mmdti_unimol_layer_*, mmdti_bert_layer_*, mmdti_bert_cross_layer_*);
         layers that carry LoRA adapters next to a frozen base have their own STACK and LAYER calls (mmdti_*_lora_*: adapter_seq);
  OPS    the op-by-op Python body of functional.py: the general path, which the tests hold the other two bit-identical to.

This module is the one place that chooses.  Pure Python on plain values (sizes, flags, the switch values of the moment), no device
work, no library: functional.py gathers the values, asks here and follows the answer.  A function that decides for a whole tower
answers STACK or LAYER, "not the stack": each layer then gets its own decision.  A stack answer also needs stack_call and stack_model.

The attention recorder (functional.record_attention) needs no flag here: it refuses a forward that keeps activations for a backward
before the first launch, and STACK is only ever answered for such a forward (keep) -- a recorded pass runs LAYER or OPS, where every
layer's logits (tower 1) or q, k and row statistics (tower 2, cross block) exist when the layer returns.
"""
from typing import NamedTuple, Sequence

STACK, LAYER, OPS = "stack", "layer", "ops"


class Switches(NamedTuple):
    """The switch values at the time of the call (functional._switches(): tests and bench.py change them between steps)."""
    layer_seq: bool             # functional.LAYER_SEQ
    stack_seq: bool             # functional.STACK_SEQ
    stack_max_rows: int         # functional.STACK_MAX_ROWS
    grouped_dw: bool            # ops.GROUPED_DW
    grouped_dw_min_rows: int    # ops.GROUPED_DW_MIN_ROWS
    fwd_f16: bool               # ops.FWD_F16: fp16 forward operands
    timer: bool                 # ops.kernel_timer is on: only the op-by-op path brackets each launch with events


# ------------------------------------------------------------------------------------------------- the recurring conditions
def grouped_dw_ok(sw: Switches, D: int, F: int, rows: int) -> bool:
    """The grouped weight-gradient launch takes the layer's [.., D] and [F, D] matrices over `rows` token rows: every sequencer that
    launches it needs this (all but the cross layer's, which leaves the weight gradients to the host)."""
    return bool(sw.grouped_dw and D % 256 == 0 and F % 256 == 0 and rows >= sw.grouped_dw_min_rows)


def cross_dims_ok(D: int, F: int) -> bool:
    """The cross-attention sequencer launches no grouped weight gradient: it only needs rows of whole 16-byte vectors."""
    return D % 8 == 0 and F % 8 == 0


def f16_operands_covered(f16_operands: bool, compact: bool) -> bool:
    """Uni-Mol sequencers with fp16 forward operands cover the compact (fp16) pair planes: the only layout with fp16 q | k | v kernels."""
    return bool(compact or not f16_operands)


def head_dim_is_8(D: int, H: int) -> bool:
    """The pair-attention kernels behind the Uni-Mol sequencers are the head-dimension-8 ones."""
    return D == H * 8


def adapter_seq_ok(switch: bool, base_trainable: Sequence[bool], adapters_trainable: Sequence[bool], fused_attn: bool = True) -> bool:
    """The `adapter_seq` of the functions below: layers that carry LoRA adapters may take the library's adapted sequencers
    (mmdti_*_lora_*).  switch: functional.LORA_SEQ; base_trainable / adapters_trainable: requires_grad of every base parameter and of
    every adapter parameter of the layers in question -- the adapted calls launch no weight gradient and every adapter's gradient
    kernel, so every base parameter is frozen and every adapter pair trains; fused_attn (tower 2, cross block): the fused attention
    kernels take the layer's lengths and head size, and its projections have biases."""
    return bool(switch and fused_attn and not any(base_trainable) and len(adapters_trainable) > 0 and all(adapters_trainable))


# ------------------------------------------------------------------------------------------------- tower 1 (Uni-Mol pair encoder)
def unimol_layer_fwd(sw: Switches, on_gpu: bool, compact: bool, D: int, H: int, adapters: bool = False, adapter_seq: bool = False) -> str:
    """The forward of the tower's layers, one answer for all: LAYER or OPS.  (A forward launches no weight gradient: grouped_dw_ok
    only bears on the backward.)  adapters: a layer of the tower carries LoRA adapters -- only the adapted sequencers launch their
    kernels, and only where adapter_seq (adapter_seq_ok over the tower's layers) holds."""
    ok = ((not adapters or adapter_seq) and sw.layer_seq and on_gpu and f16_operands_covered(sw.fwd_f16, compact) and not sw.timer
          and head_dim_is_8(D, H))
    return LAYER if ok else OPS


def unimol_tower_fwd(sw: Switches, layer_path: str, keep: bool, nlayers: int, rows: int, aux_grads: bool, final_ln: bool,
                     adapters: bool = False, adapter_seq: bool = False) -> str:
    """STACK for a small batch that keeps its activations for a backward (keep), else layer_path (unimol_layer_fwd's answer).
    aux_grads: the auxiliary outputs are differentiable; final_ln: the encoder ends in a LayerNorm."""
    ok = ((not adapters or adapter_seq) and layer_path == LAYER and keep and sw.stack_seq and nlayers > 0 and rows < sw.stack_max_rows
          and not aux_grads and final_ln)
    return STACK if ok else layer_path


def unimol_tower_bwd(sw: Switches, on_gpu: bool, nkept: int, lowest: int, f16_operands: bool, compact: bool, D: int, F: int, rows: int,
                     full: Sequence[bool], adapter_seq: bool = False) -> str:
    """LAYER: layers of this backward may take the library call (its workspace is allocated); OPS: none does.  nkept: layers the forward
    kept (0 after a stack forward); lowest: freeze.TowerPlan.lowest; f16_operands / compact: as the forward ran; full: see below.
    adapter_seq: the layers are adapted ones on a frozen base (adapter_seq_ok) -- no grouped weight gradient, and `full` is moot."""
    ok = (sw.layer_seq and on_gpu and lowest < nkept and f16_operands_covered(f16_operands, compact) and not sw.timer
          and (adapter_seq or (grouped_dw_ok(sw, D, F, rows) and any(full[lowest:]))))
    return LAYER if ok else OPS


def unimol_layer_bwd(tower_path: str, have_dx16: bool, held: bool, full: bool, adapters: bool = False, adapter_seq: bool = False) -> str:
    """One layer of the backward.  have_dx16: the LayerNorm backward above left the bf16 copy of the stream gradient; held: the layer's
    weight gradients wait for the end of the backward (functional.DEFER_WGRAD_LAYERS); full: every parameter of the layer trains -- a
    frozen or partly frozen layer runs op by op, where its gradient kernels drop out one by one; adapters: the layer's forward ran LoRA
    adapters, whose gradient kernels the op-by-op backward launches -- or, adapter_seq, the adapted library call, which has no weight
    gradient to hold back."""
    if adapters:
        return LAYER if (tower_path == LAYER and have_dx16 and adapter_seq) else OPS
    return LAYER if (tower_path == LAYER and have_dx16 and not held and full) else OPS


# ------------------------------------------------------------------------------------------------- tower 2 (RoBERTa), cross block
def bert_tower_fwd(sw: Switches, on_gpu: bool, keep: bool, nlayers: int, rows: int, adapters: bool = False, adapter_seq: bool = False) -> str:
    """STACK for a small batch that keeps its activations for a backward, else LAYER: each layer asks bert_layer_fwd.  adapters: a layer
    of the tower carries LoRA adapters; adapter_seq: adapter_seq_ok over all of the tower's layers."""
    ok = (not adapters or adapter_seq) and sw.layer_seq and sw.stack_seq and keep and on_gpu and rows < sw.stack_max_rows and nlayers > 0 and not sw.timer
    return STACK if ok else LAYER


def bert_layer_fwd(sw: Switches, self_attn: bool, fused_proj: bool, on_gpu: bool, D: int, F: int, rows: int, adapters: bool = False,
                   adapter_seq: bool = False) -> str:
    """One BERT-style layer.  fused_proj: query | key | value (cross-attention: key | value) run as one GEMM over parameters that sit
    back to back in the arena and all train -- which implies the fused attention kernels and projection biases.  rows: query rows.
    adapters: the layer carries LoRA adapters, which the op-by-op body launches -- or, adapter_seq (adapter_seq_ok over this layer), the
    adapted library call: three separate projections of a frozen base and no grouped weight gradient, so neither fused_proj nor
    grouped_dw_ok applies, only rows of whole 16-byte vectors."""
    if adapters:
        return LAYER if (adapter_seq and sw.layer_seq and on_gpu and not sw.timer and cross_dims_ok(D, F)) else OPS
    if not (sw.layer_seq and fused_proj and on_gpu and not sw.timer):
        return OPS
    return LAYER if (grouped_dw_ok(sw, D, F, rows) if self_attn else cross_dims_ok(D, F)) else OPS


def bert_layer_bwd(fwd_path: str, timer: bool, buffers_live: bool) -> str:
    """The backward follows what the forward recorded on the layer, but for what can change in between: launches are timed now, or a
    gradient buffer the sequencer writes through is gone (a parameter frozen after the forward: functional._grad_buffers_live)."""
    return LAYER if (fwd_path == LAYER and not timer and buffers_live) else OPS


# ------------------------------------------------------------------------------------------------- the stack calls' own conditions
def stack_call(sw: Switches, in_arena: bool, D: int, F: int, rows: int, attn_ok: bool = True, adapter_seq: bool = False) -> str:
    """Per call.  in_arena: the tower's parameters live in a trainer arena (the pointer tables are offsets into it); attn_ok (tower 2):
    the fused attention kernels take the sequence lengths and head size.  adapter_seq: the adapted stack calls -- in_arena speaks of the
    adapters (the frozen base is addressed through its shadows), and no grouped weight gradient is launched."""
    return STACK if (in_arena and (cross_dims_ok(D, F) if adapter_seq else grouped_dw_ok(sw, D, F, rows)) and attn_ok) else LAYER


def stack_model(trainable: Sequence[bool], same_arena: bool, uniform: bool, adjacent: bool = True) -> str:
    """Per model and trainable set (cached by functional._stack_tables): the stack calls take every parameter of every layer as trainable
    and address it through one arena.  uniform: every layer has the first one's shapes, parameter count and LayerNorm epsilon; adjacent
    (tower 2): q | k | v sit back to back, as one [3D, D] matrix and one [3D] bias."""
    return STACK if (all(trainable) and same_arena and uniform and adjacent) else LAYER
