"""mmdti_hip.paths: which of the three execution paths (stack call, per-layer call, op by op) a configuration takes.

The expected values are written down from the conditions as they stood inline in functional.py before paths.py existed (each table
quotes the expression it was read from), not from running paths.py.  Shapes: the bench step is 256 molecules x 128 atoms (130 with
BOS / EOS) x 256 SMILES tokens; the reference's batch is 32 molecules; both towers are 512 wide with a 2048-wide FFN, tower 1 has 64
heads of 8, tower 2 has 8 heads."""
import pytest

from mmdti_hip import paths
from mmdti_hip.paths import LAYER, OPS, STACK

SW = paths.Switches(layer_seq=True, stack_seq=True, stack_max_rows=8192, grouped_dw=True, grouped_dw_min_rows=128, fwd_f16=True, timer=False)
BENCH_M, REF_M = 256 * 130, 32 * 130                # tower 1 token rows
BENCH_MQ, REF_MQ, REF_MQ_PACKED = 256 * 256, 32 * 256, 5000      # tower 2 (packed rows: real tokens + one pad row per sequence)
D, F = 512, 2048


def sw(**kw):
    return SW._replace(**kw)


def test_predicates():
    # ops.GROUPED_DW and D % 256 == 0 and F % 256 == 0 and M >= ops.GROUPED_DW_MIN_ROWS
    assert paths.grouped_dw_ok(SW, 512, 2048, 128) is True
    assert paths.grouped_dw_ok(SW, 512, 2048, 127) is False
    assert paths.grouped_dw_ok(SW, 320, 2048, 4096) is False
    assert paths.grouped_dw_ok(SW, 512, 1000, 4096) is False
    assert paths.grouped_dw_ok(sw(grouped_dw=False), 512, 2048, 4096) is False
    assert paths.grouped_dw_ok(sw(grouped_dw_min_rows=64), 512, 2048, 64) is True
    # the cross layer: D % 8 == 0 and W.i_w.shape[0] % 8 == 0 -- looser, and it stays looser
    assert paths.cross_dims_ok(64, 128) and paths.cross_dims_ok(320, 1000)
    assert not paths.cross_dims_ok(516, 2048) and not paths.cross_dims_ok(512, 2052)
    # (compact or not ops.FWD_F16) / (L0.h1.dtype != torch.float16 or L0.s.dtype == torch.float16)
    assert paths.f16_operands_covered(True, True) and paths.f16_operands_covered(False, False) and paths.f16_operands_covered(False, True)
    assert not paths.f16_operands_covered(True, False)
    assert paths.head_dim_is_8(512, 64) and not paths.head_dim_is_8(512, 8)


# seq = LAYER_SEQ and emb.is_cuda and (compact or not ops.FWD_F16) and not ops.kernel_timer.names and D == H * 8
@pytest.mark.parametrize("s, on_gpu, compact, d, h, want", [
    (SW, True, True, 512, 64, LAYER),                       # bench shape and reference batch alike
    (SW, True, False, 512, 64, OPS),                        # fp16 operands without the compact planes
    (sw(fwd_f16=False), True, False, 512, 64, LAYER),       # bf16 operands: any pair layout
    (sw(timer=True), True, True, 512, 64, OPS),
    (sw(layer_seq=False), True, True, 512, 64, OPS),
    (SW, False, True, 512, 64, OPS),
    (SW, True, True, 512, 8, OPS),                          # head dimension 64
    (SW, True, True, 64, 8, LAYER),                         # a forward launches no weight gradient: D % 256 is not asked
    (sw(grouped_dw=False), True, True, 512, 64, LAYER),
])
def test_unimol_layer_fwd(s, on_gpu, compact, d, h, want):
    assert paths.unimol_layer_fwd(s, on_gpu, compact, d, h) == want


# T = tables if (seq and keep and STACK_SEQ and nlayers and M < STACK_MAX_ROWS and not aux_grads and mod.final_layer_norm is not None)
@pytest.mark.parametrize("s, layer_path, keep, nlayers, rows, aux, final_ln, want", [
    (SW, LAYER, True, 15, BENCH_M, False, True, LAYER),     # bench shape: per-layer calls, not the stack
    (SW, LAYER, True, 15, REF_M, False, True, STACK),       # reference batch
    (SW, LAYER, True, 15, 8191, False, True, STACK),
    (SW, LAYER, True, 15, 8192, False, True, LAYER),
    (sw(stack_max_rows=0), LAYER, True, 15, REF_M, False, True, LAYER),
    (sw(stack_seq=False), LAYER, True, 15, REF_M, False, True, LAYER),
    (SW, OPS, True, 15, REF_M, False, True, OPS),           # whatever sent the layers op by op (timer, LAYER_SEQ off, fp16 without compact)
    (SW, LAYER, False, 15, REF_M, False, True, LAYER),      # inference, or nothing of the tower trains
    (SW, LAYER, True, 0, REF_M, False, True, LAYER),
    (SW, LAYER, True, 15, REF_M, True, True, LAYER),
    (SW, LAYER, True, 15, REF_M, False, False, LAYER),
])
def test_unimol_tower_fwd(s, layer_path, keep, nlayers, rows, aux, final_ln, want):
    assert paths.unimol_tower_fwd(s, layer_path, keep, nlayers, rows, aux, final_ln) == want


# if arena is None or not ops.GROUPED_DW or M < ops.GROUPED_DW_MIN_ROWS: return None ... ok = D % 256 == 0 and F % 256 == 0
# tower 2 adds: D % heads or not ops.attn_eligible(st.Lq, st.Lk, D // heads, D)
@pytest.mark.parametrize("s, in_arena, d, f, rows, attn_ok, want", [
    (SW, True, D, F, REF_M, True, STACK),
    (SW, False, D, F, REF_M, True, LAYER),                  # parameters outside an arena
    (sw(grouped_dw=False), True, D, F, REF_M, True, LAYER),
    (SW, True, D, F, 127, True, LAYER),
    (SW, True, 320, F, REF_M, True, LAYER),
    (SW, True, D, 1000, REF_M, True, LAYER),
    (SW, True, D, F, REF_MQ_PACKED, False, LAYER),          # sequences or heads the fused attention kernels do not take
])
def test_stack_call(s, in_arena, d, f, rows, attn_ok, want):
    assert paths.stack_call(s, in_arena, d, f, rows, attn_ok) == want


# ok = all(q is not None and q.requires_grad and q._mmdti_arena is arena for q in ps) and shapes / eps / parameter count uniform
# tower 2: and q | k | v (weights and biases) back to back in the arena
@pytest.mark.parametrize("trainable, same_arena, uniform, extra, want", [
    ((True,) * 24, True, True, True, STACK),
    ((True,) * 23 + (False,), True, True, True, LAYER),     # one frozen parameter
    ((False,) * 24, True, True, True, LAYER),               # a fully frozen tower (reached when an input wants a gradient)
    ((True,) * 24, False, True, True, LAYER),               # a parameter outside the arena
    ((True,) * 24, True, False, True, LAYER),
    ((True,) * 24, True, True, False, LAYER),               # q | k | v not adjacent
])
def test_stack_model(trainable, same_arena, uniform, extra, want):
    assert paths.stack_model(trainable, same_arena, uniform, extra) == want


# _unimol_seq_workspace(...) if (LAYER_SEQ and dout.is_cuda and st.layers and plan.lowest < len(st.layers)) else (False, None); inside:
# ok = (L0.h1.dtype != f16 or L0.s.dtype == f16) and not kernel_timer.names and GROUPED_DW and D % 256 == 0 and F % 256 == 0
#      and M >= GROUPED_DW_MIN_ROWS and any(full[plan.lowest:])
@pytest.mark.parametrize("s, on_gpu, nkept, lowest, f16, compact, d, f, rows, full, want", [
    (SW, True, 15, 0, True, True, D, F, BENCH_M, [True] * 15, LAYER),
    (SW, True, 0, 0, True, True, D, F, REF_M, [], OPS),                          # after a stack forward: no layer was kept
    (SW, True, 15, 0, True, False, D, F, BENCH_M, [True] * 15, OPS),             # fp16 operands without compact planes
    (SW, True, 15, 0, False, False, D, F, BENCH_M, [True] * 15, LAYER),
    (sw(timer=True), True, 15, 0, True, True, D, F, BENCH_M, [True] * 15, OPS),
    (sw(layer_seq=False), True, 15, 0, True, True, D, F, BENCH_M, [True] * 15, OPS),
    (sw(grouped_dw=False), True, 15, 0, True, True, D, F, BENCH_M, [True] * 15, OPS),
    (SW, False, 15, 0, True, True, D, F, BENCH_M, [True] * 15, OPS),
    (SW, True, 15, 0, True, True, D, F, 127, [True] * 15, OPS),
    (SW, True, 15, 0, True, True, 320, F, BENCH_M, [True] * 15, OPS),
    (SW, True, 15, 0, True, True, D, 1000, BENCH_M, [True] * 15, OPS),
    (SW, True, 3, 0, True, True, D, F, BENCH_M, [True, False, True], LAYER),     # a partly frozen layer between full ones
    (SW, True, 3, 1, True, True, D, F, BENCH_M, [True, False, False], OPS),      # the only full layer lies under the lowest that runs
    (SW, True, 3, 0, True, True, D, F, BENCH_M, [False] * 3, OPS),               # frozen tower, the pair bias under it trains
    (SW, True, 3, 3, True, True, D, F, BENCH_M, [True] * 3, OPS),                # no layer runs
])
def test_unimol_tower_bwd(s, on_gpu, nkept, lowest, f16, compact, d, f, rows, full, want):
    assert paths.unimol_tower_bwd(s, on_gpu, nkept, lowest, f16, compact, d, f, rows, full) == want


def test_unimol_layer_bwd():
    # if seq_ok and dx16 is not None and not hold and full[li]
    assert paths.unimol_layer_bwd(LAYER, True, False, True) == LAYER
    assert paths.unimol_layer_bwd(OPS, True, False, True) == OPS
    assert paths.unimol_layer_bwd(LAYER, False, False, True) == OPS          # no final LayerNorm above: no bf16 copy of the gradient
    assert paths.unimol_layer_bwd(LAYER, True, True, True) == OPS            # weight gradients held back for the end
    assert paths.unimol_layer_bwd(LAYER, True, False, False) == OPS
    # a partly frozen layer runs op by op, its neighbours keep the library call
    full = [True, False, True]
    tower = paths.unimol_tower_bwd(SW, True, 3, 0, True, True, D, F, BENCH_M, full)
    assert [paths.unimol_layer_bwd(tower, True, False, f) for f in full] == [LAYER, OPS, LAYER]


# LAYER_SEQ and STACK_SEQ and keep and x32.is_cuda and Mq < STACK_MAX_ROWS and len(mod.layers) and not ops.kernel_timer.names
@pytest.mark.parametrize("s, on_gpu, keep, nlayers, rows, want", [
    (SW, True, True, 6, BENCH_MQ, LAYER),                   # bench shape
    (SW, True, True, 6, REF_MQ_PACKED, STACK),              # reference batch, packed rows
    (SW, True, True, 6, REF_MQ, LAYER),                     # 32 x 256 padded rows = 8192: the bound is strict
    (SW, True, True, 6, 8191, STACK),
    (sw(timer=True), True, True, 6, REF_MQ_PACKED, LAYER),
    (sw(layer_seq=False), True, True, 6, REF_MQ_PACKED, LAYER),
    (sw(stack_seq=False), True, True, 6, REF_MQ_PACKED, LAYER),
    (sw(stack_max_rows=0), True, True, 6, REF_MQ_PACKED, LAYER),
    (SW, True, False, 6, REF_MQ_PACKED, LAYER),             # a fully frozen tower keeps nothing
    (SW, False, True, 6, REF_MQ_PACKED, LAYER),
    (SW, True, True, 0, REF_MQ_PACKED, LAYER),
])
def test_bert_tower_fwd(s, on_gpu, keep, nlayers, rows, want):
    assert paths.bert_tower_fwd(s, on_gpu, keep, nlayers, rows) == want


# self : LAYER_SEQ and self_attn and L.fw is not None and s1_32.is_cuda and not timer and D % 256 == 0 and F % 256 == 0
#        and Mq >= GROUPED_DW_MIN_ROWS and GROUPED_DW
# cross: LAYER_SEQ and not self_attn and L.fw is not None and L.fused and s1_32.is_cuda and not timer and D % 8 == 0 and F % 8 == 0
#        and W.q_b is not None        (L.fw is only set when L.fused and W.q_b is not None)
@pytest.mark.parametrize("s, fused_proj, on_gpu, d, f, rows, want_self, want_cross", [
    (SW, True, True, D, F, BENCH_MQ, LAYER, LAYER),
    (SW, True, True, D, F, REF_MQ, LAYER, LAYER),
    (sw(timer=True), True, True, D, F, BENCH_MQ, OPS, OPS),
    (sw(layer_seq=False), True, True, D, F, BENCH_MQ, OPS, OPS),
    (SW, False, True, D, F, BENCH_MQ, OPS, OPS),            # q | k | v not adjacent, one of them frozen, or no fused attention
    (SW, True, False, D, F, BENCH_MQ, OPS, OPS),
    (SW, True, True, D, F, 64, OPS, LAYER),                 # rows below GROUPED_DW_MIN_ROWS
    (SW, True, True, 320, 1280, BENCH_MQ, OPS, LAYER),      # D not a multiple of 256
    (SW, True, True, D, 1000, BENCH_MQ, OPS, LAYER),        # F not a multiple of 256
    (SW, True, True, 64, 128, BENCH_MQ, OPS, LAYER),
    (sw(grouped_dw=False), True, True, D, F, BENCH_MQ, OPS, LAYER),
    (SW, True, True, 516, F, BENCH_MQ, OPS, OPS),
    (SW, True, True, D, 2052, BENCH_MQ, OPS, OPS),
])
def test_bert_layer_fwd(s, fused_proj, on_gpu, d, f, rows, want_self, want_cross):
    assert paths.bert_layer_fwd(s, True, fused_proj, on_gpu, d, f, rows) == want_self
    assert paths.bert_layer_fwd(s, False, fused_proj, on_gpu, d, f, rows) == want_cross


def test_bert_layer_bwd():
    # L.seq is True / == "cross" and not ops.kernel_timer.names and all(gbuf(p) is not None for p in (...))
    assert paths.bert_layer_bwd(LAYER, False, True) == LAYER
    assert paths.bert_layer_bwd(LAYER, True, True) == OPS            # the timer was switched on between forward and backward
    assert paths.bert_layer_bwd(LAYER, False, False) == OPS          # a gradient buffer is gone
    assert paths.bert_layer_bwd(OPS, False, True) == OPS


def test_switches_are_read_at_call_time(monkeypatch):
    from mmdti_hip import functional as Fn, ops
    base = Fn._switches()
    assert base == paths.Switches(Fn.LAYER_SEQ, Fn.STACK_SEQ, Fn.STACK_MAX_ROWS, ops.GROUPED_DW, ops.GROUPED_DW_MIN_ROWS, ops.FWD_F16, False)
    monkeypatch.setattr(Fn, "LAYER_SEQ", not base.layer_seq)
    monkeypatch.setattr(Fn, "STACK_SEQ", not base.stack_seq)
    monkeypatch.setattr(Fn, "STACK_MAX_ROWS", 0)
    monkeypatch.setattr(ops, "FWD_F16", not base.fwd_f16)
    monkeypatch.setattr(ops, "GROUPED_DW_MIN_ROWS", 77)
    monkeypatch.setattr(ops.kernel_timer, "names", ("gemm",))
    assert Fn._switches() == paths.Switches(not base.layer_seq, not base.stack_seq, 0, ops.GROUPED_DW, 77, not base.fwd_f16, True)
