"""Module-level forward+backward of the fine-tune step, hand-scheduled over the C-ABI kernels.

Each ``torch.autograd.Function`` below is ONE node in the autograd graph for a whole reference module (15-layer
pair-bias encoder, RoBERTa tower, cross-modal block, InfoNCE head, ...).  Forward launches the kernels and keeps the
activations the backward needs; backward launches the gradient kernels in reverse order.  Weight gradients are
accumulated by the kernels straight into ``param.grad`` (views of the gradient arena), so autograd only carries the
activation gradients between modules.  torch is plumbing here (memory, streams, graph edges) -- no ATen math.

Precision contract (matches ``oracle.mmdti_oracle`` with ``bf16=True``): GEMM operands bf16, accumulation fp32, residual
stream / LayerNorm statistics / softmax / pair-bias chain S fp32, q|k|v and attention probabilities stored bf16.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
import weakref

import math
from types import SimpleNamespace
from typing import List, Optional

import torch

from . import ops, paths
from .ops import BF16, F32
from .runtime import fused_views, wbf16, wfwd, gbuf, dropout_state, notify_grads_ready
from .freeze import layer_trainable, plan_tower, trainable_flags


# ------------------------------------------------------------------------------------------------- helpers
def _lin_bwd_params(dy_bf16, x_bf16, weight, bias, rows=None, bias_done=False):
    """dW += dy^T x ; db += colsum(dy)   (atomic accumulation into param.grad).  bias_done: the kernel that produced dy
    already accumulated its column sums (LayerNorm backward's bf16 copy).  Otherwise the bias gradient rides on the
    weight-gradient GEMM, which reads dy anyway (ops.linear_bwd_weight(db=...))."""
    gw = gbuf(weight)
    gb = gbuf(bias) if (bias is not None and not bias_done) else None
    if gw is not None:
        ops.linear_bwd_weight(dy_bf16, x_bf16, gw, rows=rows, db=gb if (gb is not None and gb.numel() == gw.shape[0]) else None)
        if gb is not None and gb.numel() == gw.shape[0]:
            gb = None
    if gb is not None:
        ops.colsum(dy_bf16, gb, cols=bias.numel())


def _lin_bwd_params_many(calls, raw_items=()):
    """calls: [(args, kwargs)] of _lin_bwd_params for Linears of ONE layer (same token rows): their weight gradients go out as a
    single grouped launch (ops.linear_bwd_weight_grouped); bias gradients ride on it, leftovers take the column-sum pass.
    raw_items: ready-made (dy, x, dw_buffer, db_buffer | None, rows | None) entries (fused query|key|value views)."""
    items, late = list(raw_items), []
    for args, kw in calls:
        dy, x, weight, bias = args[:4]
        rows, bias_done = kw.get("rows"), kw.get("bias_done", False)
        gw = gbuf(weight)
        gb = gbuf(bias) if (bias is not None and not bias_done) else None
        if gw is None:
            if gb is not None:
                late.append((dy, gb, bias.numel()))
            continue
        rides = gb is not None and gb.numel() == gw.shape[0]
        items.append((dy, x, gw, gb if rides else None, rows))
        if gb is not None and not rides:
            late.append((dy, gb, bias.numel()))
    if items:
        ops.linear_bwd_weight_grouped(items)
    for dy, gb, cols in late:
        ops.colsum(dy, gb, cols=cols)


# one C call per layer backward where the library has a sequencer for the variant at hand (csrc/layers.hip): the launch order,
# kernels and arguments of the op-by-op path below, minus ~140 us of Python per layer -- what paces a step of 16-32 molecules
# (which path a layer takes -- this call, the stack call further down, or op by op -- is decided in paths.py)
LAYER_SEQ = os.environ.get("MMDTI_LAYER_SEQ", "1") != "0"
# layers that carry LoRA adapters next to a frozen base take the library's adapted sequencers (mmdti_*_lora_*: the launches of the op-by-op
# bodies below, bit for bit); 0: they run op by op, the path the tests compare against
LORA_SEQ = os.environ.get("MMDTI_LORA_SEQ", "1") != "0"
POOL_THEN_PROJECT = os.environ.get("MMDTI_INFONCE_POOL_FIRST", "1") != "0"      # InfoNCE head: pool the GELU outputs, then project


def _join_stream_after_backward():
    """A module backward that writes parameter gradients itself leaves autograd no leaf on its stream, so the engine would
    not join that stream at the end of backward(): if we are on a side stream, queue the join."""
    here = torch.cuda.current_stream()
    if here == torch.cuda.default_stream():
        return

    def _join(stream=here):
        cur = torch.cuda.current_stream()
        if cur != stream:
            cur.wait_stream(stream)

    torch.autograd.Variable._execution_engine.queue_callback(_join)


# Weight gradients held back to the end of the pair encoder's backward: the fused pair-bias backward that follows it runs
# alone on the chip and is latency-bound (waves parked 80 % of their cycles), so the weight-gradient GEMMs of the last few
# layers -- leaves of the backward graph -- are launched on their own stream right before it and run underneath it.
DEFER_WGRAD_LAYERS = int(os.environ.get("MMDTI_DEFER_WGRAD", "4"))
_wgrad_stream_obj = None
_wgrad_keep = []


def _launch_deferred_wgrads(deferred, layers):
    """deferred: argument tuples of _lin_bwd_params whose operands must stay alive until the stream is joined."""
    if not deferred:
        return
    main = torch.cuda.current_stream()
    ws = _wgrad_stream()
    ws.wait_stream(main)
    with torch.cuda.stream(ws):
        for group in deferred:                      # one list of _lin_bwd_params calls per layer
            _lin_bwd_params_many(group)
        for layer in layers:
            notify_grads_ready(layer.parameters())     # (recorded on this stream: the reducer's event sits behind the GEMMs)
    _wgrad_keep.append(deferred)

    def _join(stream=ws):
        torch.cuda.current_stream().wait_stream(stream)
        _wgrad_keep.clear()                             # operands may be recycled now: later work is ordered behind the join

    torch.autograd.Variable._execution_engine.queue_callback(_join)


def _wgrad_stream():
    global _wgrad_stream_obj
    if _wgrad_stream_obj is None:
        _wgrad_stream_obj = torch.cuda.Stream()
    return _wgrad_stream_obj


def _switches():
    """The switch values of this moment, for the decisions of paths.py (read per call: tests and bench.py flip them between steps)."""
    return paths.Switches(LAYER_SEQ, STACK_SEQ, STACK_MAX_ROWS, ops.GROUPED_DW, ops.GROUPED_DW_MIN_ROWS, ops.FWD_F16, bool(ops.kernel_timer.names))


def _pair_grad_chain(s, key_tiles):
    """The pair-gradient chain G for logits `s`: fp32, or bf16 under MMDTI_PAIR_G_BF16; zeroed for ragged batches, whose skipped key
    tiles are never written."""
    return (torch.empty if key_tiles is None else torch.zeros)(s.shape, device=s.device, dtype=ops.pair_grad_dtype(s))


def _kept(L, li, plan):
    """What the forward keeps of layer li for the backward: everything, or -- below the lowest layer the backward reaches
    (freeze.plan_tower) -- only the dropout site numbers (the layer above reads the site of the one under it)."""
    if li >= plan.lowest:
        return L
    return SimpleNamespace(site_f=getattr(L, "site_f", None))


class _Sites:
    """Dropout site numbering inside one forward call."""

    def __init__(self):
        self.n = 0

    def next(self):
        self.n += 1
        return self.n


# ------------------------------------------------------------------------------------------------- Uni-Mol pair encoder
# ------------------------------------------------------------------------------------------------- attention maps (read-out)
class AttentionRecorder:
    """What `with record_attention(spec) as rec:` yields.  While it is live, every attention of a requested kind and layer is followed by
    ONE map kernel (ops.pair_attn_map on the layer's stored logits L.s; ops.attn_map on L.q / L.k / L.stats) that writes the
    probabilities, reduced over heads, as [B, Lq, Lk] fp32 -- positional, zeros on padding -- into `maps`:
        maps["unimol"][l] [B,N,N]    maps["bert"][l] [B,L,L]    maps["text_to_graph"][l] [B,L,N]    maps["graph_to_text"][l] [B,N,L]
    spec: which (subset of {"cross", "unimol", "bert"}), layers ("last" | "all" | [ints]), head ("mean" | int).
    counts: {"unimol": [B] int32, "bert": [B] int32} device tensors -- the real atoms / tokens of every sequence of a right-padded batch
    (MM_Model.attention_maps sets them): query rows from there on come out as zeros.  Without them every row of the padded layout is a
    query (packed rows carry their own counts).  cross_layers: {id(layer module): (direction, index, count)}.
    A forward that keeps activations for a backward, or runs a live dropout, is refused before its first launch: the maps describe an
    inference pass (and the small-batch stack path, which only a kept forward takes, is never met)."""
    KINDS = ("cross", "unimol", "bert")

    def __init__(self, which=("cross",), layers="last", head="mean"):
        which = (which,) if isinstance(which, str) else tuple(which)
        bad = [w for w in which if w not in self.KINDS]
        if bad or not which:
            raise ValueError(f"record_attention: which must be a non-empty subset of {self.KINDS} (got {which})")
        if not (layers in ("last", "all") or (isinstance(layers, (list, tuple)) and all(isinstance(i, int) and i >= 0 for i in layers))):
            raise ValueError(f"record_attention: layers must be 'last', 'all' or a list of layer indices (got {layers!r})")
        if not (head == "mean" or (isinstance(head, int) and not isinstance(head, bool) and head >= 0)):
            raise ValueError(f"record_attention: head must be 'mean' or a head index (got {head!r})")
        self.which, self.layers, self.head = which, layers if isinstance(layers, str) else tuple(layers), -1 if head == "mean" else int(head)
        self.maps = {"unimol": {}, "bert": {}, "text_to_graph": {}, "graph_to_text": {}}
        self.counts = {}
        self.cross_layers = {}
        self.keep_operands = False        # tests: also keep what each map kernel read, under operands[name][layer]
        self.operands = {"unimol": {}, "bert": {}, "text_to_graph": {}, "graph_to_text": {}}

    def wants(self, kind, li, n):
        if kind not in self.which:
            return False
        return li == n - 1 if self.layers == "last" else (True if self.layers == "all" else li in self.layers)

    def check(self, where, keep, *drop_ps):
        if keep:
            raise ops.MMDTIError(f"{where}: the attention recorder is live and this forward keeps activations for a backward -- record under "
                                 "torch.no_grad() (MM_Model.attention_maps does)")
        if any(p > 0.0 for p in drop_ps):
            raise ops.MMDTIError(f"{where}: the attention recorder is live under a live dropout -- record in eval mode")

    def _head(self, heads, where):
        if self.head >= heads:
            raise ops.MMDTIError(f"{where}: head {self.head} asked of an attention with {heads} heads")
        return self.head

    def pair(self, li, n, s, B, N, H, ld, key_tiles, pack, padding_mask):
        """tower 1, layer li of n: s is the layer's stored logits.  The two stale-memory rules: a ragged batch's key tiles past a
        molecule's covered count are never read (key_tiles), nor are the query rows from n_real on (packed rows: never stored)."""
        if not self.wants("unimol", li, n):
            return
        n_real = pack.n_real if pack is not None else self.counts.get("unimol")
        if n_real is None and key_tiles is not None:
            n_real = (N - padding_mask.sum(1)).to(torch.int32) if padding_mask is not None else torch.full((B,), N, dtype=torch.int32, device=s.device)
        self.maps["unimol"][li] = ops.pair_attn_map(s, B, N, H, ld, self._head(H, "PairEncoderFn"), key_tiles=key_tiles, n_real=n_real)
        if self.keep_operands:
            self.operands["unimol"][li] = SimpleNamespace(s=s, B=B, N=N, H=H, ld=ld, key_tiles=key_tiles, n_real=n_real)

    def bert(self, st, L):
        """a BERT-style layer whose forward just ran (tower 2 or one direction of the cross block): st.rec_tag names it"""
        tag = st.__dict__.get("rec_tag")
        if tag is None:
            return
        name, li, q_cnt, Lq_out, ld_out = tag
        head = self._head(L.heads, name)
        B, Lq, Lk, D = st.B, st.Lq, st.Lk, st.D
        if L.fused:
            m = ops.attn_map(L.q, L.k, L.key_add, L.stats, B, L.heads, Lq, Lk, 1.0 / math.sqrt(D // L.heads), head, vl=st.vl, q_cnt=q_cnt,
                             Lq_out=Lq_out, ld_out=ld_out)
        else:
            # materialised scores (sequences past the fused kernels' 512 tokens): L.p [B, heads, Lq, ld] bf16, reduced by the same head rule
            # -- heads added in ascending order, times fp32(1 / heads); padded rows only (packed sequences need the fused kernels)
            p = L.p[..., :Lk]
            if head < 0:
                m = p[:, 0].float()
                for h in range(1, L.heads):
                    m = m + p[:, h].float()
                m = m * (1.0 / L.heads)
            else:
                m = p[:, head].float()
            if q_cnt is not None:
                m = m * (torch.arange(Lq, device=m.device).view(1, Lq, 1) < q_cnt.view(B, 1, 1)).to(F32)
            m = m.contiguous()
        self.maps[name][li] = m
        if self.keep_operands:
            self.operands[name][li] = SimpleNamespace(q=L.q, k=L.k, key_add=L.key_add, stats=L.stats if L.fused else None, p=None if L.fused else L.p,
                                                      B=B, heads=L.heads, Lq=Lq, Lk=Lk, vl=st.vl, q_cnt=q_cnt, Lq_out=Lq_out, ld_out=ld_out)


_recorder: Optional[AttentionRecorder] = None


def attention_recorder() -> Optional[AttentionRecorder]:
    """the live recorder, None outside `with record_attention(...)` (a module-level context, like ops.kernel_timer)"""
    return _recorder


@contextlib.contextmanager
def record_attention(spec=None, **kw):
    """`with record_attention(dict(which=("cross",), layers="last", head="mean")) as rec:` -- see AttentionRecorder.  Not re-entrant."""
    global _recorder
    if _recorder is not None:
        raise ops.MMDTIError("record_attention: a recorder is already live")
    rec = spec if isinstance(spec, AttentionRecorder) else AttentionRecorder(**dict(spec or {}, **kw))
    _recorder = rec
    try:
        yield rec
    finally:
        _recorder = None


class PairEncoderFn(torch.autograd.Function):
    """TransformerEncoderWithPair.forward (models/transformers.py:96-183) minus the discarded aux outputs:
    emb-LN -> dropout -> zero padded rows -> L x [pre-LN pair-bias attention + FFN, S chained] -> final LN.

    inputs : emb [B,N,D] fp32, bias [B,H,N,ld] fp32 (ld >= N; standard layout is ld == N) or a tiled pair tensor (fp32, or the
             compact fp16 planes PairBiasFn produces on the hot path), padding_mask [B,N] bool|None
    outputs: x [B,N,D] fp32, S_last in the layout and dtype of bias (pre-softmax logits of the last layer, -inf at padded keys),
             x_pre [B,N,D] fp32 (stream before the final LN; only the discarded x_norm aux output reads it)
    pack (packing.PackedRows, compact tiled bias + key_tiles only): PACKED token rows -- emb / padding_mask / x / x_pre are
             [pack.M, D] / [pack.M]: every molecule's real tokens plus one representative pad row (all pad rows of a molecule
             are the same row at dropout 0); S_last then lacks the query rows past the representative one.
    """

    @staticmethod
    def forward(ctx, emb, bias, padding_mask, mod, training, key_tiles=None, pack=None, aux_grads=False, anchor=None):
        """aux_grads: S_last and x_pre are differentiable outputs (the reference's auxiliary returns -- attn, delta_pair_repr, x_norm,
        delta_pair_repr_norm, models/transformers.py:141-181 -- are functions of them); fp32 pair planes only.  MM_Model discards those
        returns (mm_model.py:559), so the hot path leaves it off and autograd never materialises a gradient for them.
        anchor: freeze.grad_anchor(mod.parameters()) -- the backward runs when a parameter of the tower trains even if neither emb nor
        bias needs a gradient (frozen embedding and pair-bias front end); no gradient is returned for it."""
        if pack is not None:
            B, N, D = pack.B, pack.S, emb.shape[-1]
            if emb.dim() != 2 or emb.shape[0] != pack.M:
                raise ops.MMDTIError("PairEncoderFn: packed rows expect emb [pack.M, D]")
        else:
            B, N, D = emb.shape
        H = mod.attention_heads
        tiled = ops.pair_is_tiled(bias)        # [B,H,nt,nt,256] tile layout (see ops.pair_tile) or row-major [B,H,N,ld]
        compact = tiled and bias.dtype == torch.float16     # logits chain as fp16 (ops.PAIR_COMPACT, PairBiasFn)
        if not compact:
            key_tiles = None                   # (only the compact tiled kernels have a ragged form)
        if pack is not None and key_tiles is None:
            raise ops.MMDTIError("PairEncoderFn: packed rows need the compact tiled pair layout and key_tiles")
        if aux_grads and (compact or pack is not None):
            raise ops.MMDTIError("PairEncoderFn: differentiable auxiliary outputs need fp32 pair planes on padded rows")
        row_off = None if pack is None else pack.off
        # The gradient of a compact (fp16) bias is NOT an fp16 tensor (fp32, or bf16 on request), and autograd casts whatever a
        # backward returns to the dtype of the input.  PairBiasFn therefore hangs a slot on the bias it produces; the backward
        # below leaves the real gradient chain there and hands autograd a zero-storage placeholder.
        slot = getattr(bias, "_mmdti_grad_slot", None) if compact else None
        if compact and slot is None and bias.requires_grad:
            raise ops.MMDTIError("PairEncoderFn: an fp16 pair bias that needs a gradient must come from PairBiasFn")
        ld = ops.pair_ld(N) if tiled else bias.shape[-1]
        M = B * N if pack is None else pack.M
        p_emb = mod.emb_dropout if training else 0.0
        p_res = mod.dropout if training else 0.0
        p_att = mod.attention_dropout if training else 0.0
        seed = dropout_state.next_seed()
        sites = _Sites()
        st = SimpleNamespace(B=B, N=N, D=D, H=H, ld=ld, M=M, seed=seed, p_emb=p_emb, p_res=p_res, p_att=p_att, layers=[], kt=key_tiles, slot=slot,
                             row_off=row_off, packed=pack is not None)
        keep = any(ctx.needs_input_grad)      # inference (torch.no_grad / frozen tower and inputs): nothing is kept for a backward --
                                              # the 15 per-layer logit tensors are freed as the stack advances
        rec = _recorder
        if rec is not None:
            rec.check("PairEncoderFn", keep, p_emb, p_res, p_att)
        if keep:
            # the backward follows the trainable set (freeze.plan_tower): it stops at the lowest layer that trains unless the embedding
            # LayerNorm or emb needs the stream gradient; the pair-gradient chain leaves layer 0 only when the bias needs a gradient
            eln = mod.emb_layer_norm
            st.plan = plan_tower(layer_trainable(mod.layers), ctx.needs_input_grad[0] or eln.weight.requires_grad or eln.bias.requires_grad,
                                 ctx.needs_input_grad[1])
        emb = emb.contiguous()
        st.emb = emb
        st.pad = padding_mask
        st.site_emb = sites.next()
        eln = mod.emb_layer_norm
        x, _, st.emb_mean, st.emb_rstd = ops.layernorm_fwd(emb.view(M, D), eln.weight, eln.bias, eln.eps, want_f32=True, want_bf16=False,
                                                           row_zero=None if padding_mask is None else padding_mask.reshape(-1),
                                                           drop_p=p_emb, seed=seed, site=st.site_emb)
        scale = (D // H) ** -0.5
        s_prev = bias.contiguous()
        st.bias0 = s_prev if not mod.layers else None     # only needed to shape a zero gradient when there is no layer
        # Every Linear that closes a residual branch runs fused with the LayerNorm that reads its output (ops.linear_ln_fwd): out_proj
        # with this layer's final_layer_norm, fc2 with the NEXT layer's self_attn_layer_norm -- or, after the last layer, with the
        # encoder's final_layer_norm.  `nxt` carries that next LayerNorm's output into the next iteration.
        nlayers = len(mod.layers)
        nxt = None
        out = None
        sw = _switches()
        adapters = _has_adapters(mod.layers)
        st.aseq = adapters and _adapter_seq(mod.layers, _self_attn_of)
        path = paths.unimol_layer_fwd(sw, emb.is_cuda, compact, D, H, adapters=adapters, adapter_seq=st.aseq)
        seq = path == paths.LAYER
        kp0 = ops._u8(padding_mask) if seq else None
        # small batches: ALL layers from one library call (see _unimol_stack_fwd); the per-layer loop below then has nothing left to do
        st.stack = None
        T = None
        if paths.unimol_tower_fwd(sw, path, keep, nlayers, M, aux_grads, mod.final_layer_norm is not None, adapters=adapters,
                                  adapter_seq=st.aseq) == paths.STACK:
            T = _lora_stack_tables(False, mod, M, sw) if adapters else _stack_tables(_unimol_stack_desc, mod, M, sw)
        if T is not None:
            x, out, s_prev = _unimol_stack_fwd(st, T, mod, x, s_prev, kp0, pack is None, scale, sites, tiled)
        for li, layer in enumerate(mod.layers if T is None else ()):
            L = SimpleNamespace(x=x)
            ln1, ln2 = layer.self_attn_layer_norm, layer.final_layer_norm
            att = layer.self_attn
            if nxt is None:
                _, L.h1, L.m1, L.r1 = ops.layernorm_fwd(x, ln1.weight, ln1.bias, ln1.eps)
            else:
                L.h1, L.m1, L.r1 = nxt
            if seq:
                # the layer's six launches from ONE library call (csrc/layers.hip: the same kernels, arguments and order as below)
                L.site_att, L.site_o, L.site_f = sites.next(), sites.next(), sites.next()
                last = li == nlayers - 1
                nl = mod.layers[li + 1].self_attn_layer_norm if not last else mod.final_layer_norm
                x, ln_out, mn, rn = _unimol_layer_fwd_seq(st, layer, L, s_prev, kp0 if li == 0 else None, last and pack is None, scale, nl,
                                                          0 if nl is None else (2 if last else 1))
                s_prev = L.s
                if rec is not None:
                    rec.pair(li, nlayers, L.s, B, N, H, ld, key_tiles, pack, padding_mask)
                if not last:
                    nxt = (ln_out, mn, rn)
                elif nl is not None:
                    out, st.f_mean, st.f_rstd = ln_out, mn, rn
                if keep:
                    st.layers.append(_kept(L, li, st.plan))
                continue
            L.qkv = ops.linear_fwd(L.h1, wfwd(att.in_proj.weight), att.in_proj.bias)
            if getattr(att, "lora_targets", None):         # LoRA: q | k | v += s.bf16(h1.A^T).B^T next to the frozen in_proj (lora.py)
                L.lt = ops.lora_fwd(L.h1, wfwd(att.lora_A), wfwd(att.lora_B), L.qkv, att.lora_scale)
            L.site_att = sites.next()
            # (ragged batches: all-padding key tiles are skipped; the last layer writes them as -inf because its S is returned)
            L.s, L.o = ops.pair_attn_fwd(L.qkv, s_prev, padding_mask if li == 0 else None, B, N, H, ld, scale, p_att, seed, L.site_att,
                                         key_tiles=key_tiles, rag_store=(li == nlayers - 1) and pack is None, row_off=row_off)
            s_prev = L.s
            if rec is not None:
                rec.pair(li, nlayers, L.s, B, N, H, ld, key_tiles, pack, padding_mask)
            L.site_o = sites.next()
            L.x1, _, L.h2, L.m2, L.r2 = ops.linear_ln_fwd(L.o, wfwd(att.out_proj.weight), att.out_proj.bias, ln2.weight, ln2.bias, ln2.eps,
                                                          residual=x, drop_p=p_res, seed=seed, site=L.site_o)
            L.u = torch.empty(M, layer.fc1.weight.shape[0], device=emb.device, dtype=BF16)
            L.a = ops.linear_fwd(L.h2, wfwd(layer.fc1.weight), layer.fc1.bias, act=ops.ACT_GELU_FWD, aux_out=L.u)
            L.site_f = sites.next()
            if li + 1 < nlayers:
                nl = mod.layers[li + 1].self_attn_layer_norm
                x, _, h1n, m1n, r1n = ops.linear_ln_fwd(L.a, wfwd(layer.fc2.weight), layer.fc2.bias, nl.weight, nl.bias, nl.eps, residual=L.x1,
                                                        drop_p=p_res, seed=seed, site=L.site_f)
                nxt = (h1n, m1n, r1n)
            elif mod.final_layer_norm is not None:
                fl = mod.final_layer_norm
                x, out, _, st.f_mean, st.f_rstd = ops.linear_ln_fwd(L.a, wfwd(layer.fc2.weight), layer.fc2.bias, fl.weight, fl.bias, fl.eps,
                                                                    residual=L.x1, drop_p=p_res, seed=seed, site=L.site_f, want_f32=True, want_bf16=False)
            else:
                x = ops.linear_fwd(L.a, wfwd(layer.fc2.weight), layer.fc2.bias, residual=L.x1, out_dtype=F32, drop_p=p_res, seed=seed, site=L.site_f)
            if keep:
                st.layers.append(_kept(L, li, st.plan))
        st.x_last = x
        if out is None:
            if mod.final_layer_norm is not None:
                fl = mod.final_layer_norm
                out, _, st.f_mean, st.f_rstd = ops.layernorm_fwd(x, fl.weight, fl.bias, fl.eps, want_f32=True, want_bf16=False)
            else:
                out = x
        if keep:
            ctx.st, ctx.mod = st, mod
        x_last = x.view(B, N, D) if pack is None else x
        if not aux_grads:
            ctx.mark_non_differentiable(s_prev, x_last)
        # (otherwise autograd hands the backward a freshly ZEROED tensor for each output nobody differentiates -- for S_last that is
        #  a 0.55 GB fill per step, found with scratch/fill_diag.py)
        ctx.set_materialize_grads(False)
        return (out.view(B, N, D) if pack is None else out), s_prev, x_last

    @staticmethod
    def backward(ctx, dout, ds_last, dx_pre):
        # ds_last / dx_pre: gradients of the auxiliary outputs (aux_grads; None otherwise -- gradients are not materialised)
        st, mod = ctx.st, ctx.mod
        if getattr(st, "consumed", False):     # (the saved activations are released layer by layer as the backward advances)
            raise ops.MMDTIError("PairEncoderFn: backward through the same forward twice (retain_graph) is not supported")
        st.consumed = True
        B, N, D, H, ld, M, seed = st.B, st.N, st.D, st.H, st.ld, st.M, st.seed
        scale = (D // H) ** -0.5
        if dout is None:                       # (nothing downstream used the encoder output)
            dout = torch.zeros(M, D, device=st.emb.device, dtype=F32)
        dout = dout.contiguous().view(M, D)
        if dx_pre is not None:
            dx_pre = dx_pre.contiguous().view(M, D).float()
        if mod.final_layer_norm is not None:
            fl = mod.final_layer_norm
            nxt = (st.p_res, st.layers[-1].site_f, gbuf(mod.layers[-1].fc2.bias)) if st.layers else None
            if st.stack is not None:
                nxt = (st.p_res, st.stack.site0 + 3 * (st.stack.T.nl - 1) + 2, gbuf(mod.layers[-1].fc2.bias))
            dx = ops.layernorm_bwd(dout, st.x_last, fl.weight, st.f_mean, st.f_rstd, gbuf(fl.weight), gbuf(fl.bias), dres=dx_pre, bf16_copy=nxt)
            dx, dx16 = dx if nxt is not None else (dx, None)
        else:
            dx, dx16 = (dout if dx_pre is None else dout + dx_pre), None
        G = None
        if ds_last is not None:
            # the chain starts from the gradient of the returned logits; padded keys carry none (the reference fills them in place,
            # transformers.py:122-135: no gradient passes a filled entry)
            G = ds_last.to(F32).contiguous().clone()
            if st.pad is not None and not ops.pair_is_tiled(G):
                G.masked_fill_(st.pad.view(B, 1, 1, N), 0.0)
            if G.shape[-1] > N and not ops.pair_is_tiled(G):
                G[..., N:] = 0.0
        if st.stack is not None:
            dx, G = _unimol_stack_bwd(st, dx, dx16, scale)
            notify_grads_ready(st.stack.T.params)
            st.stack = None
        below = [Lb.site_f for Lb in st.layers[:-1]]      # site of the FFN dropout of the layer UNDER each layer
        deferred, deferred_layers = [], []
        # (holding weight gradients back for the end pays where the pair-bias backward has work to hide -- large batches; at a few
        #  thousand rows every launch is latency-bound and the held layers would only miss the sequenced path below)
        n_defer = DEFER_WGRAD_LAYERS if (dout.is_cuda and M >= 8192) else 0
        plan = st.plan
        full = [all(p.requires_grad for p in l.parameters()) for l in mod.layers] if st.layers else []
        aseq = bool(st.layers) and st.aseq and _adapter_seq(mod.layers, _self_attn_of)      # (asked again: flags may have changed since the forward)
        seq_path, seq_ws = _unimol_seq_workspace(st, mod, full, dout.is_cuda, aseq)
        for li, layer, L in zip(range(len(st.layers) - 1, -1, -1), reversed(mod.layers), reversed(st.layers)):
            if li < plan.lowest:                         # nothing at or under this layer trains: the backward stops above it
                L.__dict__.clear()
                continue
            att, ln1, ln2 = layer.self_attn, layer.self_attn_layer_norm, layer.final_layer_norm
            hold = li < n_defer                          # this layer's weight gradients wait for the end (see _launch_deferred_wgrads)
            pending = []                                 # the layer's four weight gradients leave as ONE grouped launch
            lowest = not plan.needs_dx(li)               # the lowest layer that runs, with nothing under it that reads its dx

            def _wgrad(*args, **kw):
                pending.append((args, kw))
            if paths.unimol_layer_bwd(seq_path, dx16 is not None, hold, full[li], adapters=hasattr(L, "lt"), adapter_seq=aseq) == paths.LAYER:
                g_zero = G is None
                if g_zero:
                    G = _pair_grad_chain(L.s, st.kt)
                dx, dx16 = _unimol_layer_bwd_seq(st, layer, L, dx, dx16, G, g_zero, scale, seq_ws,
                                                 None if (li == 0 or lowest) else (below[li - 1], gbuf(mod.layers[li - 1].fc2.bias)), lowest)
                L.__dict__.clear()
                notify_grads_ready(layer.parameters())
                continue
            # ---- FFN:  x2 = x1 + drop(fc2(gelu(fc1(LN2(x1)))))
            # (dx16 = bf16 dropout-backward copy of dx, written by the LayerNorm backward that produced dx)
            dy2 = dx16 if dx16 is not None else ops.cast_bf16(dx, st.p_res, seed, L.site_f)
            _wgrad(dy2, L.a, layer.fc2.weight, layer.fc2.bias, bias_done=dx16 is not None)
            du = ops.linear_bwd_input(dy2, wbf16(layer.fc2.weight), act=ops.ACT_GELU_DX, aux_in=L.u)
            _wgrad(du, L.h2, layer.fc1.weight, layer.fc1.bias)      # (the bias gradient rides on the weight-gradient GEMM)
            dh2 = ops.linear_bwd_input(du, wbf16(layer.fc1.weight))
            dx, dy1 = ops.layernorm_bwd(dh2, L.x1, ln2.weight, L.m2, L.r2, gbuf(ln2.weight), gbuf(ln2.bias), dres=dx,
                                        bf16_copy=(st.p_res, L.site_o, gbuf(att.out_proj.bias)))
            # ---- attention:  x1 = x + drop(out_proj(attn(LN1(x))))
            _wgrad(dy1, L.o, att.out_proj.weight, att.out_proj.bias, bias_done=True)
            do = ops.linear_bwd_input(dy1, wbf16(att.out_proj.weight))
            g_zero = G is None
            if g_zero:
                G = _pair_grad_chain(L.s, st.kt)
            dqkv = ops.pair_attn_bwd(L.qkv, L.s, do, G, B, N, H, ld, scale, g_zero, st.p_att, seed, L.site_att, key_tiles=st.kt, row_off=st.row_off)
            _wgrad(dqkv, L.h1, att.in_proj.weight, att.in_proj.bias)
            lu = _lora_bwd(att, "", L.h1, dqkv, L.lt) if hasattr(L, "lt") else None
            if lowest and not (ln1.weight.requires_grad or ln1.bias.requires_grad):
                dh1 = None                               # (no dX product: nothing reads it)
            else:
                dh1 = ops.linear_bwd_input(dqkv, wbf16(att.in_proj.weight))
                if lu is not None:
                    ops.lora_dx(lu, wbf16(att.lora_A), dh1)
            if dh1 is None:
                dx, dx16 = None, None
            elif lowest or li == 0:                      # (no layer under this one reads a bf16 copy)
                dx, dx16 = ops.layernorm_bwd(dh1, L.x, ln1.weight, L.m1, L.r1, gbuf(ln1.weight), gbuf(ln1.bias), dres=dx), None
            else:
                dx, dx16 = ops.layernorm_bwd(dh1, L.x, ln1.weight, L.m1, L.r1, gbuf(ln1.weight), gbuf(ln1.bias), dres=dx,
                                             bf16_copy=(st.p_res, below[li - 1], gbuf(mod.layers[li - 1].fc2.bias)))
            if hold:
                deferred.append(pending)
                deferred_layers.append(layer)
            else:
                _lin_bwd_params_many(pending)
            L.__dict__.clear()       # release this layer's activations (S_l is ~1 GB at the bench shape)
            if not hold:
                notify_grads_ready(layer.parameters())
        eln = mod.emb_layer_norm
        demb = None
        if plan.below:
            demb = ops.layernorm_bwd(dx, st.emb.view(M, D), eln.weight, st.emb_mean, st.emb_rstd, gbuf(eln.weight), gbuf(eln.bias),
                                     row_zero=None if st.pad is None else st.pad.reshape(-1), drop_p=st.p_emb, seed=seed, site=st.site_emb)
            if not ctx.needs_input_grad[0]:
                demb = None
        notify_grads_ready(list(eln.parameters()) + ([] if mod.final_layer_norm is None else list(mod.final_layer_norm.parameters())))
        if not ctx.needs_input_grad[1]:
            G = None                                                                 # (the pair bias does not train)
        elif G is None:
            G = torch.zeros_like(st.bias0)
        if G is not None and st.slot is not None:
            st.slot.g = G                                                            # -> PairBiasFn.backward (see forward)
            G = torch.zeros((), device=G.device, dtype=torch.float16).expand(G.shape)
        _launch_deferred_wgrads(deferred, deferred_layers)
        _join_stream_after_backward()
        if demb is not None and not st.packed:
            demb = demb.view(B, N, D)
        return demb, G, None, None, None, None, None, None, None


# ---- all layers of the tower behind one library call per direction (csrc/layers.hip: mmdti_unimol_stack_fwd / _bwd).  At the
# reference's batch size (16-32 molecules) the step is paced by the host: the per-layer calls below still cost ~90 us of Python per
# layer and direction (17 allocations, the blocks' marshalling, shadow look-ups).  The stack calls take the parameters as an array of
# layer blocks cached per model and keep the saved tensors at fixed offsets of one arena: one allocation and one call for 15 layers.
# Above MMDTI_STACK_MAX_ROWS rows the GPU sets the pace and the per-layer path (which frees each layer's activations as the
# backward advances and holds the last layers' weight gradients back) stays in charge.
STACK_SEQ = os.environ.get("MMDTI_STACK_SEQ", "1") != "0"
STACK_MAX_ROWS = int(os.environ.get("MMDTI_STACK_MAX_ROWS", "8192"))
# (weight gradients of the stack backward on a side stream, under the layer below: measured at 32 molecules -- 6.92 vs 6.95 ms, no
#  gain, the step is bound by the chip's throughput on small kernels, not by the length of one stream's chain -- so it stays opt-in)
STACK_SIDE_WGRAD = os.environ.get("MMDTI_STACK_SIDE_WGRAD", "0") != "0"
_stack_layouts = {}
_stack_sides = {}


def _ptr_table(ptrs):
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return arr, ctypes.addressof(arr)


def _has_adapters(layers) -> bool:
    """Does a layer of the tower carry LoRA adapters (lora.apply_lora)?  Such layers take the adapted sequencers or run op by op."""
    return any(getattr(getattr(l, "self_attn", None), "lora_targets", None) for l in layers)


def _has_bert_adapters(layers) -> bool:
    return any(getattr(l.attention.self, "lora_targets", None) for l in layers)


_adapter_params = weakref.WeakKeyDictionary()
_adapter_params_gen = [0]          # counts rebuilt entries: the cached tables of the adapted stacks (_lora_stack_tables) are built for one value


def _adapter_seq(layers, att_of, fused_attn=True) -> bool:
    """paths.adapter_seq_ok over `layers` (att_of: a layer's attention module): every one carries adapters, every adapter trains, every
    other parameter is frozen."""
    base, adp = [], []
    for l in layers:
        att = att_of(l)
        tg = getattr(att, "lora_targets", None)
        if not tg:
            return False
        # (a layer's parameters are kept as (owning module's table, name, parameter, is an adapter): walking the modules costs more than the
        #  library call at small batches.  Every call checks that each table still holds that very object under that name -- a parameter
        #  replaced by assignment or load_state_dict(assign=True) builds the entry again -- and new adapters change lora_targets)
        ent = _adapter_params.get(l)
        if ent is None or ent[0] is not tg or any(tab.get(n) is not q for tab, n, q, _ in ent[1]):
            ent = _adapter_params[l] = (tg, [(m._parameters, n, q, n.startswith("lora_")) for m in l.modules() for n, q in m._parameters.items()
                                             if q is not None])
            _adapter_params_gen[0] += 1
        for _, _, q, is_adapter in ent[1]:
            (adp if is_adapter else base).append(q.requires_grad)
    return paths.adapter_seq_ok(LORA_SEQ, base, adp, fused_attn)


_self_attn_of = lambda l: l.self_attn                 # noqa: E731
_bert_attn_of = lambda l: l.attention.self            # noqa: E731


def _lora_pair(att, t):
    """(A, B) of the adapter of projection `t` ('' -- tower 1's fused in_proj --, 'q', 'k', 'v') on an attention module"""
    sfx = f"_{t}" if t else ""
    return getattr(att, "lora_A" + sfx), getattr(att, "lora_B" + sfx)


def _lora_fwd(att, t, x16, y):
    """y (what the frozen projection wrote) += s.bf16(x.A^T).B^T in place -> the saved t"""
    A, B = _lora_pair(att, t)
    return ops.lora_fwd(x16, wfwd(A), wfwd(B), y, att.lora_scale)


def _lora_bwd(att, t, x16, dy, lt):
    """The adapter's gradients into its gradient buffers -> u = bf16(s.dy.B) for ops.lora_dx.  A frozen adapter is refused: it has no
    gradient buffer to write to, and leaving its s.B.A out of the dX product would be wrong -- merge it first."""
    A, B = _lora_pair(att, t)
    gA, gB = gbuf(A), gbuf(B)
    if gA is None or gB is None:
        raise ops.MMDTIError("LoRA: an adapter pair trains or is frozen as a whole, and a frozen one must be merged (lora.merge_lora)")
    return ops.lora_bwd(x16, dy, lt, wbf16(B), gA, gB, att.lora_scale)


def _lora_blocks(att, targets, w16=None, wb=None, g=None):
    """The adapter blocks (mmdti_lora_adapter_t, one per entry of `targets`: ('',) tower 1, ('q', 'k', 'v') otherwise) of an attention
    module as one array; a projection without an adapter keeps r 0.  w16 / wb / g: as _layer_block."""
    S = ops.lib().struct("mmdti_lora_adapter_t")
    blocks = []
    for t in targets:
        f = {}
        if t in att.lora_targets:
            A, B = _lora_pair(att, t)
            f = dict(r=A.shape[0], scale=float(att.lora_scale))
            if w16 is not None:
                f.update(A=w16(A), B=w16(B))
            if g is not None:
                f.update(A_bf16=wb(A), B_bf16=wb(B), dA=g(A), dB=g(B))
        blocks.append(S(**f))
    return blocks


def _block_array(blocks):
    """-> (array, its address) of same-typed blocks"""
    arr = (type(blocks[0]) * len(blocks))(*blocks)
    return arr, ctypes.addressof(arr)


def _split_block(W, w16=None, wb=None):
    """The three separate projections of a BERT-style layer with a frozen base (mmdti_bert_split_t)."""
    f = {}
    for k, w, b in (("q", W.q_w, W.q_b), ("k", W.k_w, W.k_b), ("v", W.v_w, W.v_b)):
        if w16 is not None:
            f["w_" + k], f["b_" + k] = w16(w), ops._p(b)
        if wb is not None:
            f["wb_" + k] = wb(w)
    return ops.lib().struct("mmdti_bert_split_t")(**f)


def _lora_rows(buf, row_bytes, shapes):
    """[rows, r] bf16 views of the rows of a t buffer (uint8; row j at j * row_bytes), one per (rows, r) of `shapes` (None: no adapter)"""
    return [None if sh is None else buf[j * row_bytes:j * row_bytes + sh[0] * sh[1] * 2].view(BF16).view(sh) for j, sh in enumerate(shapes)]


def bert_weights(layer) -> SimpleNamespace:
    """Parameter view of an HF RobertaLayer / mm_module BertCrossAttentionLayer (identical sub-module names)."""
    a, o = layer.attention.self, layer.attention.output
    return SimpleNamespace(layer=layer, att=a, lora=getattr(a, "lora_targets", ()), q_w=a.query.weight, q_b=a.query.bias, k_w=a.key.weight, k_b=a.key.bias, v_w=a.value.weight, v_b=a.value.bias,
                           o_w=o.dense.weight, o_b=o.dense.bias, ln1_w=o.LayerNorm.weight, ln1_b=o.LayerNorm.bias,
                           i_w=layer.intermediate.dense.weight, i_b=layer.intermediate.dense.bias,
                           o2_w=layer.output.dense.weight, o2_b=layer.output.dense.bias,
                           ln2_w=layer.output.LayerNorm.weight, ln2_b=layer.output.LayerNorm.bias)


# ---- What the sequencers take, by NAME: the blocks of include/mmdti_hip.h (run: the same for every layer of one call; layer: one
# layer's parameters; saved: what its forward writes for its backward).  ops.lib().struct(name) is the ctypes class of a header struct:
# a block is built by keyword, so a misspelt field is an AttributeError here and a field left out arrives as null, which the library refuses
# before its first launch.  A call takes the ADDRESS of a block; the block must outlive the call only.
#
# A layer's description (one per tower, for the per-layer and the stack calls alike): lin -- its Linears by field suffix {suffix:
# (weight, bias)}, whose weights the forward reads through the 16-bit shadows; ln -- its LayerNorms {suffix: (weight, bias)}; extra --
# scalar fields; params -- every parameter; recast -- the weights whose shadow is refreshed after an in-place write; probe -- the [F, D]
# weight that shapes the layer and whose bindings are re-checked per call; eps -- LayerNorm epsilons that must all be one value; runs --
# parameters that must sit back to back in the arena (the call reads each run as one matrix / one bias).
def _unimol_stack_desc(l):
    a, ln1, ln2 = l.self_attn, l.self_attn_layer_norm, l.final_layer_norm
    lin = {"in": (a.in_proj.weight, a.in_proj.bias), "out": (a.out_proj.weight, a.out_proj.bias), "fc1": (l.fc1.weight, l.fc1.bias),
           "fc2": (l.fc2.weight, l.fc2.bias)}
    ln = {"ln1": (ln1.weight, ln1.bias), "ln2": (ln2.weight, ln2.bias)}
    return SimpleNamespace(struct="mmdti_unimol_layer_t", lin=lin, ln=ln, extra=dict(eps_ln1=float(ln1.eps), eps_ln2=float(ln2.eps)),
                           params=[q for pair in (*lin.values(), *ln.values()) for q in pair], recast=[w for w, _ in lin.values()], probe=l.fc1.weight,
                           eps=(ln2.eps, ln1.eps), runs=())


def _bert_stack_desc(l):
    W = bert_weights(l)
    # (q_w / q_b: where the fused [3D, D] query | key | value matrix and its bias start)
    lin = {"qkv": (W.q_w, W.q_b), "o": (W.o_w, W.o_b), "i": (W.i_w, W.i_b), "o2": (W.o2_w, W.o2_b)}
    ln = {"ln1": (W.ln1_w, W.ln1_b), "ln2": (W.ln2_w, W.ln2_b)}
    return SimpleNamespace(struct="mmdti_bert_layer_t", lin=lin, ln=ln, extra=dict(lddw_qkv=W.q_w.shape[1]),
                           params=[W.q_w, W.k_w, W.v_w, W.q_b, W.k_b, W.v_b, W.o_w, W.o_b, W.ln1_w, W.ln1_b, W.i_w, W.i_b, W.o2_w, W.o2_b, W.ln2_w, W.ln2_b],
                           recast=(W.q_w, W.k_w, W.v_w, W.o_w, W.i_w, W.o2_w), probe=W.i_w, eps=(),
                           runs=((W.q_w, W.k_w, W.v_w), (W.q_b, W.k_b, W.v_b)))


_unimol_stack_desc.probe = lambda l: l.fc1.weight
_bert_stack_desc.probe = lambda l: l.intermediate.dense.weight


_layer_descs = weakref.WeakKeyDictionary()


def _layer_desc(desc, l):
    """desc(l), kept per layer for the per-layer calls (building one walks two dozen module attributes: 16 us, more than the call it
    feeds at small batches); built again when the probe parameter is no longer the layer's."""
    d = _layer_descs.get(l)
    if d is None or d.probe is not desc.probe(l):
        d = _layer_descs[l] = desc(l)
    return d


def _layer_block(d, w16=None, wb=None, g=None, **extra):
    """One layer's parameter block from its description d (d.struct names the type).  w16 / wb / g: the address of a weight's forward
    shadow, of its bf16 shadow, of a parameter's gradient buffer.  A forward passes w16 alone -- the backward fields stay null --, a
    backward wb and g, the stack calls' cached array all three."""
    p = ops._p
    f = dict(d.extra, **extra)
    for k, (w, b) in d.lin.items():
        if w16 is not None:
            f["w_" + k], f["b_" + k] = w16(w), p(b)
        if g is not None:
            f["wb_" + k], f["dw_" + k], f["db_" + k] = wb(w), g(w), g(b)
    for k, (gm, bt) in d.ln.items():
        f["g_" + k], f["bt_" + k] = p(gm), p(bt)
        if g is not None:
            f["dg_" + k], f["dbt_" + k] = g(gm), g(bt)
    return ops.lib().struct(d.struct)(**f)


# (the per-layer calls look every address up per call, as the op-by-op path does: shadows are re-cast and gradient buffers created on demand)
_w16_ptr = lambda w: wfwd(w).data_ptr()                          # noqa: E731
_wb_ptr = lambda w: wbf16(w).data_ptr()                          # noqa: E731
_grad_ptr = lambda q: 0 if q is None else ops._p(gbuf(q))        # noqa: E731


def _saved_block(name, L, alloc=None, dev=None, **inputs):
    """A layer's saved-tensor block (struct `name`), field by field from the tensor of the same name that L holds; inputs: fields the
    caller owns and L does not keep.  alloc ({field: (shape, dtype)}, the forward): those tensors are allocated onto L first."""
    if alloc is not None:
        for k, (shape, dtype) in alloc.items():
            setattr(L, k, torch.empty(shape, device=dev, dtype=dtype))
    S = ops.lib().struct(name)
    held = L.__dict__
    f = {k: held[k].data_ptr() for k, _ in S._fields_ if held.get(k) is not None}
    f.update((k, ops._p(t)) for k, t in inputs.items())
    return S(**f)


def _ln_max_k():
    return ops.GEMM_LN_MAX_K if ops.GEMM_LN else 0


def _stack_tables(desc, mod, rows, sw, attn_ok=True):
    """The array of a tower's layer blocks for its stack calls (desc: _unimol_stack_desc / _bert_stack_desc; cached on the parameter arena),
    or None when the stack calls do not cover this model or call (paths.stack_call, paths.stack_model)."""
    layers = list(mod.layers)
    probe0 = desc.probe(layers[0])               # (per call: only this one look-up; the descriptions are built on a cache miss)
    arena = getattr(probe0, "_mmdti_arena", None)
    F, D = probe0.shape
    if paths.stack_call(sw, arena is not None, D, F, rows, attn_ok) != paths.STACK:
        return None
    cache = arena.__dict__.setdefault("_stack_tables", {})
    # (a weak reference: an id is recycled once the module dies; the flags: a parameter frozen after the first step must not be written
    #  through the raw gradient fields -- the stack calls take every parameter of every layer as trainable)
    flags = trainable_flags(q for l in layers for q in l.parameters())
    key = (weakref.ref(mod), ops.FWD_F16, desc, flags)
    T = cache.get(key)
    if T is None:
        ds = [desc(l) for l in layers]
        d0 = ds[0]
        off = arena.offsets
        same_arena = all(q is not None and getattr(q, "_mmdti_arena", None) is arena for d in ds for q in d.params)
        uniform = all(tuple(d.probe.shape) == (F, D) and len(list(l.parameters())) == len(d.params) and all(e == d0.eps[0] for e in d.eps)
                      for l, d in zip(layers, ds))
        # (offsets are read only once every parameter is known to have one)
        adjacent = same_arena and all(off[id(q)] == off[id(p)] + p.numel() for d in ds for run in d.runs for p, q in zip(run, run[1:]))
        if paths.stack_model(flags, same_arena, uniform, adjacent) != paths.STACK:
            cache[key] = False
            return None
        if ops.FWD_F16:
            arena._fresh16()
        sh16 = (arena.shadow16 if ops.FWD_F16 else arena.shadow).data_ptr()
        shb, gr = arena.shadow.data_ptr(), arena.grad.data_ptr()
        blocks = [_layer_block(d, w16=lambda q: sh16 + 2 * off[id(q)], wb=lambda q: shb + 2 * off[id(q)], g=lambda q: gr + 4 * off[id(q)]) for d in ds]
        weights = [(q, id(q)) for d in ds for q in d.recast]
        probes = [(d.probe, d.probe.data_ptr(), gr + 4 * off[id(d.probe)]) for d in ds]
        arr = (type(blocks[0]) * len(blocks))(*blocks)
        T = cache[key] = SimpleNamespace(nl=len(layers), D=D, F=F, layers=(arr, ctypes.addressof(arr)), weights=weights,
                                         params=[q for d in ds for q in d.params], f16=ops.FWD_F16, probes=probes)
    if T is False:
        return None
    ver = arena._version
    for q, i in T.weights:                       # an in-place write since the last cast (load_state_dict on a bound model): re-cast
        if q._version != ver[i]:
            arena._fresh(q)
    if T.f16:
        arena._fresh16()
    for q, dptr, gptr in T.probes:               # storage or gradient views re-bound behind our back: the per-layer path looks them up
        g = q.grad
        if g is None or g.data_ptr() != gptr or q.data_ptr() != dptr:
            return None
    return T


def _bert_lora_desc(l):
    """An adapted BERT-style layer's description for _layer_block: the Linears behind the attention (the three projections go in by
    _split_block, the adapters by _lora_blocks)."""
    W = bert_weights(l)
    return SimpleNamespace(struct="mmdti_bert_layer_t", lin={"o": (W.o_w, W.o_b), "i": (W.i_w, W.i_b), "o2": (W.o2_w, W.o2_b)},
                           ln={"ln1": (W.ln1_w, W.ln1_b), "ln2": (W.ln2_w, W.ln2_b)}, extra={}, probe=W.i_w, eps=(), W=W)


def _lora_stack_tables(bert, mod, rows, sw, attn_ok=True):
    """_stack_tables for a tower whose layers all carry adapters next to a frozen base (the caller has asked paths.adapter_seq_ok): the
    layer blocks, the adapter blocks and -- tower 2 (`bert`) -- the split-projection blocks of the adapted stack calls, cached on the
    adapters' arena; None when the stack calls do not cover this model or call.  The adapters are addressed as offsets into their arena,
    like the parameters of _stack_tables.  The frozen base is not: its 16-bit shadows are tensors of their own (runtime.wfwd / wbf16),
    kept alive by the table and re-cast into NEW storage after an in-place write (merge_lora, a checkpoint load), so every call
    compares each base weight's version and address with what the table was built from and builds it again on a difference."""
    layers = list(mod.layers)
    att_of, targets = (_bert_attn_of, ("q", "k", "v")) if bert else (_self_attn_of, ("",))
    att0 = att_of(layers[0])
    probe0 = (_bert_stack_desc if bert else _unimol_stack_desc).probe(layers[0])
    arena = getattr(_lora_pair(att0, att0.lora_targets[0])[0], "_mmdti_arena", None)
    F, D = probe0.shape
    if paths.stack_call(sw, arena is not None, D, F, rows, attn_ok, adapter_seq=True) != paths.STACK:
        return None
    cache = arena.__dict__.setdefault("_lora_stack_tables", {})
    key = (weakref.ref(mod), ops.FWD_F16, bert)
    T = cache.get(key)
    # (the caller's _adapter_seq has just checked every parameter's identity: a replaced one moved the generation)
    if T is not None and T is not False and (T.gen != _adapter_params_gen[0] or any(w._version != v or w.data_ptr() != dp for w, v, dp in T.base)):
        T = None
    if T is None:
        ds = [(_bert_lora_desc if bert else _unimol_stack_desc)(l) for l in layers]
        pairs = [q for l in layers for t in att_of(l).lora_targets for q in _lora_pair(att_of(l), t)]
        off = arena.offsets
        same_arena = all(getattr(q, "_mmdti_arena", None) is arena for q in pairs)
        uniform = all(tuple(d.probe.shape) == (F, D) and all(e == ds[0].eps[0] for e in d.eps) for d in ds)
        if paths.stack_model(trainable_flags(pairs), same_arena, uniform) != paths.STACK:
            cache[key] = False
            return None
        if ops.FWD_F16:
            arena._fresh16()
        sh16 = (arena.shadow16 if ops.FWD_F16 else arena.shadow).data_ptr()
        shb, gr = arena.shadow.data_ptr(), arena.grad.data_ptr()
        keep, base = [], []

        def shadow(cast, record=False):          # a frozen weight's shadow: kept alive; record: the weight's state, once per weight
            def ptr(w):
                t = cast(w)
                keep.append(t)
                if record:
                    base.append((w, w._version, w.data_ptr()))
                return t.data_ptr()
            return ptr
        blocks = [_layer_block(d, w16=shadow(wfwd, True), wb=shadow(wbf16), g=lambda q: 0) for d in ds]
        lora = [b for l in layers for b in _lora_blocks(att_of(l), targets, w16=lambda q: sh16 + 2 * off[id(q)], wb=lambda q: shb + 2 * off[id(q)],
                                                        g=lambda q: gr + 4 * off[id(q)])]
        split = _block_array([_split_block(d.W, w16=shadow(wfwd, True), wb=shadow(wbf16)) for d in ds]) if bert else None
        # (biases and LayerNorm parameters go in by their own fp32 address: watched like the weights)
        for d in ds:
            raw = [b for _, b in d.lin.values()] + [q for pair in d.ln.values() for q in pair] + ([d.W.q_b, d.W.k_b, d.W.v_b] if bert else [])
            base += [(q, q._version, q.data_ptr()) for q in raw if q is not None]
        T = cache[key] = SimpleNamespace(gen=_adapter_params_gen[0], nl=len(layers), D=D, F=F, layers=_block_array(blocks), lora=_block_array(lora), split=split, base=base, keep=keep,
                                         weights=[(q, id(q)) for q in pairs], params=[q for l in layers for q in l.parameters()], f16=ops.FWD_F16,
                                         probes=[(q, q.data_ptr(), gr + 4 * off[id(q)]) for q in pairs])
    if T is False:
        return None
    ver = arena._version
    for q, i in T.weights:                       # an adapter written in place since the last cast (load_lora_state_dict): re-cast
        if q._version != ver[i]:
            arena._fresh(q)
    if T.f16:
        arena._fresh16()
    for q, dptr, gptr in T.probes:               # storage or gradient views re-bound behind our back: the per-layer path looks them up
        g = q.grad
        if g is None or g.data_ptr() != gptr or q.data_ptr() != dptr:
            return None
    return T


_lora_layouts = {}


def _lora_layout(query, *args):
    """The byte counts of the adapted sequencers (mmdti_unimol_lora_stack_layout -> 3, mmdti_bert_lora_stack_layout -> 5: the header says
    which), asked of the library once per shape."""
    key = (query,) + args
    r = _lora_layouts.get(key)
    if r is None:
        out = (ctypes.c_longlong * 5)()
        getattr(ops.lib(), query)(*args, ctypes.addressof(out))
        if len(_lora_layouts) > 4096:
            _lora_layouts.clear()
        r = _lora_layouts[key] = tuple(int(v) for v in out)
    return r


# Byte counts come from the library's own arithmetic (csrc/layers.hip), asked once per shape.  A Uni-Mol layer and a BERT self-attention
# layer hand the grouped weight-gradient launch the same set of matrices -- four of [D, D] (in_proj's three and out_proj; query, key, value
# and the output dense) and two of [F, D] -- whose split-K partial sums take one fp32 slab per split.
def _dw_slab_bytes(D, F, rows):
    tiles = (D // 256) * (F // 256) * 2 + (D // 256) ** 2 * 4
    return ops.lib()._dll.mmdti_linear_dw_grouped_splits(tiles, rows) * (2 * D * F + 4 * D * D) * 4


def _attn_stat_rows(st, heads):
    """Rows of the fused attention's per-row statistics."""
    return heads * st.Mq if st.vl is not None else st.B * heads * st.Lq


def _stack_layout(query, rows, D, F, *sizes):
    """-> (arena bytes per layer, stack workspace bytes, weight-gradient slab bytes, workspace bytes of ONE layer's backward [, of a cross
    layer's]) of a tower's sequencers, asked of the library (`query`: mmdti_unimol_stack_layout / mmdti_bert_stack_layout; sizes: its own
    arguments) once per shape."""
    key = (query, rows, D, F) + sizes
    r = _stack_layouts.get(key)
    if r is None:
        slab = _dw_slab_bytes(D, F, rows)
        out = (ctypes.c_longlong * 4)()
        getattr(ops.lib(), query)(rows, D, F, *sizes, slab, ctypes.addressof(out))
        if len(_stack_layouts) > 4096:
            _stack_layouts.clear()
        r = _stack_layouts[key] = (int(out[0]), int(out[1]), slab, int(out[2]), int(out[3]))
    return r


def _layer_workspace(nbytes, dev):
    """-> (tensor, 256-byte aligned address, bytes) of one layer's backward workspace."""
    ws = torch.empty(nbytes + 256, device=dev, dtype=torch.uint8)
    return ws, (ws.data_ptr() + 255) // 256 * 256, nbytes


def _stack_side():
    """(stream handle, address of the three events) for the side-stream weight gradients of a stack backward, or (0, 0)."""
    if not STACK_SIDE_WGRAD or torch.cuda.is_current_stream_capturing():
        return 0, 0
    main = torch.cuda.current_stream()
    key = (main.device.index, main.cuda_stream)
    ent = _stack_sides.get(key)
    if ent is None:
        side = torch.cuda.Stream(device=main.device)
        evs = [torch.cuda.Event() for _ in range(3)]
        for e in evs:
            e.record(main)                       # (creates the hipEvent_t behind the handle)
        ent = _stack_sides[key] = (side, evs, _ptr_table([e.cuda_event for e in evs]))
    return ops.det_register(ent[0].cuda_stream), ent[2][1]


def _unimol_run(st, F, layout, scale, f16):
    """Tower 1's run block for one direction of one call (layout: the pair tensors' code for that direction)."""
    return ops.lib().struct("mmdti_unimol_run_t")(
        key_tiles=ops._p(st.kt), row_off=ops._p(st.row_off), seed=int(st.seed), M=st.M, B=st.B, N=st.N, H=st.H, D=st.D, F=F, ld=st.ld, pair_layout=layout,
        act_fwd=ops.ACT_GELU_FWD, act_dx=ops.ACT_GELU_DX, ln_max_k=_ln_max_k(), fwd_f16=int(f16), scale=float(scale), p_res=float(st.p_res),
        p_att=float(st.p_att))


def _unimol_stack_fwd(st, T, mod, x, s_prev, key_pad, rag_store_last, scale, sites, tiled):
    """All layers' forward as ONE library call -> (x_last fp32, final LayerNorm output fp32, S of the last layer)."""
    M, D, F, B, N, H, ld = st.M, st.D, T.F, st.B, st.N, st.H, st.ld
    dev = x.device
    ln1, fl = mod.layers[0].self_attn_layer_norm, mod.final_layer_norm
    _, h1, m1, r1 = ops.layernorm_fwd(x, ln1.weight, ln1.bias, ln1.eps)
    e = torch.empty
    s_last = torch.empty_like(s_prev) if tiled else e(B, H, N, ld, device=dev, dtype=F32)
    s_bytes = s_last.numel() * s_last.element_size()
    lora = getattr(T, "lora", None)              # (_lora_stack_tables: adapted layers on a frozen base)
    if lora is not None:
        stride, ws_bytes, slab = _lora_layout("mmdti_unimol_lora_stack_layout", M, D, F, s_bytes)[:2] + (0,)
    else:
        stride, ws_bytes, slab = _stack_layout("mmdti_unimol_stack_layout", M, D, F, s_bytes)[:3]
    arena = e(stride * T.nl, device=dev, dtype=torch.uint8)
    x_last, out = e(M, D, device=dev, dtype=F32), e(M, D, device=dev, dtype=F32)
    st.f_mean, st.f_rstd = e(M, device=dev, dtype=F32), e(M, device=dev, dtype=F32)
    site0 = sites.n + 1
    sites.n += 3 * T.nl
    f16 = h1.dtype == torch.float16
    run = _unimol_run(st, F, ops._pair_layout_s(s_prev, "pair_attn.bias"), scale, f16)
    rest = (T.nl, site0, x.data_ptr(), h1.data_ptr(), s_prev.data_ptr(), ops._p(key_pad), int(rag_store_last), fl.weight.data_ptr(), fl.bias.data_ptr(),
            float(fl.eps), arena.data_ptr(), arena.numel(), s_bytes, x_last.data_ptr(), s_last.data_ptr(), out.data_ptr(), st.f_mean.data_ptr(),
            st.f_rstd.data_ptr())
    if lora is not None:
        ops.lib().mmdti_unimol_lora_stack_fwd(ops._stream(), ctypes.addressof(run), T.layers[1], lora[1], *rest)
    else:
        ops.lib().mmdti_unimol_stack_fwd(ops._stream(), ctypes.addressof(run), T.layers[1], *rest)
    st.stack = SimpleNamespace(T=T, arena=arena, s_bytes=s_bytes, ws_bytes=ws_bytes, slab=slab, site0=site0, x0=x, h1=h1, m1=m1, r1=r1, s_last=s_last, f16=f16)
    return x_last, out, s_last


def _unimol_stack_bwd(st, dx, dx16, scale):
    """All layers' backward as ONE library call -> (gradient of the stream entering layer 0, pair-gradient chain G)."""
    S = st.stack
    T = S.T
    G = _pair_grad_chain(S.s_last, st.kt)
    run = _unimol_run(st, T.F, ops._pair_layout_s(S.s_last, "pair_attn_bwd.s") | (4 if G.dtype == BF16 else 0), scale, S.f16)
    lora = getattr(T, "lora", None)
    # (adapted layers: nothing under layer 0 may read its input gradient -- the lowest layer's dX products are then not launched)
    dx_final = torch.empty_like(dx) if (lora is None or st.plan.needs_dx(0)) else None
    ws = torch.empty(S.ws_bytes, device=dx.device, dtype=torch.uint8)
    rest = (T.nl, S.site0, dx.data_ptr(), dx16.data_ptr(), ops._p(dx_final), S.x0.data_ptr(), S.h1.data_ptr(), S.m1.data_ptr(), S.r1.data_ptr(),
            S.s_last.data_ptr(), G.data_ptr(), 1, S.arena.data_ptr(), S.arena.numel(), S.s_bytes, ws.data_ptr(), ws.numel())
    if lora is not None:
        ops.lib().mmdti_unimol_lora_stack_bwd(ops._stream(), ctypes.addressof(run), T.layers[1], lora[1], *rest)
    else:
        side, events = _stack_side()
        ops.lib().mmdti_unimol_stack_bwd(ops._stream(), ctypes.addressof(run), T.layers[1], *rest, S.slab, side, events)
    return dx_final, G


def _unimol_layer_fwd_seq(st, layer, L, s_prev, key_pad, rag_store, scale, nl, next_mode):
    """One Uni-Mol layer's forward as ONE library call (csrc/layers.hip); fills L with the tensors the backward reads and returns
    (x_out fp32, LayerNorm output of x_out | None, its mean, its rstd)."""
    M, D, F = st.M, st.D, layer.fc1.weight.shape[0]
    dev = L.x.device
    e = torch.empty
    a16 = L.h1.dtype                          # bf16, or fp16 (fp16 forward operands): the type of every forward GEMM input of the layer
    if st.__dict__.get("run") is None:        # (one run block serves every layer of this forward)
        st.run = _unimol_run(st, F, ops._pair_layout_s(s_prev, "pair_attn.bias"), scale, a16 == torch.float16)
    L.s = torch.empty_like(s_prev) if ops.pair_is_tiled(s_prev) else e(st.B, st.H, st.N, st.ld, device=dev, dtype=F32)
    saved = _saved_block("mmdti_unimol_saved_t", L, dev=dev, alloc=dict(
        qkv=((M, 3 * D), a16), o=((M, D), a16), x1=((M, D), F32), h2=((M, D), a16), m2=((M,), F32), r2=((M,), F32), u=((M, F), BF16), a=((M, F), a16)))
    P = _layer_block(_layer_desc(_unimol_stack_desc, layer), w16=_w16_ptr)
    x_out = e(M, D, device=dev, dtype=F32)
    ln_out = mn = rn = None
    if next_mode:
        ln_out = e(M, D, device=dev, dtype=a16 if next_mode == 1 else F32)
        mn, rn = e(M, device=dev, dtype=F32), e(M, device=dev, dtype=F32)
    p = ops._p
    head = (ops._stream(), ctypes.addressof(st.run), ctypes.addressof(P), ctypes.addressof(saved))
    rest = (int(L.site_att), int(L.site_o), int(L.site_f), s_prev.data_ptr(), p(key_pad), int(rag_store), next_mode, p(nl.weight) if nl is not None else 0,
            p(nl.bias) if nl is not None else 0, float(nl.eps) if nl is not None else 0.0, x_out.data_ptr(), p(ln_out), p(mn), p(rn))
    att = layer.self_attn
    if getattr(att, "lora_targets", None):       # an adapted layer on a frozen base (paths.adapter_seq_ok): L.lt is the adapter's saved t
        L.lt = e(M, att.lora_A.shape[0], device=dev, dtype=BF16)
        ad = _block_array(_lora_blocks(att, ("",), w16=_w16_ptr))
        ops.lib().mmdti_unimol_lora_layer_fwd(*head, ad[1], L.lt.data_ptr(), *rest)
    else:
        ops.lib().mmdti_unimol_layer_fwd(*head, *rest)
    return x_out, ln_out, mn, rn


def _unimol_seq_workspace(st, mod, full, on_gpu, adapter_seq=False):
    """-> (paths.LAYER, workspace) when layers of this backward may take mmdti_unimol_layer_bwd (paths.unimol_tower_bwd; full: per layer,
    every parameter trains; adapter_seq: adapted layers on a frozen base -- mmdti_unimol_lora_layer_bwd), else (paths.OPS, None).  The
    workspace holds one layer's temporaries and is shared by all layers."""
    nkept, lowest = len(st.layers), st.plan.lowest
    D, F, M = st.D, (mod.layers[0].fc1.weight.shape[0] if nkept else 0), st.M
    L0 = st.layers[lowest] if lowest < nkept else None          # (the lowest layer that runs: what the forward kept of it)
    path = paths.unimol_tower_bwd(_switches(), on_gpu, nkept, lowest, L0 is not None and L0.h1.dtype == torch.float16,
                                  L0 is not None and L0.s.dtype == torch.float16, D, F, M, full, adapter_seq=adapter_seq)
    if path != paths.LAYER:
        return path, None
    if adapter_seq:
        return path, _layer_workspace(_lora_layout("mmdti_unimol_lora_stack_layout", M, D, F, 0)[2], st.emb.device)
    return path, _layer_workspace(_stack_layout("mmdti_unimol_stack_layout", M, D, F, 0)[3], st.emb.device)


def _unimol_layer_bwd_seq(st, layer, L, dx, dx16, G, g_zero, scale, ws, below, lowest=False):
    """One Uni-Mol layer's backward as ONE library call (csrc/layers.hip): -> (dx, dx16) for the layer below (dx16 None at the
    lowest layer).  Same launches, arguments and order as the op-by-op body of PairEncoderFn.backward.  An adapted layer (L.lt) takes
    mmdti_unimol_lora_layer_bwd; lowest: nothing reads its input gradient -> (None, None)."""
    M, D, F = st.M, st.D, layer.fc1.weight.shape[0]
    adapted = hasattr(L, "lt")
    dx_out = None if (adapted and lowest) else torch.empty_like(dx)
    dx16_out = torch.empty(M, D, device=dx.device, dtype=BF16) if below is not None else None
    if st.__dict__.get("run_bwd") is None:    # (one run block serves every layer of this backward: G's type is known from the first on)
        st.run_bwd = _unimol_run(st, F, ops._pair_layout_s(L.s, "pair_attn_bwd.s") | (4 if G.dtype == BF16 else 0), scale, L.h1.dtype == torch.float16)
    saved = _saved_block("mmdti_unimol_saved_t", L)
    P = _layer_block(_layer_desc(_unimol_stack_desc, layer), wb=_wb_ptr, g=_grad_ptr)
    p = ops._p
    head = (ops._stream(), ctypes.addressof(st.run_bwd), ctypes.addressof(P), ctypes.addressof(saved))
    rest = (int(below[0]) if below is not None else 0, int(L.site_o), int(L.site_att), dx.data_ptr(), dx16.data_ptr(), p(dx_out), p(dx16_out),
            p(below[1]) if below is not None else 0, G.data_ptr(), int(g_zero), ws[1], ws[2])
    if adapted:
        ad = _block_array(_lora_blocks(layer.self_attn, ("",), wb=_wb_ptr, g=_grad_ptr))
        ops.lib().mmdti_unimol_lora_layer_bwd(*head, ad[1], L.lt.data_ptr(), *rest)
    else:
        ops.lib().mmdti_unimol_layer_bwd(*head, *rest)
    return dx_out, dx16_out


# ------------------------------------------------------------------------------------------------- Gaussian pair bias
class PairBiasFn(torch.autograd.Function):
    """gbf -> gbf_proj -> permute (models/mm_model.py:553-556): (dist [B,N,N] f32, edge_type [B,N,N] i64) ->
    bias [B,H,N,ld] fp32 -- or, on the fused hot path (K = F = 128, H = 64, N <= 272), the tiled pair layout, as fp16 unless
    MMDTI_PAIR_COMPACT=0.  The gradient chain of a compact bias is fp32 (or bf16), not fp16: PairEncoderFn.backward leaves it
    in the slot hung on the bias (``_mmdti_grad_slot``) and autograd only carries a placeholder; a gradient that reaches this
    function through autograd from any other consumer is added on top.

    Coords form (``coords=(V, pad_idx)``, edge_type None): ``dist`` is the batch's atom records ([B,N,4] int32, ops.pair_records) and no
    [B,N,N] input exists -- on the hot path (fused forward + complete backward) the kernels derive each pair from its two atoms and the
    records are what the backward keeps; every other configuration materialises the two planes once (ops.pair_inputs_from_records,
    the same pair rule, so no bit depends on which way a configuration went) and runs the planes path below on them."""

    @staticmethod
    def forward(ctx, anchor, dist, edge_type, gbf, proj, ld, key_tiles_host=None, rows_host=None, coords=None):
        # anchor: freeze.grad_anchor over gbf and proj (None when both are frozen): autograd reaches the backward whenever one of
        # them trains, whichever one it is
        # key_tiles_host ([B] ints on the HOST, ragged batches): real key tiles per molecule -- the fused compact path then
        # neither produces the bias of the all-padding key tiles nor visits them in the backward (PairEncoderFn skips them too)
        B, N, _ = dist.shape
        H = proj.linear2.weight.shape[0]
        args = [gbf.mul.weight.view(-1), gbf.bias.weight.view(-1), gbf.means.weight.view(-1), gbf.stds.weight.view(-1)]
        fused = ops.gbf_bias_eligible(args[2].numel(), proj.linear1.weight.shape[0], H, ld)
        # the complete backward kernel recomputes basis / hidden from the inputs: the forward then saves nothing
        full = fused and ops.GBF_FULL_BWD and args[0].numel() <= ops.GBF_FULL_MAXE
        rec = None
        if coords is not None:
            if coords[0] * coords[0] != args[0].numel():
                raise ops.MMDTIError(f"PairBiasFn: coords mode needs V * V edge types, got V = {coords[0]} and tables of {args[0].numel()}")
            if full:
                rec, dist = dist.contiguous(), None
            else:      # no coords kernel for this configuration: the planes, once (int64 for the unfused kernels)
                dist, edge_type = ops.pair_inputs_from_records(dist.contiguous(), coords[0], coords[1], torch.int16 if fused else torch.int64)
        if rec is None:
            dist, edge_type = dist.contiguous(), edge_type.contiguous()
        if rec is None and edge_type.dtype != torch.int64 and not fused:
            edge_type = edge_type.long()      # (the unfused kernels read the reference's int64)
        dev = (rec if rec is not None else dist).device
        if fused:
            # one kernel from distances to the [B,H,N,ld] bias (tiled pair layout whenever the MFMA pair-attention kernels can
            # take it: their loads become contiguous KiBs); without the complete backward kernel the three [P,128] intermediates
            # are kept for the backward
            keep = any(ctx.needs_input_grad) and not full  # inference: the kernel does not even write the intermediates
            tiled = ops.pair_tiled_ok(N)
            compact = tiled and ops.PAIR_COMPACT
            pre_f = pre_b = rb_f = rb_b = None
            if key_tiles_host is not None and compact and full:
                # (rows_host -- packed token rows: the bias of the query rows past a molecule's representative pad row is never read)
                if rows_host is not None:
                    pre_f, pre_b, rb_f, rb_b = ops.gbf_tile_prefixes(key_tiles_host, N, dev, rows_host)
                else:
                    pre_f, pre_b = ops.gbf_tile_prefixes(key_tiles_host, N, dev)
            if rec is not None:
                out, saved = ops.gbf_bias_fwd_coords(rec, coords[0], coords[1], *args, wbf16(proj.linear1.weight), proj.linear1.bias, wbf16(proj.linear2.weight),
                                                     proj.linear2.bias, ld, tiled=tiled, compact=compact, tile_prefix=pre_f, row_blocks=rb_f), None
            else:
                out, saved = ops.gbf_bias_fwd(dist, edge_type, *args, wbf16(proj.linear1.weight), proj.linear1.bias,
                                              wbf16(proj.linear2.weight), proj.linear2.bias, ld, save=keep, tiled=tiled,
                                              save_grad=ops.GELU_SAVE_GRAD, compact=compact, tile_prefix=pre_f, row_blocks=rb_f)
            feat, u, h = saved if keep else (None, None, None)
            ugrad = ops.GELU_SAVE_GRAD
        else:
            feat = ops.gbf_features_fwd(dist, edge_type, *args)
            u = torch.empty(feat.shape[0], proj.linear1.weight.shape[0], device=dist.device, dtype=BF16)
            h = ops.linear_fwd(feat, wbf16(proj.linear1.weight), proj.linear1.bias, act=ops.ACT_GELU_FWD, aux_out=u)
            ugrad = ops.GELU_SAVE_GRAD
            o = ops.linear_fwd(h, wbf16(proj.linear2.weight), proj.linear2.bias, out_dtype=F32)
            out = ops.pair_permute_fwd(o, B, N, H, ld)
        ctx.st = SimpleNamespace(rec=rec, coords=coords, dist=dist, et=edge_type, feat=feat, u=u, h=h, B=B, N=N, H=H, ld=ld, fused=fused, ugrad=ugrad, full=full, slot=None,
                                 pre_b=pre_b if fused else None, rb_b=rb_b if fused else None)
        ctx.gbf, ctx.proj = gbf, proj
        if out.dtype == torch.float16:
            ctx.st.slot = out._mmdti_grad_slot = SimpleNamespace(g=None)
        return out

    @staticmethod
    def backward(ctx, g):
        st, gbf, proj = ctx.st, ctx.gbf, ctx.proj
        ps = [gbf.mul.weight, gbf.bias.weight, gbf.means.weight, gbf.stds.weight]
        if st.slot is not None:
            # compact bias: the gradient chain sits in the slot (PairEncoderFn.backward); what autograd delivered is a
            # zero-storage placeholder unless another consumer of the bias contributed a real fp16 gradient
            real = any(sd != 0 for sd in g.stride())
            chain, st.slot.g = st.slot.g, None
            if chain is None:
                g = g.float()
            elif real:
                g = chain.float().add_(g) if chain.dtype != F32 else chain.add_(g)
            else:
                g = chain
        if st.full:
            # ONE kernel: recompute, both dX products, GELU', the Gaussian backward and all four weight / bias gradients
            l1, l2 = proj.linear1, proj.linear2
            allp = [l1.weight, l1.bias, l2.weight, l2.bias] + ps
            grads = [gbuf(p) if p.requires_grad else torch.zeros_like(p) for p in allp]
            if st.rec is not None:
                ops.gbf_bias_bwd_full_coords(g.contiguous(), st.rec, st.coords[0], st.coords[1], *[p.view(-1) for p in ps], wbf16(l1.weight), l1.bias,
                                             wbf16(l2.weight), st.ld, *[gr.view(-1) for gr in grads], tile_prefix=st.pre_b, row_blocks=st.rb_b)
            else:
                ops.gbf_bias_bwd_full(g.contiguous(), st.dist, st.et, *[p.view(-1) for p in ps], wbf16(l1.weight), l1.bias, wbf16(l2.weight),
                                      st.ld, *[gr.view(-1) for gr in grads], tile_prefix=st.pre_b, row_blocks=st.rb_b)
        elif st.fused and ps[0].numel() <= 4096:
            # one pass over G: re-layout, both dX products, GELU' and the Gaussian backward; only the two weight-gradient
            # GEMMs (contraction over all pairs) and their column sums remain
            grads = [gbuf(p) if p.requires_grad else torch.zeros_like(p) for p in ps]
            do, du = ops.gbf_bias_bwd(g.contiguous(), st.dist, st.et, *[p.view(-1) for p in ps], wbf16(proj.linear1.weight),
                                      wbf16(proj.linear2.weight), st.u, st.ld, *[gr.view(-1) for gr in grads], u_is_grad=st.ugrad)
            _lin_bwd_params(do, st.h, proj.linear2.weight, proj.linear2.bias)
            _lin_bwd_params(du, st.feat, proj.linear1.weight, proj.linear1.bias)
        else:
            do = ops.pair_permute_bwd(g.contiguous(), st.B, st.N, st.H, st.ld)          # [P,H] bf16
            _lin_bwd_params(do, st.h, proj.linear2.weight, proj.linear2.bias)
            du = ops.linear_bwd_input(do, wbf16(proj.linear2.weight), act=ops.ACT_MUL_AUX if st.ugrad else ops.ACT_GELU_BWD, aux_in=st.u)
            _lin_bwd_params(du, st.feat, proj.linear1.weight, proj.linear1.bias)
            dfeat = ops.linear_bwd_input(du, wbf16(proj.linear1.weight))
            if any(p.requires_grad for p in ps):
                grads = [gbuf(p) if p.requires_grad else torch.zeros_like(p) for p in ps]
                ops.gbf_features_bwd(st.dist, st.et, *[p.view(-1) for p in ps], dfeat, *[gr.view(-1) for gr in grads])
        notify_grads_ready(list(gbf.parameters()) + list(proj.parameters()))
        _join_stream_after_backward()
        return None, None, None, None, None, None, None, None, None


class PairCompactFn(torch.autograd.Function):
    """Row-major fp32 pair bias [B,H,N,ld] -> the compact tiled planes (fp16, -inf in every pad slot, gradient slot attached) that
    the ragged / packed pair-attention kernels stream.  Layout glue (plain indexing) for configurations the fused pair-bias kernel
    is not built for (head / basis counts other than 64 / 128): the hot path gets this layout straight from PairBiasFn."""

    @staticmethod
    def forward(ctx, bias, N):
        out = ops.pair_tile(bias[..., :N].float().clamp(max=65504.0), N).to(torch.float16)
        ctx.N, ctx.ld = N, bias.shape[-1]
        ctx.slot = out._mmdti_grad_slot = SimpleNamespace(g=None)
        return out

    @staticmethod
    def backward(ctx, g):
        chain, ctx.slot.g = ctx.slot.g, None
        real = any(sd != 0 for sd in g.stride())
        if chain is None:
            chain = g.float()
        elif real:
            chain = chain.float() + g.float()
        d = ops.pair_untile(chain.float(), ctx.N)
        if ctx.ld != ctx.N:
            d = torch.nn.functional.pad(d, (0, ctx.ld - ctx.N))
        return d, None


class EmbeddingFn(torch.autograd.Function):
    """nn.Embedding with padding_idx (mm_model.py:439-441,552)."""

    @staticmethod
    def forward(ctx, weight, ids, padding_idx):
        ctx.ids, ctx.w, ctx.pad = ids.contiguous(), weight, -1 if padding_idx is None else padding_idx
        return ops.embedding_fwd(ctx.ids, weight)

    @staticmethod
    def backward(ctx, dout):
        g = gbuf(ctx.w)
        if g is not None:
            ops.embedding_bwd_gemm(ctx.ids, ops.cast_bf16(dout.contiguous()), g, ctx.pad)
        notify_grads_ready([ctx.w])
        _join_stream_after_backward()
        return None, None, None


# ------------------------------------------------------------------------------------------------- BERT-style layer
def _bert_layer_fwd(st, s1_32, s1_16, s2_16, key_add, W, heads, p_hid, p_att, eps, seed, sites, self_attn):
    """Post-LN BERT layer with query from s1 and key/value from s2 (HF RobertaLayer; BertCrossAttentionLayer
    mm_module.py:615-626).  s1_32: [B*Lq,D] fp32; s1_16/s2_16 bf16; key_add [B,Lk] fp32.  Returns (out32, out16).
    Packed sequences (st.vl, an ops.AttnVarlen): the row arrays hold st.Mq / st.Mk packed rows instead of B*Lq / B*Lk, the keys of
    a sequence are its real rows only (key_add is None), Lq / Lk are the longest sequences."""
    B, Lq, Lk, D = st.B, st.Lq, st.Lk, st.D
    Mq, vl = st.Mq, st.vl
    hd = D // heads
    ld = (Lk + 7) // 8 * 8
    L = SimpleNamespace(s1_16=s1_16, s2_16=s2_16, ld=ld, heads=heads, self_attn=self_attn, W=W, eps=eps)
    L.site_att = sites.next()
    L.key_add, L.fused = key_add, ops.attn_eligible(Lq, Lk, hd, D)
    if not L.fused:
        ops.warn_unfused_length(Lq, Lk)
    # query/key/value as ONE GEMM when their parameters sit back to back in the arena (trainer._qkv_groups) and the fused
    # attention kernels (which take row-strided q/k/v) run: [3D, D] for self-attention, [2D, D] (key|value) otherwise
    L.fw = L.fb = None
    if L.fused and W.q_b is not None:
        plist_w, plist_b = ((W.q_w, W.k_w, W.v_w), (W.q_b, W.k_b, W.v_b)) if self_attn else ((W.k_w, W.v_w), (W.k_b, W.v_b))
        L.fw, L.fb = fused_views(plist_w), fused_views(plist_b)
        if L.fw is None or L.fb is None:
            L.fw = L.fb = None
    if W.lora and L.fw is not None:
        raise ops.MMDTIError("LoRA: an adapted projection must be frozen (lora.apply_lora freezes its tower; merge_lora before unfreezing)")
    aseq = bool(W.lora) and _adapter_seq((W.layer,), _bert_attn_of, L.fused and W.q_b is not None)
    L.path = paths.bert_layer_fwd(_switches(), self_attn, L.fw is not None, s1_32.is_cuda, D, W.i_w.shape[0], Mq, adapters=bool(W.lora), adapter_seq=aseq)
    if L.path == paths.LAYER:
        # the layer's six launches from ONE library call (csrc/layers.hip: the same kernels, arguments and order as below)
        ret = (_bert_layer_fwd_seq if self_attn else _bert_cross_layer_fwd_seq)(st, L, s1_32, s1_16, key_add, W, heads, p_hid, p_att, eps, seed, sites)
        if _recorder is not None:
            _recorder.bert(st, L)
        return ret
    if L.fw is not None:
        if self_attn:
            # (L.fw[3]: the forward-GEMM shadow of the fused weights; q, k, v are stored bf16 in every mode -- the attention kernels'
            #  operand type)
            L.qkv = ops.linear_fwd(s1_16, L.fw[3], L.fb[1], out_dtype=BF16)
            L.q, L.k, L.v = L.qkv[:, :D], L.qkv[:, D:2 * D], L.qkv[:, 2 * D:]
        else:
            L.q = ops.linear_fwd(s1_16, wfwd(W.q_w), W.q_b, out_dtype=BF16)
            L.qkv = ops.linear_fwd(s2_16, L.fw[3], L.fb[1], out_dtype=BF16)
            L.k, L.v = L.qkv[:, :D], L.qkv[:, D:]
    else:
        L.q = ops.linear_fwd(s1_16, wfwd(W.q_w), W.q_b, out_dtype=BF16)
        L.k = ops.linear_fwd(s2_16, wfwd(W.k_w), W.k_b, out_dtype=BF16)
        L.v = ops.linear_fwd(s2_16, wfwd(W.v_w), W.v_b, out_dtype=BF16)
        if W.lora:                                          # LoRA next to the frozen projections (lora.py)
            L.lt = {t: _lora_fwd(W.att, t, s1_16 if t == "q" else s2_16, {"q": L.q, "k": L.k, "v": L.v}[t]) for t in W.lora}
    if L.fused:
        # scores, softmax, dropout and context in one kernel: the [B,heads,Lq,Lk] tensor never reaches HBM
        L.ctx, L.stats = ops.attn_dispatch(Lq, Lk)[0](L.q, L.k, L.v, key_add, B, heads, Lq, Lk, 1.0 / math.sqrt(hd), p_att, seed, L.site_att, vl=vl)
    else:
        if vl is not None:
            raise ops.MMDTIError("packed sequences need the fused attention kernels (head_dim 16 / 32 / 64, at most 512 tokens)")
        S = torch.empty(B, heads, Lq, ld, device=s1_32.device, dtype=F32)
        ops.gemm(L.q, L.k, M=Lq, N=Lk, K=hd, lda=D, ldb=D, out=S, ldc=ld, batch=(B, heads), sA=(Lq * D, hd), sB=(Lk * D, hd),
                 sC=(heads * Lq * ld, Lq * ld), alpha=1.0 / math.sqrt(hd))
        L.p, L.pd = ops.softmax_fwd(S, key_add, B, heads, Lq, Lk, ld, p_att, seed, L.site_att)
        del S
        L.ctx = torch.empty(B * Lq, D, device=s1_32.device, dtype=ops.act16())
        ops.gemm(L.pd, L.v, M=Lq, N=hd, K=Lk, lda=ld, ldb=D, transB=True, out=L.ctx, ldc=D, batch=(B, heads),
                 sA=(heads * Lq * ld, Lq * ld), sB=(Lk * D, hd), sC=(Lq * D, hd))
    if _recorder is not None:
        _recorder.bert(st, L)
    L.site_o = sites.next()
    # (each closing Linear of a residual branch runs fused with the post-LN LayerNorm behind it: ops.linear_ln_fwd)
    L.y, L.a32, L.a16, L.am, L.ar = ops.linear_ln_fwd(L.ctx, wfwd(W.o_w), W.o_b, W.ln1_w, W.ln1_b, eps, residual=s1_32, drop_p=p_hid, seed=seed,
                                                      site=L.site_o, want_f32=True, want_bf16=True)
    L.u = torch.empty(Mq, W.i_w.shape[0], device=s1_32.device, dtype=BF16)
    L.i = ops.linear_fwd(L.a16, wfwd(W.i_w), W.i_b, act=ops.ACT_GELU_FWD, aux_out=L.u)
    L.site_f = sites.next()
    L.z, out32, out16, L.zm, L.zr = ops.linear_ln_fwd(L.i, wfwd(W.o2_w), W.o2_b, W.ln2_w, W.ln2_b, eps, residual=L.a32, drop_p=p_hid, seed=seed,
                                                      site=L.site_f, want_f32=True, want_bf16=True)
    L.p_hid, L.p_att = p_hid, p_att
    return L, out32, out16


def _grad_buffers_live(W, self_attn):
    """The re-check of a sequenced layer's backward: every gradient buffer that the library call writes through itself still exists (a
    parameter frozen between forward and backward has none).  The fused q | k | v buffers were taken as views in the forward; the
    cross-attention call leaves the weight gradients to the host, which looks each one up."""
    if W.lora:                             # (an adapted layer on a frozen base: the call writes the adapters' gradients and no other)
        ps = [q for t in W.lora for q in _lora_pair(W.att, t)]
    else:
        ps = (W.o_w, W.o_b, W.i_w, W.i_b, W.o2_w, W.o2_b, W.ln1_w, W.ln1_b, W.ln2_w, W.ln2_b) if self_attn else (W.o_b, W.o2_b, W.ln1_w, W.ln1_b, W.ln2_w, W.ln2_b)
    return all(gbuf(p) is not None for p in ps)


def _bert_layer_bwd(st, L, dout, seed, want=(True, True)):
    """-> (ds1 fp32 [B*Lq,D], ds2 fp32 [B*Lk,D] or None when self_attn (then ds1 holds the sum)).  want: (ds1, ds2) are needed -- an
    input gradient nobody reads is returned as None and its dX products are skipped where the path launches them itself (the
    self-attention sequencers compute ds1 inside their one call)."""
    B, Lq, Lk, D = st.B, st.Lq, st.Lk, st.D
    Mq, Mk, vl = st.Mq, st.Mk, st.vl
    W, heads, ld = L.W, L.heads, L.ld
    hd = D // heads
    if L.path == paths.LAYER and paths.bert_layer_bwd(L.path, bool(ops.kernel_timer.names), _grad_buffers_live(W, L.self_attn)) == paths.LAYER:
        return (_bert_layer_bwd_seq if L.self_attn else _bert_cross_layer_bwd_seq)(st, L, dout, want)
    pend, raw = [], []                     # the layer's weight gradients leave as one grouped launch (see _lin_bwd_params_many)
    dz, dzb = ops.layernorm_bwd(dout, L.z, W.ln2_w, L.zm, L.zr, gbuf(W.ln2_w), gbuf(W.ln2_b), bf16_copy=(L.p_hid, L.site_f, gbuf(W.o2_b)))
    pend.append(((dzb, L.i, W.o2_w, W.o2_b), dict(bias_done=True)))
    du = ops.linear_bwd_input(dzb, wbf16(W.o2_w), act=ops.ACT_GELU_DX, aux_in=L.u)
    pend.append(((du, L.a16, W.i_w, W.i_b), {}))
    da = ops.linear_bwd_input(du, wbf16(W.i_w))
    # a32 = LN1(y) feeds the FFN AND the residual add of z: both gradients go through LN1's backward
    dy, dyb = ops.layernorm_bwd(da, L.y, W.ln1_w, L.am, L.ar, gbuf(W.ln1_w), gbuf(W.ln1_b), dy_add=dz, bf16_copy=(L.p_hid, L.site_o, gbuf(W.o_b)))
    pend.append(((dyb, L.ctx, W.o_w, W.o_b), dict(bias_done=True)))
    dctx = ops.linear_bwd_input(dyb, wbf16(W.o_w))
    dev = dout.device
    if L.fw is not None:
        # fused q|k|v (or k|v) projection: the attention backward writes straight into one [rows, 3D | 2D] gradient, which
        # then feeds ONE weight-gradient GEMM, one column sum and ONE input-gradient GEMM
        dqkv = torch.empty_like(L.qkv)
        if L.self_attn:
            outv = (dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:])
        else:
            outv = (torch.empty(Mq, D, device=dev, dtype=BF16), dqkv[:, :D], dqkv[:, D:])
        dq, dk, dv = ops.attn_dispatch(Lq, Lk)[1](L.q, L.k, L.v, L.key_add, dctx, L.stats, B, heads, Lq, Lk, 1.0 / math.sqrt(hd), L.p_att, seed, L.site_att,
                                  out=outv, vl=vl)
        raw.append((dqkv, L.s1_16 if L.self_attn else L.s2_16, L.fw[2], L.fb[2].view(-1), None))
        ds1 = dy if want[0] else None
        if L.self_attn:
            if want[0]:
                ops.gemm(dqkv, L.fw[0], M=Mq, N=D, K=3 * D, lda=3 * D, ldb=D, transB=True, out=ds1, ldc=D, beta=1.0)
            _lin_bwd_params_many(pend, raw)
            return ds1, None
        pend.append(((dq, L.s1_16, W.q_w, W.q_b), {}))
        if want[0]:
            ops.gemm(dq, wbf16(W.q_w), M=Mq, N=D, K=D, lda=D, ldb=D, transB=True, out=ds1, ldc=D, beta=1.0)
        ds2 = ops.gemm(dqkv, L.fw[0], M=Mk, N=D, K=2 * D, lda=2 * D, ldb=D, transB=True, out_dtype=F32) if want[1] else None
        _lin_bwd_params_many(pend, raw)
        return ds1, ds2
    if L.fused:
        dq, dk, dv = ops.attn_dispatch(Lq, Lk)[1](L.q, L.k, L.v, L.key_add, dctx, L.stats, B, heads, Lq, Lk, 1.0 / math.sqrt(hd), L.p_att, seed, L.site_att, vl=vl)
    else:
        dP = torch.empty(B, heads, Lq, ld, device=dev, dtype=F32)
        ops.gemm(dctx, L.v, M=Lq, N=Lk, K=hd, lda=D, ldb=D, out=dP, ldc=ld, batch=(B, heads), sA=(Lq * D, hd), sB=(Lk * D, hd),
                 sC=(heads * Lq * ld, Lq * ld))
        dv = torch.empty(B * Lk, D, device=dev, dtype=BF16)
        ops.gemm(L.pd, dctx, M=Lk, N=hd, K=Lq, lda=ld, ldb=D, transA=True, transB=True, out=dv, ldc=D, batch=(B, heads),
                 sA=(heads * Lq * ld, Lq * ld), sB=(Lq * D, hd), sC=(Lk * D, hd))
        dS = ops.softmax_bwd(L.p, dP, B, heads, Lq, Lk, ld, 1.0 / math.sqrt(hd), L.p_att, seed, L.site_att)
        del dP
        dq = torch.empty(B * Lq, D, device=dev, dtype=BF16)
        ops.gemm(dS, L.k, M=Lq, N=hd, K=Lk, lda=ld, ldb=D, transB=True, out=dq, ldc=D, batch=(B, heads),
                 sA=(heads * Lq * ld, Lq * ld), sB=(Lk * D, hd), sC=(Lq * D, hd))
        dk = torch.empty(B * Lk, D, device=dev, dtype=BF16)
        ops.gemm(dS, L.q, M=Lk, N=hd, K=Lq, lda=ld, ldb=D, transA=True, transB=True, out=dk, ldc=D, batch=(B, heads),
                 sA=(heads * Lq * ld, Lq * ld), sB=(Lq * D, hd), sC=(Lk * D, hd))
    pend.append(((dq, L.s1_16, W.q_w, W.q_b), {}))
    pend.append(((dk, L.s2_16, W.k_w, W.k_b), {}))
    pend.append(((dv, L.s2_16, W.v_w, W.v_b), {}))
    _lin_bwd_params_many(pend, raw)
    # LoRA: the adapters' gradients from the dq / dk / dv at hand; u = bf16(s.dy.B) then adds u.A to the stream gradient wherever the
    # base dX GEMM below writes one
    lt = getattr(L, "lt", None) or {}
    lu = {t: _lora_bwd(W.att, t, L.s1_16 if t == "q" else L.s2_16, {"q": dq, "k": dk, "v": dv}[t], lt[t]) for t in lt}

    def lora_dx(t, ds):
        if t in lu:
            ops.lora_dx(lu[t], wbf16(_lora_pair(W.att, t)[0]), ds)
    # ds1 = dy (residual) + dq.Wq ; ds2 = dk.Wk + dv.Wv     (fp32, accumulated by the GEMM's beta=1 epilogue)
    ds1 = dy if want[0] else None
    if want[0]:
        ops.gemm(dq, wbf16(W.q_w), M=Mq, N=D, K=D, lda=D, ldb=D, transB=True, out=ds1, ldc=D, beta=1.0)
        lora_dx("q", ds1)
    if L.self_attn:
        if want[0]:
            ops.gemm(dk, wbf16(W.k_w), M=Mk, N=D, K=D, lda=D, ldb=D, transB=True, out=ds1, ldc=D, beta=1.0)
            ops.gemm(dv, wbf16(W.v_w), M=Mk, N=D, K=D, lda=D, ldb=D, transB=True, out=ds1, ldc=D, beta=1.0)
            lora_dx("k", ds1)
            lora_dx("v", ds1)
        return ds1, None
    if not want[1]:
        return ds1, None
    ds2 = ops.gemm(dk, wbf16(W.k_w), M=Mk, N=D, K=D, lda=D, ldb=D, transB=True, out_dtype=F32)
    ops.gemm(dv, wbf16(W.v_w), M=Mk, N=D, K=D, lda=D, ldb=D, transB=True, out=ds2, ldc=D, beta=1.0)
    lora_dx("k", ds2)
    lora_dx("v", ds2)
    return ds1, ds2


def _bert_run(st, heads, F, key_add, p_hid, p_att, eps, seed, f16):
    """The run block of tower 2's calls and of the cross block's (self-attention: st.Mk / st.Lk are st.Mq / st.Lq)."""
    vl = st.vl
    q_off, k_off, k_cnt, q_rows = ops._NO_VARLEN if vl is None else vl.args()
    return ops.lib().struct("mmdti_bert_run_t")(
        key_add=ops._p(key_add), q_off=q_off, k_off=k_off, k_cnt=k_cnt, seed=int(seed), Mq=st.Mq, Mk=st.Mk, B=st.B, Lq=st.Lq, Lk=st.Lk, heads=heads, D=st.D, F=F,
        q_rows=q_rows, act_fwd=ops.ACT_GELU_FWD, act_dx=ops.ACT_GELU_DX, ln_max_k=_ln_max_k(), fwd_f16=int(f16), scale=float(1.0 / math.sqrt(st.D // heads)),
        p_hid=float(p_hid), p_att=float(p_att), eps=float(eps))


def _bert_layer_desc(W, cross):
    """A layer's description (see _layer_block) for the per-layer calls: the fused projection goes in by its views (L.fw / L.fb), the
    cross layer's separate query projection beside it."""
    lin = {"o": (W.o_w, W.o_b), "i": (W.i_w, W.i_b), "o2": (W.o2_w, W.o2_b)}
    if cross:
        lin["q"] = (W.q_w, W.q_b)
    return SimpleNamespace(struct="mmdti_bert_layer_t", lin=lin, ln={"ln1": (W.ln1_w, W.ln1_b), "ln2": (W.ln2_w, W.ln2_b)}, extra={})


def _bert_seq_fwd(st, L, s1_32, s1_16, key_add, W, heads, p_hid, p_att, eps, seed, sites):
    """_bert_layer_fwd's fused-projection / fused-attention variants as ONE library call (csrc/layers.hip): self-attention (q | k | v one
    GEMM), or -- L.self_attn false -- cross-attention (queries from s1, the fused key | value projection of L.s2_16)."""
    cross = not L.self_attn
    B, Lq, D, Mq, Mk, vl = st.B, st.Lq, st.D, st.Mq, st.Mk, st.vl
    F = W.i_w.shape[0]
    dev = s1_32.device
    L.site_o, L.site_f = sites.next(), sites.next()          # (L.site_att was drawn by the caller: the same numbering as the op-by-op path)
    a16 = s1_16.dtype                         # bf16, or fp16 (fp16 forward operands); q | k | v and the saved gelu' stay bf16 in every mode
    rows, f32 = ((Mq, D), F32), ((Mq,), F32)
    adapted = bool(W.lora)                    # a frozen base: q, k, v as three planes of one buffer, the adapters' t rows in another
    alloc = dict(qkv=(((Mq + 2 * Mk) * D,) if adapted else (Mk, 2 * D) if cross else (Mq, 3 * D), BF16), ctx=((Mq, D), a16), stats=((B, heads, Lq, 2) if vl is None else (heads, Mq, 2), F32),
                 y=rows, a32=rows, a16=((Mq, D), a16), am=f32, ar=f32, u=((Mq, F), BF16), i=((Mq, F), a16), z=rows, zm=f32, zr=f32)
    if cross and not adapted:
        alloc["q"] = ((Mq, D), BF16)
    saved = _saved_block("mmdti_bert_saved_t", L, alloc, dev, s1_32=s1_32)
    if adapted:
        L.q, L.k, L.v = L.qkv[:Mq * D].view(Mq, D), L.qkv[Mq * D:(Mq + Mk) * D].view(Mk, D), L.qkv[(Mq + Mk) * D:].view(Mk, D)
    elif cross:
        L.k, L.v = L.qkv[:, :D], L.qkv[:, D:]
    else:
        L.q, L.k, L.v = L.qkv[:, :D], L.qkv[:, D:2 * D], L.qkv[:, 2 * D:]
    out32, out16 = torch.empty(Mq, D, device=dev, dtype=F32), torch.empty(Mq, D, device=dev, dtype=a16)
    L.fused, L.p_hid, L.p_att = True, p_hid, p_att
    if st.__dict__.get("run") is None:        # (one run block serves every layer of a tower's forward -- and the backward)
        st.run = _bert_run(st, heads, F, key_add, p_hid, p_att, eps, seed, a16 == torch.float16)
    L.run = st.run
    rest = (int(L.site_att), int(L.site_o), int(L.site_f), out32.data_ptr(), out16.data_ptr())
    if adapted:
        row3 = _lora_layout("mmdti_bert_lora_stack_layout", Mq, Mk, D, F, 0, 0)[4]
        L.lt_buf = torch.empty(row3, device=dev, dtype=torch.uint8)
        shapes = [((Mk if t != "q" else Mq), _lora_pair(W.att, t)[0].shape[0]) if t in W.lora else None for t in ("q", "k", "v")]
        L.lt = {t: v for t, v in zip(("q", "k", "v"), _lora_rows(L.lt_buf, row3 // 3, shapes)) if v is not None}
        P = _layer_block(_bert_layer_desc(W, False), w16=_w16_ptr)
        split, ad = _split_block(W, w16=_w16_ptr), _block_array(_lora_blocks(W.att, ("q", "k", "v"), w16=_w16_ptr))
        (ops.lib().mmdti_bert_lora_cross_layer_fwd if cross else ops.lib().mmdti_bert_lora_layer_fwd)(
            ops._stream(), ctypes.addressof(L.run), ctypes.addressof(P), ctypes.addressof(split), ad[1], ctypes.addressof(saved), L.lt_buf.data_ptr(), *rest)
        return L, out32, out16
    P = _layer_block(_bert_layer_desc(W, cross), w16=_w16_ptr, w_qkv=L.fw[3].data_ptr(), b_qkv=L.fb[1].data_ptr())
    (ops.lib().mmdti_bert_cross_layer_fwd if cross else ops.lib().mmdti_bert_layer_fwd)(
        ops._stream(), ctypes.addressof(L.run), ctypes.addressof(P), ctypes.addressof(saved), *rest)
    return L, out32, out16


def _bert_seq_bwd(st, L, dout, want=(True, True)):
    """_bert_layer_bwd of a layer that went through _bert_seq_fwd -> (ds1, ds2) fp32.  Self-attention: ONE library call, ds2 None.
    Cross: its ten launches up to the weight gradients as one call, then the weight gradients exactly as the op-by-op path launches
    them (the layer has two token-row counts)."""
    cross = not L.self_attn
    D, Mq, Mk = st.D, st.Mq, st.Mk
    W, heads = L.W, L.heads
    F = W.i_w.shape[0]
    dev = dout.device
    dout = dout.contiguous()
    e = torch.empty
    ds1 = e(Mq, D, device=dev, dtype=F32)
    nrow = _attn_stat_rows(st, heads)
    if W.lora:
        # an adapted layer on a frozen base: the whole backward is the call's -- no weight gradient is left for the host
        _, ws, ws_bytes = _layer_workspace(_lora_layout("mmdti_bert_lora_stack_layout", Mq, Mk, D, F, nrow * 8, nrow)[3 if cross else 2], dev)
        saved = _saved_block("mmdti_bert_saved_t", L)
        P = _layer_block(_bert_layer_desc(W, False), wb=_wb_ptr, g=_grad_ptr)
        split, ad = _split_block(W, wb=_wb_ptr), _block_array(_lora_blocks(W.att, ("q", "k", "v"), wb=_wb_ptr, g=_grad_ptr))
        head = (ops._stream(), ctypes.addressof(L.run), ctypes.addressof(P), ctypes.addressof(split), ad[1], ctypes.addressof(saved), L.lt_buf.data_ptr(),
                int(L.site_att), int(L.site_o), int(L.site_f), dout.data_ptr(), ds1.data_ptr(), int(bool(want[0])))
        if not cross:
            ops.lib().mmdti_bert_lora_layer_bwd(*head, ws, ws_bytes)
            return (ds1 if want[0] else None), None
        ds2 = e(Mk, D, device=dev, dtype=F32) if want[1] else None
        ops.lib().mmdti_bert_lora_cross_layer_bwd(*head, ops._p(ds2), int(ds2 is not None), ws, ws_bytes)
        return (ds1 if want[0] else None), ds2
    _, ws, ws_bytes = _layer_workspace(_stack_layout("mmdti_bert_stack_layout", Mq, D, F, nrow * 8, nrow)[4 if cross else 3], dev)
    saved = _saved_block("mmdti_bert_saved_t", L)
    P = _layer_block(_bert_layer_desc(W, cross), wb=_wb_ptr, g=_grad_ptr, wb_qkv=L.fw[0].data_ptr(), dw_qkv=L.fw[2].data_ptr(), lddw_qkv=L.fw[2].stride(0),
                     db_qkv=L.fb[2].view(-1).data_ptr())
    head = (ops._stream(), ctypes.addressof(L.run), ctypes.addressof(P), ctypes.addressof(saved), int(L.site_att), int(L.site_o), int(L.site_f), dout.data_ptr(),
            ds1.data_ptr())
    if not cross:
        ops.lib().mmdti_bert_layer_bwd(*head, ws, ws_bytes)
        return ds1, None
    ds2 = e(Mk, D, device=dev, dtype=F32) if want[1] else None   # (ds2 null: not launched)
    dzb, du, dyb = e(Mq, D, device=dev, dtype=BF16), e(Mq, F, device=dev, dtype=BF16), e(Mq, D, device=dev, dtype=BF16)
    dq, dqkv = e(Mq, D, device=dev, dtype=BF16), torch.empty_like(L.qkv)
    ops.lib().mmdti_bert_cross_layer_bwd(*head, ops._p(ds2), dzb.data_ptr(), du.data_ptr(), dyb.data_ptr(), dq.data_ptr(), dqkv.data_ptr(), ws, ws_bytes)
    # the weight gradients, as the op-by-op path hands them over (same items, same order: _lin_bwd_params_many groups them by row count)
    pend = [((dzb, L.i, W.o2_w, W.o2_b), dict(bias_done=True)), ((du, L.a16, W.i_w, W.i_b), {}), ((dyb, L.ctx, W.o_w, W.o_b), dict(bias_done=True)),
            ((dq, L.s1_16, W.q_w, W.q_b), {})]
    _lin_bwd_params_many(pend, [(dqkv, L.s2_16, L.fw[2], L.fb[2].view(-1), None)])
    return (ds1 if want[0] else None), ds2


# (the self-attention and the cross layer enter the one body under their own names: the suite counts each kind's calls by them)
_bert_layer_fwd_seq = lambda *args: _bert_seq_fwd(*args)         # noqa: E731
_bert_layer_bwd_seq = lambda *args: _bert_seq_bwd(*args)         # noqa: E731
_bert_cross_layer_fwd_seq = lambda *args: _bert_seq_fwd(*args)   # noqa: E731
_bert_cross_layer_bwd_seq = lambda *args: _bert_seq_bwd(*args)   # noqa: E731


def _bert_stack_fwd(st, T, x32, x16, key_add, cfg, p_hid, p_att, seed, sites):
    """All layers of tower 2 as ONE library call -> the tower's fp32 output [Mq, D]."""
    nrow = _attn_stat_rows(st, st.heads)
    stats_bytes = nrow * 8
    lora = getattr(T, "lora", None)              # (_lora_stack_tables: adapted layers on a frozen base)
    if lora is not None:
        stride, ws_bytes, slab = _lora_layout("mmdti_bert_lora_stack_layout", st.Mq, st.Mq, T.D, T.F, stats_bytes, nrow)[:2] + (0,)
    else:
        stride, ws_bytes, slab = _stack_layout("mmdti_bert_stack_layout", st.Mq, T.D, T.F, stats_bytes, nrow)[:3]
    dev = x32.device
    arena = torch.empty(stride * T.nl, device=dev, dtype=torch.uint8)
    out32 = torch.empty(st.Mq, T.D, device=dev, dtype=F32)
    site0 = sites.n + 1
    sites.n += 3 * T.nl
    run = _bert_run(st, st.heads, T.F, key_add, p_hid, p_att, cfg.ln_eps, seed, x16.dtype == torch.float16)
    rest = (T.nl, site0, x32.data_ptr(), x16.data_ptr(), arena.data_ptr(), arena.numel(), stats_bytes, out32.data_ptr())
    if lora is not None:
        ops.lib().mmdti_bert_lora_stack_fwd(ops._stream(), ctypes.addressof(run), T.layers[1], T.split[1], lora[1], *rest)
    else:
        ops.lib().mmdti_bert_stack_fwd(ops._stream(), ctypes.addressof(run), T.layers[1], *rest)
    # (x16, key_add: the run block and the backward read them -- kept alive here)
    st.stack = SimpleNamespace(T=T, arena=arena, ws_bytes=ws_bytes, slab=slab, stats_bytes=stats_bytes, site0=site0, x16=x16, key_add=key_add, run=run)
    return out32


def _bert_stack_bwd(st, dout):
    """All layers' backward as ONE library call -> the gradient of the embeddings' LayerNorm output (fp32 [Mq, D])."""
    S = st.stack
    T = S.T
    dev = dout.device
    ds1 = torch.empty(st.Mq, T.D, device=dev, dtype=F32)
    ws = torch.empty(S.ws_bytes, device=dev, dtype=torch.uint8)
    tail = (S.x16.data_ptr(), S.arena.data_ptr(), S.arena.numel(), S.stats_bytes, ws.data_ptr(), ws.numel())
    if getattr(T, "lora", None) is not None:
        ops.lib().mmdti_bert_lora_stack_bwd(ops._stream(), ctypes.addressof(S.run), T.layers[1], T.split[1], T.lora[1], T.nl, S.site0, dout.data_ptr(),
                                            ds1.data_ptr(), int(st.plan.needs_dx(0)), *tail)
    else:
        ops.lib().mmdti_bert_stack_bwd(ops._stream(), ctypes.addressof(S.run), T.layers[1], T.nl, S.site0, dout.data_ptr(), ds1.data_ptr(), *tail, S.slab)
    return ds1


class RobertaEncoderFn(torch.autograd.Function):
    """self.bert(input_ids, attention_mask)[0]  (mm_model.py:562): embeddings + L post-LN layers.
    `mod` exposes: word/position/token_type embedding weights, emb LayerNorm, layers, cfg (heads, eps, dropouts, pad)."""

    @staticmethod
    def forward(ctx, anchor, input_ids, attention_mask, mod, training, pack=None):
        """anchor: freeze.grad_anchor(mod.parameters()), None when the whole tower is frozen (it then runs forward only and keeps
        nothing).
        pack (packing.PackedRows over the right-padded input_ids): the tower runs on the packed rows -- every sequence's real
        tokens plus ONE representative pad row (pad word embedding + position padding_idx: all masked slots are that row) -- and
        returns [pack.M, D]; masked keys are left out of the attention instead of being added finfo.min (probability 0 either way)."""
        B, Lq = input_ids.shape
        cfg = mod.cfg
        D = mod.word.shape[1]
        seed = dropout_state.next_seed()
        sites = _Sites()
        p_hid = cfg.hidden_dropout if training else 0.0
        p_att = cfg.attn_dropout if training else 0.0
        rec = _recorder
        if rec is not None:
            rec.check("RobertaEncoderFn", any(ctx.needs_input_grad), p_hid, p_att)
        S_pad = Lq
        ids = input_ids.contiguous()
        pos = ops.roberta_position_ids(ids, cfg.pad_idx)
        vl, Mq = None, B * Lq
        if pack is not None:
            ids, pos = ids.view(-1)[pack.gather], pos.view(-1)[pack.gather]      # (integer plumbing: the packed rows' ids)
            vl, Mq, Lq = ops.AttnVarlen(pack, pack), pack.M, pack.max_rows
        e = ops.embedding_fwd3(ids, mod.word, pos, mod.position, mod.token_type)      # word + position + token type 0, one pass
        zeros = None
        st = SimpleNamespace(B=B, Lq=Lq, Lk=Lq if vl is None else vl.Lk, D=D, seed=seed, ids=ids, pos=pos, zeros=zeros, e=e, layers=[], p_hid=p_hid, Mq=Mq, Mk=Mq, vl=vl,
                             heads=cfg.heads)
        keep = any(ctx.needs_input_grad)      # inference (or a frozen tower): no per-layer activations are kept
        if keep:
            # the backward stops at the lowest layer that trains unless the embeddings train (freeze.plan_tower)
            st.plan = plan_tower(layer_trainable(mod.layers), any(p.requires_grad for p in mod.embeddings.parameters()))
        st.site_emb = sites.next()
        x32, x16, st.em, st.er = ops.layernorm_fwd(e.view(Mq, D), mod.emb_ln_w, mod.emb_ln_b, cfg.ln_eps, want_f32=True, want_bf16=True,
                                                   drop_p=p_hid, seed=seed, site=st.site_emb)
        key_add = ((1.0 - attention_mask.to(F32)) * torch.finfo(torch.float32).min).contiguous() if vl is None else None
        # small batches: ALL layers from one library call (see _bert_stack_fwd); the per-layer loop then has nothing left to do
        st.stack = None
        T = None
        sw = _switches()
        adapters = _has_bert_adapters(mod.layers)
        attn_ok = D % cfg.heads == 0 and ops.attn_eligible(Lq, st.Lk, D // cfg.heads, D)
        aseq = adapters and _adapter_seq(mod.layers, _bert_attn_of, attn_ok and all(l.attention.self.query.bias is not None for l in mod.layers))
        if paths.bert_tower_fwd(sw, x32.is_cuda, keep, len(mod.layers), Mq, adapters=adapters, adapter_seq=aseq) == paths.STACK:
            T = _lora_stack_tables(True, mod, Mq, sw, attn_ok) if adapters else _stack_tables(_bert_stack_desc, mod, Mq, sw, attn_ok)
        if T is not None:
            x32 = _bert_stack_fwd(st, T, x32, x16, key_add, cfg, p_hid, p_att, seed, sites)
        for li, layer in enumerate(mod.layers if T is None else ()):
            if rec is not None:
                st.rec_tag = ("bert", li, pack.n_real if pack is not None else rec.counts.get("bert"), S_pad, S_pad) \
                    if rec.wants("bert", li, len(mod.layers)) else None
            L, x32, x16 = _bert_layer_fwd(st, x32, x16, x16, key_add, bert_weights(layer), cfg.heads, p_hid, p_att, cfg.ln_eps, seed, sites, True)
            if keep:
                st.layers.append(_kept(L, li, st.plan))
        if keep:
            ctx.st, ctx.mod = st, mod
        return x32.view(B, Lq, D) if vl is None else x32

    @staticmethod
    def backward(ctx, dout):
        st, mod = ctx.st, ctx.mod
        if getattr(st, "consumed", False):
            raise ops.MMDTIError("RobertaEncoderFn: backward through the same forward twice (retain_graph) is not supported")
        st.consumed = True
        B, Lq, D = st.B, st.Lq, st.D
        dx = dout.contiguous().view(st.Mq, D)
        if st.stack is not None:
            dx = _bert_stack_bwd(st, dx)
            notify_grads_ready(st.stack.T.params)
            st.stack = None
        plan = st.plan
        for li, layer, L in zip(range(len(st.layers) - 1, -1, -1), reversed(list(mod.layers)), reversed(st.layers)):
            if li < plan.lowest:                 # nothing at or under this layer trains
                L.__dict__.clear()
                continue
            dx, _ = _bert_layer_bwd(st, L, dx, st.seed, (plan.needs_dx(li), False))
            L.__dict__.clear()
            notify_grads_ready(layer.parameters())
        if not plan.below:                       # frozen embeddings: no LayerNorm backward, no embedding-gradient kernels
            _join_stream_after_backward()
            return None, None, None, None, None, None
        de = ops.layernorm_bwd(dx, st.e.view(st.Mq, D), mod.emb_ln_w, st.em, st.er, gbuf(mod.emb_ln_w), gbuf(mod.emb_ln_b),
                               drop_p=st.p_hid, seed=st.seed, site=st.site_emb)
        cfg = mod.cfg
        de16 = ops.cast_bf16(de)
        for ids, w, pad in ((st.ids, mod.word, cfg.pad_idx), (st.pos, mod.position, cfg.pad_idx), (None, mod.token_type, -1)):
            g = gbuf(w)
            if g is not None:
                if ids is None:        # token type 0 everywhere: a one-row table is a column sum (ids unused), else explicit zeros
                    ids = st.ids if w.shape[0] == 1 else torch.zeros_like(st.ids)
                ops.embedding_bwd_gemm(ids, de16, g, pad)
        notify_grads_ready(mod.embeddings.parameters())
        _join_stream_after_backward()   # (MM_Model runs this tower on a side stream)
        return None, None, None, None, None, None


class CrossLayerFn(torch.autograd.Function):
    """One BertCrossEncoder layer (mm_module.py:663-677, :615-626): s1 attends to s2 under an additive key mask."""

    @staticmethod
    def forward(ctx, s1, s2, key_add, layer, cfg, training, packs=None, anchor=None):
        """anchor: freeze.grad_anchor(layer.parameters()) -- the backward runs when the layer trains even if neither input needs a
        gradient.
        packs = (PackedRows of s1, PackedRows of s2): s1 [M1, D] / s2 [M2, D] are packed rows, key_add is None -- the keys of a
        sequence are the REAL rows of s2 (the reference adds -10000 to padded keys, mm_model.py:392-393: probability exactly 0)."""
        seed = dropout_state.next_seed()
        sites = _Sites()
        p_hid = cfg.hidden_dropout if training else 0.0
        p_att = cfg.attn_dropout if training else 0.0
        if packs is not None:
            vl = ops.AttnVarlen(packs[0], packs[1])
            D = s1.shape[-1]
            st = SimpleNamespace(B=packs[0].B, Lq=vl.Lq, Lk=vl.Lk, D=D, seed=seed, Mq=vl.q_rows, Mk=vl.k_rows, vl=vl)
        else:
            B, Lq, D = s1.shape
            Lk = s2.shape[1]
            st = SimpleNamespace(B=B, Lq=Lq, Lk=Lk, D=D, seed=seed, Mq=B * Lq, Mk=B * Lk, vl=None)
        rec = _recorder
        if rec is not None:
            rec.check("CrossLayerFn", any(ctx.needs_input_grad), p_hid, p_att)
            name, li, n = rec.cross_layers.get(id(layer), ("text_to_graph", 0, 1))
            if rec.wants("cross", li, n):
                q_cnt = packs[0].n_real if packs is not None else rec.counts.get("bert" if name == "text_to_graph" else "unimol")
                st.rec_tag = (name, li, q_cnt, st.Lq if packs is None else packs[0].S, st.Lk if packs is None else packs[1].S)
        s1c = s1.contiguous().view(st.Mq, D)
        s1_16 = ops.cast_act16(s1c)
        s2_16 = ops.cast_act16(s2.contiguous().view(st.Mk, D))
        L, out32, _ = _bert_layer_fwd(st, s1c, s1_16, s2_16, None if key_add is None else key_add.contiguous(), bert_weights(layer), cfg.heads,
                                      p_hid, p_att, cfg.ln_eps, seed, sites, False)
        if any(ctx.needs_input_grad):
            ctx.st, ctx.L, ctx.layer = st, L, layer
        ctx.shapes = (s1.shape, s2.shape)
        return out32.view(s1.shape)

    @staticmethod
    def backward(ctx, dout):
        st, L = ctx.st, ctx.L
        want = ctx.needs_input_grad[:2]          # (a frozen tower feeding s1 / s2: its input gradient is not computed)
        ds1, ds2 = _bert_layer_bwd(st, L, dout.contiguous().view(st.Mq, st.D), st.seed, want)
        L.__dict__.clear()
        notify_grads_ready(ctx.layer.parameters())
        return (None if ds1 is None else ds1.view(ctx.shapes[0]), None if ds2 is None else ds2.view(ctx.shapes[1]), None, None, None, None, None,
                None)


class DropoutFn(torch.autograd.Function):
    """F.dropout on fp32 activations (mm_model.py:390-391, 79, 82)."""

    @staticmethod
    def forward(ctx, x, p, training):
        if not training or p == 0.0:
            ctx.p = 0.0
            return x
        ctx.p, ctx.seed = p, dropout_state.next_seed()
        return ops.dropout_f32(x.contiguous(), p, ctx.seed, 1)

    @staticmethod
    def backward(ctx, d):
        if ctx.p == 0.0:
            return d, None, None
        return ops.dropout_f32(d.contiguous(), ctx.p, ctx.seed, 1), None, None


# ------------------------------------------------------------------------------------------------- InfoNCE
def _pad8(n):
    return (n + 7) // 8 * 8


def _infonce_pool(real, pack, mask):
    """The pooling of one InfoNCE side as (forward, backward), both called as (x | dout, B, n, D, ld[, aux=, aux_mode=]): the mean over
    the real positions (mask plane or pad-free pack), over all positions of packed rows (the pad row weighted), or over all positions."""
    if real:
        return (lambda x, *a: ops.seq_mean_real_fwd(x, *a, mask=mask, pack=pack),
                lambda dout, *a, **aux: ops.seq_mean_real_bwd(dout, *a, mask=mask, pack=pack, **aux))
    if pack is not None:
        return (lambda x, B, n, D, ld: ops.seq_mean_packed_fwd(x, pack, D, ld),
                lambda dout, B, n, D, ld, **aux: ops.seq_mean_packed_bwd(dout, pack, D, ld, **aux))
    return ops.seq_mean_fwd, ops.seq_mean_bwd


class InfoNCEFn(torch.autograd.Function):
    """InfoNCE.forward (models/infonce.py:23-38) + info_nce (:42-98) with implicit negatives.

    Under data parallelism `gather` is a callable [B_loc,2*d] -> [B_glob,2*d] (all-gather in rank order) and
    `reduce_scatter` its adjoint; anchors of this rank are rows [row0,row0+B_loc) of the global batch and the value
    returned is this rank's share of the global loss (the sum over ranks equals the single-process loss)."""

    @staticmethod
    def forward(ctx, query, positive, mod, training, gather, reduce_scatter, row0, packs=None, anchor=None, masks=None, bank=None):
        """anchor: freeze.grad_anchor(mod.parameters()) -- the backward runs when the head trains even if neither input needs a gradient.
        packs = (PackedRows of query, PackedRows of positive): [M, D] packed rows; the unmasked mean over the padded positions
        (infonce.py:32-33) weights each representative pad row by the number of padded positions it stands for.
        mod.pool == "real" (InfoNCE(pool="real")): the mean runs over the real positions only, in either order of pooling and
        projecting -- masks = ([B,Nq], [B,Np]) planes (non-zero = real) for padded inputs, pad-free packs for packed rows.
        bank = (ring of past query-side embeddings, ring of past positive-side ones, sample_ids [B] int64 | None), models/infonce.py's
        MemoryRing: the valid slots are extra keys without a gradient (direction a reads the positive-side ring, direction b the
        query-side one; a slot holding the anchor's own id is skipped), then all Bg rows of both sides are pushed -- under data
        parallelism the gathered rows, so every rank holds the same rings (the ids ride a second, int64 all-gather).  None: no bank,
        the launches below are the bank-less ones."""
        real = getattr(mod, "pool", "all") == "real"
        if real and (packs is None) == (masks is None):
            raise ops.MMDTIError("InfoNCEFn(pool='real'): exactly one of masks (padded rows) and packs (pad-free packed rows) is given")
        if packs is not None and real:
            B, D = packs[0].B, query.shape[-1]
            Nq, Np = packs[0].S, packs[1].S
        elif packs is not None:
            B, D = packs[0].B, query.shape[-1]
            Nq, Np = packs[0].M, packs[1].M           # (rows of the whole side, not per sequence)
            if not (POOL_THEN_PROJECT and mod.info_proj_query[0].weight.shape[0] % 8 == 0 and mod.info_proj_positive[0].weight.shape[0] % 8 == 0):
                raise ops.MMDTIError("InfoNCEFn: packed rows need the pool-then-project form (hidden width % 8 == 0)")
        else:
            B, Nq, D = query.shape
            Np = positive.shape[1]
        d = mod.d_l
        ldp = _pad8(d)
        seed = dropout_state.next_seed()
        p = mod.embed_dropout if training else 0.0
        st = SimpleNamespace(B=B, Nq=Nq, Np=Np, D=D, d=d, ldp=ldp, seed=seed, p=p)
        dev = query.device

        def proj(x, seq, n, dropout_p, site, pack, mask):
            L = SimpleNamespace()
            rows = B * n if pack is None else pack.M
            L.x16 = ops.cast_act16(x.contiguous().view(rows, D), dropout_p, seed, site)
            L.u = torch.empty(rows, seq[0].weight.shape[0], device=dev, dtype=BF16)
            # (h is pooled, not multiplied: bf16 in every mode)
            h = ops.linear_fwd(L.x16, wfwd(seq[0].weight), seq[0].bias, act=ops.ACT_GELU_FWD, aux_out=L.u, out_dtype=BF16)
            Hd = h.shape[1]
            pool = _infonce_pool(real, pack, mask)[0]
            if POOL_THEN_PROJECT and Hd % 8 == 0:             # (always, for packed rows with a pad row: checked above)
                # mean_t(W2 h_t + b2) == W2 mean_t(h_t) + b2: pool the GELU outputs (fp32), then ONE [B, Hd] x [d, Hd] fp32 linear
                # -- instead of a 50-wide bf16 GEMM over every token, its three backward GEMMs and a bf16 round of the
                # per-token projections.  (The unmasked mean over all positions is the reference's, infonce.py:32-33.)
                L.hbar = pool(h, B, n, Hd, Hd)
                L.mean = ops.linear_f32_fwd(L.hbar, seq[2].weight.detach(), seq[2].bias.detach())
                L.h = None
                return L
            L.h = h
            pr = torch.zeros(rows, ldp, device=dev, dtype=BF16)
            ops.gemm(L.h, wbf16(seq[2].weight), M=rows, N=d, K=Hd, lda=Hd, ldb=seq[2].weight.shape[1], out=pr, ldc=ldp, bias=seq[2].bias)
            L.mean = pool(pr, B, n, d, ldp)
            return L

        st.packs, st.masks, st.real = packs, masks, real
        pk, mk = packs or (None, None), masks or (None, None)
        st.Lq = proj(query, mod.info_proj_query, Nq, p, 1, pk[0], mk[0])
        st.Lp = proj(positive, mod.info_proj_positive, Np, 0.0, 2, pk[1], mk[1])
        both = torch.cat((st.Lq.mean, st.Lp.mean), dim=1)            # [B, 2d] (tiny; one message under DDP)
        both_all = gather(both) if gather is not None else both
        Bg = both_all.shape[0]
        qh, st.qinv = ops.l2norm_fwd(both_all[:, :d])
        kh, st.kinv = ops.l2norm_fwd(both_all[:, d:])
        loss = torch.zeros(1, device=dev, dtype=F32)
        dqh, dkh = torch.zeros_like(qh), torch.zeros_like(kh)
        T = mod.temperature
        if bank is None:
            ops.infonce_dir(qh, kh, row0, B, T, loss, dqh, dkh)
            ops.infonce_dir(kh, qh, row0, B, T, loss, dkh, dqh)
        else:
            ring_q, ring_k, ids = bank
            if Bg > ring_q.rows.shape[0]:
                raise ValueError(f"InfoNCE: memory_bank={ring_q.rows.shape[0]} is smaller than the global batch ({Bg} rows are pushed per step)")
            if ids is not None:
                ids = ids.contiguous()
                ids = gather(ids.view(-1, 1)).view(-1).contiguous() if gather is not None else ids
            ops.infonce_bank_dir(qh, kh, row0, B, T, loss, dqh, dkh, ring_k.rows, ring_k.valid, ring_k.ids, ids)
            ops.infonce_bank_dir(kh, qh, row0, B, T, loss, dkh, dqh, ring_q.rows, ring_q.valid, ring_q.ids, ids)
            ops.infonce_bank_push(ring_q.rows, ring_q.valid, ring_q.ids, ring_q.head, qh, ids)
            ops.infonce_bank_push(ring_k.rows, ring_k.valid, ring_k.ids, ring_k.head, kh, ids)
        st.qh, st.kh, st.dqh, st.dkh, st.Bg, st.row0 = qh, kh, dqh, dkh, Bg, row0
        ctx.st, ctx.mod, ctx.rs = st, mod, reduce_scatter
        return (loss / (2.0 * Bg)).view(())

    @staticmethod
    def backward(ctx, dloss):
        st, mod = ctx.st, ctx.mod
        B, d, ldp = st.B, st.d, st.ldp
        dq = ops.l2norm_bwd(st.dqh, st.qh, st.qinv)
        dk = ops.l2norm_bwd(st.dkh, st.kh, st.kinv)
        dboth = torch.cat((dq, dk), dim=1)
        if ctx.rs is not None:
            dboth = ctx.rs(dboth)                                   # sum over ranks, keep own rows
        dboth = (dboth * dloss).contiguous()

        def proj_bwd(L, dmean, seq, n, dropout_p, site, want_dx, pack, mask):
            # (pool="real": masked rows of du / dpr are exact zeros -- padded rows enter no weight gradient and receive a zero input gradient)
            pool_bwd = _infonce_pool(st.real, pack, mask)[1]
            if L.h is None:                                                                  # pooled first (see forward)
                gw, gb = gbuf(seq[2].weight), gbuf(seq[2].bias)
                dhbar = ops.linear_f32_bwd(L.hbar, seq[2].weight.detach(), None, dmean.contiguous(), gw, gb)
                Hd = L.hbar.shape[1]
                du = pool_bwd(dhbar, B, n, Hd, Hd, aux=L.u, aux_mode=1 if ops.GELU_SAVE_GRAD else 2)
            else:
                dpr = pool_bwd(dmean.contiguous(), B, n, d, ldp)                             # [rows, ldp] bf16, pad cols 0
                gw = gbuf(seq[2].weight)
                if gw is not None:
                    ops.linear_bwd_weight(dpr, L.h, gw)
                gb = gbuf(seq[2].bias)
                if gb is not None:
                    ops.colsum(dpr, gb, cols=d)
                du = ops.gemm(dpr, wbf16(seq[2].weight), M=L.h.shape[0], N=L.h.shape[1], K=d, lda=ldp, ldb=seq[2].weight.shape[1], transB=True,
                              act=ops.ACT_GELU_DX, aux_in=L.u)
            _lin_bwd_params(du, L.x16, seq[0].weight, seq[0].bias)
            if not want_dx:
                return None
            dx = ops.linear_bwd_input(du, wbf16(seq[0].weight), out_dtype=F32)
            if dropout_p > 0:
                dx = ops.dropout_f32(dx, dropout_p, st.seed, site)
            return dx

        pk, mk = st.packs or (None, None), st.masks or (None, None)
        dxq = proj_bwd(st.Lq, dboth[:, :d], mod.info_proj_query, st.Nq, st.p, 1, ctx.needs_input_grad[0], pk[0], mk[0])
        dxp = proj_bwd(st.Lp, dboth[:, d:], mod.info_proj_positive, st.Np, 0.0, 2, ctx.needs_input_grad[1], pk[1], mk[1])
        notify_grads_ready(mod.parameters())
        if st.packs is not None:
            return dxq, dxp, None, None, None, None, None, None, None, None, None
        return (None if dxq is None else dxq.view(B, st.Nq, st.D), None if dxp is None else dxp.view(B, st.Np, st.D), None, None, None, None, None, None,
                None, None, None)


def infonce_rows_grad(both_all, d, temperature, row0, B):
    """What InfoNCEFn's backward hands to ``reduce_scatter`` for the rank whose anchors are rows [row0, row0 + B) of the gathered
    message ``both_all`` [Bg, 2 d] (query | positive): the gradient of that rank's share with respect to every row of the message,
    before the factor dloss.  Same launches as the Fn's loss tail and the head of its backward (accumulate.TimeChannel.prepare)."""
    qh, qinv = ops.l2norm_fwd(both_all[:, :d])
    kh, kinv = ops.l2norm_fwd(both_all[:, d:])
    loss = torch.zeros(1, device=both_all.device, dtype=F32)
    dqh, dkh = torch.zeros_like(qh), torch.zeros_like(kh)
    ops.infonce_dir(qh, kh, row0, B, temperature, loss, dqh, dkh)
    ops.infonce_dir(kh, qh, row0, B, temperature, loss, dkh, dqh)
    return torch.cat((ops.l2norm_bwd(dqh, qh, qinv), ops.l2norm_bwd(dkh, kh, kinv)), dim=1)


class InfoNCELossFn(torch.autograd.Function):
    """info_nce(query, positive_key) on already-pooled [B,d] embeddings (models/infonce.py:42-98, implicit negatives)."""

    @staticmethod
    def forward(ctx, q, k, temperature):
        B, d = q.shape
        qh, qinv = ops.l2norm_fwd(q.contiguous())
        kh, kinv = ops.l2norm_fwd(k.contiguous())
        loss = torch.zeros(1, device=q.device, dtype=F32)
        dqh, dkh = torch.zeros_like(qh), torch.zeros_like(kh)
        ops.infonce_dir(qh, kh, 0, B, temperature, loss, dqh, dkh)
        ops.infonce_dir(kh, qh, 0, B, temperature, loss, dkh, dqh)
        ctx.sv = (qh, qinv, kh, kinv, dqh, dkh)
        return (loss / (2.0 * B)).view(())

    @staticmethod
    def backward(ctx, dl):
        qh, qinv, kh, kinv, dqh, dkh = ctx.sv
        return ops.l2norm_bwd(dqh, qh, qinv) * dl, ops.l2norm_bwd(dkh, kh, kinv) * dl, None


# ------------------------------------------------------------------------------------------------- ConR / SupCon
class CTLossFn(torch.autograd.Function):
    """CT_Regress / CT_Single / CT_Multi (models/contrastive.py).  Only `feature` receives a gradient (the masks built
    from labels / predictions are not differentiable in the reference either).

    negatives (optional, trailing): global negatives under data parallelism -- anything with ``gather(x [B_loc, C]) -> [B_glob, C]`` in
    rank order, ``reduce_scatter(g [B_glob, C]) -> [B_loc, C]`` (sum over ranks, own rows) and ``row0`` (this rank's first global row:
    an int, or a callable of B_loc as parallel.GlobalNegatives.row0).  The local rows are normalised here, the payload is gathered
    (parallel.CTPayload), this rank's anchors meet every rank's keys, and the value returned is this rank's SHARE of the loss of the
    union batch: (1/B_glob) sum over own anchors.  The backward produces own anchors' contribution to every row, the adjoint of the
    gather returns the rows of own molecules, and the normalisation's backward stays local."""

    @staticmethod
    def forward(ctx, feature, mode, labels_f, labels_i, pred, weights, w, t, e, coef, negatives=None):
        f = feature.reshape(feature.shape[0], -1).contiguous()
        fh, inv = ops.l2norm_fwd(f)
        ctx.negatives = negatives
        if negatives is not None:
            from .parallel import CTPayload
            Bl = fh.shape[0]
            row0 = negatives.row0
            row0 = int(row0(Bl) if callable(row0) else row0)
            fa, la, lia, pa, wa = CTPayload.gather(negatives, fh, labels_f=labels_f, labels_i=labels_i, pred=pred, weights=weights)
            if fa.shape[0] % Bl != 0 or row0 + Bl > fa.shape[0]:
                raise ValueError(f"CTLossFn: gathered {fa.shape[0]} rows for {Bl} local ones at row0 = {row0}")
            loss, G, _ = ops.ct_loss_rows_fwd(mode, fa, row0, Bl, labels_f=la, labels_i=lia, pred=pa, weights=wa, w=w, t=t, e=e, coef=coef)
            ctx.sv, ctx.t, ctx.shape, ctx.row0 = (fh, inv, G, fa), t, feature.shape, row0
            return loss.view(())
        loss, G = ops.ct_loss_fwd(mode, fh, labels_f=labels_f, labels_i=labels_i, pred=pred, weights=weights, w=w, t=t, e=e, coef=coef)
        ctx.sv, ctx.t, ctx.shape = (fh, inv, G), t, feature.shape
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        if ctx.negatives is not None:
            fh, inv, G, fa = ctx.sv
            dfa = ops.ct_loss_rows_bwd(fa, G, ctx.row0, ctx.t)
            df = ops.l2norm_bwd(ctx.negatives.reduce_scatter(dfa).contiguous(), fh, inv)
            return (df * dl).view(ctx.shape), None, None, None, None, None, None, None, None, None, None
        fh, inv, G = ctx.sv
        df = ops.l2norm_bwd(ops.ct_loss_bwd(fh, G, ctx.t), fh, inv)
        return (df * dl).view(ctx.shape), None, None, None, None, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------- FDS smooth / pool / head / losses
class FDSSmoothFn(torch.autograd.Function):
    """FDS.smooth (models/fds.py:157-190).  Out-of-place; the module wrapper copies back to keep the reference's
    in-place aliasing visible to the caller."""

    @staticmethod
    def forward(ctx, x, bins, flags, bs, bn, m1, v1, m2, v2):
        y, sc = ops.fds_smooth(x.contiguous(), bins, flags, bs, bn, m1, v1, m2, v2, want_scale=True)
        ctx.sc = sc
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.sc, None, None, None, None, None, None, None, None


class MaskedPoolFn(torch.autograd.Function):
    """mm_model.py:572-576: zero padded rows, concat, sum / (#atom tokens + #SMILES tokens)."""

    @staticmethod
    def forward(ctx, a, t, mask_a, mask_t, packs=None):
        if packs is not None:          # packed rows: a [M1, D], t [M2, D]; the masks are implied by the packings
            ctx.packs = packs
            return ops.masked_pool_packed_fwd(a.contiguous(), t.contiguous(), packs[0], packs[1])
        ctx.packs = None
        ma, mt = ops._u8(mask_a), ops._u8(mask_t)
        ctx.sv = (ma, mt, a.shape[1], t.shape[1])
        return ops.masked_pool_fwd(a.contiguous(), t.contiguous(), ma, mt)

    @staticmethod
    def backward(ctx, dp):
        if ctx.packs is not None:
            da, dt = ops.masked_pool_packed_bwd(dp.contiguous(), ctx.packs[0], ctx.packs[1])
            return da, dt, None, None, None
        ma, mt, Na, Nt = ctx.sv
        da, dt = ops.masked_pool_bwd(dp.contiguous(), ma, mt, Na, Nt)
        return da, dt, None, None, None


class LinearF32Fn(torch.autograd.Function):
    """Small fp32 Linear (+tanh) for the classification head (mm_model.py:44-84)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        x = x.contiguous()
        y = ops.linear_f32_fwd(x, weight, bias, act)
        # y is this node's OUTPUT: it must go through save_for_backward -- kept as a plain attribute it closes a reference
        # cycle (node -> y -> grad_fn -> node) that keeps the whole step's graph alive until the cyclic GC runs
        ctx.save_for_backward(y)
        ctx.sv = (x, weight, bias, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, act = ctx.sv
        (y,) = ctx.saved_tensors
        dx = ops.linear_f32_bwd(x, weight, y, dy.contiguous(), gbuf(weight), None if bias is None else gbuf(bias), act, want_dx=ctx.needs_input_grad[0])
        notify_grads_ready([weight] if bias is None else [weight, bias])
        return dx, None, None, None


class MSELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        loss, d = ops.mse_loss(pred.contiguous(), target.contiguous().to(F32))
        ctx.d = d
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        return (ctx.d * dl).view_as(ctx.d), None


class CELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        loss, d = ops.ce_loss(logits.contiguous(), target.contiguous().view(-1).long())
        ctx.d = d
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        return ctx.d * dl, None


class BCELogitsLossFn(torch.autograd.Function):
    """nn.BCEWithLogitsLoss() on [B, C] logits (models/nnmodel.py:28-29, multilabel_classification 'bce'); the reference hands the
    targets over as int64 (tasks/trainer.py:119), the kernel reads them as fp32."""

    @staticmethod
    def forward(ctx, logits, target):
        loss, d = ops.bce_logits_loss(logits.contiguous(), target.contiguous().to(F32))
        ctx.d = d
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        return ctx.d * dl, None


class FocalLogitsLossFn(torch.autograd.Function):
    """FocalLossWithLogits on [B, C] logits (models/loss.py:233-276; the default multilabel_classification loss, models/nnmodel.py:
    90-93).  Targets of any dtype: the kernel reads them as fp32 and takes every value other than 0 and 1 (NaN, -1) as a missing label."""

    @staticmethod
    def forward(ctx, logits, target, alpha=0.25, gamma=2.0):
        loss, d = ops.focal_logits_loss(logits.contiguous(), target.contiguous().to(F32), alpha, gamma)
        ctx.d = d
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        return ctx.d * dl, None, None, None


class GHMCLogitsLossFn(torch.autograd.Function):
    """GHMC_Loss on [B, C] logits (models/loss.py:63-132).  ``state``: the [bins + 1] device buffer of the bin counts, updated by the call."""

    @staticmethod
    def forward(ctx, logits, target, state, bins=10, alpha=0.5):
        loss, d = ops.ghmc_logits_loss(logits.contiguous(), target.contiguous().to(F32), state, bins, alpha)
        ctx.d = d
        return loss.view(())

    @staticmethod
    def backward(ctx, dl):
        return ctx.d * dl, None, None, None, None
