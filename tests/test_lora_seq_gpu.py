"""Adapted layers through the library's sequencers (csrc/layers.hip, mmdti_*_lora_*; DESIGN.md "LoRA adapters"): a layer that carries
adapters next to a frozen base issues, from one call per layer (LAYER) or per tower (STACK), the launches of the op-by-op body of
functional.py (OPS, what MMDTI_LORA_SEQ=0 gives back).  Same kernels, arguments and order, so everything without atomics -- outputs,
input gradients, the saved t of every adapter, the pair-gradient chain -- is BIT-identical; the adapter gradients, whose partial sums
meet in fp32 atomics (mmdti_lora_bwd), agree to the atomics' noise (relative norm 2e-4, the band of the sequencer tests in
tests/test_modules_gpu.py) and bit for bit in the deterministic mode.  Train mode, dropout 0.1, the dropout stream reseeded before each
run; the library calls are counted, so a silent fall-back to the op-by-op path fails.  Shapes: widths 64 and 512; 6 sequences of 40
(174 packed -- 169 real tokens and 5 representative pad rows -- / 240 padded token rows) or 14 (ragged atom counts) positions: a partial 128-row block in every LoRA kernel."""
import gc
from types import SimpleNamespace

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

NOISE = 2e-4
TOKENS, ATOMS = [40, 23, 31, 12, 35, 28], [14, 9, 12, 5, 13, 11]


@pytest.fixture(autouse=True, scope="module")
def _free():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def M():
    assert torch.cuda.is_available()
    import mmdti_hip.models.transformers as tr
    import mmdti_hip.models.bert_layers as bl
    return SimpleNamespace(tr=tr, bl=bl)


def _adapt(module, sites, kind, targets, rank, seed):
    """Freeze `module` and hang adapters on its attention modules the way lora.apply_lora does (B non-zero: the adapters are in the forward)."""
    from mmdti_hip.lora import adapter_names
    for p in module.parameters():
        p.requires_grad = False
    g = torch.Generator().manual_seed(seed)
    for att in sites:
        names = adapter_names(kind, targets)
        for _, na, nb, lin in names:
            n_out, n_in = getattr(att, lin).weight.shape
            att.register_parameter(na, nn.Parameter(((torch.rand(rank, n_in, generator=g) * 2 - 1) * n_in ** -0.5).cuda()))
            att.register_parameter(nb, nn.Parameter((torch.randn(n_out, rank, generator=g) * 0.05).cuda()))
        att.lora_targets, att.lora_scale = tuple(s for s, *_ in names), 16.0 / rank


def _seed_params(module, std=0.05):
    with torch.no_grad():
        for i, p in enumerate(module.parameters()):
            p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)) * (std if p.dim() > 1 else 0.1) + (1.0 if p.dim() == 1 and i % 2 == 0 else 0.0))


def _row_bytes(rows):
    return (rows * 32 * 2 + 255) // 256 * 256            # MMDTI_LORA_ROW_BYTES


def _stack_ts(st, nl, rows, ranks):
    """the saved t of every adapter of a stack forward: the rows that end each layer's slice of the arena (ranks: per row, None = no adapter)"""
    arena = st.stack.arena
    stride, row = arena.numel() // nl, _row_bytes(rows)
    out = []
    for l in range(nl):
        base = (l + 1) * stride - len(ranks) * row
        out += [arena[base + j * row:base + j * row + rows * r * 2].view(torch.bfloat16).view(rows, r).clone() for j, r in enumerate(ranks) if r]
    return out


class _Spy:
    """counts the sequencer helpers of functional.py by tag and keeps the saved t of every adapter of the run"""

    def __init__(self, Fn, ops, monkeypatch, tags):
        self.calls, self.ts, self.st = [], [], None
        real = ops.lora_fwd
        monkeypatch.setattr(ops, "lora_fwd", lambda *a, **k: self._keep(real(*a, **k)))
        for name, tag in tags.items():
            monkeypatch.setattr(Fn, name, self._wrap(getattr(Fn, name), tag))

    def _keep(self, t):
        self.ts.append(t.clone())
        return t

    def _wrap(self, real, tag):
        def f(*a, **k):
            self.calls.append(tag)
            r = real(*a, **k)
            if tag in ("F", "uF"):                         # a stack forward: (st, T, ...) -- st.stack holds the arena afterwards
                self.st = a[0]
            elif tag == "f":                               # a BERT-style layer: -> (L, out32, out16), L.lt {target: t}
                self.ts += [t.clone() for t in r[0].lt.values()]
            elif tag == "uf":                              # a Uni-Mol layer: (st, layer, L, ...), L.lt
                self.ts.append(a[2].lt.clone())
            return r
        return f

    def reset(self):
        self.calls, self.ts, self.st = [], [], None


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


def _compare(tag, ref, got, det, base_params):
    """ref / got: (outputs and input gradients [tensors or None], saved t list, {adapter name: gradient})"""
    assert len(ref[0]) == len(got[0])
    for i, (a, b) in enumerate(zip(ref[0], got[0])):
        assert (a is None) == (b is None) and (a is None or _same(a, b)), (tag, "tensor", i)
    assert len(ref[1]) == len(got[1]) > 0 and all(_same(a, b) for a, b in zip(ref[1], got[1])), (tag, "saved t")
    assert set(ref[2]) == set(got[2]) and any(".lora_A" in n for n in ref[2])
    for n in ref[2]:
        a, b = ref[2][n], got[2][n]
        assert float(a.abs().max()) > 0.0, (tag, n)
        if det:
            assert torch.equal(a, b), (tag, n)
        else:
            d = float((a.double() - b.double()).norm()) / (float(a.double().norm()) + 1e-30)
            print(f"{tag} {n}: relative norm {d:.3e}")
            assert d < NOISE, (tag, n, d)
    assert all(p.grad is None for p in base_params)


def _modes(run, spy, counts, det_too=True):
    """OPS, LAYER and STACK runs (counts: the helper tags a LAYER / a STACK run must produce, in order), in the default and the deterministic mode"""
    from mmdti_hip import ops
    try:
        for det in ((False, True) if det_too else (False,)):
            ops.set_deterministic(det)
            res = {}
            for mode in ("ops", "layer", "stack"):
                spy.reset()
                res[mode] = run(mode, spy)
                assert spy.calls == ([] if mode == "ops" else counts[mode]), (mode, spy.calls)
            _compare(f"layer vs ops (det {det})", res["ops"][:3], res["layer"][:3], det, res["ops"][3])
            _compare(f"stack vs layer (det {det})", res["layer"][:3], res["stack"][:3], det, res["ops"][3])
    finally:
        ops.set_deterministic(False)
    return res


# ----------------------------------------------------------------------------------------------------------------------------- tower 2
def _tower2(M, width, rank, targets, emb_trains, layers=2):
    from mmdti_hip.runtime import ParamArena
    heads, ffn = (4, 128) if width == 64 else (8, 256)
    cfg = SimpleNamespace(layers=layers, dim=width, heads=heads, ffn=ffn, vocab=40, max_pos=64, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1,
                          attn_dropout=0.1)
    torch.manual_seed(7)
    tower = M.bl.RobertaTower(cfg).cuda().train()
    _adapt(tower, [l.attention.self for l in tower.layers], "split", targets, rank, seed=5)
    tower.embeddings.word_embeddings.weight.requires_grad = emb_trains
    return tower, ParamArena(tower.parameters())


def _tower2_run(tower, arena, packed, monkeypatch):
    from mmdti_hip import functional as Fn
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.runtime import dropout_state
    B, L = 6, 40
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(4, 40, (B, L), generator=g)
    am = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(TOKENS):
        am[b, :n] = 1
        ids[b, n:] = 1
    ids, am = ids.cuda(), am.cuda()
    pk = PackedRows(torch.tensor(TOKENS), L, "cuda") if packed else None
    rows = pk.M if packed else B * L
    nl = len(tower.layers)
    ranks = [getattr(tower.layers[0].attention.self, f"lora_A_{t}").shape[0] if t in tower.layers[0].attention.self.lora_targets else None for t in "qkv"]
    base = [p for p in tower.parameters() if not p.requires_grad]

    def run(mode, spy):
        monkeypatch.setattr(Fn, "LORA_SEQ", mode != "ops")
        monkeypatch.setattr(Fn, "STACK_SEQ", mode == "stack")
        arena.zero_grad()
        dropout_state.reseed(777)
        out = tower(ids, am, return_dict=True, pack=pk)[0]
        ts = _stack_ts(spy.st, nl, rows, ranks) if spy.st is not None else list(spy.ts)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return [out.detach().clone()], ts, {n: p.grad.clone() for n, p in tower.named_parameters() if p.grad is not None}, base
    return run, rows


BERT_TAGS = {"_bert_layer_fwd_seq": "f", "_bert_layer_bwd_seq": "b", "_bert_stack_fwd": "F", "_bert_stack_bwd": "B"}


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("targets", [("q", "v"), ("k",), ("q", "k", "v")])
@pytest.mark.parametrize("width, rank", [(64, 8), (512, 8), (512, 32)])
def test_tower2_adapted_layers_leave_from_the_library(M, width, rank, targets, packed, f16, monkeypatch):
    """the word embeddings train in two of the three target sets: the lowest layer then hands its input gradient down (want_ds1), and the
    table's gradient -- collected by one-hot GEMMs with atomics -- is held to the band of the adapters'"""
    from mmdti_hip import functional as Fn, ops
    monkeypatch.setattr(ops, "FWD_F16", f16)
    tower, arena = _tower2(M, width, rank, targets, emb_trains=targets != ("k",))
    run, rows = _tower2_run(tower, arena, packed, monkeypatch)
    assert rows == (174 if packed else 240)             # (packed: the 169 real tokens and one representative pad row per shorter sequence)
    spy = _Spy(Fn, ops, monkeypatch, BERT_TAGS)
    _modes(run, spy, {"layer": ["f", "f", "b", "b"], "stack": ["F", "B"]})


def test_tower2_stack_tables_follow_a_recast_frozen_weight(M, monkeypatch):
    """an in-place write to a FROZEN weight (merge_lora, a checkpoint loaded into a bound model) re-casts its 16-bit shadow into new
    storage: the cached tables of the adapted stack are built again"""
    from mmdti_hip import functional as Fn, ops
    tower, arena = _tower2(M, 64, 8, ("q", "v"), emb_trains=False)
    run, _ = _tower2_run(tower, arena, True, monkeypatch)
    spy = _Spy(Fn, ops, monkeypatch, BERT_TAGS)
    res = _modes(run, spy, {"layer": ["f", "f", "b", "b"], "stack": ["F", "B"]}, det_too=False)
    with torch.no_grad():
        tower.layers[1].intermediate.dense.weight.mul_(0.5)
        tower.layers[0].attention.self.value.weight.mul_(1.5)
    after = _modes(run, spy, {"layer": ["f", "f", "b", "b"], "stack": ["F", "B"]}, det_too=False)
    assert not torch.equal(after["stack"][0][0], res["stack"][0][0])


# ----------------------------------------------------------------------------------------------------------------------------- tower 1
UNI_TAGS = {"_unimol_layer_fwd_seq": "uf", "_unimol_layer_bwd_seq": "ub", "_unimol_stack_fwd": "uF", "_unimol_stack_bwd": "uB"}


def _tower1(M, D, rank, layers=2):
    from mmdti_hip.runtime import ParamArena
    H, ffn = D // 8, (128 if D == 64 else 256)
    torch.manual_seed(11)
    enc = M.tr.TransformerEncoderWithPair(encoder_layers=layers, embed_dim=D, ffn_embed_dim=ffn, attention_heads=H, no_final_head_layer_norm=True).cuda().train()
    _seed_params(enc)
    _adapt(enc, [l.self_attn for l in enc.layers], "fused", ("q",), rank, seed=9)
    return enc, ParamArena(enc.parameters()), H


def _tower1_run(enc, arena, H, rank, packed, null_dx, monkeypatch):
    from mmdti_hip import functional as Fn
    from mmdti_hip.functional import PairCompactFn
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.runtime import dropout_state
    B, N, D = 6, 14, enc.embed_dim
    g = torch.Generator().manual_seed(6)
    pad = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(ATOMS):
        pad[b, n:] = True
    emb, bias0 = torch.randn(B, N, D, generator=g).cuda(), torch.randn(B, H, N, N, generator=g).cuda()
    counts = torch.tensor(ATOMS)
    kt = ((counts + 15) // 16).to(torch.int32).cuda()
    pk = PackedRows(counts, N, "cuda") if packed else None
    rows = pk.M if packed else B * N
    nl = len(enc.layers)
    base = [p for p in enc.parameters() if not p.requires_grad]

    def run(mode, spy):
        monkeypatch.setattr(Fn, "LORA_SEQ", mode != "ops")
        monkeypatch.setattr(Fn, "STACK_SEQ", mode == "stack")
        arena.zero_grad()
        dropout_state.reseed(4242)
        bias = bias0.clone().requires_grad_()
        e = (emb.reshape(B * N, D)[pk.gather] if packed else emb).clone().requires_grad_(not null_dx)
        planes = PairCompactFn.apply(bias, N)              # the compact fp16 planes the ragged / packed pair kernels (and every mode's sequencers) take
        x = enc.encode(e, planes, pad.cuda().reshape(-1)[pk.gather] if packed else pad.cuda(), kt, pack=pk)[0]
        ts = _stack_ts(spy.st, nl, rows, [rank]) if mode == "stack" else list(spy.ts)
        w = torch.randn(x.shape, generator=torch.Generator().manual_seed(9)).cuda()
        (x * w).sum().backward()
        torch.cuda.synchronize()
        assert bias.grad is not None and float(bias.grad.abs().max()) > 0.0
        return ([x.detach().clone(), None if null_dx else e.grad.clone(), bias.grad.clone()], ts,
                {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}, base)
    return run


@pytest.mark.parametrize("f16", [True, False])
@pytest.mark.parametrize("null_dx", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("D, rank", [(64, 8), (512, 16)])
def test_tower1_adapted_layers_leave_from_the_library(M, D, rank, packed, null_dx, f16, monkeypatch):
    """null_dx: the embeddings need no gradient, so the lowest layer gets a null dx_out -- its in_proj input gradient, the adapter's dx and
    the LayerNorm-1 backward are not launched; the pair-gradient chain still runs through every layer (the bias needs its gradient)"""
    from mmdti_hip import functional as Fn, ops
    monkeypatch.setattr(ops, "FWD_F16", f16)
    enc, arena, H = _tower1(M, D, rank)
    run = _tower1_run(enc, arena, H, rank, packed, null_dx, monkeypatch)
    spy = _Spy(Fn, ops, monkeypatch, UNI_TAGS)
    _modes(run, spy, {"layer": ["uf", "uf", "ub", "ub"], "stack": ["uF", "uB"]})


def test_tower1_stack_tables_follow_a_recast_frozen_weight(M, monkeypatch):
    from mmdti_hip import functional as Fn, ops
    enc, arena, H = _tower1(M, 64, 8)
    run = _tower1_run(enc, arena, H, 8, True, False, monkeypatch)
    spy = _Spy(Fn, ops, monkeypatch, UNI_TAGS)
    counts = {"layer": ["uf", "uf", "ub", "ub"], "stack": ["uF", "uB"]}
    res = _modes(run, spy, counts, det_too=False)
    with torch.no_grad():
        enc.layers[1].fc1.weight.mul_(0.5)
    after = _modes(run, spy, counts, det_too=False)
    assert not torch.equal(after["stack"][0][0], res["stack"][0][0])


def test_a_partly_trainable_base_layer_runs_op_by_op(M, monkeypatch):
    from mmdti_hip import functional as Fn, ops
    tower, _ = _tower2(M, 64, 8, ("q", "v"), emb_trains=False)
    tower.layers[1].output.dense.bias.requires_grad = True
    from mmdti_hip.runtime import ParamArena
    run, _ = _tower2_run(tower, ParamArena(tower.parameters()), False, monkeypatch)
    spy = _Spy(Fn, ops, monkeypatch, BERT_TAGS)
    run("stack", spy)
    assert spy.calls == ["f", "b"]                       # (each layer decides for itself: the fully frozen one still takes its call)
    assert float(tower.layers[1].output.dense.bias.grad.abs().max()) > 0.0


def test_a_base_parameter_replaced_by_assignment_is_seen(M, monkeypatch):
    """the kept parameter lists and the cached stack tables follow the layer's parameter OBJECTS: a trainable replacement sends its layer
    op by op (and gets its gradient), a frozen one at a new address is what the rebuilt tables point at"""
    from mmdti_hip import functional as Fn, ops
    tower, arena = _tower2(M, 64, 8, ("q", "v"), emb_trains=False)
    run, _ = _tower2_run(tower, arena, False, monkeypatch)
    spy = _Spy(Fn, ops, monkeypatch, BERT_TAGS)
    first = run("stack", spy)
    assert spy.calls == ["F", "B"]
    dense = tower.layers[1].output.dense
    old = dense.bias
    dense.bias = nn.Parameter(old.detach().clone())
    spy.reset()
    run("stack", spy)
    assert spy.calls == ["f", "b"] and float(dense.bias.grad.abs().max()) > 0.0
    dense.bias = nn.Parameter(old.detach() + 0.5, requires_grad=False)
    spy.reset()
    a = run("stack", spy)
    assert spy.calls == ["F", "B"]
    spy.reset()
    b = run("ops", spy)
    assert torch.equal(a[0][0], b[0][0]) and not torch.equal(a[0][0], first[0][0])


# ----------------------------------------------------------------------------------------------------------------------------- cross layer
@pytest.mark.parametrize("want_ds2", [True, False])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("targets", [("q", "v"), ("k",)])
@pytest.mark.parametrize("width, rank", [(64, 8), (512, 32)])
def test_cross_adapted_layer_leaves_from_the_library(M, width, rank, targets, packed, want_ds2, monkeypatch):
    """14 atoms attend to 40 tokens; want_ds2 False: the token side needs no gradient, its two input-gradient products and the key / value
    adapters' dx are not launched (their mmdti_lora_bwd still is)"""
    from mmdti_hip import functional as Fn, ops
    from mmdti_hip.packing import PackedRows
    from mmdti_hip.runtime import dropout_state, ParamArena
    heads, ffn = (4, 128) if width == 64 else (8, 256)
    ccfg = SimpleNamespace(hidden_size=width, num_attention_heads=heads, intermediate_size=ffn, attention_probs_dropout_prob=0.1, hidden_dropout_prob=0.1,
                           hidden_act="gelu", layer_norm_eps=1e-12)
    enc = M.bl.BertCrossEncoder(ccfg, 1).cuda().train()
    _seed_params(enc)
    _adapt(enc, [l.attention.self for l in enc.layer], "split", targets, rank, seed=13)
    arena = ParamArena(enc.parameters())
    B, Lq, Lk = 6, 14, 40
    g = torch.Generator().manual_seed(11)
    s1, s2 = torch.randn(B, Lq, width, generator=g).cuda(), torch.randn(B, Lk, width, generator=g).cuda()
    mask2 = torch.zeros(B, Lk)
    for b, n in enumerate(TOKENS):
        mask2[b, :n] = 1
    ext = ((1.0 - mask2) * -10000.0).view(B, 1, 1, Lk).cuda()
    pq, pk = (PackedRows(torch.tensor(ATOMS), Lq, "cuda"), PackedRows(torch.tensor(TOKENS), Lk, "cuda")) if packed else (None, None)
    base = [p for p in enc.parameters() if not p.requires_grad]

    def run(mode, spy):
        monkeypatch.setattr(Fn, "LORA_SEQ", mode != "ops")
        arena.zero_grad()
        dropout_state.reseed(31)
        if packed:
            a = s1.reshape(B * Lq, width)[pq.gather].clone().requires_grad_()
            b_ = s2.reshape(B * Lk, width)[pk.gather].clone().requires_grad_(want_ds2)
            out = enc(a, b_, None, packs=(pq, pk))[-1]
        else:
            a, b_ = s1.clone().requires_grad_(), s2.clone().requires_grad_(want_ds2)
            out = enc(a, b_, ext)[-1]
        ts = list(spy.ts)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
        (out * w).sum().backward()
        torch.cuda.synchronize()
        assert (b_.grad is not None) == want_ds2
        return ([out.detach().clone(), a.grad.clone(), b_.grad.clone() if want_ds2 else None], ts,
                {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}, base)

    spy = _Spy(Fn, ops, monkeypatch, {"_bert_cross_layer_fwd_seq": "f", "_bert_cross_layer_bwd_seq": "b"})
    try:
        for det in (False, True):
            ops.set_deterministic(det)
            res = {}
            for mode in ("ops", "layer"):
                spy.reset()
                res[mode] = run(mode, spy)
                assert spy.calls == ([] if mode == "ops" else ["f", "b"]), (mode, spy.calls)
            _compare(f"layer vs ops (det {det})", res["ops"][:3], res["layer"][:3], det, base)
    finally:
        ops.set_deterministic(False)


# ----------------------------------------------------------------------------------------------------------------------------- the engine
ENGINE_TAGS = {"_bert_stack_fwd": "F", "_bert_stack_bwd": "B", "_bert_cross_layer_fwd_seq": "cf", "_bert_cross_layer_bwd_seq": "cb",
               "_bert_layer_fwd_seq": "f", "_unimol_layer_fwd_seq": "uf", "_unimol_stack_fwd": "uF"}


def _engine_steps(seq, steps, monkeypatch, deterministic, calls=None, packed=False):
    """`steps` optimizer steps of the tiny adapted model of tests/test_lora_gpu.py -> (losses, parameters)"""
    from mmdti_hip import functional as Fn
    from mmdti_hip.collate import device_payload
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    from test_lora_gpu import _batch, _bits, _lora_model
    monkeypatch.setattr(Fn, "LORA_SEQ", seq)
    if calls is not None:
        for name, tag in ENGINE_TAGS.items():
            monkeypatch.setattr(Fn, name, (lambda real, tag: lambda *a, **k: (calls.append(tag), real(*a, **k))[1])(getattr(Fn, name), tag))
    batch, label, dev = _batch()
    model = _lora_model(b_seed=21)
    tuner = FineTuner(model, "classification", total_steps=10, learning_rate=1e-3, deterministic=deterministic)
    if packed:
        model.strict_reference = False
        full = device_payload(batch)
        dev.update({k: full[k] for k in ("atom_counts", "token_counts", "token_pad_id", "packable")})
    dropout_state.reseed(99)
    losses = [_bits(tuner.step(dev, label.cuda()).loss) for _ in range(steps)]
    torch.cuda.synchronize()
    assert model.last_layout == ("packed" if packed else "padded")
    return losses, {n: _bits(p) for n, p in model.named_parameters()}


@pytest.mark.parametrize("packed", [False, True])
def test_engine_steps_are_the_op_by_op_steps_bit_for_bit_in_the_deterministic_mode(packed, monkeypatch):
    from mmdti_hip import ops
    try:
        calls = []
        on = _engine_steps(True, 2, monkeypatch, True, calls, packed)
        # tower 2 from its stack calls, both cross layers from their per-layer calls; packed rows bring tower 1 its compact planes
        assert calls.count("F") == 2 and calls.count("B") == 2 and calls.count("cf") == 4 and calls.count("cb") == 4, calls
        assert not packed or "uF" in calls or "uf" in calls, calls
        monkeypatch.undo()
        del calls[:]
        off = _engine_steps(False, 2, monkeypatch, True, calls, packed)
        assert not calls
        assert all(torch.equal(a, b) for a, b in zip(on[0], off[0]))
        assert on[1].keys() == off[1].keys() and all(torch.equal(on[1][n], off[1][n]) for n in on[1])
    finally:
        ops.set_deterministic(False)


def test_engine_first_loss_is_the_op_by_op_one_in_the_default_mode(monkeypatch):
    on = _engine_steps(True, 1, monkeypatch, False)
    monkeypatch.undo()
    off = _engine_steps(False, 1, monkeypatch, False)
    assert torch.equal(on[0][0], off[0][0])


def test_graphed_steps_replay_the_eager_ones_with_the_sequencers_on(monkeypatch):
    from mmdti_hip import functional as Fn, ops
    from mmdti_hip.trainer import FineTuner
    from test_lora_gpu import _batch, _lora_model
    calls = []
    for name, tag in ENGINE_TAGS.items():
        monkeypatch.setattr(Fn, name, (lambda real, tag: lambda *a, **k: (calls.append(tag), real(*a, **k))[1])(getattr(Fn, name), tag))
    _, label, dev = _batch(ragged=False)
    y = label.cuda()
    try:
        assert Fn.LORA_SEQ
        eager = FineTuner(_lora_model(b_seed=7), "classification", total_steps=20, learning_rate=1e-3)
        state = {k: v.clone() for k, v in eager.model.state_dict().items()}
        graphed = FineTuner(_lora_model(), "classification", total_steps=20, learning_rate=1e-3)
        graphed.model.load_state_dict(state)
        for _ in range(4):
            a, b = eager.step(dev, y), graphed.graphed_step(dev, y)
        torch.cuda.synchronize()
        assert len(graphed._graphs) == 1 and "F" in calls and "cf" in calls
        la, lb = float(a.loss), float(b.loss)
        print(f"eager {la:.6f} graphed {lb:.6f}")
        assert abs(la - lb) <= 1e-4 * max(1.0, abs(la))
        for (n, p), (_, q) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
            if ".lora_" in n:
                assert torch.allclose(p.detach(), q.detach(), rtol=1e-3, atol=1e-5), n
    finally:
        ops.seed_salt_reset()
