"""MM_Model.attention_maps on the device: a 2-layer-per-tower model of width 512 (64 / 8 / 16 heads: the reference's head sizes) and
three molecules of 5 / 17 / 33 atom tokens and 4 / 20 / 40 SMILES tokens, in the padded layout and on packed rows.

  * every map of either layout lies inside the bound of the float64 reference (tests/maps_cases.py) built from what THAT pass's map
    kernel read -- q, k, the key mask (tower 2, cross block) or the stored logits (tower 1) --, is zero outside real x real, and its
    rows over real queries sum to 1 within (Lk + 8) 2^-23; the two layouts' maps then agree within the sum of their bounds;
  * tower 2 and cross maps against the head mean of the bf16 probabilities L.p of a pass with ops.FUSED_ATTN = False: 2^-8 relative
    per probability (the bf16 store) plus the bound;
  * the last Uni-Mol map against the float64 softmax of the S_last the encoder returns;
  * `outputs` equals model(**net_input) under no_grad, bit for bit;
  * a training step before and after an attention_maps call gives the bits of two steps without it (deterministic mode);
  * the recorder refuses a forward that keeps activations for a backward, and a live dropout."""
import numpy as np
import pytest
import torch

from mmdti_hip import ops
from mmdti_hip._abi import MMDTIError

from oracle import mmdti_oracle as O
from g9util import tiny_cfg, product_model, load_fixture_weights, host_fields
import maps_cases as M

pytestmark = pytest.mark.gpu
ATOMS, TOKENS = (5, 17, 33), (4, 20, 40)
EPS = 2.0 ** -23
ALL = ("cross", "unimol", "bert")


def _cfg():
    ocfg = tiny_cfg("classification", 40)
    ocfg.unimol = O.UniMolCfg(layers=2, dim=512, ffn=256, heads=64, K=128, vocab=31)
    ocfg.cross, ocfg.roberta = O.CrossCfg(dim=512, heads=16, ffn=128), O.RobertaCfg(layers=2, dim=512, heads=8, ffn=128, vocab=40, max_pos=48)
    return ocfg


def _batch(ocfg, seed=7):
    from mmdti_hip.synth import molecule
    from mmdti_hip.collate import right_pad
    rng = np.random.default_rng(seed)
    V = ocfg.unimol.vocab
    elem_p = np.zeros(V)
    elem_p[8], elem_p[4], elem_p[5], elem_p[6] = 0.5, 0.3, 0.1, 0.1
    toks, dists, edges, ids = [], [], [], []
    for na, nt in zip(ATOMS, TOKENS):
        t, d, e = molecule(rng, na - 2, V, elem_p)
        toks.append(torch.from_numpy(t)); dists.append(torch.from_numpy(d)); edges.append(torch.from_numpy(e))
        ids.append(torch.from_numpy(np.concatenate([[0], rng.integers(4, ocfg.roberta.vocab, size=nt - 2), [2]]).astype(np.int64)))
    input_ids = right_pad(ids, 1)
    return {"src_tokens": right_pad(toks, 0), "src_distance": right_pad(dists, 0.0, square=True), "src_edge_type": right_pad(edges, 0, square=True),
            "input_ids": input_ids, "attention_mask": input_ids.ne(1).long()}


@pytest.fixture(scope="module")
def world():
    ocfg = _cfg()
    model = product_model(ocfg).cuda().eval()
    load_fixture_weights(model, O.init_params(ocfg, seed=5, std=0.05))
    batch = _batch(ocfg)
    dev = {k: v.cuda() for k, v in batch.items()}
    host = host_fields(batch)
    assert host["packable"]
    w = dict(model=model, dev=dev, host=host)

    def run(layout, fused=True):
        from mmdti_hip.functional import AttentionRecorder
        rec = AttentionRecorder(ALL, "all", "mean")
        rec.keep_operands = True
        old = ops.FUSED_ATTN
        ops.FUSED_ATTN = fused
        try:
            am = model.attention_maps(**dev, **dict(host, packable=layout == "packed"), which=rec)
        finally:
            ops.FUSED_ATTN = old
        torch.cuda.synchronize()
        assert model.last_layout == layout
        return am, rec

    w["padded"], w["packed"] = run("padded"), run("packed")
    w["unfused"] = run("padded", fused=False)
    return w


def _names(am):
    return [(n, l, m) for n in ("text_to_graph", "graph_to_text", "unimol", "bert") for l, m in sorted(getattr(am, n).items())]


def _lengths(name):
    q = ATOMS if name in ("unimol", "graph_to_text") else TOKENS
    k = ATOMS if name in ("unimol", "text_to_graph") else TOKENS
    return q, k


def _reference(name, op):
    """float64 reference and bound of one recorded map from what its kernel read"""
    if name == "unimol":
        S = ops.pair_untile(op.s, op.N).float().cpu()
        nt = M.cdiv(op.N, 16)
        lens = op.n_real.tolist()
        for b, n in enumerate(lens):                   # what the forward never stored: -inf keys (not read), rows the reference zeroes
            k0 = 16 * M.pa_kt_effective(int(op.key_tiles[b]), nt) if op.key_tiles is not None else op.N
            S[b, :, :, k0:] = float("-inf")
            S[b, :, n:, :] = 0.0
            assert bool(torch.isinf(S[b, :, :n, n:]).all()) and bool(torch.isfinite(S[b, :, :n, :n]).all())
        c = dict(B=op.B, H=op.H, N=op.N, ld_out=op.N, lens=lens, layout=3)
        return M.pair_reference(c, dict(S=S, lens=lens))
    B, H = op.B, op.heads
    hd = op.q.shape[1] // H
    if op.vl is None:
        seqs = [(b * op.Lq, op.Lq, b * op.Lk, op.Lk, op.Lk) for b in range(B)]
    else:
        qo, ko, kc = op.vl.q_off.tolist(), op.vl.k_off.tolist(), op.vl.k_cnt.tolist()
        seqs = [(qo[b], qo[b + 1] - qo[b], ko[b], kc[b], ko[b + 1] - ko[b]) for b in range(B)]
    t = dict(seqs=seqs, q=op.q.contiguous().cpu(), k=op.k.contiguous().cpu(), add=None if op.key_add is None else op.key_add.reshape(B, -1).cpu(),
             scale=hd ** -0.5)
    c = dict(hd=hd, heads=H, B=B, Lq_out=op.Lq_out, ld_out=op.ld_out, qcnt=None if op.q_cnt is None else op.q_cnt.tolist())
    return M.attn_reference(c, t)


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_maps_inside_their_reference_and_zero_on_padding(world, layout):
    am, rec = world[layout]
    assert sorted(am.unimol) == [0, 1] and sorted(am.bert) == [0, 1] and sorted(am.text_to_graph) == [0] and sorted(am.graph_to_text) == [0]
    N, L = max(ATOMS), max(TOKENS)
    shapes = {"unimol": (3, N, N), "bert": (3, L, L), "text_to_graph": (3, L, N), "graph_to_text": (3, N, L)}
    for name, l, m in _names(am):
        assert tuple(m.shape) == shapes[name] and m.dtype == torch.float32 and bool(torch.isfinite(m).all()), (name, l)
        ref, bnd = _reference(name, rec.operands[name][l])
        ratio = M.worst_ratio(m.cpu(), ref, bnd)
        print(layout, name, l, "ratio", round(ratio, 4))
        assert ratio <= 1.0, (layout, name, l, ratio)
        ql, kl = _lengths(name)
        for b in range(3):
            assert float(m[b, ql[b]:].abs().max() if ql[b] < m.shape[1] else 0.0) == 0.0, (name, l, b, "a padded query row")
            assert float(m[b, :, kl[b]:].abs().max() if kl[b] < m.shape[2] else 0.0) == 0.0, (name, l, b, "a padded key")
            rows = m[b, :ql[b], :kl[b]].double().sum(-1)
            assert float((rows - 1.0).abs().max()) <= (kl[b] + 8) * EPS, (name, l, b, float((rows - 1.0).abs().max()))


def test_padded_and_packed_agree(world):
    """each layout is held to the reference of its own operands (above), so the two maps differ by no more than the sum of the two bounds
    and the distance of the two references (the towers round layout-dependently below the map kernels)"""
    (a, ra), (p, rp) = world["padded"], world["packed"]
    for (name, l, ma), (_, _, mp) in zip(_names(a), _names(p)):
        refa, ba = _reference(name, ra.operands[name][l])
        refp, bp = _reference(name, rp.operands[name][l])
        d = (ma.cpu().double() - mp.cpu().double()).abs()
        print(name, l, "padded - packed", float(d.max()), "references", float((refa - refp).abs().max()))
        assert bool((d <= ba + bp + (refa - refp).abs()).all()), (name, l, float(d.max()))


def test_fused_maps_against_materialised_probabilities(world):
    (a, ra), (u, ru) = world["padded"], world["unfused"]
    for name in ("bert", "text_to_graph", "graph_to_text"):
        for l in getattr(a, name):
            op = ru.operands[name][l]
            assert op.p is not None and op.stats is None, "the unfused pass must run the materialised-scores path"
            # the recorder's reduction of L.p: the head mean of the stored bf16 probabilities
            want = op.p[..., :op.Lk].double().mean(1).cpu()
            for b, n in enumerate(op.q_cnt.tolist()):
                want[b, n:] = 0
            mu = getattr(u, name)[l].cpu().double()
            assert float((mu - want).abs().max()) <= (op.heads + 2) * EPS, (name, l)
            # fused map against it: 2^-8 relative per probability (the bf16 store of p) plus the bound of each side's float64 reference
            # (its own q, k) and the distance of the two references
            refa, bnda = _reference(name, ra.operands[name][l])
            refu, bndu = _reference(name, op)
            d = (getattr(a, name)[l].cpu().double() - mu).abs()
            print(name, l, "fused - materialised", float(d.max()))
            assert bool((d <= 2.0 ** -8 * refu + bnda + bndu + (refa - refu).abs()).all()), (name, l, float(d.max()))


def test_last_unimol_map_is_the_softmax_of_the_returned_logits(world):
    model, dev, host = world["model"], world["dev"], world["host"]
    seen = {}
    real = model.encoder.encode

    def spy(*a, **k):
        out = real(*a, **k)
        seen["S"] = out[1]
        return out

    model.encoder.encode = spy
    try:
        am = model.attention_maps(**dev, **dict(host, packable=False), which=("unimol",), layers="last")
    finally:
        del model.encoder.encode
    N = max(ATOMS)
    S = ops.pair_untile(seen["S"], N).double().cpu()
    p = torch.softmax(S, -1).mean(1)
    m = am.unimol[1].cpu().double()
    assert sorted(am.unimol) == [1]
    for b, n in enumerate(ATOMS):
        ref, bnd = M.pair_reference(dict(B=1, H=S.shape[1], N=N, ld_out=N, lens=[n], layout=3), dict(S=S[b:b + 1].float(), lens=[n]))
        assert float((ref[0, :n] - p[b, :n]).abs().max()) <= 1e-12
        assert M.worst_ratio(m[b:b + 1], ref, bnd) <= 1.0, b


def test_head_selection_and_layers(world):
    model, dev, host = world["model"], world["dev"], world["host"]
    full = world["packed"][0]
    heads = [model.attention_maps(**dev, **dict(host, packable=True), which=("cross",), head=h).text_to_graph[0] for h in range(16)]
    mean = torch.stack(heads).double().mean(0)
    assert float((mean - full.text_to_graph[0].double()).abs().max()) <= 20 * EPS
    one = model.attention_maps(**dev, **host, which=("bert",), layers=[0])
    assert sorted(one.bert) == [0] and not one.unimol and not one.text_to_graph
    with pytest.raises(MMDTIError, match="head 16 asked of an attention with 16 heads"):
        model.attention_maps(**dev, **host, which=("cross",), head=16)


def test_outputs_are_the_forward_and_relevance_sums_to_one(world):
    model, dev, host = world["model"], world["dev"], world["host"]
    for layout in ("padded", "packed"):
        kw = dict(host, packable=layout == "packed")
        with torch.no_grad():
            want = model(**dev, **kw)
        am = model.attention_maps(**dev, **kw)
        assert torch.equal(am.outputs, want), layout
        assert not model.training
        ar, tr = am.atom_relevance(), am.token_relevance()
        assert ar.shape == (3, max(ATOMS)) and tr.shape == (3, max(TOKENS))
        for b in range(3):
            assert abs(float(ar[b].double().sum()) - 1.0) <= 64 * EPS and abs(float(tr[b].double().sum()) - 1.0) <= 64 * EPS
            assert float(ar[b, ATOMS[b]:].abs().sum()) == 0.0 and float(tr[b, TOKENS[b]:].abs().sum()) == 0.0
    model.train()
    try:
        am = model.attention_maps(**dev, **host)            # a training-mode model: the pass itself is an eval pass, the mode comes back
        assert model.training and all(m.training for m in model.modules())
        assert torch.equal(am.outputs, want)
    finally:
        model.eval()


def test_a_training_step_is_the_same_with_a_recording_in_between():
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    ocfg = _cfg()
    batch = _batch(ocfg)
    host = host_fields(batch)
    label = torch.tensor([[0], [1], [0]])

    def run(record):
        torch.manual_seed(0)
        model = product_model(ocfg, dropout=True).cuda().train()
        load_fixture_weights(model, O.init_params(ocfg, seed=5, std=0.05))
        dropout_state.reseed(77)
        tuner = FineTuner(model, "classification", learning_rate=1e-3, warmup_ratio=0.25, total_steps=8, max_norm=5.0, deterministic=True)
        dev = {k: v.cuda() for k, v in batch.items()}
        try:
            tuner.step(dict(dev, **host), label.cuda())
            if record:
                am = model.attention_maps(**dev, **host, which=ALL, layers="all")
                assert model.training and len(am.unimol) == 2
            tuner.step(dict(dev, **host), label.cuda())
            torch.cuda.synchronize()
            a = tuner.arena
            return a.data.clone(), a.adam_m.clone(), a.adam_v.clone()
        finally:
            ops.set_deterministic(False)

    plain, recorded = run(False), run(True)
    for what, a, b in zip(("parameters", "adam_m", "adam_v"), plain, recorded):
        assert torch.equal(a, b), what


def test_recorder_refuses_a_backward_and_a_live_dropout(world):
    from mmdti_hip.functional import record_attention, attention_recorder
    dev, host = world["dev"], world["host"]
    ocfg = _cfg()
    model = product_model(ocfg, dropout=True).cuda()
    assert attention_recorder() is None
    model.eval()
    with record_attention(dict(which=ALL)) as rec:
        assert attention_recorder() is rec
        with pytest.raises(MMDTIError, match="keeps activations for a backward"):
            model(**dev, **host)                       # parameters need gradients, no torch.no_grad(): this forward would keep its activations
    assert attention_recorder() is None
    model.train()
    with record_attention(dict(which=ALL)), torch.no_grad():
        with pytest.raises(MMDTIError, match="live dropout"):
            model(**dev, **host)
    assert attention_recorder() is None
    with record_attention(dict(which=("cross",))):
        with pytest.raises(MMDTIError, match="already live"):
            with record_attention(dict(which=("cross",))):
                pass
