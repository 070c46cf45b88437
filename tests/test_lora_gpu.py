"""LoRA adapters through the model and the engine (lora.apply_lora, DESIGN.md "LoRA adapters") on the tiny synthetic model the freeze
and trainer tests use (width 64, two layers per tower): a fresh adapter (B = 0) changes no bit of the forward; adapter and head
gradients against the oracle's autograd on the merged weights W + s.B.A, within the bands tests/test_freeze_gpu.py grants the weight
gradients of the same layers (relative error 3.2e-2, cosine 0.9996); frozen base parameters never move; merge_lora reproduces the
adapted forward and its attention maps; graphed steps, the state round trip, packed rows, coordinate inputs, accumulated steps with
union negatives, the one-rank reducer and the Trainer."""
import gc
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from test_trainer_gpu import _model, _ocfg

REL, COS = 3.2e-2, 0.9996          # tests/test_freeze_gpu.py::test_recipe_step
ZERO_GRADS = ("pooler", "key.bias", "gbf_proj.linear2.bias")
TARGETS = ("q", "k", "v")


@pytest.fixture(autouse=True, scope="module")
def _free_tuners():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu()


def _batch(seed=3, B=6, ragged=True):
    batch, label = O.synth_batch(B, 10, 14, _ocfg("classification", 2), seed=seed, ragged=ragged)
    return batch, label, {k: v.cuda() for k, v in batch.items()}


def _lora_model(rank=8, targets=TARGETS, towers=None, b_seed=None, state=None):
    from mmdti_hip import lora
    model = _model("classification", 2).eval()
    if state is not None:
        model.load_state_dict(state)
    cfg = lora.LoRAConfig(rank=rank, alpha=16.0, targets=targets, towers=towers or lora.TOWERS, seed=4)
    lora.apply_lora(model, cfg)
    if b_seed is not None:
        g = torch.Generator().manual_seed(b_seed)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if ".lora_B" in n:
                    p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(p.device))
    return model


def test_fresh_adapters_leave_the_forward_bit_identical(monkeypatch):
    from mmdti_hip import functional, lora
    monkeypatch.setattr(functional, "LAYER_SEQ", False)                # the op-by-op path on both sides
    _, _, dev = _batch()
    plain = _model("classification", 2).eval()
    state = {k: v.clone() for k, v in plain.state_dict().items()}
    for n, p in plain.named_parameters():
        if n.startswith(tuple(q for t in lora.TOWERS for q in lora.TOWER_PREFIXES[t])):
            p.requires_grad = False
    adapted = _lora_model(state=state)
    with torch.no_grad():
        a, b = plain(**dev), adapted(**dev)
    assert torch.equal(_bits(a), _bits(b))
    # and a non-zero B does change it (the adapters are in the forward)
    with torch.no_grad():
        for n, p in adapted.named_parameters():
            if ".lora_B" in n:
                p.fill_(0.05)
        c = adapted(**dev)
    assert not torch.equal(_bits(a), _bits(c))


def _oracle(model, batch, label):
    """autograd through the oracle on the merged weights W + s.B.A, the adapters as leaves -> dict(loss, infonce, ct, grads)"""
    from mmdti_hip import lora
    P = {k: v.detach().cpu().float().clone().requires_grad_() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    names = {id(m): n for n, m in model.named_modules()}
    Pm = {k: v for k, v in P.items() if ".lora_" not in k}
    for att, na, nb, lin in lora._adapters(model):
        pre = names[id(att)]
        Pm[f"{pre}.{lin}.weight"] = P[f"{pre}.{lin}.weight"] + att.lora_scale * (P[f"{pre}.{nb}"] @ P[f"{pre}.{na}"])
    ocfg = _ocfg("classification", 2)
    ref = O.mm_forward(batch, Pm, ocfg, net_target=label, bf16=True)
    loss, _ = O.step_loss(ref, label, "classification")
    loss.backward()
    return dict(loss=loss.detach(), infonce=ref["infonce"].detach(), ct=ref["ct"].detach(), grads={k: v.grad for k, v in P.items() if v.grad is not None})


def _oracle_grads(model, batch, label):
    return {k: g for k, g in _oracle(model, batch, label)["grads"].items()}


@pytest.mark.parametrize("layout", ["padded", "packed", "coords"])
def test_adapter_and_head_gradients_and_frozen_base(layout):
    """coords: the batch carries src_coord and no [B, N, N] plane (pair_inputs="coords"); the oracle reads the stored planes of the same
    molecules"""
    from mmdti_hip.collate import device_payload
    from mmdti_hip.trainer import FineTuner
    batch, label, dev = _batch()
    if layout == "coords":
        from mmdti_hip.synth import synth_batch
        full, label = synth_batch(6, 10, 14, seed=3, ragged=True, smiles_vocab=40, with_coord=True)
        batch = {k: v for k, v in full.items() if k != "src_coord"}
        dev = {k: v.cuda() for k, v in full.items() if k not in ("src_distance", "src_edge_type")}
        assert "src_coord" in dev
    model = _lora_model(b_seed=11)
    g_ref = _oracle_grads(model, batch, label)
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and all(".lora_" not in n for n in frozen)
    tuner = FineTuner(model, "classification", total_steps=10, learning_rate=1e-3)
    if layout == "packed":
        model.strict_reference = False
        full = device_payload(batch)
        dev.update({k: full[k] for k in ("atom_counts", "token_counts", "token_pad_id", "packable")})
    else:
        model.strict_reference = True
    tuner.forward_backward(dev, label.cuda())
    torch.cuda.synchronize()
    assert model.last_layout == ("packed" if layout == "packed" else "padded")
    worst, cos_min = ("", 0.0), 1.0
    # tower 1: one pair per layer; tower 2's two layers and the two cross layers: q, k, v each
    assert sum(".lora_" in n and p.requires_grad for n, p in model.named_parameters()) == 2 * (2 + 3 * (2 + 2))
    for n, p in model.named_parameters():
        if n in frozen:
            assert p.grad is None, n
            continue
        g = g_ref.get(n)
        if g is None or any(z in n for z in ZERO_GRADS) or float(g.abs().max()) == 0.0:
            continue
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, n
        a, b = p.grad.detach().float().cpu().reshape(-1), g.reshape(-1)
        rel, cos = float((a - b).norm() / (b.norm() + 1e-20)), float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30))
        print(f"{n}: rel {rel:.3e} cos {cos:.6f}")
        worst, cos_min = max(worst, (n, rel), key=lambda t: t[1]), min(cos_min, cos)
    assert worst[1] < REL and cos_min > COS, (worst, cos_min)
    # three optimizer steps: the frozen base parameters and their 16-bit shadows keep every bit
    from mmdti_hip.runtime import wbf16, wfwd
    w = model.encoder.layers[0].self_attn.in_proj.weight
    sh = (_bits(wbf16(w)), _bits(wfwd(w)))
    for _ in range(3):
        tuner.step(dev, label.cuda())
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        if n in frozen:
            assert p.grad is None and torch.equal(_bits(p), _bits(frozen[n])), n
    assert torch.equal(sh[0], _bits(wbf16(w))) and torch.equal(sh[1], _bits(wfwd(w)))
    assert any(float(p.detach().abs().max()) > 0 for n, p in model.named_parameters() if ".lora_B" in n)


def test_merge_reproduces_the_adapted_forward():
    from mmdti_hip import lora
    _, _, dev = _batch()
    model = _lora_model(b_seed=5)
    reference_keys = set(_model("classification", 2).state_dict())
    with torch.no_grad():
        before = model(**dev).float()
    merged_sd = lora.merged_state_dict(model)
    lora.merge_lora(model)
    assert set(model.state_dict()) == reference_keys == set(merged_sd) and not lora.has_lora(model)
    for k, v in model.state_dict().items():
        assert torch.equal(_bits(v), _bits(merged_sd[k])), k
    with torch.no_grad():
        after = model(**dev).float()
    err = float((after - before).abs().max())
    print(f"merged vs adapted logits: max |diff| {err:.3e}")
    assert err < 1e-3 * max(1.0, float(before.abs().max()))


def test_attention_maps_include_the_adapters():
    """maps of the adapted model against maps of the merged model (whose forward has no adapter launch), in the band of the merge test"""
    from mmdti_hip import lora
    _, _, dev = _batch()
    model = _lora_model(b_seed=5)
    plain_maps = None
    with torch.no_grad():
        for n, p in model.named_parameters():          # B = 0 first: the maps of the frozen base
            if ".lora_B" in n:
                p.data, p._saved = torch.zeros_like(p), p.data.clone()
        plain_maps = model.attention_maps(which=("cross", "unimol", "bert"), **dev)
        for n, p in model.named_parameters():
            if ".lora_B" in n:
                p.data = p._saved * 4.0                  # (large enough to move the maps well past the band)
    adapted = model.attention_maps(which=("cross", "unimol", "bert"), **dev)
    lora.merge_lora(model)
    merged = model.attention_maps(which=("cross", "unimol", "bert"), **dev)
    moved = 0.0
    for kind in ("text_to_graph", "graph_to_text", "unimol", "bert"):
        a, m, p0 = getattr(adapted, kind), getattr(merged, kind), getattr(plain_maps, kind)
        assert a.keys() == m.keys() and a
        for l in a:
            err = float((a[l] - m[l]).abs().max())
            moved = max(moved, float((a[l] - p0[l]).abs().max()))
            print(f"{kind}[{l}]: adapted vs merged max |diff| {err:.3e}")
            assert err < 1e-3, (kind, l, err)            # (attention weights are in [0, 1])
    assert moved > 1e-2, moved                           # the adapters are in the recorded pass
    assert float((adapted.outputs.float() - merged.outputs.float()).abs().max()) < 1e-3 * max(1.0, float(merged.outputs.abs().max()))


def test_accumulated_union_step_is_the_union_batch_with_adapters():
    """step_accumulated(negatives="union") with adapters: 3 x 4 molecules against one forward_backward over the 12, both held to the
    oracle on the merged weights with the band of tests/test_accumulate_gpu.py (deterministic mode, as there)"""
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    from test_accumulate_gpu import _band, _case, _cuda, _distances, _grads, _ref_max, _scalars, _split
    batch, label, _, uw = _case("classification")
    try:
        model = _lora_model(b_seed=17)
        tuner = FineTuner(model, "classification", total_steps=10, deterministic=True)
        ref = _oracle(model, batch, label)
        dev, lab = _cuda(batch, label)
        micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
        single = tuner.forward_backward(dev, lab, use_weight=uw)
        d_single = _distances(_scalars(single), _grads(model), ref)
        union = tuner.forward_backward_accumulated(micro, use_weight=uw, negatives="union")
        d_union = _distances(_scalars(union), _grads(model), ref)
        assert d_single.keys() == d_union.keys() and sum(".lora_" in w for w in d_single) >= 20
        bad = [w for w in d_single if not _band(w, d_union[w], d_single[w], _ref_max(ref, w))]
        assert not bad, bad
    finally:
        ops.set_deterministic(False)


def test_graphed_steps_replay_the_eager_ones():
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    _, label, dev = _batch(ragged=False)
    y = label.cuda()
    try:
        eager = FineTuner(_lora_model(b_seed=7), "classification", total_steps=20, learning_rate=1e-3)
        state = {k: v.clone() for k, v in eager.model.state_dict().items()}
        graphed = FineTuner(_lora_model(state=None), "classification", total_steps=20, learning_rate=1e-3)
        graphed.model.load_state_dict(state)
        for _ in range(4):
            a, b = eager.step(dev, y), graphed.graphed_step(dev, y)
        torch.cuda.synchronize()
        assert len(graphed._graphs) == 1
        la, lb = float(a.loss), float(b.loss)
        print(f"eager {la:.6f} graphed {lb:.6f}")
        assert abs(la - lb) <= 1e-4 * max(1.0, abs(la))
        for (n, p), (_, q) in zip(eager.model.named_parameters(), graphed.model.named_parameters()):
            if ".lora_" in n:
                assert torch.allclose(p.detach(), q.detach(), rtol=1e-3, atol=1e-5), n
    finally:
        ops.seed_salt_reset()


def test_state_round_trip_continues_in_the_same_bits():
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    _, label, dev = _batch()
    y = label.cuda()
    try:
        one = FineTuner(_lora_model(b_seed=9), "classification", total_steps=20, learning_rate=1e-3, deterministic=True)
        for _ in range(2):
            one.step(dev, y)
        sd = one.state_dict()
        assert any(".lora_A" in k for k in sd["model"])
        two = FineTuner(_lora_model(), "classification", total_steps=20, learning_rate=1e-3, deterministic=True)
        two.load_state_dict(sd)
        for _ in range(2):
            a, b = one.step(dev, y), two.step(dev, y)
            assert torch.equal(_bits(a.loss), _bits(b.loss))
        torch.cuda.synchronize()
        assert torch.equal(_bits(one.arena.data), _bits(two.arena.data))
    finally:
        ops.set_deterministic(False)


def test_one_rank_reducer_reduces_the_adapters(monkeypatch):
    """a 1-rank RCCL group (MMDTI_FORCE_DDP=1): the adapters sit in the ordinary buckets and report from inside the backward"""
    import torch.distributed as dist
    from mmdti_hip.parallel import init_from_env
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    monkeypatch.setenv("MMDTI_FORCE_DDP", "1")
    monkeypatch.setenv("MASTER_PORT", "29577")
    for k in ("RANK", "LOCAL_RANK"):
        monkeypatch.setenv(k, "0")
    monkeypatch.setenv("WORLD_SIZE", "1")
    _, label, dev = _batch()
    m1, m2 = _lora_model(b_seed=13), _lora_model(b_seed=13)
    init_from_env(force=True)
    try:
        base0 = dropout_state.base
        tuner = FineTuner(m1, "classification", distributed=True, bucket_bytes=16 << 10)
        red = tuner.reducer
        assert red.active
        dropout_state.reseed(base0)
        tuner.forward_backward(dev, label.cuda())
        torch.cuda.synchronize()
        names = {id(p): n for n, p in m1.named_parameters()}
        in_buckets = {names[id(p)] for p in tuner.arena.params}
        assert sum(".lora_" in n for n in in_buckets) == 28
        for ids in red.unreported():
            for i in ids:                                  # a parameter may stay silent only if it has no gradient at all
                g = next(p for p in tuner.arena.params if id(p) == i).grad
                assert float(g.abs().max()) == 0.0, names[i]
        g1 = {names[id(p)]: p.grad.clone() for p in tuner.arena.params}
    finally:
        dist.destroy_process_group()
    monkeypatch.delenv("MMDTI_FORCE_DDP")
    plain = FineTuner(m2, "classification")
    plain.forward_backward(dev, label.cuda())
    names2 = {id(p): n for n, p in m2.named_parameters()}
    for p in plain.arena.params:
        torch.testing.assert_close(g1[names2[id(p)]], p.grad, rtol=1e-3, atol=1e-5)


def test_trainer_writes_a_merged_checkpoint(tmp_path):
    from mmdti_hip.tasks import Trainer
    from test_ema_gpu import _Tok, _samples
    samples = _samples(40, 5)
    model = _model("regression", 1, _tokenizer=_Tok())
    reference_keys = set(model.state_dict())
    trainer = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=2, warmup_ratio=0.1,
                      patience=20, max_norm=5.0, use_cuda=True, use_amp=True, seed=1, lora_rank=8, save_train_state=True)
    y_pred = trainer.fit_predict(model, samples[:32], samples[32:], torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None)
    assert y_pred.shape == (8, 1) and np.isfinite(y_pred).all()
    sd = torch.load(os.path.join(str(tmp_path), "model_0.pth"), map_location="cuda", weights_only=True)["model_state_dict"]
    assert set(sd) == reference_keys and set(model.state_dict()) == reference_keys
    ts = torch.load(os.path.join(str(tmp_path), "train_state_0.pth"), map_location="cpu", weights_only=False)
    assert any(".lora_B" in k for k in ts["engine"]["model"])
    # a fresh reference-shaped model (no adapters) loads the checkpoint and reproduces the closing prediction
    fresh = _model("regression", 1, _tokenizer=_Tok())
    again, _, _ = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", batch_size=8, use_cuda=True, use_amp=True, seed=1).predict(
        fresh, samples[32:], torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None, load_model=True)
    assert np.array_equal(np.asarray(again), np.asarray(y_pred))
