"""GPU tests of partial fine-tuning (the reference's freeze_layers / freeze_layers_reversed, models/nnmodel.py:112-127): frozen
parameters never change and get no gradient, every trainable parameter gets its gradient (against the CPU oracle), a parameter
frozen after the engine was built keeps its value and Adam moments, and freezing tower 1 removes its backward."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RECIPES = {
    "R1": ("embed_tokens,gbf", False),
    "R2": ("bert.embeddings", False),
    "R3": ("embed_tokens,encoder,gbf,bert", False),
    "R4": ("encoder,gbf", False),
    "R5": ("classification_head", True),
    "R6": (["embed_tokens", "gbf", "encoder.emb_layer_norm"] + [f"encoder.layers.{i}." for i in range(8)], False),
}
ZERO_GRADS = ("pooler", "key.bias", "gbf_proj.linear2.bias")      # (zero in the reference too: see test_reference_sized_step_vs_oracle)


@pytest.fixture(scope="module")
def oracle_grads():
    """Oracle gradients of every parameter of bench.build_model() at a small ragged batch.  Freezing a parameter does not change the
    gradient of any other one, so the all-trainable oracle holds the reference gradient of every recipe's trainable set."""
    import bench
    model, _ = bench.build_model()
    ocfg = O.ModelCfg(task="classification", output_dim=2)
    ocfg.roberta = O.RobertaCfg(layers=6, dim=512, heads=8, ffn=2048, vocab=600, max_pos=514, pad_idx=1)
    batch, label = O.synth_batch(6, 40, 48, ocfg, seed=21, ragged=True)
    P = {k: v.detach().cpu().float().clone().requires_grad_() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    ref = O.mm_forward(batch, P, ocfg, net_target=label, bf16=True)
    ref_loss, _ = O.step_loss(ref, label, "classification")
    ref_loss.backward()
    return batch, label, {k: v.grad for k, v in P.items()}


def _host_fields(batch):
    from mmdti_hip.collate import device_payload
    full = device_payload(batch)
    return {k: full[k] for k in ("atom_counts", "token_counts", "token_pad_id", "packable")}


@pytest.mark.parametrize("path", ["stack", "per_layer"])
@pytest.mark.parametrize("layout", ["padded", "packed"])
@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_recipe_step(oracle_grads, recipe, layout, path, monkeypatch):
    import bench
    from mmdti_hip import functional
    from mmdti_hip.freeze import freeze_layers
    from mmdti_hip.trainer import FineTuner
    if path == "per_layer":
        monkeypatch.setattr(functional, "STACK_MAX_ROWS", 0)          # the per-layer library calls (what M >= 8192 rows takes)
    batch, label, g_ref = oracle_grads
    model, _ = bench.build_model()
    model = model.cuda().eval()                                       # dropout off: value parity
    prefixes, rev = RECIPES[recipe]
    freeze_layers(model, prefixes, rev)
    frozen = {n: p.detach().clone() for n, p in model.named_parameters() if not p.requires_grad}
    assert frozen and len(frozen) < len(list(model.parameters()))
    tuner = FineTuner(model, "classification", total_steps=10)
    dev = {k: v.cuda() for k, v in batch.items()}
    if layout == "packed":
        model.strict_reference = False
        dev.update(_host_fields(batch))
    else:
        model.strict_reference = True
    tuner.step(dev, label.cuda())
    torch.cuda.synchronize()
    assert model.last_layout == layout
    worst, cos_min, missing = ("", 0.0), 1.0, []
    for n, p in model.named_parameters():
        if n in frozen:
            assert p.grad is None, n
            assert torch.equal(p.detach(), frozen[n]), n
            continue
        g = g_ref[n]
        if any(z in n for z in ZERO_GRADS) or float(g.abs().max()) == 0.0:
            continue
        if p.grad is None or float(p.grad.abs().max()) == 0.0:
            missing.append(n)
            continue
        a, b = p.grad.detach().float().cpu().reshape(-1), g.reshape(-1)
        worst = max(worst, (n, float((a - b).norm() / (b.norm() + 1e-20))), key=lambda t: t[1])
        cos_min = min(cos_min, float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-30)))
    assert not missing, f"{recipe}: trainable parameters without a gradient: {missing[:8]} (+{max(0, len(missing) - 8)})"
    assert worst[1] < 3.2e-2 and cos_min > 0.9996, (recipe, worst, cos_min)


def _small_model():
    from types import SimpleNamespace
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 2, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1,
                           attn_dropout=0.1)
    torch.manual_seed(0)
    return mm.MM_Model.from_configs(2, "classification", mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16).cuda().eval()


@pytest.mark.parametrize("guard", [False, True])
def test_freeze_after_construction(guard):
    """3 steps, freeze one layer, 3 more: the layer's value and Adam moments do not move over the last 3 steps (masked Adam pass), it has
    no gradient, and the rest keeps training."""
    from mmdti_hip.trainer import FineTuner
    ocfg = O.ModelCfg(unimol=O.UniMolCfg(layers=2, dim=64, ffn=128, heads=8, K=16, vocab=31),
                      roberta=O.RobertaCfg(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40),
                      cross=O.CrossCfg(dim=64, heads=4, ffn=128), task="classification", output_dim=2)
    batch, label = O.synth_batch(8, 10, 14, ocfg, seed=3, ragged=True)
    dev, y = {k: v.cuda() for k, v in batch.items()}, label.cuda()
    model = _small_model()
    tuner = FineTuner(model, "classification", total_steps=20, warmup_ratio=0.0, skip_nonfinite=guard)
    for _ in range(3):
        tuner.step(dev, y)
    layer = model.encoder.layers[1]
    for p in layer.parameters():
        p.requires_grad_(False)
    ar = tuner.arena
    rng = [(ar.offsets[id(p)], p.numel()) for p in layer.parameters()]
    snap = lambda: [torch.cat([t[o:o + n] for o, n in rng]).clone() for t in (ar.data, ar.adam_m, ar.adam_v, ar.shadow)]
    others = [p for n, p in model.named_parameters() if p.requires_grad]
    before, before_other = snap(), [p.detach().clone() for p in others]
    for _ in range(3):
        out = tuner.step(dev, y)
    torch.cuda.synchronize()
    if guard:
        assert float(out.skipped) == 0.0
    for a, b in zip(before, snap()):
        assert torch.equal(a, b)
    assert all(p.grad is None for p in layer.parameters())
    assert ar.skip_mask is not None
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before_other, others))
    # unfreezing again restores the plain pass; a parameter that was frozen at construction is never added
    for p in layer.parameters():
        p.requires_grad_(True)
    tuner.step(dev, y)
    assert ar.skip_mask is None


@pytest.mark.parametrize("guard", [False, True])
def test_masked_adam_kernel_bitwise(guard):
    """adam_step_masked: elements under the mask keep value, moments and both shadows to the bit; the others get exactly the unmasked
    (or guarded) update."""
    from mmdti_hip import ops
    torch.manual_seed(7)
    n = 8 * 1000 + 5
    p0, g = torch.randn(n, device="cuda"), torch.randn(n, device="cuda")
    m0, v0 = torch.randn(n, device="cuda") * 0.1, torch.rand(n, device="cuda") * 0.01
    skip = (torch.rand((n + 7) // 8, device="cuda") < 0.3).to(torch.uint8)
    gd = None
    if guard:
        gd = torch.zeros(8, device="cuda")
        gd[3], gd[4] = 1 - 0.9 ** 3, (1 - 0.999 ** 3) ** 0.5
    res = []
    for masked in (False, True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        sb, sh = torch.zeros(n, device="cuda", dtype=torch.bfloat16), torch.zeros(n, device="cuda", dtype=torch.float16)
        if masked:
            ops.adam_step_masked(p, g, m, v, sb, 1e-3, 0.9, 0.999, 1e-6, 0.0, 3, skip, guard=gd, p_f16=sh)
        elif guard:
            ops.adam_step_guarded(p, g, m, v, sb, 1e-3, 0.9, 0.999, 1e-6, 0.0, gd, p_f16=sh)
        else:
            ops.adam_step(p, g, m, v, sb, 1e-3, 0.9, 0.999, 1e-6, 0.0, 3, p_f16=sh)
        res.append((p, m, v, sb, sh))
    keep = skip.bool().repeat_interleave(8)[:n]
    init = (p0, m0, v0, torch.zeros(n, device="cuda", dtype=torch.bfloat16), torch.zeros(n, device="cuda", dtype=torch.float16))
    for a, b, c in zip(res[0], res[1], init):
        assert torch.equal(b[~keep].view(torch.int16 if b.element_size() == 2 else torch.int32),
                           a[~keep].view(torch.int16 if a.element_size() == 2 else torch.int32))
        assert torch.equal(b[keep], c[keep])


def test_frozen_tower1_step_is_cheaper():
    """At the bench batch shape, freezing tower 1 (embed_tokens, encoder, gbf) takes its backward off the step: less peak memory and at
    most 0.8x the step time (median of 10 steps, same process)."""
    import time
    import bench
    from mmdti_hip.freeze import freeze_layers
    from mmdti_hip.trainer import FineTuner
    _, batch, label = bench.synth(256, 128, 256, seed=1234)
    dev, y = {k: v.cuda() for k, v in batch.items()}, label.cuda()
    res = {}
    for name, prefixes in (("unfrozen", None), ("tower1", "embed_tokens,encoder,gbf")):
        model, _ = bench.build_model()
        model = model.cuda().train()
        if prefixes:
            freeze_layers(model, prefixes)
        tuner = FineTuner(model, "classification", total_steps=10_000)
        for _ in range(3):
            tuner.step(dev, y, epoch=0)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            tuner.step(dev, y, epoch=0)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        res[name] = (sorted(ts)[5], torch.cuda.max_memory_allocated())
        del tuner, model
        torch.cuda.empty_cache()
    print("freeze timing", {k: (round(v[0] * 1e3, 2), round(v[1] / 2 ** 30, 2)) for k, v in res.items()})
    assert res["tower1"][1] < 0.8 * res["unfrozen"][1], res
    assert res["tower1"][0] <= 0.8 * res["unfrozen"][0], res


@pytest.mark.parametrize("guard", [False, True])
def test_freeze_after_first_step_on_stack_path(oracle_grads, guard):
    """Reference architecture at a small batch, where both towers run the stack calls (cached pointer tables): after one step,
    freeze a Uni-Mol layer and a RoBERTa layer.  The next backward writes nothing into their gradient slots (the tables are keyed
    on the trainable flags), and the masked Adam pass leaves their value and moments alone while every other arena element gets
    exactly what an unmasked Adam pass computes from the same gradients."""
    import bench
    from mmdti_hip.trainer import FineTuner
    batch, label, _ = oracle_grads
    model, _ = bench.build_model()
    model = model.cuda().eval()
    tuner = FineTuner(model, "classification", total_steps=10, skip_nonfinite=guard)
    dev, y = {k: v.cuda() for k, v in batch.items()}, label.cuda()
    tuner.step(dev, y)
    frozen = [p for n, p in model.named_parameters() if n.startswith(("encoder.layers.3.", "bert.encoder.layer.2."))]
    assert len(frozen) == 12 + 16
    for p in frozen:
        p.requires_grad_(False)
    ar = tuner.arena
    tuner.forward_backward(dev, y)
    torch.cuda.synchronize()
    idx = torch.cat([torch.arange(ar.offsets[id(p)], ar.offsets[id(p)] + p.numel()) for p in frozen]).cuda()
    assert all(p.grad is None for p in frozen)
    assert float(ar.grad[idx].abs().max()) == 0.0
    assert ar.skip_mask is not None
    state = lambda: [t.clone() for t in (ar.data, ar.adam_m, ar.adam_v, ar.shadow)]
    saved = state() + ([tuner.guard.clone()] if guard else [])
    tuner.optimizer_step()
    masked = state()
    # the same optimizer step again from the same state and gradients, unmasked
    for t, s in zip((ar.data, ar.adam_m, ar.adam_v, ar.shadow) + ((tuner.guard,) if guard else ()), saved):
        t.copy_(s)
    ar.step_count -= 1
    tuner.sched_step -= 1
    keep, ar.skip_mask = ar.skip_mask, None
    tuner.optimizer_step()
    ar.skip_mask = keep
    plain = state()
    torch.cuda.synchronize()
    other = torch.ones(ar.numel, dtype=torch.bool, device="cuda")
    other[idx] = False
    for m, u, s in zip(masked, plain, saved):
        assert torch.equal(m[idx], s[idx])                       # frozen: value, moments and bf16 shadow untouched
        assert torch.equal(m[other], u[other])                   # the rest: bit-identical to the unmasked pass
    assert not torch.equal(plain[0][idx], saved[0][idx])         # (the unmasked pass would have moved them)
