"""Parameter groups through the engine (FineTuner(weight_decay=, decoupled_weight_decay=, param_groups=), set_group) on the small model
of tests/test_trainer_gpu.py -- 2 layers, D = 64, 8 molecules x 10 atoms x 14 tokens, eval mode: the grouped pass against
torch.optim.Adam / AdamW with the same parameter groups, fed the engine's own gradients and clip coefficient; the default engine never
reaches the grouped entry point; graphed_step with groups, and set_group between two replays; the non-finite guard and a parameter
frozen after construction compose with the groups."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O

from test_trainer_gpu import _model, _ocfg

LR, WD, MAX_NORM, STEPS = 1e-3, 0.01, 5.0, 3
# The yardstick of test_grouped_pass_matches_torch: score = max over elements of |p_engine - p_torch| / (2^-23 |p| + 2^-23 lr) after three
# steps.  The same comparison with ONE default group on the ungrouped pass (FineTuner without the new arguments, i.e. adam_kernel as it was
# before the grouped pass existed) against torch.optim.Adam, measured on MI355X: 28.97 (twice, at encoder.layers.0.self_attn.out_proj.weight).
# The grouped pass is allowed twice that, for its extra roundings (lr * s; decoupled: lr_i * wd, 1 - ., p * .); it measured 27.18 coupled
# and 28.04 decoupled with no_decay + layerwise_decay(0.5) + weight_decay 0.01.
MEASURED_DEFAULT_SCORE = 28.97
BOUND = 2.0 * MEASURED_DEFAULT_SCORE


def _batch(seed=3, ragged=True):
    ocfg = _ocfg("classification", 2)
    batch, label = O.synth_batch(8, 10, 14, ocfg, seed=seed, ragged=ragged)
    return {k: v.cuda() for k, v in batch.items()}, label.cuda()


def _groups(model):
    from mmdti_hip.param_groups import layerwise_decay, no_decay
    return no_decay(model) + layerwise_decay(model, 0.5)


def score_against_torch(decoupled, grouped, printer=print):
    """three engine steps; after each forward_backward the arena's gradients and the engine's clip coefficient go to a torch optimizer
    over copies of the parameters with the same groups -> the score of the comment above"""
    from mmdti_hip.param_groups import resolve
    from mmdti_hip.trainer import FineTuner, linear_warmup_lr
    model = _model("classification", 2).eval()
    kw = dict(weight_decay=WD, decoupled_weight_decay=decoupled, param_groups=_groups(model)) if grouped else {}
    tuner = FineTuner(model, "classification", learning_rate=LR, warmup_ratio=0.5, total_steps=4, max_norm=MAX_NORM, **kw)
    index, table = resolve(model, _groups(model), WD) if grouped else ([0] * len(list(model.parameters())), [[1.0, 0.0]])
    a = tuner.arena
    held = [(n, p, gid) for (n, p), gid in zip(model.named_parameters(), index) if id(p) in a.offsets]        # (what the optimizer holds)
    names, params = [n for n, _, _ in held], [p for _, p, _ in held]
    copies = [torch.nn.Parameter(p.detach().clone()) for p in params]
    by_gid = {}
    for q, (_, _, gid) in zip(copies, held):
        by_gid.setdefault(gid, []).append(q)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=ps, weight_decay=table[gid][1], scale=table[gid][0]) for gid, ps in sorted(by_gid.items())], lr=LR, eps=1e-6)
    dev, y = _batch()
    for s in range(STEPS):
        tuner.forward_backward(dev, y)
        grads = [a.grad[a.offsets[id(p)]:a.offsets[id(p)] + p.numel()].view(p.shape).clone() for p in params]       # (what the Adam pass reads)
        lr = linear_warmup_lr(LR, tuner.sched_step, tuner.warmup, tuner.total_steps)
        _, norm = tuner.optimizer_step()
        coef = torch.clamp(MAX_NORM / (norm + 1e-6), max=1.0)
        for q, g in zip(copies, grads):
            q.grad = g * coef
        for grp in opt.param_groups:
            grp["lr"] = lr * grp["scale"]
        opt.step()
    torch.cuda.synchronize()
    worst, where = 0.0, None
    for n, p, q in zip(names, params, copies):
        sc = float(((p.detach() - q.detach()).abs() / (2.0 ** -23 * q.detach().abs() + 2.0 ** -23 * LR)).max())
        if sc > worst:
            worst, where = sc, n
    printer(f"score_against_torch(decoupled={decoupled}, grouped={grouped}): {worst:.4g} at {where}")
    return worst, tuner, model


@pytest.mark.parametrize("decoupled", [False, True])
def test_grouped_pass_matches_torch(decoupled):
    worst, tuner, model = score_against_torch(decoupled, True)
    assert worst <= BOUND, (worst, BOUND)
    rows = tuner.param_group_summary()
    assert rows[0][0] == "default" and rows[1][0] == "no_decay" and rows[1][4] == 0.0 and rows[0][4] == WD
    assert sum(r[1] for r in rows) == len(tuner.arena.params) and sum(r[2] for r in rows) == sum(p.numel() for p in tuner.arena.params)
    assert {r[3] for r in rows} >= {1.0, 0.5, 0.25, 0.125}


def test_the_default_engine_never_reaches_the_grouped_entry_point(monkeypatch):
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    calls = []
    real = ops.adam_step_grouped
    monkeypatch.setattr(ops, "adam_step_grouped", lambda *a, **k: (calls.append(1), real(*a, **k)))
    dev, y = _batch()
    t = FineTuner(_model("classification", 2).eval(), "classification", learning_rate=LR, total_steps=10)
    t.step(dev, y)
    assert not calls and t.arena.group_ids is None and t.arena.group_table is None and t.param_groups is None
    assert t.param_group_summary() == [("default", len(t.arena.params), sum(p.numel() for p in t.arena.params), 1.0, 0.0)]
    with pytest.raises(RuntimeError):
        t.set_group(0, lr_scale=0.5)
    # coupled decay without groups: still the existing entry points, the decay by value
    m = _model("classification", 2).eval()
    t = FineTuner(m, "classification", learning_rate=LR, total_steps=10, weight_decay=0.1, max_norm=None)
    w = m.classification_head.dense.weight
    before = w.detach().clone()
    t.step(dev, y)
    assert not calls and t.arena.group_ids is None
    m2 = _model("classification", 2).eval()
    t2 = FineTuner(m2, "classification", learning_rate=LR, total_steps=10, max_norm=None)
    t2.step(dev, y)
    assert not torch.equal(w.detach(), m2.classification_head.dense.weight.detach()) and not torch.equal(w.detach(), before)
    # decoupled decay, or an empty list of groups, takes the grouped pass with the default group alone
    t3 = FineTuner(_model("classification", 2).eval(), "classification", learning_rate=LR, total_steps=10, weight_decay=0.1, decoupled_weight_decay=True)
    t3.step(dev, y)
    assert len(calls) == 1 and t3.arena.group_table.shape == (1, 2) and t3.arena.decoupled


def test_graphed_step_with_groups_equals_eager_and_set_group_reaches_captured_graphs():
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    m1, m2 = _model("classification", 2).eval(), _model("classification", 2).eval()
    m2.load_state_dict(m1.state_dict())
    kw = dict(learning_rate=LR, warmup_ratio=0.5, total_steps=8, max_norm=MAX_NORM, weight_decay=WD, decoupled_weight_decay=True)
    t1, t2 = FineTuner(m1, "classification", param_groups=_groups(m1), **kw), FineTuner(m2, "classification", param_groups=_groups(m2), **kw)
    try:
        batches = [_batch(20 + i, ragged=False) for i in range(4)]          # (one padded shape: one graph)
        for dev, y in batches:
            o1, o2 = t1.step(dev, y), t2.graphed_step(dev, y)
            assert abs(float(o1.loss) - float(o2.loss)) <= 2e-4 * abs(float(o1.loss)) + 1e-6, (float(o1.loss), float(o2.loss))
        assert len(t2._graphs) == 1 and t2.sched_step == 4
        errs = [float((p1.detach() - p2.detach()).norm() / (p1.detach().norm() + 1e-12)) for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters())
                if p1.requires_grad and not any(z in n for z in ("key.bias", "gbf_proj.linear2.bias", "pooler"))]
        assert float(np.median(errs)) < 1e-4 and max(errs) < 5e-2, (float(np.median(errs)), max(errs))
        # freeze the top BERT layer's group between two replays: its parameters and shadows keep their bits, the rest moves on
        name = "bert.depth2"
        frozen = [p for n, p in m2.named_parameters() if n.startswith("bert.encoder.layer.1.") and p.dim() == 2]
        other = m2.classification_head.dense.weight
        assert frozen and t2.param_group_summary()[t2._group_names.index(name)][1] == len(frozen)
        graph = next(iter(t2._graphs.values()))[2]
        table_ptr = t2.arena.group_table.data_ptr()
        t2.set_group(name, lr_scale=0.0)
        snap = [(p.detach().clone(), t2.arena.bf16(p).clone()) for p in frozen]
        o_before = other.detach().clone()
        t2.graphed_step(*batches[0])
        torch.cuda.synchronize()
        for p, (v, sh) in zip(frozen, snap):
            assert torch.equal(p.detach(), v) and torch.equal(t2.arena.bf16(p), sh)
        assert not torch.equal(other.detach(), o_before)
        assert len(t2._graphs) == 1 and next(iter(t2._graphs.values()))[2] is graph and t2.arena.group_table.data_ptr() == table_ptr
        t2.set_group(name, lr_scale=1.0)                                  # ... and thaws again
        t2.graphed_step(*batches[1])
        torch.cuda.synchronize()
        assert all(not torch.equal(p.detach(), v) for p, (v, _) in zip(frozen, snap)) and len(t2._graphs) == 1
        assert t2.param_group_summary()[t2._group_names.index(name)][3] == 1.0
    finally:
        ops.seed_salt_reset()


def test_a_poisoned_step_with_groups_leaves_everything_untouched():
    from mmdti_hip.trainer import FineTuner
    m = _model("classification", 2).eval()
    t = FineTuner(m, "classification", learning_rate=LR, total_steps=10, skip_nonfinite=True, weight_decay=WD, param_groups=_groups(m), decoupled_weight_decay=True)
    dev, y = _batch()
    t.step(dev, y)
    a = t.arena
    a.f16(a.params[0])                                                  # (the fp16 shadow exists from here on)
    t.step(dev, y)
    t.forward_backward(dev, y)
    a.grad[a.numel // 2] = float("inf")
    snap = [x.clone() for x in (a.data, a.adam_m, a.adam_v, a.shadow, a.shadow16)]
    skipped, _ = t.optimizer_step()
    torch.cuda.synchronize()
    assert float(skipped) == 1.0 and float(t.skipped_steps) == 1.0 and float(t.optimizer_steps) == 2.0
    for x, s in zip((a.data, a.adam_m, a.adam_v, a.shadow, a.shadow16), snap):
        assert torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int16), s.view(torch.int32 if s.dtype == torch.float32 else torch.int16))
    o = t.step(dev, y)                                                  # ... and training continues
    assert float(o.skipped) == 0.0 and not torch.equal(a.data, snap[0])


def test_a_parameter_frozen_after_construction_composes_with_the_groups():
    from mmdti_hip.trainer import FineTuner
    m = _model("classification", 2).eval()
    t = FineTuner(m, "classification", learning_rate=LR, total_steps=10, weight_decay=WD, param_groups=_groups(m))
    dev, y = _batch()
    t.step(dev, y)
    w = m.classification_head.dense.weight
    w.requires_grad = False
    a = t.arena
    o, n = a.offsets[id(w)], w.numel()
    snap = [x[o:o + n].clone() for x in (a.data, a.adam_m, a.adam_v, a.shadow)]
    rest = m.classification_head.out_proj.weight.detach().clone()
    t.step(dev, y)
    torch.cuda.synchronize()
    assert a.skip_mask is not None and a.group_ids is not None
    for x, s in zip((a.data, a.adam_m, a.adam_v, a.shadow), snap):
        assert torch.equal(x[o:o + n], s)
    assert not torch.equal(m.classification_head.out_proj.weight.detach(), rest)


def test_the_trainer_hands_groups_and_layer_decay_to_the_engine_and_logs_them(tmp_path, caplog):
    import logging
    from g9util import product_model, tiny_cfg
    from mmdti_hip.param_groups import no_decay
    from mmdti_hip.tasks import Trainer
    from test_nonfinite_gpu import _Tok, _samples
    torch.manual_seed(0)
    model = product_model(tiny_cfg("regression", 40), tokenizer=_Tok())
    trainer = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=1, warmup_ratio=0.1, patience=20,
                      max_norm=5.0, use_cuda=True, seed=1, weight_decay=WD, decoupled_weight_decay=True, param_groups=no_decay(model), layer_decay=0.5)
    with caplog.at_level(logging.INFO):
        trainer.fit_predict(model, _samples(16, 5), _samples(8, 6), torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None)
    eng = trainer._engine
    rows = eng.param_group_summary()
    assert eng.arena.group_ids is not None and eng.arena.decoupled and eng.weight_decay == WD
    assert [r[0] for r in rows][:3] == ["default", "no_decay", "unimol.depth0"] and "bert.depth0" in [r[0] for r in rows]
    assert rows[1][4] == 0.0 and rows[0][3:] == (1.0, WD) and min(r[3] for r in rows) < 1.0
    logged = [r.getMessage() for r in caplog.records if r.getMessage().startswith("param group ")]
    assert len(logged) == len(rows) and "no_decay" in logged[1] and "(decoupled)" in logged[1]
    assert torch.isfinite(eng.arena.data).all() and eng.sched_step == 2
