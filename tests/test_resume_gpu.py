"""Resuming a run (DESIGN.md "Resuming a run"): FineTuner.state_dict / load_state_dict and tasks.Trainer(resume=True) on the small model
of tests/test_trainer_gpu.py.  Every comparison is bit equality or integer equality: in the deterministic mode a run that was saved,
loaded into a fresh engine and continued ends in the bits of the uninterrupted run; in the default mode what is restored is exact and
nothing is claimed about the steps that follow (atomics)."""
import gc
import hashlib
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from test_trainer_gpu import _model, _ocfg
from test_ema_gpu import _Tok, _samples, _same_bits


@pytest.fixture(autouse=True, scope="module")
def _free_tuners():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _batch(task, odim, seed, ragged=True, **kw):
    b, y = O.synth_batch(8, 10, 14, _ocfg(task, odim), seed=seed, ragged=ragged, **kw)
    return {k: v.cuda() for k, v in b.items()}, y.cuda()


def _other_weights(model):
    """a differently initialised model: every parameter moved"""
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.05 * torch.randn(p.shape, device=p.device, generator=g))
    return model


BUFFERS = ("data", "adam_m", "adam_v", "ema", "shadow")


def _snap(tuner):
    torch.cuda.synchronize()
    out = {k: getattr(tuner.arena, k) for k in BUFFERS}
    out["guard"] = tuner.guard
    return {k: None if v is None else v.clone() for k, v in out.items()}


def _assert_same(a, b, what=""):
    assert set(a) == set(b)
    for k in a:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert _same_bits(a[k], b[k]), (what, k, float((a[k].float() - b[k].float()).abs().max()))


def _through_a_file(sd, path):
    from mmdti_hip import checkpoint
    torch.save(sd, path)
    return checkpoint.load(path)


# ------------------------------------------------------------------------------------------------ 1: bit-exact continuation
def _poisoned_ce(logits, target):
    """Classification targets are int64 and cannot hold a NaN: the step is poisoned where a NaN target poisons a regression step -- the
    task loss is NaN, and with it every gradient the task term reaches."""
    from mmdti_hip.functional import CELossFn
    return CELossFn.apply(logits, target) * float("nan")


def _full_engine(model):
    from mmdti_hip.param_groups import no_decay
    from mmdti_hip.trainer import FineTuner
    return FineTuner(model, "classification", learning_rate=1e-3, total_steps=20, deterministic=True, skip_nonfinite=True, ema_decay=0.9,
                     param_groups=no_decay(model), weight_decay=0.01, decoupled_weight_decay=True)


def _steps(tuner, idx, losses):
    for i in idx:
        kw = dict(loss_func=_poisoned_ce) if i == 3 else {}
        o = tuner.step(*_batch("classification", 2, 40 + i), **kw)
        losses.append((o.loss.clone(), o.skipped.clone()))


def test_a_resumed_engine_continues_bit_for_bit_in_the_deterministic_mode(tmp_path):
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    base = dropout_state.base
    try:
        # run A: six steps, the fourth skipped by the guard, one group changed after the third
        dropout_state.reseed(77)
        ta, la = _full_engine(_model("classification", 2).train()), []
        _steps(ta, range(3), la)
        ta.set_group("no_decay", lr_scale=0.5, weight_decay=0.001)
        _steps(ta, range(3, 6), la)
        end_a = _snap(ta)
        # run B: three steps, saved; a fresh engine on other weights and another dropout stream loads the file and takes the rest
        dropout_state.reseed(77)
        tb, lb = _full_engine(_model("classification", 2).train()), []
        _steps(tb, range(3), lb)
        tb.set_group("no_decay", lr_scale=0.5, weight_decay=0.001)
        sd = _through_a_file(tb.state_dict(), tmp_path / "engine.pth")
        assert sd["dropout"]["base"] == 77 and sd["dropout"]["calls"] == dropout_state.mark() > 0 and sd["schedule"]["sched_step"] == 3
        del tb
        tc = _full_engine(_other_weights(_model("classification", 2)).train())
        dropout_state.reseed(4242)
        dropout_state.next_seed()
        tc.load_state_dict(sd)
        assert tc.sched_step == 3 and tc.arena.step_count == 3 and tc._group_table[1] == [0.5, 0.001]
        _steps(tc, range(3, 6), lb)
        end_c = _snap(tc)
        _assert_same(end_a, end_c, "after six steps")
        assert tc.sched_step == ta.sched_step == 6 and tc.arena.step_count == ta.arena.step_count == 6
        assert [float(s) for _, s in la] == [float(s) for _, s in lb] == [0.0, 0.0, 0.0, 1.0, 0.0, 0.0]
        for i, ((x, _), (y, _)) in enumerate(zip(la, lb)):
            assert _same_bits(x.reshape(1), y.reshape(1)), (i, float(x), float(y))
        assert float(tc.optimizer_steps) == 5.0 and float(tc.skipped_steps) == 1.0
        assert not _same_bits(end_c["ema"], end_c["data"])
    finally:
        dropout_state.reseed(base)
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 2: default mode, what is restored is exact
def test_the_restored_state_is_exact_in_the_default_mode(tmp_path):
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    kw = dict(learning_rate=1e-3, total_steps=20, skip_nonfinite=True, ema_decay=0.9)
    t1 = FineTuner(_model("classification", 2).train(), "classification", **kw)
    for i in range(3):
        t1.step(*_batch("classification", 2, 50 + i))
    saved = _snap(t1)
    sd = _through_a_file(t1.state_dict(), tmp_path / "engine.pth")
    _assert_same(saved, _snap(t1), "state_dict() writes nothing")
    t2 = FineTuner(_other_weights(_model("classification", 2)).train(), "classification", **kw)
    assert t2.arena.adam_m is None                                   # (no step yet: load allocates the moments)
    ptrs = [getattr(t2.arena, k).data_ptr() for k in ("data", "ema", "shadow")]
    t2.load_state_dict(sd)
    _assert_same(saved, _snap(t2), "fresh engine")
    assert ptrs == [getattr(t2.arena, k).data_ptr() for k in ("data", "ema", "shadow")]
    assert t2.sched_step == 3 and t2.arena.step_count == 3
    a = t2.arena
    dev, y = _batch("classification", 2, 53)

    def shadows_follow(arena, model):
        model.eval()
        with torch.no_grad():
            model(**dev)                                             # a forward asks for the weights' 16-bit shadows
        model.train()
        assert _same_bits(arena.shadow, ops.cast_bf16(arena.data))
        if ops.FWD_F16:
            assert arena.shadow16 is not None and arena._epoch16 == arena._epoch
            assert _same_bits(arena.shadow16, ops.cast_act16(arena.data))

    shadows_follow(a, t2.model)
    t2.step(dev, y)
    torch.cuda.synchronize()
    assert not _same_bits(a.data, saved["data"]) and float(t2.optimizer_steps) == 4.0
    # the engine that wrote the state, its fp16 shadow live and two steps further on, goes back to it as well
    t1.step(dev, y); t1.step(dev, y)
    t1.load_state_dict(sd)
    _assert_same(saved, _snap(t1), "the writer itself")
    shadows_follow(t1.arena, t1.model)
    assert t1.sched_step == 3 and float(t1.optimizer_steps) == 3.0


# ------------------------------------------------------------------------------------------------ 3: frozen after construction
def test_a_parameter_frozen_after_construction_stays_frozen(tmp_path):
    from mmdti_hip.trainer import FineTuner
    m1 = _model("classification", 2).train()
    t1 = FineTuner(m1, "classification", learning_rate=1e-3, total_steps=20)
    t1.step(*_batch("classification", 2, 60))
    m1.classification_head.dense.weight.requires_grad_(False)
    t1.step(*_batch("classification", 2, 61))
    sd = _through_a_file(t1.state_dict(), tmp_path / "engine.pth")
    assert sd["trainable"]["classification_head.dense.weight"] is False and sum(not f for f in sd["trainable"].values()) == 1
    m2 = _other_weights(_model("classification", 2)).train()
    t2 = FineTuner(m2, "classification", learning_rate=1e-3, total_steps=20)
    w = m2.classification_head.dense.weight
    assert w.requires_grad
    t2.load_state_dict(sd)
    a = t2.arena
    assert not w.requires_grad and a.skip_mask is not None and a._flags.count(False) == 1 and w.grad is None
    o, n = a.offsets[id(w)], w.numel()
    before = [x[o:o + n].clone() for x in (a.data, a.adam_m, a.adam_v)]
    others = a.data.clone()
    assert _same_bits(before[0], t1.arena.data[o:o + n]) and float(before[1].abs().max()) > 0.0
    t2.step(*_batch("classification", 2, 62))
    torch.cuda.synchronize()
    for x, b in zip((a.data, a.adam_m, a.adam_v), before):
        assert _same_bits(x[o:o + n], b)
    assert not _same_bits(a.data, others)


# ------------------------------------------------------------------------------------------------ 4: GHM's bin history
def test_ghm_bin_history_survives_and_the_next_loss_is_the_uninterrupted_one(tmp_path):
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    task, C = "multilabel_classification", 12
    mk = lambda model: FineTuner(model, task, learning_rate=1e-3, total_steps=20, loss_key="ghm", deterministic=True)
    batch = lambda i: _batch(task, C, 70 + i, n_labels=C)
    base = dropout_state.base
    try:
        dropout_state.reseed(78)
        ta = mk(_model(task, C).train())
        la = [ta.step(*batch(i)).loss.clone() for i in range(4)]
        dropout_state.reseed(78)
        tb = mk(_model(task, C).train())
        lb = [tb.step(*batch(i)).loss.clone() for i in range(3)]
        history = tb.task_loss.last_bin_count
        assert history is not None and float(history.sum()) > 0.0
        sd = _through_a_file(tb.state_dict(), tmp_path / "engine.pth")
        assert sd["task_loss"]["bins"] == 10 and torch.equal(sd["task_loss"]["last_bin_count"], history.cpu())
        tc = mk(_other_weights(_model(task, C)).train())
        assert tc.task_loss.last_bin_count is None
        dropout_state.reseed(1)
        tc.load_state_dict(sd)
        assert _same_bits(tc.task_loss.last_bin_count.cuda(), history)
        lb.append(tc.step(*batch(3)).loss.clone())
        for i, (x, y) in enumerate(zip(la, lb)):
            assert _same_bits(x.reshape(1), y.reshape(1)), (i, float(x), float(y))
        assert _same_bits(ta.task_loss.last_bin_count, tc.task_loss.last_bin_count)
        assert _same_bits(ta.arena.data, tc.arena.data)
    finally:
        dropout_state.reseed(base)
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 5: graph continuity
def test_graph_replays_continue_the_device_counters(tmp_path):
    """default mode (graphed_step is refused in the deterministic one): the integers are compared, the parameters are not"""
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    gc.collect()
    kw = dict(learning_rate=1e-3, total_steps=20, max_norm=5.0, warmup_ratio=0.25)
    batch = lambda i: _batch("classification", 2, 80 + i, ragged=False)
    try:
        ta = FineTuner(_model("classification", 2).train(), "classification", **kw)
        for i in range(4):
            ta.graphed_step(*batch(i))
        tb = FineTuner(_model("classification", 2).train(), "classification", **kw)
        for i in range(2):
            tb.graphed_step(*batch(i))
        sd = _through_a_file(tb.state_dict(), tmp_path / "engine.pth")
        assert sd["graph"]["salted"] is True and float(sd["graph"]["state"][0]) == 2.0
        tc = FineTuner(_other_weights(_model("classification", 2)).train(), "classification", **kw)
        assert tc._state is None
        tc.load_state_dict(sd)
        assert tc._state is not None and tc._salted and torch.equal(tc._salt.cpu(), sd["graph"]["salt"])
        for i in range(2, 4):
            tc.graphed_step(*batch(i))
        torch.cuda.synchronize()
        assert len(tc._graphs) == 1
        assert tc.sched_step == ta.sched_step == 4 and tc.arena.step_count == ta.arena.step_count == 4
        assert float(tc._state[0]) == float(ta._state[0]) == 4.0
        assert torch.equal(tc._salt, ta._salt) and not torch.equal(tc._salt.cpu(), sd["graph"]["salt"])
        assert _same_bits(tc._state[1:2], ta._state[1:2])             # (the learning rate of step 4, from the same schedule)
    finally:
        ops.seed_salt_reset()


# ------------------------------------------------------------------------------------------------ 6: errors write nothing
def _model_with_one_more_layer(task, odim):
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 3, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1, attn_dropout=0.1)
    torch.manual_seed(0)
    return mm.MM_Model.from_configs(odim, task, mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16).cuda()


def test_refused_loads_write_nothing(tmp_path):
    from mmdti_hip.trainer import FineTuner
    kw = dict(learning_rate=1e-3, total_steps=20)
    with_ema = FineTuner(_model("classification", 2).train(), "classification", ema_decay=0.9, **kw)
    with_ema.step(*_batch("classification", 2, 90))
    sd = _through_a_file(with_ema.state_dict(), tmp_path / "engine.pth")

    def refused(tuner, exc, match, state=sd):
        tuner.step(*_batch("classification", 2, 91))
        before, counters = _snap(tuner), (tuner.sched_step, tuner.arena.step_count)
        with pytest.raises(exc, match=match):
            tuner.load_state_dict(state)
        _assert_same(before, _snap(tuner), match)
        assert counters == (tuner.sched_step, tuner.arena.step_count)

    refused(FineTuner(_other_weights(_model("classification", 2)).train(), "classification", **kw), ValueError, "weight averaging")
    refused(FineTuner(_model_with_one_more_layer("classification", 2).train(), "classification", ema_decay=0.9, **kw), ValueError,
            r"encoder\.layers\.2\.")
    refused(with_ema, ValueError, "version 2", dict(sd, version=2))
    # inside averaged(): neither a load nor a state_dict
    before = _snap(with_ema)
    with with_ema.averaged():
        with pytest.raises(RuntimeError, match="averaged"):
            with_ema.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="averaged"):
            with_ema.state_dict()
    _assert_same(before, _snap(with_ema), "averaged")
    with_ema.load_state_dict(sd)                                      # and outside it the same file loads
    assert with_ema.sched_step == 1


# ------------------------------------------------------------------------------------------------ 7, 8: tasks.Trainer
TRAINER = dict(task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=4, warmup_ratio=0.1, patience=20, max_norm=5.0,
               use_cuda=True, use_amp=True, seed=1, deterministic=True)


def _fit(dump_dir, samples, **params):
    from mmdti_hip.tasks import Trainer
    model = _model("regression", 1, _tokenizer=_Tok())
    trainer = Trainer(save_path=str(dump_dir), **dict(TRAINER, **params))
    y = trainer.fit_predict(model, samples[:32], samples[32:], torch.nn.MSELoss(), lambda x: x, str(dump_dir), 0, None)
    return trainer, y


def _checkpoint_tensors(dump_dir):
    return torch.load(os.path.join(str(dump_dir), "model_0.pth"), map_location="cpu", weights_only=True)["model_state_dict"]


def _same_checkpoint(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


def test_trainer_resumes_at_an_epoch_boundary_bit_for_bit(tmp_path, monkeypatch):
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.tasks import Trainer
    from mmdti_hip.trainer import FineTuner
    samples = _samples(40, 5)
    seen = []
    real_step = FineTuner.step

    def step(self, net_input, net_target, *a, **k):
        h = hashlib.sha1(net_input["input_ids"].cpu().numpy().tobytes() + net_input["src_tokens"].cpu().numpy().tobytes()).hexdigest()
        seen.append((k.get("epoch"), h))
        return real_step(self, net_input, net_target, *a, **k)

    monkeypatch.setattr(FineTuner, "step", step)
    real_write = Trainer._save_train_state
    kill_after = []

    def write(self, engine, task_loss, dump_dir, fold, epoch, *a, **k):
        real_write(self, engine, task_loss, dump_dir, fold, epoch, *a, **k)
        if kill_after and epoch == kill_after[0]:
            raise KeyboardInterrupt("the job's time is up")

    monkeypatch.setattr(Trainer, "_save_train_state", write)
    base = dropout_state.base
    dirs = [tmp_path / n for n in ("a", "b1")]
    for d in dirs:
        d.mkdir()
    try:
        dropout_state.reseed(79)
        tr_a, y_a = _fit(dirs[0], samples, ema_decay=0.9, resume=True)           # (no file: a run from epoch 0 that writes one)
        order_a, hist_a = list(seen), tr_a.history
        assert [e for e, _ in order_a] == [e for e in range(4) for _ in range(4)] and len({h for _, h in order_a}) > 4
        assert os.path.exists(dirs[0] / "train_state_0.pth")
        # run B: killed right after the second epoch's file is complete
        del seen[:]
        dropout_state.reseed(79)
        kill_after.append(1)
        with pytest.raises(KeyboardInterrupt):
            _fit(dirs[1], samples, ema_decay=0.9, resume=True)
        del kill_after[:]
        assert len(seen) == 8
        b2 = tmp_path / "b2"
        shutil.copytree(dirs[1], b2)
        assert sorted(os.listdir(b2)) == ["model_0.pth", "train_state_0.pth"]
        dropout_state.reseed(31337)                                              # (a new process knows nothing of the old stream)
        torch.manual_seed(123); np.random.seed(123)
        tr_b, y_b = _fit(b2, samples, ema_decay=0.9, resume=True)
        assert [e for e, _ in seen[8:]] == [2] * 4 + [3] * 4
        assert seen == order_a, "batch order"
        assert y_a.dtype == y_b.dtype and y_a.tobytes() == y_b.tobytes()
        _same_checkpoint(_checkpoint_tensors(dirs[0]), _checkpoint_tensors(b2))
        assert [h["epoch"] for h in tr_b.history] == [h["epoch"] for h in hist_a] == [0, 1, 2, 3]
        for ha, hb in zip(hist_a, tr_b.history):
            assert ha["steps"].dtype == hb["steps"].dtype and ha["steps"].shape == hb["steps"].shape == (4, 4)
            assert ha["steps"].tobytes() == hb["steps"].tobytes(), ha["epoch"]
            assert ha["val_loss"] == hb["val_loss"] and ha["score"] == hb["score"] and ha["metric"] == hb["metric"] and ha["skipped"] == hb["skipped"]
        # a third call finds the finished run: no step, the same prediction
        del seen[:]
        tr_c, y_c = _fit(b2, samples, ema_decay=0.9, resume=True)
        assert seen == [] and y_c.tobytes() == y_a.tobytes() and len(tr_c.history) == 4
        # other settings than the file's are refused
        with pytest.raises(ValueError, match="epochs"):
            _fit(b2, samples, ema_decay=0.9, resume=True, epochs=5)
    finally:
        dropout_state.reseed(base)
        ops.set_deterministic(False)


def test_trainer_writes_no_train_state_by_default(tmp_path):
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    samples = _samples(40, 5)
    base = dropout_state.base
    try:
        outs = []
        for name in ("one", "two"):
            d = tmp_path / name
            d.mkdir()
            dropout_state.reseed(80)
            trainer, y = _fit(d, samples, epochs=2)
            assert trainer.resume is False and trainer.save_train_state is False
            assert os.listdir(d) == ["model_0.pth"]
            outs.append((_checkpoint_tensors(d), y))
        _same_checkpoint(outs[0][0], outs[1][0])
        assert outs[0][1].tobytes() == outs[1][1].tobytes()
    finally:
        dropout_state.reseed(base)
        ops.set_deterministic(False)
