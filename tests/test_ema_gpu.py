"""Weight averaging end to end (FineTuner(ema_decay=...), engine.averaged(), tasks.Trainer(ema_decay=...)) on the small model of
tests/test_trainer_gpu.py: the average follows the float64 recurrence of tests/ema_cases.py over the parameters of every applied step --
eager, under the non-finite guard and from a captured graph --, it never feeds back into training, averaged() puts it into the model and
takes it out again to the bit, and the Trainer validates and checkpoints on it.

The bound is ema_cases.recurrence's: 3 * k * 2^-24 * M for k applied updates (derived there, not measured)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from test_trainer_gpu import _model, _ocfg

import ema_cases as E


@pytest.fixture(autouse=True, scope="module")
def _free_tuners():
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _batch(task, odim, seed, ragged=True, nan_row=None):
    b, y = O.synth_batch(8, 10, 14, _ocfg(task, odim), seed=seed, ragged=ragged)
    y = y.cuda()
    if nan_row is not None:
        y[nan_row] = float("nan")
    return {k: v.cuda() for k, v in b.items()}, y


def _bits(x):
    return x.contiguous().view({4: torch.int32, 2: torch.int16}[x.element_size()])


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(tuner, e0, snaps, decay, warmup, what):
    """arena.ema against the float64 recurrence over the parameter snapshots (None: a skipped step); t counts applied steps only"""
    k = sum(s is not None for s in snaps)
    ws = [E.weight32(t, decay, warmup) for t in range(1, k + 1)]
    ref, bound = E.recurrence(e0.cpu(), [None if s is None else s.cpu() for s in snaps], ws)
    err = (tuner.arena.ema.cpu().to(E.F64) - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"{what}: {k} updates, worst |ema - ref| / (3 * {k} * 2^-24 * M) = {ratio:.3f}")
    assert bool((err <= bound).all()), (what, ratio)
    moved = float((tuner.arena.ema - e0).abs().max())
    assert moved > 0.0, "the average never moved"


def test_six_steps_follow_the_float64_recurrence():
    from mmdti_hip.trainer import FineTuner
    tuner = FineTuner(_model("classification", 2).train(), "classification", learning_rate=1e-3, total_steps=20, ema_decay=0.9)
    a = tuner.arena
    assert a.ema is not None and a.ema.dtype == torch.float32 and a.ema.shape == a.data.shape and a.ema.data_ptr() != a.data.data_ptr()
    assert _same_bits(a.ema, a.data)                                   # initialised as a copy
    e0, snaps = a.ema.clone(), []
    for i in range(6):
        tuner.step(*_batch("classification", 2, 40 + i))
        snaps.append(a.data.clone())
    assert not _same_bits(a.ema, a.data)
    _check(tuner, e0, snaps, 0.9, True, "eager")


def test_default_engine_has_no_average_and_the_average_never_feeds_back(monkeypatch):
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    calls = []
    real_update, real_swap = ops.ema_update, ops.ema_swap
    monkeypatch.setattr(ops, "ema_update", lambda *a, **k: (calls.append("update"), real_update(*a, **k))[1])
    monkeypatch.setattr(ops, "ema_swap", lambda *a, **k: (calls.append("swap"), real_swap(*a, **k))[1])
    plain = FineTuner(_model("classification", 2).train(), "classification", total_steps=20)
    assert plain.ema_decay is None and plain.arena.ema is None
    for i in range(2):
        plain.step(*_batch("classification", 2, 50 + i))
    assert plain.arena.ema is None and calls == []
    with pytest.raises(RuntimeError, match="without weight averaging"):
        with plain.averaged():
            pass
    for bad in (1.0, 0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            FineTuner(plain.model, "classification", ema_decay=bad)
    # deterministic mode: three steps with the average on and off end in the same bits (parameters and both moments)
    base = dropout_state.base
    ends = []
    try:
        for decay in (None, 0.9):
            dropout_state.reseed(77)
            t = FineTuner(_model("classification", 2).train(), "classification", learning_rate=1e-3, total_steps=20, deterministic=True, ema_decay=decay)
            for i in range(3):
                t.step(*_batch("classification", 2, 60 + i))
            torch.cuda.synchronize()
            ends.append((t.arena.data.clone(), t.arena.adam_m.clone(), t.arena.adam_v.clone()))
    finally:
        dropout_state.reseed(base)
        ops.set_deterministic(False)
    assert calls == ["update"] * 3
    for x, y in zip(*ends):
        assert _same_bits(x, y)


def test_a_skipped_step_leaves_the_average_and_t_counts_applied_steps_only():
    from mmdti_hip.trainer import FineTuner
    tuner = FineTuner(_model("regression", 1).train(), "regression", learning_rate=1e-3, total_steps=20, max_norm=5.0, skip_nonfinite=True,
                      ema_decay=0.9)
    a = tuner.arena
    e0, snaps = a.ema.clone(), []
    o = tuner.step(*_batch("regression", 1, 31))
    assert float(o.skipped) == 0.0
    snaps.append(a.data.clone())
    before = a.ema.clone()
    o = tuner.step(*_batch("regression", 1, 32, nan_row=3))
    assert float(o.skipped) == 1.0
    assert _same_bits(a.ema, before) and _same_bits(a.data, snaps[0])
    snaps.append(None)
    o = tuner.step(*_batch("regression", 1, 33))
    assert float(o.skipped) == 0.0 and float(tuner.optimizer_steps) == 2.0 and float(tuner.skipped_steps) == 1.0
    snaps.append(a.data.clone())
    assert not _same_bits(a.ema, before) and torch.isfinite(a.ema).all()
    _check(tuner, e0, snaps, 0.9, True, "guarded")               # weights of t = 1, 2: the skipped step consumed none
    # the same three batches counted as three applied steps is a different average: the check above can tell
    ws3 = [E.weight32(t, 0.9, True) for t in (1, 3)]
    wrong, bound = E.recurrence(e0.cpu(), [snaps[0].cpu(), snaps[2].cpu()], ws3)
    assert not bool(((a.ema.cpu().to(E.F64) - wrong).abs() <= bound).all())


def test_averaged_puts_the_average_into_the_model_and_takes_it_out_again():
    from mmdti_hip.trainer import FineTuner
    model = _model("classification", 2).train()
    tuner = FineTuner(model, "classification", learning_rate=1e-3, total_steps=20, ema_decay=0.9)
    a = tuner.arena
    dev, y = _batch("classification", 2, 70)
    for i in range(3):
        tuner.step(*_batch("classification", 2, 70 + i))
    model.eval()
    with torch.no_grad():
        raw_logits = model(**dev).clone()
    assert a.shadow16 is not None and a._epoch16 == a._epoch              # the fp16 shadow is live (fp16 forward operands, the default)
    data0, ema0, sh0, sh16_0 = a.data.clone(), a.ema.clone(), a.shadow.clone(), a.shadow16.clone()
    with tuner.averaged() as eng:
        assert eng is tuner
        for p in a.params:
            o, n = a.offsets[id(p)], p.numel()
            assert _same_bits(p.detach().reshape(-1), ema0[o:o + n])
        assert _same_bits(a.ema, data0)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        with torch.no_grad():
            inside = model(**dev).clone()
        for call in (lambda: tuner.step(dev, y), lambda: tuner.graphed_step(dev, y), lambda: tuner.optimizer_step(),
                     lambda: tuner.averaged().__enter__()):
            with pytest.raises(RuntimeError, match="averaged"):
                call()
        assert _same_bits(a.ema, data0)                                   # the refused calls touched nothing
    torch.cuda.synchronize()
    assert _same_bits(a.data, data0) and _same_bits(a.ema, ema0) and _same_bits(a.shadow, sh0) and _same_bits(a.shadow16, sh16_0)
    assert a._epoch16 == a._epoch
    with torch.no_grad():
        assert torch.equal(model(**dev), raw_logits)
    assert not torch.equal(inside, raw_logits)
    # a fresh model that loads the state dict taken inside (bound to an arena of its own, so that it runs the same kernels)
    fresh = _model("classification", 2)
    fresh.load_state_dict(sd)
    FineTuner(fresh, "classification", total_steps=20)
    fresh.eval()
    with torch.no_grad():
        assert torch.equal(fresh(**dev), inside)
    # training goes on from the raw weights
    model.train()
    tuner.step(dev, y)
    assert not _same_bits(a.data, data0)


@pytest.mark.parametrize("guarded", [False, True], ids=["t_from_step_state", "t_from_guard"])
def test_graphed_step_updates_the_average_and_the_capture_does_not(guarded, monkeypatch):
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    after_capture = []
    real = FineTuner._capture

    def capture(self, *args, **kw):
        ent = real(self, *args, **kw)
        torch.cuda.synchronize()
        after_capture.append((self.arena.ema.clone(), self.arena.data.clone()))
        return ent

    # (patched on the class, not as an attribute of the engine: a closure over the engine stored on the engine is a reference cycle,
    #  and an engine that dies in a cycle takes its captured graph with it whenever the collector next runs -- inside a later capture,
    #  where destroying a graph is not allowed)
    monkeypatch.setattr(FineTuner, "_capture", capture)
    tuner = FineTuner(_model("classification", 2).train(), "classification", learning_rate=1e-3, total_steps=20, max_norm=5.0,
                      skip_nonfinite=guarded, ema_decay=0.9)
    a = tuner.arena
    e0, snaps = a.ema.clone(), []
    data0 = a.data.clone()
    try:
        for i in range(4):
            tuner.graphed_step(*_batch("classification", 2, 80 + i, ragged=False))
            snaps.append(a.data.clone())
        assert len(tuner._graphs) == 1 and len(after_capture) == 1
        assert _same_bits(after_capture[0][0], e0) and _same_bits(after_capture[0][1], data0)     # warm-up steps and capture: no trace
        _check(tuner, e0, snaps, 0.9, True, "graphed, " + ("guard" if guarded else "step state"))
    finally:
        ops.seed_salt_reset()


class _Tok:
    pad_token_id = 1

    def __call__(self, smiles, padding=True, truncation=True, return_tensors="pt"):
        L = max(len(s) for s in smiles) + 2
        ids = torch.ones(len(smiles), L, dtype=torch.long)
        att = torch.zeros(len(smiles), L, dtype=torch.long)
        for r, s in enumerate(smiles):
            ids[r, :len(s) + 2] = torch.tensor([0] + [5 + (ord(c) % 7) for c in s] + [2])
            att[r, :len(s) + 2] = 1
        return {"input_ids": ids, "attention_mask": att}


def _samples(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        na = int(rng.integers(4, 10))
        atoms = rng.choice(np.arange(4, 30), size=na)
        d = O.coords2unimol(atoms, rng.normal(0, 3.0, size=(na, 3)), 31)
        d["smile"] = "C" * int(rng.integers(3, 10))
        out.append((d, np.array([0.1 * float((atoms == 4).sum())], dtype=np.float32)))
    return out


def test_trainer_validates_and_checkpoints_on_the_average(tmp_path, monkeypatch):
    import os
    from mmdti_hip.tasks import Trainer
    samples = _samples(40, 5)
    model = _model("regression", 1, _tokenizer=_Tok())
    seen = []
    real_save = Trainer._save

    def save(self, m, dump_dir, fold):
        eng = self._engine
        seen.append((eng._averaged, eng.arena.ema.clone(), eng.arena.data.clone()))     # inside averaged(): `ema` holds the raw weights
        return real_save(self, m, dump_dir, fold)

    monkeypatch.setattr(Trainer, "_save", save)
    trainer = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=1, warmup_ratio=0.1,
                      patience=20, max_norm=5.0, use_cuda=True, use_amp=True, seed=1, ema_decay=0.9)
    y_pred = trainer.fit_predict(model, samples[:32], samples[32:], torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None)
    assert y_pred.shape == (8, 1) and np.isfinite(y_pred).all()
    eng = trainer._engine
    assert eng.ema_decay == 0.9 and eng.ema_warmup is True and not eng._averaged
    assert len(seen) == 1 and seen[0][0] is True                      # one epoch, one checkpoint, written inside averaged()
    raw, avg_at_save = seen[0][1], seen[0][2]
    assert _same_bits(eng.arena.ema, avg_at_save)                     # the block's exit put the average back into its buffer
    sd = torch.load(os.path.join(str(tmp_path), "model_0.pth"), map_location="cuda", weights_only=True)["model_state_dict"]
    assert set(sd) == set(model.state_dict())                         # the reference's keys
    names = {id(p): n for n, p in model.named_parameters()}
    differ = 0
    for p in eng.arena.params:
        o, n = eng.arena.offsets[id(p)], p.numel()
        saved = sd[names[id(p)]].reshape(-1)
        assert _same_bits(saved, eng.arena.ema[o:o + n]), names[id(p)]
        differ += int(not _same_bits(saved, raw[o:o + n]))
        assert _same_bits(p.detach().reshape(-1), saved)              # predict(load_model=True) loaded the checkpoint into the model
    assert differ > len(eng.arena.params) // 2, "the checkpoint holds the raw parameters"
    assert float(eng.optimizer_steps) == 4.0
