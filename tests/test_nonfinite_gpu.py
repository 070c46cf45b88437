"""GPU tests of the non-finite step guard (FineTuner(skip_nonfinite=True)): the skip half of the reference's GradScaler
(tasks/trainer.py:268-282) -- an optimizer step whose gradients hold any inf / NaN element writes nothing, Adam's step count stays,
the learning-rate schedule advances -- decided on the device by the fused check + norm pass (ops.sumsq_check) and the guarded Adam
pass (ops.adam_step_guarded)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from g9util import product_model, tiny_cfg


@pytest.fixture(autouse=True, scope="module")
def _free_tuners():
    """The engines built here hold their parameter arenas in a reference cycle (ParamArena <-> its Parameters): collect them when the
    module is done, so that their device memory is not released by a cyclic collection in the middle of a later test's measurement."""
    yield
    import gc
    gc.collect()
    torch.cuda.empty_cache()


def _tuners(task, n, dropout=False, **kw):
    """n FineTuners over identically initialised tiny product models."""
    from mmdti_hip.trainer import FineTuner
    ocfg = tiny_cfg(task, 40)
    torch.manual_seed(0)
    models = [product_model(ocfg, dropout=dropout).cuda().train() for _ in range(n)]
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    kw = dict(dict(learning_rate=1e-3, total_steps=20, max_norm=5.0), **kw)
    return ocfg, [FineTuner(m, task, **kw) for m in models]


def _batch(ocfg, seed, nan_row=None):
    b, y = O.synth_batch(8, 10, 14, ocfg, seed=seed, ragged=False)
    y = y.cuda()
    if nan_row is not None:
        y[nan_row] = float("nan")
    return {k: v.cuda() for k, v in b.items()}, y


def _state(t):
    a = t.arena
    return [x.clone() for x in (a.data, a.adam_m, a.adam_v, a.shadow) + ((a.shadow16,) if a.shadow16 is not None else ())]


def _param_errs(t1, t2):
    """per-parameter relative L2 differences (parameters whose gradient is analytically zero -- key.bias, gbf_proj.linear2.bias --
    take sign-noise Adam steps and are left out, as in test_trainer_gpu)."""
    return [float((p1 - p2).norm() / (p1.norm() + 1e-12))
            for (n, p1), (_, p2) in zip(t1.model.named_parameters(), t2.model.named_parameters())
            if p1.requires_grad and not any(z in n for z in ("key.bias", "gbf_proj.linear2.bias", "pooler"))]


def test_poisoned_step_is_a_noop_and_training_continues():
    ocfg, (t1, t2, t3) = _tuners("regression", 3, skip_nonfinite=True)
    t2.skip_nonfinite, t2.guard = False, None            # t2, t3: unguarded twins that never see the bad batch
    t3.skip_nonfinite, t3.guard = False, None
    a, bad, c = _batch(ocfg, 31), _batch(ocfg, 32, nan_row=3), _batch(ocfg, 33)
    o = t1.step(*a)
    assert float(o.skipped) == 0.0 and np.isfinite(float(o.grad_norm))
    before = _state(t1)
    o = t1.step(*bad)
    assert float(o.skipped) == 1.0 and np.isnan(float(o.loss))
    after = _state(t1)
    for x, y in zip(before, after):
        assert torch.equal(x, y) and torch.isfinite(x.float()).all()
    assert float(t1.skipped_steps) == 1.0 and float(t1.optimizer_steps) == 1.0 and t1.sched_step == 2
    o = t1.step(*c)
    assert float(o.skipped) == 0.0 and float(t1.optimizer_steps) == 2.0 and float(t1.skipped_steps) == 1.0
    assert torch.isfinite(t1.arena.data).all() and not torch.equal(t1.arena.data, before[0])
    for t in (t2, t3):
        t.step(*a)
        t.sched_step += 1                                # the reference's scheduler.step() on the skipped iteration
        t.step(*c)
    band, errs = _param_errs(t2, t3), _param_errs(t1, t2)
    # two unguarded runs differ by the fp32 atomics of LayerNorm gamma/beta, embedding rows and split-K dW;
    # the guarded run with one skipped step sits in the same band (MI355X: band median 9.3e-9 / max 9.2e-5, guarded vs twin the same)
    print("nonfinite twin band: median %.2e max %.2e | guarded vs twin: median %.2e max %.2e"
          % (np.median(band), max(band), np.median(errs), max(errs)))
    assert float(np.median(errs)) < 1e-6 and max(errs) < 1e-3, (float(np.median(errs)), max(errs))


def test_single_nonfinite_element_skips_and_huge_finite_does_not():
    from mmdti_hip import ops
    ocfg, (t,) = _tuners("classification", 1, skip_nonfinite=True)
    a = _batch(ocfg, 41)
    t.step(*a)
    k = t.arena.numel // 3
    for n, bad in enumerate((float("inf"), float("nan"))):
        t.forward_backward(*a)
        before = _state(t)
        t.arena.grad[k] = bad
        buf = torch.zeros(2 + 4096, device="cuda")
        ops.sumsq_check(t.arena.grad, buf[:2], buf[2:])
        assert float(buf[1]) == 1.0
        skipped, norm = t.optimizer_step()
        assert float(skipped) == 1.0 and float(t.skipped_steps) == n + 1 and float(t.optimizer_steps) == 1.0
        for x, y in zip(before, _state(t)):
            assert torch.equal(x, y)
    # a finite 1e30 overflows the sum of squares (norm inf -> clip coefficient 0) but no element is inf / NaN: unscale_ does not skip
    t.forward_backward(*a)
    t.arena.grad[k] = 1e30
    skipped, norm = t.optimizer_step()
    assert float(skipped) == 0.0 and float(t.optimizer_steps) == 2.0 and float(norm) == float("inf")
    assert torch.isfinite(t.arena.data).all()


def test_step_reports_the_guard_when_optimizer_step_is_wrapped():
    """Callers wrap FineTuner.optimizer_step (bench.py's loader-fed workload times it with events and drops its return value):
    step() still runs and reports this step's skip flag and norm; a replacement that takes no step reports none."""
    ocfg, (t,) = _tuners("regression", 1, skip_nonfinite=True)
    real = t.optimizer_step

    def timed():
        real()                                           # return value dropped, as a timing wrapper does

    t.optimizer_step = timed
    o = t.step(*_batch(ocfg, 81, nan_row=2))
    assert float(o.skipped) == 1.0 and float(t.skipped_steps) == 1.0 and np.isnan(float(o.grad_norm))
    o = t.step(*_batch(ocfg, 82))
    assert float(o.skipped) == 0.0 and np.isfinite(float(o.grad_norm)) and float(t.optimizer_steps) == 1.0
    t.optimizer_step = lambda: None
    o = t.step(*_batch(ocfg, 83))
    assert o.skipped is None and o.grad_norm is None and t.sched_step == 2


@pytest.mark.parametrize("n", [3_000_001, 1_234_567, 1001])
def test_fused_pass_sum_is_the_reproducible_sumsq(n):
    from mmdti_hip import ops
    assert n % 4 != 0
    g = torch.randn(n + 8, device="cuda", generator=torch.Generator("cuda").manual_seed(n))[:n] * 3.0
    ref = torch.zeros(1 + 2048, device="cuda")
    ops.sumsq(g, ref[:1], ref[1:])
    out = torch.zeros(3 + 4096, device="cuda")
    guard = torch.zeros(8, device="cuda")
    ops.sumsq_check(g, out[:3], out[3:], guard)
    assert torch.equal(out[:1], ref[:1]) and float(out[1]) == 0.0 and float(out[2]) == 0.0
    assert float(guard[0]) == 1.0 and float(guard[1]) == 0.0
    g[n - 1] = float("-inf")                                     # (in the ragged tail)
    out.zero_()
    ops.sumsq_check(g, out[:3], out[3:], guard)
    assert float(out[1]) == 1.0 and float(out[2]) == 1.0 and float(guard[0]) == 1.0 and float(guard[1]) == 1.0


@pytest.mark.parametrize("clip", [False, True])
def test_guarded_adam_with_clear_flag_is_the_unguarded_update(clip):
    """Identical gradients, flag clear: the guarded pass is the unguarded one to the bit -- eager (host bias corrections by value vs
    the guard's table) and graphed (step-state bias corrections vs the guard's device expression), for several t."""
    from mmdti_hip import ops
    n = 1 << 18
    gen = torch.Generator("cuda").manual_seed(7)
    p0, g, m0 = (torch.randn(n, device="cuda", generator=gen) for _ in range(3))
    v0 = torch.rand(n, device="cuda", generator=gen)
    scale = torch.tensor([0.37], device="cuda") if clip else None
    table = ops.adam_bias_table(0.9, 0.999, 64, "cuda")
    try:
        for t in (1, 2, 7, 50):
            for graphed in (False, True):
                outs = []
                for guarded in (False, True):
                    p, m, v = p0.clone(), m0.clone(), v0.clone()
                    pb, ph = torch.empty(n, device="cuda", dtype=torch.bfloat16), torch.empty(n, device="cuda", dtype=torch.float16)
                    state = None
                    if graphed:
                        state, salt = torch.zeros(4, device="cuda"), torch.zeros(2, device="cuda", dtype=torch.int64)
                        state[0] = t - 1
                        ops.step_state_advance(state, salt, 1e-3, 3, 100)
                    if guarded:
                        guard = torch.zeros(8, device="cuda")
                        guard[0] = t - 1
                        out = torch.zeros(3 + 4096, device="cuda")
                        ops.sumsq_check(g, out[:3], out[3:], guard, None if graphed else table)
                        assert float(guard[0]) == t and float(guard[2]) == 0.0
                        ops.adam_step_guarded(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-6, 0.0, guard, scale, state, p_f16=ph)
                    else:
                        ops.adam_step(p, g, m, v, pb, 1e-3, 0.9, 0.999, 1e-6, 0.0, t, scale, state, p_f16=ph)
                    outs.append((p, m, v, pb, ph))
                for x, y in zip(*outs):
                    assert torch.equal(x, y), (t, graphed)
    finally:
        ops.seed_salt_reset()


@pytest.mark.parametrize("graphed", [False, True])
def test_guard_changes_nothing_on_finite_data(graphed):
    """4 steps with dropout on, guard on vs off: the same trajectory up to the run-to-run band of the unguarded step."""
    from mmdti_hip import ops
    from mmdti_hip.runtime import dropout_state
    ocfg, tuners = _tuners("classification", 3, dropout=True)
    tuners[0].skip_nonfinite, tuners[0].guard = True, torch.zeros(8, device="cuda")
    batches = [_batch(ocfg, 50 + i) for i in range(4)]
    base = dropout_state.base
    losses = []
    try:
        for t in tuners:
            dropout_state.reseed(base)
            losses.append([float((t.graphed_step if graphed else t.step)(*b).loss) for b in batches])
    finally:
        dropout_state.reseed(base)
        ops.seed_salt_reset()
    assert float(tuners[0].optimizer_steps) == 4.0 and float(tuners[0].skipped_steps) == 0.0
    band, errs = _param_errs(tuners[1], tuners[2]), _param_errs(tuners[0], tuners[1])
    print("finite data (%s): unguarded band median %.2e max %.2e | guarded: median %.2e max %.2e"
          % ("graphed" if graphed else "eager", np.median(band), max(band), np.median(errs), max(errs)))
    np.testing.assert_allclose(losses[0], losses[1], rtol=2e-4)
    # MI355X, 4 steps with dropout: unguarded band median 8.2e-5 / 5.5e-5, max 1.6e-3 / 1.3e-3 (eager / graphed); guarded vs unguarded
    # median 7.4e-5 / 6.2e-5, max 2.2e-3 / 1.6e-3
    assert float(np.median(errs)) < 5e-4 and max(errs) < 2e-2, (float(np.median(errs)), max(errs))


def test_graphed_guard_skips_a_poisoned_replay():
    from mmdti_hip import ops
    ocfg, (t,) = _tuners("regression", 1, skip_nonfinite=True)
    a, bad, c = _batch(ocfg, 61), _batch(ocfg, 62, nan_row=0), _batch(ocfg, 63)
    try:
        o = t.graphed_step(*a)
        assert float(o.skipped) == 0.0 and float(t.optimizer_steps) == 1.0
        before = _state(t)
        o = t.graphed_step(*bad)
        assert float(o.skipped) == 1.0
        for x, y in zip(before, _state(t)):
            assert torch.equal(x, y)
        assert float(t.optimizer_steps) == 1.0 and float(t.skipped_steps) == 1.0 and t.sched_step == 2 and float(t._state[0]) == 2.0
        o = t.graphed_step(*c)
        assert len(t._graphs) == 1 and float(o.skipped) == 0.0 and float(t.optimizer_steps) == 2.0
        assert torch.isfinite(t.arena.data).all() and not torch.equal(t.arena.data, before[0])
    finally:
        ops.seed_salt_reset()


@pytest.mark.parametrize("mode", ["padded", "ddp"])
def test_guarded_step_has_no_host_synchronisation(mode, monkeypatch):
    import torch.distributed as dist
    from mmdti_hip.parallel import init_from_env
    if mode == "ddp":
        monkeypatch.setenv("MMDTI_FORCE_DDP", "1")
        monkeypatch.setenv("MASTER_PORT", "29577")
        for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")):
            monkeypatch.setenv(k, v)
        init_from_env(force=True)
    try:
        ocfg, (t,) = _tuners("regression", 1, skip_nonfinite=True, distributed=mode == "ddp")
        a, bad = _batch(ocfg, 71), _batch(ocfg, 72, nan_row=1)
        t.step(*a)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            o1 = t.step(*bad)
            o2 = t.step(*a)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert float(o1.skipped) == 1.0 and float(o2.skipped) == 0.0 and float(t.optimizer_steps) == 2.0
    finally:
        if mode == "ddp":
            import mmdti_hip.parallel as par
            par._HOST_GROUP = None
            dist.destroy_process_group()


def _samples(n, seed, nan_at=None):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        na = int(rng.integers(4, 10))
        atoms = rng.choice(np.arange(4, 30), size=na)
        d = O.coords2unimol(atoms, rng.normal(0, 3.0, size=(na, 3)), 31)
        d["smile"] = "C" * int(rng.integers(3, 10))
        y = 0.1 * float((atoms == 4).sum()) if i != nan_at else float("nan")
        out.append((d, np.array([y], dtype=np.float32)))
    return out


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


@pytest.mark.parametrize("amp", [True, False])
def test_trainer_skips_nan_target_steps_under_amp(amp, tmp_path):
    """use_amp=True: the engine is guarded (the reference's GradScaler) and a NaN target costs one skipped step per epoch; use_amp=False:
    unguarded, as the reference without a scaler (run on clean data: a NaN step would leave no finite checkpoint to reload)."""
    from mmdti_hip.tasks import Trainer
    samples = _samples(40, 5, nan_at=7 if amp else None)
    torch.manual_seed(0)
    model = product_model(tiny_cfg("regression", 40), tokenizer=_Tok())
    trainer = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=2,
                      warmup_ratio=0.1, patience=20, max_norm=5.0, use_cuda=True, use_amp=amp, seed=1)
    trainer.fit_predict(model, samples[:32], _samples(8, 6), torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None)
    eng = trainer._engine
    assert eng.skip_nonfinite == amp
    if amp:
        assert (eng.guard is not None and all(h["steps"].shape == (4, 4) for h in trainer.history)
                and [h["skipped"] for h in trainer.history] == [1, 1])           # the NaN sample is in one batch per epoch
        assert float(eng.skipped_steps) == 2.0 and float(eng.optimizer_steps) == 6.0
        assert torch.isfinite(eng.arena.data).all()
    else:
        assert eng.guard is None and all(h["skipped"] == 0 and h["steps"].shape == (4, 4) for h in trainer.history)
