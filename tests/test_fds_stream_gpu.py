"""GPU tests of the streaming FDS statistics (FineTuner(fds_stats="streaming")): mmdti_fds_stream_accumulate / _merge / _finish, the
FDS.stream_* methods, MM_Model's accumulate site, the engine's begin / finish and the captured step -- against the float64 second pass
(head_refs.FDS64.update_running_stats on the concatenated epoch, models/fds.py:116-155, tasks/trainer.py:288-306) on the cases of
fds_stream_cases.py.

THE BAND.  Nothing is fixed by hand: on the same inputs the existing one-shot kernel (ops.fds_update_stats, through
FDS.update_running_stats) is measured against the same float64 reference, and the streaming path may be off by at most
2 x that figure + 8 * 2^-24 (nerr: max|got - ref| / max|ref|) -- the factor 2 for the one extra merge rounding per end bucket, the floor
a few fp32 roundings for tensors where the one-shot error is 0.  Both figures of every case go to profiles/fds_streaming.json."""
import functools
import json
import os

import pytest
import torch

import fds_stream_cases as C
from head_refs import FDS64, nerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 8 * 2.0 ** -24
KEYS = ("running_mean", "running_var", "num_samples_tracked")
IDS = dict(ids=lambda k: "D%d_bs%d_bn%d" % k)
_FIGURES = {}


def _record(name, figures):
    """profiles/fds_streaming.json: {case: {epoch: {tensor: [one-shot nerr, streaming nerr]}}}"""
    _FIGURES[name] = figures
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fds_streaming.json"), "w") as f:
        json.dump(_FIGURES, f, indent=1, sort_keys=True)
        f.write("\n")


def _fds(c):
    from mmdti_hip.models.fds import FDS
    return FDS(c.D, c.raw, "", False, bucket_num=c.bn, bucket_start=c.bs, start_update=0, start_smooth=1, ks=c.ks, sigma=2,
               momentum=C.MOMENTUM).cuda()


def _state(fds):
    return {k: getattr(fds, k).detach().clone() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _one_shot(key):
    """The existing path on the case: update_last_epoch_stats + update_running_stats per epoch, then the no-op call -> states"""
    c, fds, states = C.case(*key), _fds(C.case(*key)), []
    for e, (feats, labels, _) in enumerate(c.epochs):
        fds.update_last_epoch_stats(e)
        fds.update_running_stats(feats.cuda(), labels.cuda(), e)
        states.append(_state(fds))
    fds.update_running_stats(c.epochs[0][0].cuda(), c.epochs[0][1].cuda(), c.noop_epoch)
    states.append(_state(fds))
    return states


def _streamed(key, sizes, shards=1):
    """The streaming path: per epoch stream_reset, the batches of `sizes` (dealt to `shards` accumulators in turn and merged in order when
    shards > 1), update_last_epoch_stats, stream_finish; then a finish with epoch < FDS.epoch.  -> (states, accumulators per epoch)"""
    from mmdti_hip import ops
    c, fds, states, accs = C.case(*key), _fds(C.case(*key)), [], []
    for e, (feats, labels, _) in enumerate(c.epochs):
        fds.stream_reset()
        parts = [ops.fds_stream_new(c.nb, c.D, "cuda") for _ in range(shards)] if shards > 1 else None
        for i, (f, y) in enumerate(zip(C.chunks(feats, sizes), C.chunks(labels, sizes))):
            if parts is None:
                fds.stream_accumulate(f.cuda(), y.cuda())
            elif f.shape[0]:
                ops.fds_stream_accumulate(f.cuda(), fds._bins(y.cuda())[0], c.bs, c.bn, parts[i % shards])
        for p in parts or ():
            ops.fds_stream_merge(fds.stream_state(), p)
        fds.update_last_epoch_stats(e)
        fds.stream_finish(e)
        states.append(_state(fds))
        accs.append(fds.stream_state().clone())
    fds.stream_finish(c.noop_epoch)                                      # epoch < FDS.epoch: returns at once (the accumulator is full)
    states.append(_state(fds))
    return states, accs


def _check_band(key, got, tag, record=False):
    """every state of `got` against the float64 second pass, inside 2 x the one-shot kernel's own error + FLOOR; counts exactly"""
    ref, one = C.second_pass(*key), _one_shot(key)
    figures = {}
    for e, (g, r, o) in enumerate(zip(got, ref, one)):
        assert torch.equal(g["num_samples_tracked"].cpu().double(), r["num_samples_tracked"]), (tag, e)
        figures[f"epoch{e}"] = {}
        for k in KEYS:
            e_one, e_str = nerr(o[k], r[k]), nerr(g[k], r[k])
            figures[f"epoch{e}"][k] = [e_one, e_str]
            print(f"{tag} epoch {e} {k}: one-shot {e_one:.3e} streaming {e_str:.3e} band {2 * e_one + FLOOR:.3e}")
    if record:
        _record("D%d_bs%d_bn%d" % key, figures)
    for e, per in figures.items():
        for k, (e_one, e_str) in per.items():
            assert e_str <= 2 * e_one + FLOOR, (tag, e, k, e_str, e_one)


@pytest.mark.parametrize("key", C.CASE_KEYS, **IDS)
def test_chunk_invariance(key):
    """One call or any split of the epoch's rows into calls -- an empty batch among them -- leaves bit-identical accumulators and buffers."""
    from mmdti_hip import ops
    base_states, base_accs = _streamed(key, C.CHUNKINGS[0])
    for sizes in C.CHUNKINGS[1:]:
        states, accs = _streamed(key, sizes)
        for e, (a, b) in enumerate(zip(accs, base_accs)):
            assert torch.equal(a, b), (sizes, e)                         # (int32 words: bit for bit)
        for e, (s, b) in enumerate(zip(states, base_states)):
            for k in KEYS:
                assert torch.equal(s[k], b[k]), (sizes, e, k)
    # n == 0 at the library is a no-op too
    c = C.case(*key)
    acc = base_accs[0].clone()
    ops.fds_stream_accumulate(torch.empty(0, c.D, device="cuda"), torch.empty(0, device="cuda", dtype=torch.int32), c.bs, c.bn, acc)
    assert torch.equal(acc, base_accs[0])


@pytest.mark.parametrize("key", C.CASE_KEYS, **IDS)
def test_against_float64_second_pass(key):
    from mmdti_hip import ops
    c = C.case(*key)
    got, accs = _streamed(key, (256, 44))
    ref = C.second_pass(*key)
    prev = dict(running_mean=torch.zeros(c.nb, c.D), running_var=torch.ones(c.nb, c.D), num_samples_tracked=torch.zeros(c.nb))
    prev_tracked = torch.zeros(c.nb, dtype=torch.float64)
    zero_var = torch.zeros(c.nb, dtype=torch.bool)
    for e, (g, r) in enumerate(zip(got, ref)):
        untouched = r["num_samples_tracked"] == prev_tracked
        assert bool(untouched.any()) or c.nb == 1
        for k in KEYS:                                                  # a bucket the epoch did not touch keeps every bit
            assert torch.equal(g[k].cpu()[untouched], prev[k][untouched]), (e, k)
        # the constant column: variance exactly 0 wherever the factor-0 epoch wrote it, and it stays 0 under the momentum
        if e == 0:
            zero_var = ~untouched
            assert bool(zero_var.any())
        assert bool((g["running_var"].cpu()[zero_var, C.CONST_COL] == 0).all()), e
        prev, prev_tracked = {k: g[k].cpu() for k in KEYS}, r["num_samples_tracked"].clone()
    for acc in accs:                                                    # ... because every slot's M2 of that column is exactly 0
        rows, mean, m2 = ops.fds_stream_views(acc)
        assert bool((m2[:, C.CONST_COL] == 0).all()) and bool((mean[rows > 0, C.CONST_COL] == C.CONST_VALUE).all())
        assert int(rows.sum()) == C.ROWS                                # every row sits in exactly one slot
    for k in KEYS:                                                      # the no-op call
        assert torch.equal(got[-1][k], got[-2][k]), k
    _check_band(key, got, "D%d_bs%d_bn%d" % key, record=True)


@pytest.mark.parametrize("key", C.CASE_KEYS, **IDS)
def test_merge_of_shards(key):
    """The ranks' accumulators under data parallelism: the batches dealt to two and three accumulators, merged in order."""
    from mmdti_hip import ops
    c = C.case(*key)
    sizes = (40, 60, 1, 99, 56, 44)
    for shards in (2, 3):
        got, _ = _streamed(key, sizes, shards)
        _check_band(key, got, "D%d_bs%d_bn%d/%d shards" % (key + (shards,)))
    # an empty side leaves the other as it is, to the bit
    _, accs = _streamed(key, (300,))
    full, empty = accs[0], ops.fds_stream_new(c.nb, c.D, "cuda")
    dst = empty.clone()
    ops.fds_stream_merge(dst, full)
    assert torch.equal(dst, full)
    dst = full.clone()
    ops.fds_stream_merge(dst, empty)
    assert torch.equal(dst, full)


# ------------------------------------------------------------------------------------------------ module and engine
def _dropout_probabilities(model):
    from types import SimpleNamespace
    ps = []
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            ps.append(float(m.p))
        for k, v in vars(m).items():
            items = vars(v).items() if isinstance(v, SimpleNamespace) else [(k, v)]
            ps += [float(x) for n, x in items if "dropout" in n and isinstance(x, (int, float)) and not isinstance(x, bool)]
    return ps


def _tiny(seed_batches=(4, 5, 6), B=8):
    """The tiny regression + FDS model of test_trainer_gpu.test_training_reduces_loss_and_fds_pass (6 buckets over the batches' own
    labels, no scaler) with every dropout probability 0, twice with the same weights, and a fixed list of device batches."""
    from oracle import mmdti_oracle as O
    from g9util import product_model, tiny_cfg
    ocfg = tiny_cfg("regression", 40)
    host = [O.synth_batch(B, 10, 14, ocfg, seed=s, ragged=True) for s in seed_batches]
    raw = torch.cat([y for _, y in host]).numpy().reshape(-1)
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(product_model(ocfg, fds=True, fds_num=6, _fds_raw_values=raw, use_scaler=False).cuda().train())
    models[1].load_state_dict(models[0].state_dict())
    for m in models:
        ps = _dropout_probabilities(m)
        assert ps and max(ps) == 0.0, ps                                 # no dropout probability is > 0: the two modes see the same features
    batches = [({k: v.cuda() for k, v in b.items()}, y.cuda()) for b, y in host]
    return models, batches


def _ref64_like(fds):
    return FDS64(fds.feature_dim, float(fds.min_value), float(fds.bin_width), fds.kernel_window.cpu(), bucket_num=fds.bucket_num,
                 bucket_start=fds.bucket_start, start_update=fds.start_update, start_smooth=fds.start_smooth, momentum=fds.momentum)


def test_engine_streaming_against_epoch_pass():
    """Two identical engines at learning rate 0, one per mode, two epochs over the same batches: after each epoch every FDS buffer of
    both sits by the float64 second pass on the epoch's features -- the streaming one inside 2 x the epoch pass's own error + FLOOR --
    and the counts agree exactly.  fds_epoch_pass raises in the streaming mode; an eval forward leaves the accumulator alone."""
    from head_refs import FDS_BUFFERS
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    (m_pass, m_str), batches = _tiny()
    t_pass = FineTuner(m_pass, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100)
    t_str = FineTuner(m_str, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100, fds_stats="streaming")
    assert t_pass.fds_stats == "epoch_pass"
    ref = _ref64_like(m_pass.FDS)
    for epoch in range(2):
        t_str.fds_epoch_begin(epoch)
        feats = []
        for i, (dev, y) in enumerate(batches):
            t_pass.step(dev, y, epoch=epoch)
            t_str.step(dev, y, epoch=epoch)
            if i == 0:                                                  # an eval forward between steps
                before = m_str.FDS.stream_state().clone()
                m_str.eval()
                with torch.no_grad():
                    m_str(**dev, epoch=epoch, net_target=y)
                m_str.train()
                assert torch.equal(m_str.FDS.stream_state(), before)
            with torch.no_grad():                                       # what the epoch pass will see (same weights, no dropout)
                feats.append(m_pass(**dev, epoch=epoch, return_feature=True, net_target=y)[1].cpu())
        rows, _, _ = ops.fds_stream_views(m_str.FDS.stream_state())
        assert int(rows.sum()) == sum(y.shape[0] for _, y in batches)
        with pytest.raises(RuntimeError, match="streaming"):
            t_str.fds_epoch_pass(batches, epoch)
        t_pass.fds_epoch_pass(batches, epoch)
        t_str.fds_epoch_finish(epoch)
        assert not m_str.fds_streaming
        ref.update_last_epoch_stats(epoch)
        ref.update_running_stats(torch.cat(feats), torch.cat([y for _, y in batches]).cpu(), epoch)
        assert float(m_str.FDS.epoch) == float(m_pass.FDS.epoch) == float(ref.epoch)
        assert torch.equal(m_str.FDS.num_samples_tracked, m_pass.FDS.num_samples_tracked)
        assert torch.equal(m_str.FDS.num_samples_tracked.cpu().double(), ref.num_samples_tracked)
        for k in FDS_BUFFERS:
            e_one, e_str = nerr(getattr(m_pass.FDS, k), getattr(ref, k)), nerr(getattr(m_str.FDS, k), getattr(ref, k))
            print(f"engine epoch {epoch} {k}: epoch pass {e_one:.3e} streaming {e_str:.3e} band {2 * e_one + FLOOR:.3e}")
            assert e_str <= 2 * e_one + FLOOR, (epoch, k, e_str, e_one)
    assert set(m_str.state_dict()) == set(m_pass.state_dict())
    m_pass.load_state_dict(m_str.state_dict(), strict=True)


def test_default_mode_never_touches_the_streaming_path(monkeypatch):
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    calls = []
    for name in ("fds_stream_new", "fds_stream_accumulate", "fds_stream_merge", "fds_stream_finish"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **kw: calls.append(_n))
    (model, _), batches = _tiny()
    tuner = FineTuner(model, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100)
    for epoch in range(2):
        for dev, y in batches:
            tuner.step(dev, y, epoch=epoch)
        tuner.fds_epoch_pass(batches, epoch)
    assert calls == [] and model.FDS._stream_acc is None and model.fds_streaming is False
    with pytest.raises(RuntimeError, match="epoch_pass"):
        tuner.fds_epoch_begin(0)


def test_graphed_step_streams_and_undoes_its_warm_up():
    """graphed_step in the streaming mode: the accumulate launch is in the graph, and the two warm-up steps of the capture are undone --
    after the capture plus k replays the accumulator holds exactly k * B rows -- and the finished buffers sit where k eager steps on the
    same batch put them (both inside the band of the float64 second pass on those k * B rows)."""
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    (m_eager, m_graph), batches = _tiny()
    dev, y = batches[0]
    B, k = y.shape[0], 3
    t_eager = FineTuner(m_eager, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100, fds_stats="streaming")
    t_graph = FineTuner(m_graph, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100, fds_stats="streaming")
    try:
        t_eager.fds_epoch_begin(0)
        t_graph.fds_epoch_begin(0)
        for _ in range(k):
            t_eager.step(dev, y, epoch=0)
            t_graph.graphed_step(dev, y, epoch=0)
        assert len(t_graph._graphs) == 1
        for m in (m_eager, m_graph):
            assert int(ops.fds_stream_views(m.FDS.stream_state())[0].sum()) == k * B
        with torch.no_grad():
            f = m_eager(**dev, epoch=0, return_feature=True, net_target=y)[1]
        feats, labels = torch.cat([f] * k), torch.cat([y] * k)
        t_eager.fds_epoch_finish(0)
        t_graph.fds_epoch_finish(0)
        ref = _ref64_like(m_eager.FDS)
        ref.update_running_stats(feats.cpu(), labels.cpu(), 0)
        one = _ref64_like(m_eager.FDS)                                  # (only its geometry: the one-shot kernel on fresh device buffers)
        rm, rv, tr = one.running_mean.float().cuda(), one.running_var.float().cuda(), one.num_samples_tracked.float().cuda()
        bins, flags = m_eager.FDS._bins(labels)
        ops.fds_update_stats(feats.contiguous(), bins, flags, one.bucket_start, one.bucket_num, 0.0, rm, rv, tr)
        for name, o in (("running_mean", rm), ("running_var", rv), ("num_samples_tracked", tr)):
            e_one = nerr(o, getattr(ref, name))
            for tag, m in (("eager", m_eager), ("graph", m_graph)):
                e_str = nerr(getattr(m.FDS, name), getattr(ref, name))
                print(f"graph test {tag} {name}: one-shot {e_one:.3e} streaming {e_str:.3e}")
                assert e_str <= 2 * e_one + FLOOR, (tag, name, e_str, e_one)
        assert torch.equal(m_graph.FDS.num_samples_tracked, m_eager.FDS.num_samples_tracked)
    finally:
        ops.seed_salt_reset()


def test_trainer_streaming_replaces_the_epoch_pass(tmp_path, monkeypatch):
    """tasks.Trainer(fds=True, fds_stats="streaming").fit_predict: begin / finish bracket every epoch's steps, the loader is iterated once
    per epoch, fds_epoch_pass is never reached, and the FDS buffers have seen every training row of both epochs."""
    import numpy as np
    from oracle import mmdti_oracle as O
    from g9util import product_model, tiny_cfg
    from mmdti_hip.tasks import Trainer
    from mmdti_hip.trainer import FineTuner

    class _Tok:
        pad_token_id = 1

        def __call__(self, smiles, padding=True, truncation=True, return_tensors="pt"):
            L = max(len(s) for s in smiles) + 2
            ids, att = torch.ones(len(smiles), L, dtype=torch.long), torch.zeros(len(smiles), L, dtype=torch.long)
            for r, s in enumerate(smiles):
                ids[r, :len(s) + 2] = torch.tensor([0] + [5 + (ord(c) % 7) for c in s] + [2])
                att[r, :len(s) + 2] = 1
            return {"input_ids": ids, "attention_mask": att}

    rng = np.random.default_rng(3)
    samples = []
    for _ in range(40):
        na = int(rng.integers(4, 10))
        atoms = rng.choice(np.arange(4, 30), size=na)
        d = O.coords2unimol(atoms, rng.normal(0, 3.0, size=(na, 3)), 31)
        d["smile"] = "C" * int(rng.integers(3, 10))
        samples.append((d, np.array([0.3 * float((atoms == 4).sum()) + 0.1 * rng.normal()], dtype=np.float32)))
    raw = np.array([float(y[0]) for _, y in samples[:32]])
    model = product_model(tiny_cfg("regression", 40), _Tok(), fds=True, fds_num=6, _fds_raw_values=raw, use_scaler=False)
    calls = []
    for name in ("fds_epoch_begin", "fds_epoch_finish", "fds_epoch_pass"):
        real = getattr(FineTuner, name)
        monkeypatch.setattr(FineTuner, name, lambda self, *a, _n=name, _r=real, **kw: (calls.append((_n, a[-1])), _r(self, *a, **kw))[1])
    trainer = Trainer(save_path=str(tmp_path), task="regression", metrics="mse", learning_rate=1e-3, batch_size=8, epochs=2, warmup_ratio=0.1,
                      patience=20, max_norm=5.0, use_cuda=True, use_amp=True, alpha=1, beta=0.1, seed=1, fds=True, fds_stats="streaming")
    y_pred = trainer.fit_predict(model, samples[:32], samples[32:], torch.nn.MSELoss(), lambda x: x, str(tmp_path), 0, None,
                                 return_infonce_loss=True, return_ct_loss=True, use_weight=False)
    assert y_pred.shape == (8, 1) and np.isfinite(y_pred).all()
    assert calls == [("fds_epoch_begin", 0), ("fds_epoch_finish", 0), ("fds_epoch_begin", 1), ("fds_epoch_finish", 1)]
    assert trainer._engine.fds_stats == "streaming" and not model.fds_streaming
    # (the best checkpoint is reloaded at the end: the buffers are those of the epoch it was saved after.)  Every epoch sees all 32 training
    # rows once; a row above the range counts only if the last bin is present (models/fds.py:134-139)
    lb = O.fds_label_bins(torch.tensor(raw, dtype=torch.float32), float(model.FDS.min_value), float(model.FDS.bin_width))
    assert int(lb.min()) == 0
    kept = int(((lb <= 5) | bool((lb == 5).any())).sum())
    epochs_done = float(model.FDS.epoch) + 1
    assert epochs_done in (1.0, 2.0) and float(model.FDS.num_samples_tracked.sum()) == epochs_done * kept
    assert torch.isfinite(model.FDS.running_mean).all() and float(model.FDS.running_var.min()) >= 0


def test_data_parallel_finish_gathers_and_merges_on_a_one_rank_group(monkeypatch):
    """The data-parallel form of fds_epoch_finish on one GPU (a 1-rank RCCL group, MMDTI_FORCE_DDP=1): the accumulators are all-gathered
    in one collective and merged in rank order into an empty one -- which leaves every bit as it was, so the buffers equal the
    single-process engine's.  (Rank order over two ranks: tests/test_fds_stream_parallel_cpu.py.)"""
    import torch.distributed as dist
    import mmdti_hip.parallel as par
    from mmdti_hip import ops
    from mmdti_hip.trainer import FineTuner
    monkeypatch.setenv("MMDTI_FORCE_DDP", "1")
    monkeypatch.setenv("MASTER_PORT", "29579")
    for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")):
        monkeypatch.setenv(k, v)
    (m_one, m_ddp), batches = _tiny()
    merges, gathers = [], []
    real_merge, real_gather = ops.fds_stream_merge, par.gather_fds_accumulators
    monkeypatch.setattr(ops, "fds_stream_merge", lambda d, s: (merges.append(s.clone()), real_merge(d, s))[1])
    monkeypatch.setattr(par, "gather_fds_accumulators", lambda a, g=None: (gathers.append(1), real_gather(a, g))[1])
    par.init_from_env(force=True)
    try:
        t_one = FineTuner(m_one, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100, fds_stats="streaming")
        t_ddp = FineTuner(m_ddp, "regression", learning_rate=0.0, warmup_ratio=0.0, total_steps=100, fds_stats="streaming", distributed=True)
        assert t_ddp.negs.active and t_ddp.world == 1
        for epoch in range(2):
            t_one.fds_epoch_begin(epoch)
            t_ddp.fds_epoch_begin(epoch)
            for dev, y in batches:
                t_one.step(dev, y, epoch=epoch)
                t_ddp.step(dev, y, epoch=epoch)
            before = m_ddp.FDS.stream_state().clone()
            t_one.fds_epoch_finish(epoch)
            t_ddp.fds_epoch_finish(epoch)
            assert len(gathers) == epoch + 1 and len(merges) == epoch + 1 and torch.equal(merges[-1], before)
            assert torch.equal(m_ddp.FDS.stream_state(), before)                      # empty (+) gathered == gathered, to the bit
            assert torch.equal(m_ddp.FDS.stream_state(), m_one.FDS.stream_state())
            for k in ("running_mean", "running_var", "num_samples_tracked", "smoothed_mean_last_epoch", "smoothed_var_last_epoch"):
                assert torch.equal(getattr(m_ddp.FDS, k), getattr(m_one.FDS, k)), (epoch, k)
    finally:
        par._HOST_GROUP = None
        dist.destroy_process_group()
