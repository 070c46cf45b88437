"""GPU tests of accumulated steps (FineTuner.step_accumulated / forward_backward_accumulated, DESIGN.md "Accumulated steps"): k micro-batches
make one optimizer step; with negatives="union" their contrastive terms are those of the concatenated batch.

Micro-batches are cut by row-slicing ONE collated batch, so padded lengths agree and every molecule's forward is the one it has in the
whole batch.  The band rule is tests/test_ct_global_gpu.py::_within_band's: both sides are measured as max-abs distance from the CPU
oracle (bf16 rounding points), and the accumulated side may sit at most twice as far as the single call + 1e-7 max|ref|."""
import functools
import socket

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from test_trainer_gpu import _model, _ocfg

ZERO_GRADS = ("pooler", "key.bias", "gbf_proj.linear2.bias")          # analytically zero: test_reference_sized_step_vs_oracle's list
B_UNION = 12


# ------------------------------------------------------------------------------------------------ helpers
def _rows(batch, label, sl):
    """rows `sl` of a collated batch: every per-molecule field, host-side length lists included; the padded lengths stay"""
    B = label.shape[0]
    cut = {}
    for k, v in batch.items():
        if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == B:
            cut[k] = v[sl]
        elif isinstance(v, (list, tuple)) and len(v) == B:
            cut[k] = type(v)(v[sl])
        else:
            cut[k] = v
    return cut, label[sl]


def _split(batch, label, sizes):
    out, r = [], 0
    for b in sizes:
        out.append(_rows(batch, label, slice(r, r + b)))
        r += b
    assert r == label.shape[0]
    return out


def _cuda(batch, label):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}, label.cuda()


@functools.lru_cache(maxsize=None)
def _case(task):
    """12 ragged molecules whose contrastive terms NEED the union: every ConR positive pair (labels within ct_w) and half of the SupCon
    positives sit in different micro-batches of the 3 x 4 cut.  -> (host batch incl. weights, label, odim, use_weight)"""
    odim = 1 if task == "regression" else 2
    batch, label = O.synth_batch(B_UNION, 10, 14, _ocfg(task, odim), seed=3, ragged=True)
    i = torch.arange(B_UNION)
    if task == "regression":
        # clusters at 0, 0.5, 1, 1.5 (members i, i + 4, i + 8, within 0.1): positives only ACROSS the 3 x 4 micro-batches
        label = ((i % 4).float() * 0.5 + (i // 4).float() * 0.05).view(label.shape).to(label.dtype)
        batch = dict(batch, weights=torch.linspace(0.5, 1.5, B_UNION))
    else:
        label = torch.tensor([0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 0, 1], dtype=label.dtype).view(label.shape)
    return batch, label, odim, task == "regression"


def _engine(task, odim, state=None, train=False, **kw):
    from mmdti_hip.trainer import FineTuner
    model = _model(task, odim, **kw.pop("model_kw", {}))
    model = model.train() if train else model.eval()
    if state is not None:
        model.load_state_dict(state)
    kw.setdefault("total_steps", 10)
    return FineTuner(model, task, **kw)


def _oracle(model, task, odim, parts, use_weight):
    """float64-free CPU oracle with the kernels' rounding points: sum_i (b_i / B) step_loss(part i), each part on its own.
    -> dict(loss, infonce, ct, grads {name: tensor})"""
    P = {k: v.detach().cpu().float().clone().requires_grad_() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
    ocfg = _ocfg(task, odim)
    B = sum(lab.shape[0] for _, lab in parts)
    loss = infonce = ct = 0.0
    for batch, lab in parts:
        w = lab.shape[0] / B
        ref = O.mm_forward({k: v for k, v in batch.items() if k != "weights"}, P, ocfg, net_target=lab, weights=batch.get("weights"),
                           use_weight=use_weight, bf16=True)
        l, _ = O.step_loss(ref, lab, task)
        loss, infonce, ct = loss + w * l, infonce + w * ref["infonce"].detach(), ct + w * ref["ct"].detach()
    loss.backward()
    return dict(loss=loss.detach(), infonce=infonce, ct=ct, grads={n: p.grad for n, p in P.items() if p.grad is not None})


def _grads(model):
    return {n: p.grad.detach().double().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}


def _distances(out, grads, ref):
    """max-abs distance from the oracle of the three scalars and of every parameter gradient the oracle does not hold at zero"""
    d = {"loss": abs(float(out["loss"]) - float(ref["loss"])), "infonce": abs(float(out["infonce"]) - float(ref["infonce"])),
         "ct": abs(float(out["ct"]) - float(ref["ct"]))}
    for n, g in grads.items():
        g_ref = ref["grads"].get(n)
        if g_ref is None or any(z in n for z in ZERO_GRADS) or float(g_ref.abs().max()) == 0.0:
            continue
        d["grad " + n] = float((g - g_ref.double()).abs().max())
    return d


def _ref_max(ref, what):
    return float(ref["grads"][what[5:]].abs().max()) if what.startswith("grad ") else abs(float(ref[what]))


def _band(what, d_accum, d_single, ref_max):
    floor = 1e-7 * ref_max
    print(f"{what}: accumulated {d_accum:.3e}  single {d_single:.3e}  allowed {2 * d_single + floor:.3e}")
    return d_accum <= 2 * d_single + floor


def _scalars(out):
    return dict(loss=out.loss, infonce=out.infonce_loss, ct=out.ct_loss)


@pytest.fixture
def deterministic_off():
    from mmdti_hip import ops
    try:
        yield
    finally:
        ops.set_deterministic(False)


def _state_of(tuner):
    a = tuner.arena
    return a.data.clone(), a.adam_m.clone(), a.adam_v.clone()


# ------------------------------------------------------------------------------------------------ 1. k = 1
@pytest.mark.parametrize("negatives", ["union", "micro"])
def test_one_micro_batch_is_step_bit_for_bit(negatives, deterministic_off):
    batch, label, odim, uw = _case("regression")
    dev, lab = _cuda(batch, label)
    plain = _engine("regression", odim, deterministic=True, learning_rate=1e-3)
    state = {k: v.detach().clone() for k, v in plain.model.state_dict().items()}
    accum = _engine("regression", odim, state=state, deterministic=True, learning_rate=1e-3)
    for _ in range(2):
        a = plain.step(dev, lab, use_weight=uw)
        b = accum.step_accumulated([(dev, lab)], use_weight=uw, negatives=negatives)
        for f in ("loss", "task_loss", "infonce_loss", "ct_loss", "logits", "skipped", "grad_norm"):
            x, y = getattr(a, f), getattr(b, f)
            assert (x is None and y is None) or torch.equal(x, y), f
    for x, y, what in zip(_state_of(plain), _state_of(accum), ("parameters", "adam_m", "adam_v")):
        assert torch.equal(x, y), what
    assert plain.sched_step == accum.sched_step == 2


# ------------------------------------------------------------------------------------------------ 2. union mode equals the union
@pytest.mark.parametrize("task", ["regression", "classification"])
def test_union_mode_is_the_union_batch(task, deterministic_off):
    """(deterministic mode: every sum into a parameter gradient has a fixed order, so both sides of the band are the same numbers in
    every run -- with atomics a gradient element that is rounding noise on both sides would make the comparison a coin toss)"""
    batch, label, odim, uw = _case(task)
    tuner = _engine(task, odim, deterministic=True)
    ref = _oracle(tuner.model, task, odim, [(batch, label)], uw)
    assert float(ref["ct"]) > 0.0 and float(ref["infonce"]) > 0.0
    dev, lab = _cuda(batch, label)
    micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    single = tuner.forward_backward(dev, lab, use_weight=uw)
    d_single = _distances(_scalars(single), _grads(tuner.model), ref)
    union = tuner.forward_backward_accumulated(micro, use_weight=uw, negatives="union")
    d_union = _distances(_scalars(union), _grads(tuner.model), ref)
    assert union.logits.shape == single.logits.shape and len(d_union) == len(d_single) > 50
    bad = [w for w in d_single if not _band(w, d_union[w], d_single[w], _ref_max(ref, w))]
    assert not bad, bad
    # the test can tell the modes apart: each micro-batch contrasting against itself gives another InfoNCE value, far outside the band
    own = tuner.forward_backward_accumulated(micro, use_weight=uw, negatives="micro")
    allowed = 2 * d_single["infonce"] + 1e-7 * abs(float(ref["infonce"]))
    d_own = abs(float(own.infonce_loss) - float(ref["infonce"]))
    print(f"negatives='micro' InfoNCE: {d_own:.3e} from the union's, allowed {allowed:.3e}")
    assert d_own > 10 * allowed
    assert tuner.model._ct_negatives is None and tuner.model.infonce._gather is None          # the providers were taken out again


# ------------------------------------------------------------------------------------------------ 3. micro mode is the weighted sum
def test_micro_mode_is_the_weighted_sum_of_the_micro_batches(deterministic_off):
    task = "regression"
    batch, label, odim, uw = _case(task)
    sizes = [5, 4, 3]
    parts = _split(batch, label, sizes)
    tuner = _engine(task, odim, deterministic=True)           # (as above: reproducible figures on both sides)
    ref = _oracle(tuner.model, task, odim, parts, uw)
    assert float(ref["ct"]) > 0.0
    micro = [_cuda(*p) for p in parts]
    # single: three separate calls, weighted and summed in float64
    acc_s, acc_g = dict(loss=0.0, infonce=0.0, ct=0.0), {}
    for (dev, lab), b in zip(micro, sizes):
        o = tuner.forward_backward(dev, lab, use_weight=uw)
        for k, v in _scalars(o).items():
            acc_s[k] += b / B_UNION * float(v.double())
        for n, g in _grads(tuner.model).items():
            acc_g[n] = acc_g.get(n, 0.0) + b / B_UNION * g
    d_single = _distances(acc_s, acc_g, ref)
    out = tuner.forward_backward_accumulated(micro, use_weight=uw, negatives="micro")
    d_micro = _distances(_scalars(out), _grads(tuner.model), ref)
    assert out.logits.shape[0] == B_UNION and len(d_micro) == len(d_single) > 50
    bad = [w for w in d_single if not _band(w, d_micro[w], d_single[w], _ref_max(ref, w))]
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 4. dropout replay
def _replay_run(monkeypatch, deterministic):
    from mmdti_hip.accumulate import TimeChannel
    from mmdti_hip.runtime import dropout_state
    batch, label, odim, uw = _case("regression")
    micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    tuner = _engine("regression", odim, train=True, deterministic=deterministic)
    seen, seeds = [], []
    real_gather, real_seed = TimeChannel.gather, dropout_state.next_seed

    def gather(self, x):
        seen.append((self.phase, self.index, x.dtype, x.detach().clone()))
        return real_gather(self, x)

    def next_seed():
        s = real_seed()
        tn = tuner._time_negatives
        seeds.append((None if tn is None else (tn.infonce.phase, tn.infonce.index), s))
        return s

    monkeypatch.setattr(TimeChannel, "gather", gather)
    monkeypatch.setattr(dropout_state, "next_seed", next_seed)
    dropout_state.reseed(77)
    tuner.forward_backward(*micro[0], use_weight=uw)
    per_forward = dropout_state.mark()
    assert per_forward == len(seeds) > 0
    del seeds[:]
    tuner.step_accumulated(micro, use_weight=uw, negatives="union")
    return tuner, seen, seeds, per_forward, dropout_state.mark()


def test_pass_two_draws_the_masks_of_pass_one(monkeypatch, deterministic_off):
    tuner, seen, seeds, per_forward, end = _replay_run(monkeypatch, deterministic=True)
    k = 3
    assert end == per_forward * (1 + k)                                 # the counter advanced by k forwards, not 2 k
    first = [[s for tag, s in seeds if tag == ("record", i)] for i in range(k)]
    second = [[s for tag, s in seeds if tag == ("replay", i)] for i in range(k)]
    assert all(len(f) == per_forward for f in first) and first == second
    flat = [s for f in first for s in f]
    assert len(set(flat)) == len(flat)                                  # different micro-batches draw different seeds
    rec = [(i, dt, x) for ph, i, dt, x in seen if ph == "record"]
    rep = [(i, dt, x) for ph, i, dt, x in seen if ph == "replay"]
    assert len(rec) == len(rep) == 2 * k                                # InfoNCE's message and the CT payload of every micro-batch
    for (i, dt, x), (j, dt2, y) in zip(rec, rep):
        assert i == j and dt == dt2 and torch.equal(x, y), f"micro-batch {i}: the live message of pass 2 is not pass 1's"
    assert tuner._time_negatives is None


def test_pass_two_in_the_default_mode_prints_its_distance(monkeypatch):
    _, seen, _, _, _ = _replay_run(monkeypatch, deterministic=False)
    rec = [x for ph, i, dt, x in seen if ph == "record"]
    rep = [x for ph, i, dt, x in seen if ph == "replay"]
    assert len(rec) == len(rep) > 0
    print("default mode, largest |pass 2 - pass 1| over the live messages:", max(float((a - b).abs().max()) for a, b in zip(rec, rep)))


# ------------------------------------------------------------------------------------------------ 5. once per step
def _second_call_without_sync(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("negatives", ["union", "micro"])
def test_one_inf_label_skips_the_whole_step_once(negatives):
    batch, label, odim, uw = _case("regression")
    micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    tuner = _engine("regression", odim, skip_nonfinite=True, learning_rate=1e-3)
    tuner.step_accumulated(micro, use_weight=uw, negatives=negatives)
    before, sched = _state_of(tuner), tuner.sched_step
    poisoned = [(d, y.clone()) for d, y in micro]
    poisoned[1][1][2] = float("inf")
    out = _second_call_without_sync(lambda: tuner.step_accumulated(poisoned, use_weight=uw, negatives=negatives))
    for x, y, what in zip(before, _state_of(tuner), ("parameters", "adam_m", "adam_v")):
        assert torch.equal(x, y), what
    assert float(tuner.skipped_steps) == 1.0 and float(tuner.optimizer_steps) == 1.0 and float(out.skipped) == 1.0
    assert tuner.sched_step == sched + 1 == 2


def test_the_average_moves_once():
    """ema += (1 - d)(p - ema) with d = ema_decay_at(t) once per optimizer step.  Moving once per micro-batch would leave the average
    (1 - d_2) d_1 (p - ema_0) ~ 0.14 lr = 1.4e-4 away; the fp32 arithmetic of one update on values below 2 rounds at 2^-23 ~ 1.2e-7 per
    operation, so 1e-6 separates the two."""
    from mmdti_hip.trainer import ema_decay_at
    batch, label, odim, uw = _case("regression")
    micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    tuner = _engine("regression", odim, ema_decay=0.999, learning_rate=1e-3, warmup_ratio=0.0)
    ema0 = tuner.arena.ema.clone()
    assert float(ema0.abs().max()) < 2.0
    tuner.step_accumulated(micro, use_weight=uw)
    d = float(ema_decay_at(1, 0.999))
    p = tuner.arena.data
    moved = float((p - ema0).abs().max())
    assert moved > 5e-4                                                  # Adam's first step: ~lr on every element with a gradient
    expect = ema0.double() + (1.0 - d) * (p.double() - ema0.double())
    assert float((tuner.arena.ema.double() - expect).abs().max()) <= 1e-6
    assert tuner.arena.step_count == 1 and tuner.sched_step == 1
    _second_call_without_sync(lambda: tuner.step_accumulated(micro, use_weight=uw))
    assert tuner.arena.step_count == 2 and tuner.sched_step == 2
    with tuner.averaged():                                               # blocked inside averaged(), as step is
        for call in (tuner.step_accumulated, tuner.forward_backward_accumulated):
            with pytest.raises(RuntimeError, match="averaged"):
                call(micro, use_weight=uw)


def test_streaming_fds_sees_every_row_once():
    from mmdti_hip import ops
    batch, label, odim, uw = _case("regression")
    micro = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    tuner = _engine("regression", odim, train=True, fds_stats="streaming",
                    model_kw=dict(fds=True, fds_num=6, _fds_raw_values=label.numpy().reshape(-1), use_scaler=False))
    epoch = tuner.model.fds_cfg.start_update
    tuner.fds_epoch_begin(epoch)
    tuner.step_accumulated(micro, epoch=epoch, use_weight=uw, negatives="union")
    _second_call_without_sync(lambda: tuner.step_accumulated(micro, epoch=epoch, use_weight=uw, negatives="union"))
    rows, _, _ = ops.fds_stream_views(tuner.model.FDS.stream_state())
    assert int(rows.sum()) == 2 * B_UNION                               # two steps: B rows each, not 2 B (pass 1 does not feed it)
    assert tuner.model.fds_streaming is True
    tuner.fds_epoch_finish(epoch)


# ------------------------------------------------------------------------------------------------ 6. memory
def test_accumulated_peak_memory_is_below_the_big_batch():
    task, odim = "classification", 2
    batch, label = O.synth_batch(32, 20, 30, _ocfg(task, odim), seed=9, ragged=True)
    label = (torch.arange(32) % 2).view(label.shape).to(label.dtype)
    dev, lab = _cuda(batch, label)
    micro = [_cuda(*p) for p in _split(batch, label, [8, 8, 8, 8])]
    tuner = _engine(task, odim, train=True, model_kw=dict(wide=True))
    peaks = {}
    for what, call in (("step(32)", lambda: tuner.step(dev, lab)), ("step_accumulated(4 x 8)", lambda: tuner.step_accumulated(micro))):
        call()                                                           # (first call: Adam moments, workspaces, streams)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        call()
        torch.cuda.synchronize()
        peaks[what] = torch.cuda.max_memory_allocated()
        print(f"{what}: peak {peaks[what] / 2**20:.2f} MiB ({(peaks[what] - base) / 2**20:.2f} MiB over the resident state)")
    assert peaks["step_accumulated(4 x 8)"] < peaks["step(32)"]


# ------------------------------------------------------------------------------------------------ 7. one-rank group
@pytest.fixture
def one_rank_group(monkeypatch):
    import torch.distributed as dist
    import mmdti_hip.parallel as par
    from mmdti_hip import ops
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("MMDTI_FORCE_DDP", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MMDTI_GLOBAL_CT", raising=False)
    par.init_from_env(force=True)
    try:
        yield
    finally:
        ops.set_deterministic(False)
        par._HOST_GROUP = None
        dist.destroy_process_group()


def test_one_rank_group_reduces_each_bucket_once(one_rank_group, monkeypatch):
    from mmdti_hip.parallel import ArenaReducer
    task = "classification"
    batch, label, odim, uw = _case(task)
    sizes = [5, 4, 3]
    micro = [_cuda(*p) for p in _split(batch, label, sizes)]
    equal = [_cuda(*p) for p in _split(batch, label, [4, 4, 4])]
    alone = _engine(task, odim, deterministic=True, learning_rate=1e-3)
    state = {k: v.detach().clone() for k, v in alone.model.state_dict().items()}
    ddp = _engine(task, odim, state=state, deterministic=True, learning_rate=1e-3, distributed=True, bucket_bytes=64 << 10)
    assert ddp.negs.active and ddp.reducer.active and len(ddp.reducer.buckets) > 3
    log = []
    real_launch, real_fb = ArenaReducer._launch, ddp.forward_backward
    monkeypatch.setattr(ArenaReducer, "_launch", lambda self, s, e, events=None: (log.append((s, e)), real_launch(self, s, e, events=events))[1])
    ddp.forward_backward = lambda *a, **k: (log.append("forward_backward"), real_fb(*a, **k))[1]

    def check_log():
        calls = [i for i, x in enumerate(log) if x == "forward_backward"]
        launches = [x for x in log if x != "forward_backward"]
        assert len(calls) == 3 and all(x == "forward_backward" for x in log[:calls[-1]])      # nothing leaves before the last backward
        assert sorted(launches) == sorted(ddp.reducer.buckets)                                 # every bucket exactly once
        del log[:]

    for negatives, parts in (("micro", micro), ("union", equal)):
        a = alone.step_accumulated(parts, negatives=negatives)
        b = _second_call_without_sync(lambda: ddp.step_accumulated(parts, negatives=negatives)) if negatives == "union" \
            else ddp.step_accumulated(parts, negatives=negatives)
        check_log()
        for f in ("loss", "task_loss", "infonce_loss", "ct_loss", "logits"):
            assert torch.equal(getattr(a, f), getattr(b, f)), (negatives, f)
        for x, y, what in zip(_state_of(alone), _state_of(ddp), ("parameters", "adam_m", "adam_v")):
            assert torch.equal(x, y), (negatives, what)
    assert ddp.reducer.armed
    with pytest.raises(ValueError, match="equal size"):
        ddp.step_accumulated(micro, negatives="union")
    # a plain step afterwards binds the collectives' providers again
    ddp.step(*equal[0])
    assert ddp.model.infonce._gather == ddp.negs.gather
