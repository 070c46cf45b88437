"""The InfoNCE memory bank through the engine (FineTuner(memory_bank=Q), DESIGN.md "Memory bank of InfoNCE negatives") on the tiny synthetic
model: B = 4 molecules per step, Q = 8 slots per side, so the ring wraps within three steps.

The host reference (tests/infonce_bank_ref.py) is evaluated in float64 on the step's own L2-normalised embeddings -- read back from the
slots the step pushed -- against a host model of the ring that is fed the same rows: the value of a step depends on the ring exactly as
the model says, wrap-around and id mask included.  Tolerance of the mean loss: the kernel test's bound on the row sum (rtol 2e-5,
atol 1e-4) divided by the 2 B = 8 the caller divides by."""
import gc

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from g9util import product_model, tiny_cfg
from infonce_bank_ref import RingModel, symmetric_ref
from oracle import mmdti_oracle as O

B, Q = 4, 8
RTOL, ATOL = 2e-5, 1e-4 / (2 * B)


@pytest.fixture(autouse=True, scope="module")
def _free_tuners():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _cfg():
    return tiny_cfg("classification", 40)


def _batch(step, ids=True):
    b, y = O.synth_batch(B, 10, 14, _cfg(), seed=60 + step, ragged=False)
    dev = {k: v.cuda() for k, v in b.items()}
    if ids:
        dev["sample_ids"] = (torch.arange(B) + B * (step % 2)).cuda()          # (step 2 brings step 0's molecules back: the id mask bites)
    return dev, y.cuda()


def _engine(state=None, **kw):
    from mmdti_hip.trainer import FineTuner
    model = product_model(_cfg()).cuda().train()
    if state is not None:
        model.load_state_dict(state)
    kw.setdefault("learning_rate", 1e-3)
    kw.setdefault("total_steps", 10)
    return FineTuner(model, "classification", **kw)


def _ring_host(head):
    return {n: t.detach().cpu().clone() for n, t in head.memory_bank_state()}


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu()


def test_memory_bank_zero_is_the_engine_without_the_argument():
    from mmdti_hip import ops
    try:
        plain = _engine(deterministic=True)
        state = {k: v.clone() for k, v in plain.model.state_dict().items()}
        zero = _engine(state, deterministic=True, memory_bank=0)
        assert zero.memory_bank == 0 and zero.model.infonce.bank_q is None and "memory_bank" not in zero.state_dict()
        for step in range(2):
            dev, y = _batch(step, ids=False)
            a, b = plain.step(dev, y), zero.step(dev, y)
            assert torch.equal(_bits(a.loss), _bits(b.loss)) and torch.equal(_bits(a.infonce_loss), _bits(b.infonce_loss))
        assert torch.equal(_bits(plain.arena.data), _bits(zero.arena.data))
    finally:
        ops.set_deterministic(False)


def test_steps_follow_the_host_reference_across_the_wrap():
    plain = _engine()
    state = {k: v.clone() for k, v in plain.model.state_dict().items()}
    eng = _engine(state, memory_bank=Q)
    head = eng.model.infonce
    assert eng.memory_bank == Q and set(eng.model.state_dict()) == set(state)
    rings = RingModel(Q, 50), RingModel(Q, 50)
    for step in range(4):
        dev, y = _batch(step)
        out = eng.step(dev, y)
        if step == 0:
            # the bank is still empty: the bank-less engine's value (same weights, no dropout), up to the summation order
            ref0 = plain.step({k: v for k, v in dev.items() if k != "sample_ids"}, y)
            torch.testing.assert_close(out.infonce_loss.cpu(), ref0.infonce_loss.cpu(), rtol=RTOL, atol=ATOL)
        now = _ring_host(head)
        slots = [(rings[0].head + i) % Q for i in range(B)]
        q, k, ids = now["q.rows"][slots], now["k.rows"][slots], dev["sample_ids"].cpu()
        want = symmetric_ref(q, k, rings[0], rings[1], ids)
        seen = int(rings[0].valid.sum())
        print(f"step {step}: {seen} slots seen, infonce {float(out.infonce_loss):.6f}, reference {float(want):.6f}")
        torch.testing.assert_close(out.infonce_loss.double().cpu().reshape(()), want, rtol=RTOL, atol=ATOL)
        if step > 0:                       # and the bank matters: the bank-less value of the same embeddings is another number
            empty = RingModel(Q, 50)
            assert abs(float(symmetric_ref(q, k, empty, empty)) - float(want)) > 100 * ATOL
        rings[0].push(q, ids)
        rings[1].push(k, ids)
        for side, ring in zip("qk", rings):
            assert int(now[f"{side}.head"]) == ring.head and torch.equal(now[f"{side}.valid"], ring.valid)
            assert torch.equal(now[f"{side}.ids"], ring.ids) and torch.equal(now[f"{side}.rows"], ring.rows)
    assert rings[0].head == (4 * B) % Q and int(rings[0].valid.sum()) == Q


def test_eval_and_no_grad_forwards_leave_the_bank_alone():
    eng = _engine(memory_bank=Q)
    head = eng.model.infonce
    dev, y = _batch(0)
    eng.step(dev, y)
    before = _ring_host(head)
    kw = dict(return_infonce_loss=True, return_ct_loss=True, net_target=y)
    with torch.no_grad():
        train_value = eng.model(**dev, **kw)[1]
    eng.model.eval()
    with torch.no_grad():
        eng.model(**dev, **kw)
    eval_value = eng.model(**dev, **kw)[1].detach()    # (eval with gradients enabled)
    eng.model.train()
    after = _ring_host(head)
    for n in before:
        assert torch.equal(_bits(before[n]), _bits(after[n])), n
    assert abs(float(train_value) - float(eval_value)) <= RTOL * abs(float(eval_value)) + ATOL
    # ... and they do not read it either: a training forward with gradients pushes these inputs' embeddings (slots B .. 2 B - 1), whose
    # bank-less reference is the value above, while its own, banked value is another number
    banked = eng.model(**dev, **kw)[1].detach()
    pushed = _ring_host(head)
    q, k = pushed["q.rows"][B:2 * B], pushed["k.rows"][B:2 * B]
    empty = RingModel(Q, 50)
    torch.testing.assert_close(train_value.double().cpu().reshape(()), symmetric_ref(q, k, empty, empty), rtol=RTOL, atol=ATOL)
    assert abs(float(banked) - float(train_value)) > 100 * ATOL and int(pushed["q.head"]) == 2 * B % Q
    head.reset_memory_bank()
    assert int(head.bank_q.valid.sum()) == 0 and int(head.bank_k.head) == 0


def test_graphed_replays_match_eager_steps():
    from mmdti_hip import ops
    t1 = _engine(memory_bank=Q, warmup_ratio=0.5, max_norm=5.0)
    state = {k: v.clone() for k, v in t1.model.state_dict().items()}
    t2 = _engine(state, memory_bank=Q, warmup_ratio=0.5, max_norm=5.0)
    try:
        for step in range(3):
            dev, y = _batch(step)
            o1, o2 = t1.step(dev, y), t2.graphed_step(dev, y)
            assert abs(float(o1.loss) - float(o2.loss)) <= 2e-4 * abs(float(o1.loss)) + 1e-6, (step, float(o1.loss), float(o2.loss))
            assert abs(float(o1.infonce_loss) - float(o2.infonce_loss)) <= 2e-4 * abs(float(o1.infonce_loss)), step
        assert len(t2._graphs) == 1
        r1, r2 = _ring_host(t1.model.infonce), _ring_host(t2.model.infonce)
        for n in r1:
            if n.endswith("rows"):          # (the capture's two warm-up steps were undone: the same three pushes, embeddings as close as the losses)
                torch.testing.assert_close(r1[n], r2[n], rtol=0, atol=2e-4)
            else:
                assert torch.equal(r1[n], r2[n]), n
        assert int(r1["q.head"]) == (3 * B) % Q and int(r1["q.valid"].sum()) == Q
        errs = [float((p1 - p2).norm() / (p1.norm() + 1e-12)) for (n, p1), (_, p2) in zip(t1.model.named_parameters(), t2.model.named_parameters())
                if p1.requires_grad and not any(z in n for z in ("key.bias", "gbf_proj.linear2.bias", "pooler"))]
        assert float(np.median(errs)) < 1e-4 and max(errs) < 5e-2, (float(np.median(errs)), max(errs))
    finally:
        ops.seed_salt_reset()


def test_state_round_trip_continues_in_the_same_bits(tmp_path):
    from mmdti_hip import checkpoint, ops
    try:
        ta = _engine(deterministic=True, memory_bank=Q)
        state = {k: v.clone() for k, v in ta.model.state_dict().items()}
        la = [ta.step(*_batch(s)).loss.clone() for s in range(3)]
        tb = _engine(state, deterministic=True, memory_bank=Q)
        lb = [tb.step(*_batch(s)).loss.clone() for s in range(2)]
        torch.save(tb.state_dict(), tmp_path / "engine.pth")
        sd = checkpoint.load(tmp_path / "engine.pth")
        assert sd["memory_bank"]["slots"] == Q and int(sd["memory_bank"]["q.head"]) == 0 and int(sd["memory_bank"]["k.valid"].sum()) == Q
        tc = _engine(deterministic=True, memory_bank=Q)
        with torch.no_grad():
            for p in tc.model.parameters():
                p.add_(0.05)
        ptrs = [t.data_ptr() for _, t in tc.model.infonce.memory_bank_state()]
        tc.load_state_dict(sd)
        assert ptrs == [t.data_ptr() for _, t in tc.model.infonce.memory_bank_state()]          # (copied into the existing buffers)
        lb.append(tc.step(*_batch(2)).loss.clone())
        for x, y in zip(la, lb):
            assert torch.equal(_bits(x), _bits(y)), (float(x), float(y))
        assert torch.equal(_bits(ta.arena.data), _bits(tc.arena.data))
        for (n, x), (_, y) in zip(ta.model.infonce.memory_bank_state(), tc.model.infonce.memory_bank_state()):
            assert torch.equal(_bits(x), _bits(y)), n
        # a state with a bank on one side only, or another Q, is refused before anything is written
        for other in (_engine(deterministic=True), _engine(deterministic=True, memory_bank=2 * Q)):
            was = _bits(other.arena.data)
            with pytest.raises(ValueError, match="memory bank"):
                other.load_state_dict(sd)
            assert torch.equal(was, _bits(other.arena.data))
        with pytest.raises(ValueError, match="memory bank"):
            tc.load_state_dict(_engine(deterministic=True).state_dict())
    finally:
        ops.set_deterministic(False)


def test_accumulated_steps_micro_reads_then_pushes_and_union_is_refused():
    eng = _engine(memory_bank=Q)
    micro = [_batch(0), _batch(1)]
    with pytest.raises(ValueError, match="union"):
        eng.step_accumulated(micro, negatives="union")
    assert int(eng.model.infonce.bank_q.valid.sum()) == 0            # (refused before anything ran)
    out = eng.step_accumulated(micro, negatives="micro")
    ring = _ring_host(eng.model.infonce)
    assert int(ring["q.head"]) == (2 * B) % Q and int(ring["q.valid"].sum()) == 2 * B and torch.isfinite(out.infonce_loss)
    assert ring["q.ids"].tolist() == list(range(2 * B))
    # a bank smaller than the batch cannot hold a step's rows
    small = _engine(memory_bank=2)
    with pytest.raises(ValueError, match="smaller than the global batch"):
        small.step(*_batch(0))
