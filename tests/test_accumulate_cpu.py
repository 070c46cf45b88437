"""Accumulated steps, the parts that need no GPU (mmdti_hip/accumulate.py, DESIGN.md "Accumulated steps"): the time-provider on
float64 torch shares, DropoutState's mark / rewind, the Trainer's grouping functions, and the reducer's one-reduction-per-bucket under
gloo."""
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "mm-dti_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ct_rows_ref as R                                     # noqa: E402
from oracle import mmdti_oracle as O                       # noqa: E402

F64 = torch.float64
T_INFO = 0.1
B_LOC = 3


# ------------------------------------------------------------------------------------------------ 8. the time-provider alone
def _infonce_share(both, d, row0, rows):
    """float64 share of the symmetric InfoNCE loss of `both` [Bg, 2 d] (query | positive) that anchors row0 .. row0 + rows - 1 own:
    (1 / (2 Bg)) sum over them of the two cross-entropy terms (what mmdti_infonce_dir adds up in its two calls)"""
    q = torch.nn.functional.normalize(both[:, :d], dim=1)
    k = torch.nn.functional.normalize(both[:, d:], dim=1)
    logits = q @ k.T / T_INFO
    idx = torch.arange(row0, row0 + rows)
    a = torch.logsumexp(logits[idx], dim=1) - logits[idx, idx]
    b = torch.logsumexp(logits.T[idx], dim=1) - logits[idx, idx]
    return (a.sum() + b.sum()) / (2.0 * both.shape[0])


def _grad(fn, x):
    x = x.detach().clone().requires_grad_()
    y = fn(x)
    (g,) = torch.autograd.grad(y, x, allow_unused=True)
    return y.detach(), (torch.zeros_like(x) if g is None else g)


def _share_fn(kind, k):
    """-> (messages [k][b, C] float64, share(union, row0, rows)) for the InfoNCE message or a ConR / SupCon f-hat message"""
    Bg = k * B_LOC
    if kind == "infonce":
        d = 5
        g = torch.Generator().manual_seed(11 + k)
        msg = torch.randn(Bg, 2 * d, generator=g, dtype=F64)
        return list(msg.split(B_LOC)), lambda u, row0, rows: _infonce_share(u, d, row0, rows)
    for seed in range(5 + k, 60):           # (6 or 9 molecules: the first seeded case whose masks leave the term a gradient)
        c = R.ct_inputs(kind, Bg, 8, seed=seed)
        fh = torch.nn.functional.normalize(c["f"].to(F64), dim=1)
        kw = R.ref_kwargs(kind, c)
        share = lambda u, row0, rows, c=c, kw=kw: R.share(kind, u, c["labels"], row0, rows, normalize=False, **kw)
        if float(_grad(lambda u: share(u, 0, Bg), fh)[1].abs().max()) > 0.0:
            return list(fh.split(B_LOC)), share
    raise AssertionError(f"no seeded {kind} case with a non-zero gradient")


def _through_provider(msgs, share, live=None):
    """record, prepare, replay -> (sum of the replayed shares, the gradient every micro-batch's live message receives [k][b, C])"""
    from mmdti_hip.accumulate import TimeChannel
    k = len(msgs)
    ch = TimeChannel(k)
    for i, m in enumerate(msgs):
        assert ch.at(i).row0 == 0 and ch.gather(m) is m                    # pass 1: the message alone, anchors at row 0
    ch.seal()
    ch.prepare(lambda c, j: _grad(lambda u: share(u, j * c.b, c.b), c.union["f"])[1])
    total, grads = 0.0, []
    for i in range(k):
        x = (msgs if live is None else live)[i]
        gathered = ch.at(i).gather(x)
        assert ch.row0 == i * B_LOC and gathered.shape[0] == k * B_LOC
        assert torch.equal(gathered[i * B_LOC:(i + 1) * B_LOC], x)          # the live rows, not the cached ones
        s, G = _grad(lambda u: share(u, ch.row0, B_LOC), gathered)
        total = total + s
        grads.append(ch.reduce_scatter(G))
    return total, grads


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("kind", ["infonce", "regress", "single", "multi"])
def test_time_provider_assembles_the_union_loss_and_gradient(kind, k):
    msgs, share = _share_fn(kind, k)
    union = torch.cat(msgs)
    Bg = union.shape[0]
    ref_loss, ref_grad = _grad(lambda u: share(u, 0, Bg), union)
    total, grads = _through_provider(msgs, share)
    assert float(ref_grad.abs().max()) > 0.0
    assert abs(float(total - ref_loss)) <= 1e-12 * max(1.0, abs(float(ref_loss)))
    assert float((torch.cat(grads) - ref_grad).abs().max()) <= 1e-12 * max(1.0, float(ref_grad.abs().max()))
    if kind == "infonce":                                    # the share formula itself: the oracle's symmetric info_nce on the union
        d = union.shape[1] // 2
        sym = 0.5 * (O.info_nce(union[:, :d], union[:, d:], temperature=T_INFO) + O.info_nce(union[:, d:], union[:, :d], temperature=T_INFO))
        assert abs(float(ref_loss - sym)) <= 1e-12


@pytest.mark.parametrize("kind", ["infonce", "single"])
def test_the_live_rows_receive_the_gradient(kind):
    """Pass 2 does not reproduce pass 1 exactly (another dropout mask, another rounding): micro-batch i's gradient is the live share's
    own rows, taken at the LIVE message, plus the cached contributions -- not the gradient at the cached message."""
    k = 3
    msgs, share = _share_fn(kind, k)
    g = torch.Generator().manual_seed(3)
    live = [m + 1e-3 * torch.randn(m.shape, generator=g, dtype=F64) for m in msgs]
    _, at_cached = _through_provider(msgs, share)
    _, at_live = _through_provider(msgs, share, live=live)
    union = torch.cat(msgs)
    for i in range(k):
        rows = slice(i * B_LOC, (i + 1) * B_LOC)
        mixed = union.clone()
        mixed[rows] = live[i]
        # expected, term by term: own anchors at the mixed union, the other virtual ranks' anchors at the cached union
        own = _grad(lambda u: share(u, i * B_LOC, B_LOC), mixed)[1][rows]
        others = sum(_grad(lambda u, j=j: share(u, j * B_LOC, B_LOC), union)[1][rows] for j in range(k) if j != i)
        assert float((at_live[i] - (own + others)).abs().max()) <= 1e-12
        assert float((at_live[i] - at_cached[i]).abs().max()) > 1e-6          # and it does differ from the all-cached gradient


def test_provider_refuses_what_it_cannot_place():
    from mmdti_hip.accumulate import TimeChannel
    ch = TimeChannel(2)
    ch.at(0).gather(torch.zeros(3, 4))
    ch.at(1).gather(torch.zeros(2, 4))
    with pytest.raises(ValueError):
        ch.seal()
    ch = TimeChannel(2)
    for i in range(2):
        ch.at(i).gather(torch.zeros(3, 4))
    ch.seal()
    with pytest.raises(RuntimeError):
        ch.at(0).reduce_scatter(torch.zeros(6, 4))                     # before prepare()
    ch.prepare(lambda c, j: torch.zeros(6, 4))
    with pytest.raises(ValueError):
        ch.at(0).gather(torch.zeros(2, 4))                             # another row count than pass 1 recorded


# ------------------------------------------------------------------------------------------------ 9. DropoutState
def test_dropout_state_seeds_are_unchanged_and_rewind_replays_them():
    from mmdti_hip.runtime import DropoutState
    st = DropoutState()
    st.reseed(77)
    # (77 * 0x9E3779B97F4A7C15 + n * 0xD1B54A32D192ED03) mod 2^64 for n = 1, 2, 3, written out
    pinned = [0x6864E6FE1AFA3F54, 0x3A1A3130EC8D2C57, 0x0BCF7B63BE20195A]
    assert pinned == [(77 * 0x9E3779B97F4A7C15 + n * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF for n in (1, 2, 3)]
    first = st.next_seed()
    mark = st.mark()
    rest = [st.next_seed(), st.next_seed()]
    assert [first] + rest == pinned
    end = st.mark()
    st.rewind(mark)
    assert [st.next_seed(), st.next_seed()] == rest and st.mark() == end
    st.rewind(mark)
    st.rewind(end)                                                     # forwards, past a replay
    fourth = st.next_seed()
    assert fourth == (77 * 0x9E3779B97F4A7C15 + 4 * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
    st.reseed(77)
    assert st.mark() == 0 and st.next_seed() == pinned[0]
    with pytest.raises(ValueError):
        st.rewind(-1)


# ------------------------------------------------------------------------------------------------ 10. grouping
def _cpu_batch(B, N, L, fill):
    return {"src_tokens": torch.full((B, N), fill, dtype=torch.long), "src_distance": torch.full((B, N, N), float(fill)),
            "src_edge_type": torch.full((B, N, N), fill, dtype=torch.long), "src_coord": torch.full((B, N, 3), float(fill)),
            "input_ids": torch.full((B, L), fill + 10, dtype=torch.long), "attention_mask": torch.ones(B, L, dtype=torch.long),
            "atom_counts": [N] * B, "packable": True}


def test_trainer_groups_batches_and_counts_optimizer_steps():
    from mmdti_hip.accumulate import groups_of, optimizer_steps_per_epoch
    from mmdti_hip.tasks.trainer import Trainer
    assert optimizer_steps_per_epoch(7, 3) == 2 and optimizer_steps_per_epoch(7, 1) == 7 and optimizer_steps_per_epoch(2, 3) == 0
    assert list(groups_of(range(7), 3)) == [[0, 1, 2], [3, 4, 5]]                  # the trailing incomplete group is dropped
    tr = Trainer(task="regression", metrics="mse", epochs=5, accum_steps=3, accum_negatives="micro")
    assert tr.total_optimizer_steps(7) == 10
    assert Trainer(task="regression", metrics="mse", epochs=5).total_optimizer_steps(7) == 35      # default: one batch, one step
    batches = [(_cpu_batch(2, 4 + i, 6 + (i % 2), i + 1), torch.full((2, 1), float(i))) for i in range(7)]
    groups = list(tr.accumulation_groups(iter(batches), pool="all"))
    assert len(groups) == 2 and all(len(g) == 3 for g in groups)
    assert [float(t[0]) for g in groups for _, t in g] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    for bad in (dict(accum_steps=0), dict(accum_negatives="all")):
        with pytest.raises(ValueError):
            Trainer(task="regression", metrics="mse", **bad)


def test_group_padding_pads_every_key_with_its_pad_value():
    from mmdti_hip.parallel import PAD_VALUES, pad_group_to_common_lengths
    group = [_cpu_batch(2, 4, 7, 3), _cpu_batch(2, 6, 5, 4), _cpu_batch(2, 5, 6, 5)]
    out = pad_group_to_common_lengths(group, pool="all")
    for src, got in zip(group, out):
        n, l = src["src_tokens"].shape[1], src["input_ids"].shape[1]
        assert got["src_tokens"].shape == (2, 6) and got["src_distance"].shape == (2, 6, 6) and got["src_edge_type"].shape == (2, 6, 6)
        assert got["src_coord"].shape == (2, 6, 3) and got["input_ids"].shape == (2, 7) and got["attention_mask"].shape == (2, 7)
        for key in PAD_VALUES:
            v, s = got[key], src[key]
            assert v.dtype == s.dtype
            if key in ("src_distance", "src_edge_type"):
                assert torch.equal(v[:, :n, :n], s)
                grown = torch.ones_like(v, dtype=torch.bool)
                grown[:, :n, :n] = False
            elif key in ("src_tokens", "src_coord"):
                assert torch.equal(v[:, :n], s)
                grown = torch.ones_like(v, dtype=torch.bool)
                grown[:, :n] = False
            else:
                assert torch.equal(v[:, :l], s)
                grown = torch.ones_like(v, dtype=torch.bool)
                grown[:, :l] = False
            assert bool((v[grown] == PAD_VALUES[key]).all()), key
        assert got["atom_counts"] is src["atom_counts"] and got["packable"] is True            # host fields pass through
    assert out[1]["src_tokens"] is group[1]["src_tokens"] and out[0]["input_ids"] is group[0]["input_ids"]      # nothing to add: no copy
    same = pad_group_to_common_lengths(group, pool="real")
    assert all(a is b for a, b in zip(same, group))
    for a in same:
        assert a["src_tokens"].shape[1] in (4, 5, 6)


def test_check_refuses_union_over_ranks_and_unequal_sizes():
    from mmdti_hip.accumulate import check_accumulation
    assert check_accumulation([4, 4, 4], "union") == (3, 12)
    assert check_accumulation([5, 4, 3], "micro", world=2) == (3, 12)
    assert check_accumulation([8], "union", world=2) == (1, 8)                 # one micro-batch is step() itself
    with pytest.raises(RuntimeError, match="more than one rank"):
        check_accumulation([4, 4], "union", world=2)
    with pytest.raises(ValueError, match="equal size"):
        check_accumulation([5, 4, 3], "union")
    with pytest.raises(ValueError):
        check_accumulation([4, 4], "all")
    with pytest.raises(ValueError):
        check_accumulation([], "micro")


# ------------------------------------------------------------------------------------------------ 11. the reducer under gloo
class _Arena:
    def __init__(self):
        self.numel = 1000
        self.grad = torch.zeros(1000)
        self.params = [torch.nn.Parameter(torch.zeros(n)) for n in (300, 200, 268, 232)]
        self.offsets, off = {}, 0
        for p in self.params:
            self.offsets[id(p)] = off
            off += p.numel()


def _worker_accumulated_reduce(rank, world, initfile, out):
    """2 ranks x 2 micro-batches of synthetic gradients: the unarmed first backward launches nothing, the armed second one reduces
    every bucket exactly once, and the arena ends as the rank-mean of the per-rank sums."""
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"file://{initfile}")
    from mmdti_hip.parallel import ArenaReducer
    arena = _Arena()
    red = ArenaReducer(arena, bucket_bytes=4 * 256)                      # buckets [0,256) [256,512) [512,768) [768,1000)
    launched = []
    real = red._launch
    red._launch = lambda s, e, events=None: (launched.append((s, e)), real(s, e, events=events))[1]
    base = torch.arange(1000, dtype=torch.float32)
    micro = [base * (rank + 1), base * 10.0 * (rank + 1)]
    # micro-batch 0: adds to the rank's sum, the reducer is not armed
    red.armed = False
    for p in reversed(arena.params):
        lo = arena.offsets[id(p)]
        arena.grad[lo:lo + p.numel()] += micro[0][lo:lo + p.numel()]
        red.on_grads_ready([p])
    assert launched == [] and red._pending == []
    # micro-batch 1: armed -- buckets leave as their parameters report, the rest in finish()
    red.armed = True
    red.begin_step()
    for p in reversed(arena.params[1:]):
        lo = arena.offsets[id(p)]
        arena.grad[lo:lo + p.numel()] += micro[1][lo:lo + p.numel()]
        red.on_grads_ready([p])
    assert launched == [(768, 1000), (512, 768)]
    arena.grad[:300] += micro[1][:300]                                   # (the last parameter never reports: finish() takes its buckets)
    red.finish()
    assert sorted(launched) == [(0, 256), (256, 512), (512, 768), (768, 1000)]      # one reduction per bucket
    torch.testing.assert_close(arena.grad, base * 11.0 * 1.5)            # mean over ranks of (1 + 10)(rank + 1) base
    if rank == 0:
        torch.save({"ok": True}, out)
    dist.destroy_process_group()


def test_reducer_reduces_the_accumulated_sum_once_under_gloo():
    with tempfile.TemporaryDirectory() as td:
        initfile, out = os.path.join(td, "init"), os.path.join(td, "out.pt")
        mp.spawn(_worker_accumulated_reduce, args=(2, initfile, out), nprocs=2, join=True)
        assert torch.load(out)["ok"]
