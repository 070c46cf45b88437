"""Cases and float64 references of the streaming FDS statistics (FineTuner(fds_stats="streaming"): the training steps feed per-bucket
running moments, the epoch's end is one small kernel -- in place of update_running_stats on a second forward, models/fds.py:116-155,
tasks/trainer.py:288-306).  Shared by test_fds_stream_cases_cpu.py (which shows that every case holds the situations it claims and pins
the slot / merge / finish semantics in float64) and test_fds_stream_gpu.py (which holds the kernels to the same references).

The reference of every numeric check is the float64 SECOND PASS: head_refs.FDS64.update_running_stats on the concatenation of an
epoch's batches, the bins decided in fp32 as head_refs does.  Labels are `bin + 0.5` on a unit grid (min_value 0, bin_width 1), so the
bin of a row is exact and known by construction."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

from head_refs import F64, FDS64
from oracle import mmdti_oracle as O

ROWS = 300                                   # rows of one epoch
WIDTHS = (512, 48)                           # production width; a width below the workgroup size
GEOMETRIES = ((0, 30), (3, 9), (2, 3))       # (bucket_start, bucket_num); the last is the single-bucket case
CHUNKINGS = ((300,), (256, 44), (1,) * 7 + (293,), (100, 0, 200))
CONST_COL, CONST_VALUE = 3, 1.25
MOMENTUM = 0.9
SITUATIONS = ("single_row_bucket", "never_seen_bucket", "below_first_present", "below_first_absent", "above_last_present",
              "above_last_absent", "constant_column", "factor0_then_momentum", "epoch_before_fds_epoch")
CASE_KEYS = tuple((D, bs, bn) for D in WIDTHS for bs, bn in GEOMETRIES)


def _epoch_bins(bs, bn, e, g):
    """The bins of epoch e's 300 rows, shuffled.  nb >= 6: bucket bs + 1 gets exactly one row, bs + 2 none in any epoch; epoch 0 has the
    first bin present and the last absent, epoch 1 the other way round; both have rows below and above the range.  nb == 1 (the only
    bucket is first and last at once): epoch 0 bin present with rows below and above, epoch 1 ONE row of the bin and none below, epoch
    2 bin absent."""
    nb = bn - bs
    if nb == 1:
        below, above = [bs - 1, bs - 2, bs - 3], [bn, bn + 2]
        if e == 0:
            fixed = [bs] * 40 + [below[i % 3] for i in range(200)] + [above[i % 2] for i in range(60)]
        elif e == 1:
            fixed = [bs] + [above[i % 2] for i in range(299)]
        else:
            fixed = [below[i % 3] for i in range(150)] + [above[i % 2] for i in range(150)]
        bins = torch.tensor(fixed)
    else:
        assert nb >= 6
        fixed = [bs + 1] + [bs - 1, bs - 3] * 4 + [bn, bn + 2] * 5 + [bs if e == 0 else bn - 1] * 11
        pool = torch.arange(bs + 3, bn - 1)                              # interior buckets but the single-row and the never-seen one
        rest = pool[torch.randint(0, pool.numel(), (ROWS - len(fixed),), generator=g)]
        bins = torch.cat((torch.tensor(fixed), rest))
    assert bins.numel() == ROWS
    return bins[torch.randperm(ROWS, generator=g)]


@functools.lru_cache(maxsize=None)
def case(D, bs, bn):
    """-> namespace(D, bs, bn, nb, min_value, bin_width, raw, ks, epochs=[(feats fp32 [300, D], labels fp32 [300, 1], bins int64 [300])],
    noop_epoch, claims).  Built once; nobody writes to it."""
    g = torch.Generator().manual_seed(1000 * D + 31 * bs + bn)
    nb = bn - bs
    raw = np.array([0.0, float(bn)])                                     # -> min_value 0, bin_width 1 (FDS.__init__, using_scale False)
    min_value, bin_width = O.FDSOracle.bins_from_raw(raw, bn, False)
    assert (min_value, bin_width) == (0.0, 1.0)
    epochs = []
    for e in range(3 if nb == 1 else 2):
        bins = _epoch_bins(bs, bn, e, g)
        labels = (bins.float() + 0.5).view(-1, 1)
        feats = 0.5 * torch.randn(ROWS, D, generator=g) + 0.1 * bins.float().view(-1, 1) + 0.3 * e
        feats[:, CONST_COL] = CONST_VALUE
        epochs.append((feats, labels, bins))
    claims = {"below_first_present", "below_first_absent", "above_last_absent", "constant_column", "factor0_then_momentum",
              "epoch_before_fds_epoch", "single_row_bucket"}
    if nb > 1:
        claims |= {"never_seen_bucket", "above_last_present"}
    return SimpleNamespace(D=D, bs=bs, bn=bn, nb=nb, min_value=min_value, bin_width=bin_width, raw=raw, ks=1 if nb == 1 else 5,
                           epochs=epochs, noop_epoch=0, claims=frozenset(claims))


def chunks(t, sizes):
    assert sum(sizes) == t.shape[0]
    return list(torch.split(t, list(sizes)))


def situations(c):
    """What the case's epochs really hold, recomputed from the fp32 bin arithmetic of the reference (not from `bins` as built)."""
    found = set()
    touched_first = []
    for e, (feats, labels, bins) in enumerate(c.epochs):
        lb = O.fds_label_bins(labels, c.min_value, c.bin_width)
        assert torch.equal(lb, bins)
        first, last = bool((lb == c.bs).any()), bool((lb == c.bn - 1).any())
        below, above = bool((lb < c.bs).any()), bool((lb > c.bn - 1).any())
        touched_first.append(first)
        if below:
            found.add("below_first_present" if first else "below_first_absent")
        if above and c.nb > 1:
            found.add("above_last_present" if last else "above_last_absent")
        if above and c.nb == 1:
            found.add("above_last_absent")           # (one bucket: rows above it are dropped whether its bin is present or not)
        for b in range(c.bs, c.bn):
            n = int(((lb <= b) if (b == c.bs and first) else (lb >= b) if (b == c.bn - 1 and last and c.nb > 1) else (lb == b)).sum())
            if n == 1 and bool((lb == b).any()):
                found.add("single_row_bucket")
        if bool((feats[:, CONST_COL] == CONST_VALUE).all()):
            found.add("constant_column")
    seen = torch.cat([b for _, _, b in c.epochs])
    if any(not bool((seen == b).any()) for b in range(c.bs + 1, c.bn - 1)):
        found.add("never_seen_bucket")
    if len(c.epochs) >= 2:
        found.add("factor0_then_momentum")           # (epoch 0 == start_update: factor 0; epoch 1: momentum)
    if c.noop_epoch < len(c.epochs) - 1:
        found.add("epoch_before_fds_epoch")          # (after the last epoch FDS.epoch == len(epochs) - 1 > noop_epoch)
    return found


def new_fds64(c, window):
    return FDS64(c.D, c.min_value, c.bin_width, window, bucket_num=c.bn, bucket_start=c.bs, start_update=0, start_smooth=1, momentum=MOMENTUM)


@functools.lru_cache(maxsize=None)
def second_pass(D, bs, bn):
    """The float64 second pass: -> [state after epoch 0, after epoch 1, ..., after the no-op call], each {buffer name: float64 tensor}"""
    c = case(D, bs, bn)
    window = torch.ones(1) if c.ks == 1 else O.fds_kernel_window("gaussian", c.ks, 2)
    ref = new_fds64(c, window)
    states = []
    for e, (feats, labels, _) in enumerate(c.epochs):
        ref.update_last_epoch_stats(e)
        ref.update_running_stats(feats, labels, e)
        states.append(ref.state())
    ref.update_running_stats(*c.epochs[0][:2], c.noop_epoch)             # epoch < FDS.epoch: returns at once
    states.append(ref.state())
    return states


# ------------------------------------------------------------------------------------------------ float64 restatement of the kernels
class Acc64:
    """The accumulator of mmdti_fds_stream_*: nb + 2 slots of (rows, mean[D], M2[D]); slot s < nb: bin exactly bs + s, slot nb: bins
    below the range, slot nb + 1: bins above it."""

    def __init__(self, nb, D):
        self.n = torch.zeros(nb + 2, dtype=torch.int64)
        self.mean = torch.zeros(nb + 2, D, dtype=F64)
        self.m2 = torch.zeros(nb + 2, D, dtype=F64)

    def accumulate(self, feats, bins, bs, bn):
        nb = bn - bs
        slot = torch.where(bins < bs, nb, torch.where(bins > bn - 1, nb + 1, bins - bs))
        part = Acc64(nb, feats.shape[1])
        for s in torch.unique(slot).tolist():
            rows = feats[slot == s].to(F64)
            part.n[s], part.mean[s] = rows.shape[0], rows.mean(0)
            part.m2[s] = ((rows - part.mean[s]) ** 2).sum(0)
        self.merge(part)

    def merge(self, other):
        """Chan's pairwise merge, slot by slot"""
        for s in range(self.n.numel()):
            na, nb = int(self.n[s]), int(other.n[s])
            if nb == 0:
                continue
            if na == 0:
                self.mean[s], self.m2[s] = other.mean[s].clone(), other.m2[s].clone()
            else:
                delta = other.mean[s] - self.mean[s]
                self.mean[s] = self.mean[s] + delta * nb / (na + nb)
                self.m2[s] = self.m2[s] + other.m2[s] + delta * delta * na * nb / (na + nb)
            self.n[s] = na + nb

    def finish(self, bs, bn, factor, running_mean, running_var, tracked):
        nb = bn - bs
        for j in range(nb):
            if int(self.n[j]) == 0:
                continue
            one = Acc64(-1, self.mean.shape[1])
            one.n[0], one.mean[0], one.m2[0] = self.n[j], self.mean[j].clone(), self.m2[j].clone()
            folds = ([nb] if j == 0 else []) + ([nb + 1] if (j == nb - 1 and bs != bn - 1) else [])
            for s in folds:
                other = Acc64(-1, self.mean.shape[1])
                other.n[0], other.mean[0], other.m2[0] = self.n[s], self.mean[s], self.m2[s]
                one.merge(other)
            cnt = int(one.n[0])
            var = one.m2[0] / (cnt - 1 if cnt > 1 else cnt)
            running_mean[j] = (1 - factor) * one.mean[0] + factor * running_mean[j]
            running_var[j] = (1 - factor) * var + factor * running_var[j]
            tracked[j] += cnt


def streamed64(c, sizes, shards=1):
    """The float64 restatement run like the engine runs the kernels: per epoch the batches of `sizes` dealt to `shards` accumulators in
    turn, merged in order, finished.  -> the states in the layout of second_pass (running_mean, running_var, num_samples_tracked only)."""
    rm, rv, tr = torch.zeros(c.nb, c.D, dtype=F64), torch.ones(c.nb, c.D, dtype=F64), torch.zeros(c.nb, dtype=F64)
    states = []
    for e, (feats, labels, _) in enumerate(c.epochs):
        bins = O.fds_label_bins(labels, c.min_value, c.bin_width)
        parts = [Acc64(c.nb, c.D) for _ in range(shards)]
        for i, (f, b) in enumerate(zip(chunks(feats, sizes), chunks(bins, sizes))):
            if f.shape[0]:
                parts[i % shards].accumulate(f, b, c.bs, c.bn)
        total = Acc64(c.nb, c.D)
        for p in parts:
            total.merge(p)
        total.finish(c.bs, c.bn, 0.0 if e == 0 else MOMENTUM, rm, rv, tr)
        states.append(dict(running_mean=rm.clone(), running_var=rv.clone(), num_samples_tracked=tr.clone()))
    states.append(states[-1])                                            # the no-op call
    return states
