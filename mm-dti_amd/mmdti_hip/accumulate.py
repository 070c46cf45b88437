"""Gradient accumulation whose contrastive terms see the union of the micro-batches: ranks laid out in time.

``parallel.GlobalNegatives`` makes N ranks optimise the single-process loss of their union batch: every rank gathers the others'
messages (InfoNCE's pooled projections [b, 2 d]; ConR / SupCon's ``CTPayload`` [b, D + 3], plus int64 labels for multilabel), computes
its anchors' share of the union loss and receives, through ``reduce_scatter``, what the other ranks' anchors send to its rows.
``TimeNegatives`` offers the same three members -- ``gather``, ``reduce_scatter``, ``row0`` -- to k micro-batches of ONE process that run
one after the other (``FineTuner.step_accumulated(negatives="union")``, DESIGN.md "Accumulated steps"):

  record   pass 1, under no_grad: ``gather`` keeps a copy of the micro-batch's message and returns it alone (row0 = 0: the loss
           functions compute a local value that nobody reads);
  prepare  between the passes, on the cached union only: for every virtual rank j the gradient its anchors' share sends to every row
           of the union, from a function the caller supplies (the row-block kernels on the device, float64 torch in the tests);
  replay   pass 2, forward + backward: ``gather`` returns the union with the own rows replaced by the LIVE message, ``reduce_scatter(G)``
           the own rows of the live share's gradient plus the cached contributions of the other micro-batches' anchors to them --
           what a rank sees under data parallelism, with the other ranks' halves computed a little earlier.

Nothing here touches a device API: the object works on any tensors.
"""
from __future__ import annotations

from typing import Callable, List, Optional

import torch

ACCUM_NEGATIVES = ("union", "micro")


def check_accumulation(sizes, negatives: str, world: int = 1):
    """The rules of an accumulated step, on host integers alone: ``sizes`` the micro-batches' row counts, ``world`` the ranks behind
    the engine.  -> (k, B).  union mode needs equal sizes (ValueError: the row-block entry points assume equal blocks) and one rank
    (RuntimeError: ranks x micro-batches is a follow-up)."""
    sizes = [int(s) for s in sizes]
    if negatives not in ACCUM_NEGATIVES:
        raise ValueError(f"step_accumulated: negatives must be one of {ACCUM_NEGATIVES}, got {negatives!r}")
    if not sizes or min(sizes) < 1:
        raise ValueError(f"step_accumulated: needs at least one micro-batch, none of them empty (sizes {sizes})")
    if negatives == "union" and len(sizes) > 1:
        if world > 1:
            raise RuntimeError(f"step_accumulated: negatives='union' is not supported with more than one rank (world = {world}): the union "
                               "of ranks x micro-batches is not built yet -- use negatives='micro', or global_ct with a larger per-rank batch")
        if len(set(sizes)) != 1:
            raise ValueError(f"step_accumulated: negatives='union' needs micro-batches of equal size, got {sizes} (use negatives='micro')")
    return len(sizes), sum(sizes)


def optimizer_steps_per_epoch(batches_per_epoch: int, accum_steps: int) -> int:
    """Loader batches are taken k at a time; a trailing incomplete group is dropped (as the loader's drop_last drops a short batch)."""
    if int(accum_steps) < 1:
        raise ValueError(f"accum_steps must be >= 1, got {accum_steps!r}")
    return int(batches_per_epoch) // int(accum_steps)


def groups_of(batches, accum_steps: int):
    """Consecutive groups of ``accum_steps`` items of an iterable; the incomplete last one is dropped."""
    group = []
    for b in batches:
        group.append(b)
        if len(group) == accum_steps:
            yield group
            group = []


class TimeChannel:
    """One message stream of the k micro-batches (InfoNCE's, or ConR / SupCon's with its optional int64 label message).  A plain object
    with ``gather``, ``reduce_scatter`` and ``row0``: pass them to ``InfoNCE.set_global_negatives`` / ``MM_Model.set_global_contrast``
    after ``at(i)`` has chosen the micro-batch (both read ``row0`` when they are set)."""

    def __init__(self, k: int):
        self.k = int(k)
        self.phase = "record"
        self.index = 0
        self.recorded: List[dict] = [dict() for _ in range(self.k)]
        self.union: dict = {}                       # "f": the float message of all k micro-batches, "i": the integer one (if any)
        self.b = 0
        self.other: Optional[torch.Tensor] = None   # [k, b, C]: what the OTHER micro-batches' anchors send to micro-batch i's rows

    @staticmethod
    def _kind(x):
        return "f" if x.is_floating_point() else "i"

    def at(self, i: int) -> "TimeChannel":
        if not 0 <= i < self.k:
            raise IndexError(f"TimeChannel.at: micro-batch {i} of {self.k}")
        self.index = int(i)
        return self

    @property
    def used(self) -> bool:
        return bool(self.recorded[0])

    @property
    def row0(self) -> int:
        return 0 if self.phase == "record" else self.index * self.b

    def _rows(self):
        return slice(self.index * self.b, (self.index + 1) * self.b)

    def gather(self, x: torch.Tensor) -> torch.Tensor:
        if self.phase == "record":
            self.recorded[self.index][self._kind(x)] = x.detach().clone()
            return x
        u = self.union.get(self._kind(x))
        if u is None or x.shape[0] != self.b or x.shape[1:] != u.shape[1:]:
            raise ValueError(f"TimeChannel.gather: a {tuple(x.shape)} message in pass 2 where pass 1 recorded "
                             f"{None if u is None else (self.b,) + tuple(u.shape[1:])} per micro-batch")
        out = u.clone()
        out[self._rows()] = x
        return out

    def reduce_scatter(self, g: torch.Tensor) -> torch.Tensor:
        if self.phase == "record":
            return g
        if self.other is None:
            raise RuntimeError("TimeChannel.reduce_scatter: prepare() has not run -- the other micro-batches' contributions are unknown")
        return g[self._rows()] + self.other[self.index]

    def seal(self):
        """End of pass 1: the union of what was recorded, in micro-batch order."""
        for kind in self.recorded[0]:
            parts = [r.get(kind) for r in self.recorded]
            if any(p is None for p in parts) or len({tuple(p.shape) for p in parts}) != 1:
                raise ValueError("TimeChannel.seal: the micro-batches recorded messages of different shapes: "
                                 f"{[None if p is None else tuple(p.shape) for p in parts]}")
            self.union[kind] = torch.cat(parts, dim=0)
            self.b = parts[0].shape[0]
        self.phase = "sealed"

    def prepare(self, share_grad: Callable):
        """``share_grad(channel, j) -> [k b, C]``: the gradient of virtual rank j's share of the union loss with respect to the rows the
        loss function hands to ``reduce_scatter`` (the whole gathered message for InfoNCE, its first D columns for ConR / SupCon).
        Keeps, for every micro-batch i, the sum over j != i of rows [i b, (i + 1) b) -- added in the order of j, one adder per element."""
        if self.phase != "sealed":
            raise RuntimeError("TimeChannel.prepare: seal() first")
        k, b = self.k, self.b
        sent = torch.stack([share_grad(self, j).detach() for j in range(k)])       # [k (anchors of j), k b, C]
        sent = sent.reshape(k, k, b, sent.shape[-1]).clone()
        for j in range(k):
            sent[j, j].zero_()                       # (the own anchors' part comes live, from the pass-2 share)
        self.other = sent.sum(dim=0)
        self.phase = "replay"


class UnionProbe:
    """For ``prepare`` through a loss function itself: a provider whose ``gather`` ignores the message it is handed and returns the
    cached union, and whose ``reduce_scatter`` keeps what it is handed -- virtual rank j's contribution to every row -- in ``sent``.
    ``models.contrastive`` called with it computes rank j's share with its own mode and constants (none is restated elsewhere)."""

    def __init__(self, channel: TimeChannel, j: int):
        self.channel, self.row0, self.sent = channel, j * channel.b, None
        self._rows = slice(j * channel.b, (j + 1) * channel.b)

    def gather(self, x):
        return self.channel.union[TimeChannel._kind(x)]

    def reduce_scatter(self, g):
        self.sent = g.detach().clone()
        return g[self._rows]


class TimeNegatives:
    """The two channels of an accumulated step over k micro-batches."""

    def __init__(self, k: int):
        self.k = int(k)
        self.infonce, self.ct = TimeChannel(k), TimeChannel(k)

    def seal(self):
        for c in (self.infonce, self.ct):
            if c.used:
                c.seal()
