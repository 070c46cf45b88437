"""Partial fine-tuning: the reference's ``freeze_layers`` (models/nnmodel.py:112-127) sets ``requires_grad = False`` on every
parameter whose name starts with one of the given prefixes.  This module decides, from those flags alone, which part of a
tower's backward has to run.  Pure Python, no device work: the autograd Functions of functional.py follow the plan.

A tower is a stack of layers over something "below" layer 0 (embedding LayerNorm, embedding tables, the module's own inputs).
The backward walks the layers from the top down; it stops at the lowest layer that has a trainable parameter, unless something
below layer 0 wants the stream gradient (then every layer runs down to 0).  The pair tower also chains a pair gradient G from
layer to layer; when the pair-bias front end trains, that chain must reach layer 0, so every layer runs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional, Sequence, Tuple

import torch


def freeze_layers(model: torch.nn.Module, freeze_layers, freeze_layers_reversed: bool = False) -> None:
    """NNModel._init_model's freezing (models/nnmodel.py:117-122), for callers that build the model themselves: every parameter whose
    name starts with one of the prefixes (a list, or a comma-separated string) gets requires_grad = False -- or, reversed, every other
    one.  Prefix matching as in the reference: "encoder.layers.1" also matches layers 10-14.  Call it before building the FineTuner."""
    if isinstance(freeze_layers, str):
        freeze_layers = freeze_layers.replace(' ', '').split(',')
    prefixes = list(freeze_layers)
    for name, p in model.named_parameters():
        hit = any(name.startswith(f) for f in prefixes)
        p.requires_grad = not (freeze_layers_reversed ^ hit)


def first_trainable(params: Iterable[torch.Tensor]) -> Optional[torch.Tensor]:
    """The first parameter that requires grad, or None.  A Function that covers `params` takes it as an extra input (and returns no
    gradient for it): autograd then reaches the Function's backward whenever one of its parameters trains."""
    for p in params:
        if p is not None and p.requires_grad:
            return p
    return None


def grad_anchor(params: Iterable[torch.Tensor]) -> Optional[torch.Tensor]:
    """first_trainable(params) when grad mode is on, else None: the extra input of a module-level Function.  (A Function's
    needs_input_grad reports requires_grad even under torch.no_grad(), so the anchor is left out there: inference keeps nothing.)"""
    return first_trainable(params) if torch.is_grad_enabled() else None


def trainable_flags(params: Iterable[torch.Tensor]) -> Tuple[bool, ...]:
    return tuple(bool(p.requires_grad) for p in params)


def layer_trainable(layers) -> Tuple[bool, ...]:
    """Per layer: does it hold a trainable parameter?"""
    return tuple(first_trainable(l.parameters()) is not None for l in layers)


@dataclass(frozen=True)
class TowerPlan:
    lowest: int                 # lowest layer whose backward runs (== number of layers: none runs)
    dx_out: bool                # the lowest running layer hands a stream gradient down (to layer 0's input)
    below: bool                 # the part under layer 0 runs its backward

    def needs_dx(self, layer: int) -> bool:
        """Does `layer` need the gradient of the stream entering it (its LayerNorm's dx, its input-side dX products)?"""
        return layer > self.lowest or self.dx_out


def plan_tower(layers_trainable: Sequence[bool], below_needs: bool, bias_needs: bool = False) -> TowerPlan:
    """layers_trainable: per layer (bottom first), does it hold a trainable parameter.  below_needs: something under layer 0 wants the
    stream gradient (a trainable embedding LayerNorm or table, or an input that requires grad).  bias_needs: the pair bias entering
    layer 0 requires grad (pair towers), so the G chain runs through every layer."""
    nl = len(layers_trainable)
    if below_needs or bias_needs:
        lowest = 0
    else:
        lowest = next((i for i, t in enumerate(layers_trainable) if t), nl)
    return TowerPlan(lowest=lowest, dx_out=lowest == 0 and bool(below_needs), below=bool(below_needs))


def arena_skip_mask(flags: Sequence[bool], offsets: Sequence[int], sizes: Sequence[int], numel: int, align: int = 8):
    """The per-`align`-element skip mask of the masked Adam pass (ops.adam_step_masked), on the host as a uint8 tensor, or None
    when every parameter trains.  flags / offsets / sizes: per arena parameter (offsets are multiples of `align`)."""
    if all(flags):
        return None
    m = torch.zeros((numel + align - 1) // align, dtype=torch.uint8)
    for f, o, n in zip(flags, offsets, sizes):
        if not f:
            assert o % align == 0
            m[o // align:(o + n + align - 1) // align] = 1
    return m


def arena_group_ids(indices: Sequence[int], offsets: Sequence[int], sizes: Sequence[int], numel: int, align: int = 8):
    """The per-`align`-element group ids of the grouped Adam pass (ops.adam_step_grouped), on the host as a uint8 tensor of
    (numel + align - 1) // align ids.  indices / offsets / sizes: per arena parameter (offsets are multiples of `align`); the padding
    slots behind a parameter, its last ragged block included, take their owner's id."""
    ids = torch.zeros((numel + align - 1) // align, dtype=torch.uint8)
    for g, o, n in zip(indices, offsets, sizes):
        assert o % align == 0 and 0 <= int(g) < 256
        ids[o // align:(o + n + align - 1) // align] = int(g)
    return ids
