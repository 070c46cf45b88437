"""Parameter groups of the fused Adam pass: which learning-rate scale and which weight decay each parameter gets.  Pure Python, no
device work: ``resolve`` turns a list of ParamGroup into one group index per parameter and the [ngroups, 2] table (lr_scale,
weight_decay) that ops.adam_step_grouped reads; freeze.arena_group_ids spreads the indices over the arena's blocks of 8 elements.

The rule.  Groups are tried in list order and the FIRST match wins; a parameter no group matches falls into group 0, the default group
(lr_scale 1, the engine's weight_decay).  A group whose weight_decay is None takes the engine's.  Lists concatenate: in
``no_decay(model) + layerwise_decay(model, 0.5)`` a bias is claimed by no_decay (scale 1, no decay) before its layer's group sees it.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass
from typing import Callable, Iterable, List, Optional, Sequence, Tuple, Union

import torch

MAX_GROUPS = 256          # one byte per block of 8 elements names the group


@dataclass
class ParamGroup:
    """match: a name prefix or a comma-separated list of prefixes (freeze.freeze_layers' rule: spaces dropped, str.startswith -- so
    "encoder.layers.1" also matches layers 10-14, "encoder.layers.1." does not); or a callable (name, parameter) -> bool; or an iterable
    of Parameters (matched by identity)."""
    match: Union[str, Callable[[str, torch.nn.Parameter], bool], Iterable[torch.nn.Parameter]]
    lr_scale: float = 1.0
    weight_decay: Optional[float] = None
    name: Optional[str] = None

    def __post_init__(self):
        if not isinstance(self.match, str) and (isinstance(self.match, torch.nn.Module) or not callable(self.match)):
            self.match = tuple(self.match)              # (a generator is read once; a ParameterList is a callable Module)

    def matcher(self) -> Callable[[str, torch.nn.Parameter], bool]:
        m = self.match
        if isinstance(m, str):
            prefixes = [f for f in m.replace(' ', '').split(',') if f]
            return lambda name, p: any(name.startswith(f) for f in prefixes)
        if callable(m):
            return m
        ids = {id(q) for q in m}
        return lambda name, p: id(p) in ids

    def label(self, index: int) -> str:
        if self.name is not None:
            return self.name
        return self.match if isinstance(self.match, str) else f"group{index}"


def _check(what: str, label: str, x: float) -> float:
    x = float(x)
    if not math.isfinite(x) or x < 0.0:
        raise ValueError(f"param_groups: {what} of group {label!r} must be finite and >= 0, got {x!r}")
    return x


def resolve(model: torch.nn.Module, groups: Sequence[ParamGroup], default_weight_decay: float = 0.0) -> Tuple[List[int], List[List[float]]]:
    """-> (index, table): index[k] = the group of the k-th entry of model.named_parameters(), table[g] = [lr_scale, weight_decay].
    Group 0 is the default group (1.0, default_weight_decay); groups[j] is group j + 1.  ValueError: a group that matches no parameter,
    more than 256 groups with the default one, a negative or non-finite lr_scale or weight_decay."""
    groups = list(groups or ())
    if len(groups) + 1 > MAX_GROUPS:
        raise ValueError(f"param_groups: {len(groups)} groups and the default one are more than {MAX_GROUPS}")
    table = [[1.0, _check("weight_decay", "default", default_weight_decay)]]
    for j, g in enumerate(groups):
        label = g.label(j + 1)
        table.append([_check("lr_scale", label, g.lr_scale), table[0][1] if g.weight_decay is None else _check("weight_decay", label, g.weight_decay)])
    matchers = [g.matcher() for g in groups]
    hits = [0] * len(groups)
    index = []
    for name, p in model.named_parameters():
        gid = 0
        for j, match in enumerate(matchers):
            if match(name, p):
                hits[j] += 1                   # (counted for every group it would match: a shadowed group still "matches")
                if gid == 0:
                    gid = j + 1
        index.append(gid)
    for j, g in enumerate(groups):
        if hits[j] == 0:
            raise ValueError(f"param_groups: group {g.label(j + 1)!r} matches no parameter of the model")
    return index, table


def group_names(groups: Sequence[ParamGroup]) -> List[str]:
    """the names of resolve's table rows: "default", then each group's name (or its prefix string, or group<j>)"""
    return ["default"] + [g.label(j + 1) for j, g in enumerate(groups or ())]


# ---------------------------------------------------------------------------------------------- helpers: each returns a list of groups
def no_decay(model: torch.nn.Module) -> List[ParamGroup]:
    """weight_decay = 0 for every parameter with at most one dimension larger than 1: biases, LayerNorm weight and bias, and the pair-bias
    tables gbf.mul / bias / means / stds ([n, 1] and [1, K] embeddings)."""
    return [ParamGroup(lambda name, p: sum(d > 1 for d in p.shape) <= 1, lr_scale=1.0, weight_decay=0.0, name="no_decay")]


def by_prefix(scales: dict) -> List[ParamGroup]:
    """{"encoder": 0.1, "bert": 0.1, ...}: one group per entry, the key a prefix (or a comma-separated list), the value its lr_scale."""
    return [ParamGroup(str(k), lr_scale=float(v), name=str(k)) for k, v in scales.items()]


# (layer-name stem, what sits below layer 0, the group names' stem) of the two pretrained towers
TOWERS = (("encoder.layers.", ("embed_tokens.", "gbf.", "gbf_proj.", "encoder.emb_layer_norm."), "unimol"),
          ("bert.encoder.layer.", ("bert.embeddings.",), "bert"))


def layerwise_decay(model: torch.nn.Module, decay: float) -> List[ParamGroup]:
    """Layer-wise learning-rate decay, per tower: scale = decay ** (L + 1 - depth) with L the tower's layer count; depth 0 is what sits
    below layer 0 (embed_tokens, gbf, gbf_proj and the embedding LayerNorm; the BERT embeddings), layer i is depth i + 1.  Everything
    outside the two towers -- and what sits above a tower's last layer -- keeps scale 1 (the default group).  Layers are matched as
    "...layers.{i}." WITH the trailing dot, so layer 1 does not capture layers 10-14; the names come from named_parameters()."""
    decay = _check("decay", "layerwise_decay", decay)
    names = [n for n, _ in model.named_parameters()]
    out = []
    for stem, below, label in TOWERS:
        pat = re.compile(re.escape(stem) + r"(\d+)\.")
        layers = sorted({int(m.group(1)) for m in map(pat.match, names) if m})
        if not layers:
            continue
        L = layers[-1] + 1
        under = [b for b in below if any(n.startswith(b) for n in names)]
        if under:
            out.append(ParamGroup(",".join(under), lr_scale=decay ** (L + 1), name=f"{label}.depth0"))
        for i in layers:
            out.append(ParamGroup(f"{stem}{i}.", lr_scale=decay ** (L - i), name=f"{label}.depth{i + 1}"))
    return out
