"""LoRA adapters on the attention projections (DESIGN.md "LoRA adapters"): an extension, nothing in the reference does this.

``apply_lora(model, cfg)`` freezes every parameter of the selected towers and registers, on each of their attention modules, a rank-r
pair per adapted projection ``W``: ``A`` [r, in] (seeded Kaiming-uniform) and ``B`` [out, r] (zero), so that the projection computes
``x.(W + (alpha / r).B.A)^T``.  The adapters are ordinary parameters (``lora_A`` / ``lora_B`` on tower 1's ``self_attn``, whose fused
``in_proj`` [3D, D] is adapted as a whole; ``lora_A_q`` / ``lora_B_q`` ... on ``attention.self`` of tower 2 and the cross block): the
parameter arena, parameter groups (``ParamGroup(match="lora_")``), EMA, resume and the gradient reducer see them by name.  Call it
before building the FineTuner.  functional.py runs the base projection exactly as before and ops.lora_fwd / lora_bwd / lora_dx next to
it (csrc/lora.hip); adapted layers on a frozen base leave from the library's adapted sequencers (paths.py; ``MMDTI_LORA_SEQ=0``: op by op).

``merge_lora(model)`` folds ``s.B.A`` into the fp32 base weights and removes the adapters: the state dict then has the reference's keys.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Iterator, Sequence, Tuple

import torch
from torch import nn

RANKS = (8, 16, 32)
TARGETS = ("q", "k", "v")
TOWERS = ("bert", "cross", "unimol")
# the parameters a tower name freezes (prefixes of MM_Model's parameter names)
TOWER_PREFIXES = {"unimol": ("embed_tokens.", "encoder.", "gbf.", "gbf_proj."), "bert": ("bert.",), "cross": ("cross_modal_module.",)}
_LINEAR_OF = {"q": "query", "k": "key", "v": "value"}


@dataclass(frozen=True)
class LoRAConfig:
    rank: int = 8
    alpha: float = 16.0
    targets: Sequence[str] = ("q", "v")
    towers: Sequence[str] = TOWERS
    seed: int = 0

    def __post_init__(self):
        object.__setattr__(self, "targets", tuple(self.targets))
        object.__setattr__(self, "towers", tuple(self.towers))
        if self.rank not in RANKS:
            raise ValueError(f"LoRAConfig: rank must be one of {RANKS} (got {self.rank})")
        if not self.targets or any(t not in TARGETS for t in self.targets) or len(set(self.targets)) != len(self.targets):
            raise ValueError(f"LoRAConfig: targets must be a non-empty subset of {TARGETS} (got {self.targets})")
        if not self.towers or any(t not in TOWERS for t in self.towers) or len(set(self.towers)) != len(self.towers):
            raise ValueError(f"LoRAConfig: towers must be a non-empty subset of {TOWERS} (got {self.towers})")
        if not self.alpha > 0:
            raise ValueError(f"LoRAConfig: alpha must be positive (got {self.alpha})")

    @property
    def scale(self) -> float:
        return float(self.alpha) / self.rank


def attention_sites(model, towers: Sequence[str] = TOWERS) -> Iterator[Tuple[str, str, nn.Module]]:
    """(tower, kind, attention module) of every attention of the given towers, in model order.  kind 'fused': tower 1's self_attn
    (one in_proj); 'split': attention.self of tower 2 and of the cross block (query, key, value)."""
    if "unimol" in towers:
        for layer in model.encoder.layers:
            yield "unimol", "fused", layer.self_attn
    if "bert" in towers:
        for layer in model.bert.encoder.layer:
            yield "bert", "split", layer.attention.self
    if "cross" in towers:
        cm = model.cross_modal_module
        for enc in (cm.text_attention, cm.graph_attention):
            for layer in enc.layer:
                yield "cross", "split", layer.attention.self


def adapter_names(kind: str, targets: Sequence[str]):
    """-> [(suffix, name of A, name of B, name of the adapted Linear)]"""
    if kind == "fused":
        return [("", "lora_A", "lora_B", "in_proj")]
    return [(t, f"lora_A_{t}", f"lora_B_{t}", _LINEAR_OF[t]) for t in TARGETS if t in targets]


def _kaiming_uniform(shape, gen):
    """nn.Linear's default (kaiming_uniform_ with a = sqrt(5)): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)), from a seeded host generator"""
    bound = 1.0 / math.sqrt(shape[1])
    return (torch.rand(shape, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound


def has_lora(module: nn.Module) -> bool:
    return any(getattr(m, "lora_targets", None) for m in module.modules())


def apply_lora(model, cfg: LoRAConfig = LoRAConfig()):
    """Freeze the selected towers and attach the adapters (see the module docstring).  Returns the model."""
    if has_lora(model):
        raise ValueError("apply_lora: the model already has adapters (merge_lora first)")
    prefixes = tuple(p for t in cfg.towers for p in TOWER_PREFIXES[t])
    for name, p in model.named_parameters():
        if name.startswith(prefixes):
            p.requires_grad = False
    gen = torch.Generator().manual_seed(int(cfg.seed))
    for _, kind, att in attention_sites(model, cfg.towers):
        names = adapter_names(kind, cfg.targets)
        for _, na, nb, lin in names:
            w = getattr(att, lin).weight
            n_out, n_in = w.shape
            if n_in % 64 or n_out % 64:
                raise ValueError(f"apply_lora: the adapted projections must be multiples of 64 wide (got {lin} [{n_out}, {n_in}])")
            att.register_parameter(na, nn.Parameter(_kaiming_uniform((cfg.rank, n_in), gen).to(w.device)))
            att.register_parameter(nb, nn.Parameter(torch.zeros(n_out, cfg.rank, device=w.device)))
        att.lora_targets = tuple(s for s, *_ in names)
        att.lora_scale = cfg.scale
    model.lora_config = cfg
    return model


def _adapters(model):
    for tower, kind, att in attention_sites(model):
        tg = getattr(att, "lora_targets", None)
        if tg:
            for s, na, nb, lin in adapter_names(kind, TARGETS):
                if s in tg:
                    yield att, na, nb, lin


def lora_state_dict(model) -> Dict[str, torch.Tensor]:
    """the adapters only, under their state-dict names (host copies)"""
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if ".lora_A" in k or ".lora_B" in k}


def load_lora_state_dict(model, sd: Dict[str, torch.Tensor]):
    """Copy adapters into a model that apply_lora has shaped the same way; names and shapes must match exactly."""
    own = {k: v for k, v in model.state_dict().items() if ".lora_A" in k or ".lora_B" in k}
    if set(own) != set(sd):
        raise KeyError(f"load_lora_state_dict: adapter names differ (missing {sorted(set(own) - set(sd))}, unexpected {sorted(set(sd) - set(own))})")
    params = dict(model.named_parameters())
    with torch.no_grad():
        for k, v in sd.items():
            if tuple(v.shape) != tuple(params[k].shape):
                raise ValueError(f"load_lora_state_dict: {k} is {tuple(v.shape)}, the model holds {tuple(params[k].shape)}")
            params[k].copy_(v)        # (an in-place write: an arena re-casts the parameter's shadow at its next use)


def merged_state_dict(model) -> Dict[str, torch.Tensor]:
    """model.state_dict() as merge_lora would leave it -- every adapted W replaced by W + s.B.A (fp32), no adapter keys -- without
    touching the model: what a checkpoint under the reference's keys holds while training goes on."""
    sd = {k: v for k, v in model.state_dict().items() if ".lora_A" not in k and ".lora_B" not in k}
    names = {id(m): n for n, m in model.named_modules()}
    for att, na, nb, lin in _adapters(model):
        key = f"{names[id(att)]}.{lin}.weight"
        A, B = getattr(att, na).detach().float(), getattr(att, nb).detach().float()
        sd[key] = sd[key].detach().float() + att.lora_scale * (B @ A)
    return sd


def merge_lora(model):
    """W <- W + s.B.A in fp32 for every adapted projection, then remove the adapters: state_dict() has the reference's keys again and the
    model runs the ordinary paths.  The base weights stay frozen or trainable as they were.  The fold is an in-place write, so the
    16-bit shadows (an arena's, or the cache of parameters outside one) are re-cast at their next use."""
    with torch.no_grad():
        for att, na, nb, lin in list(_adapters(model)):
            A, B = getattr(att, na), getattr(att, nb)
            w = getattr(att, lin).weight
            w.add_(att.lora_scale * (B.detach().float() @ A.detach().float()).to(w.device))
            delattr(att, na)
            delattr(att, nb)
    for _, _, att in attention_sites(model):
        if hasattr(att, "lora_targets"):
            del att.lora_targets, att.lora_scale
    if hasattr(model, "lora_config"):
        del model.lora_config
    return model
