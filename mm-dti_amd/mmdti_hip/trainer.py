"""The fine-tune step of the reference's ``Trainer.fit_predict`` (tasks/trainer.py:177-283) as an MI355X-native engine.

Same loss composition (``alpha*task + beta*infonce + beta*ct``, :192-193), same optimizer maths (Adam, eps 1e-6, :160),
same linear warm-up schedule (HF ``get_linear_schedule_with_warmup``, :161-162), same gradient clipping (max_norm 5.0,
AMP branch :274), same per-epoch FDS statistics pass (:288-306).  What changes is where the work runs:

  * bf16 MFMA compute with fp32 master weights instead of fp16 autocast + GradScaler (no loss scaling needed);
  * parameters, gradients, Adam moments and the bf16 weight shadow are flat arenas: zero-grad, gradient all-reduce,
    clip + Adam + shadow refresh are each ONE pass over contiguous HBM;
  * no host synchronisation inside the step: the four logged scalars stay on the device (``StepOutput``) and are
    fetched by the caller when it wants them (the reference does four ``float(t.data)`` syncs per step, :195-197,238);
  * optional data parallelism (``parallel.py``): global InfoNCE negatives + bucketed gradient all-reduce over RCCL;
  * ``skip_nonfinite``: the other half of the reference's GradScaler (:268-282) -- an optimizer step whose gradients hold an inf or
    NaN is skipped (parameters and Adam state untouched, the schedule advances), decided on the device;
  * ``ema_decay``: an exponential moving average of the parameters, one launch after the Adam pass; ``averaged()`` puts it into the
    model for validation and checkpoints (not in the reference, off by default).
"""
from __future__ import annotations

import contextlib
import logging
import math
import os
from dataclasses import dataclass
from typing import Optional

import torch

from .functional import CELossFn, MSELossFn, BCELogitsLossFn
from .parallel import ArenaReducer, GlobalNegatives, gather_features
from .runtime import ParamArena, add_grad_ready_hook, remove_grad_ready_hook, dropout_state, new_nonfinite_guard

logger = logging.getLogger(__name__)


@dataclass
class StepOutput:
    loss: torch.Tensor                      # this rank's step loss (alpha*task + beta*infonce_global + beta*ct)
    task_loss: torch.Tensor
    infonce_loss: Optional[torch.Tensor]    # the GLOBAL InfoNCE value (under DDP: sum of the ranks' shares)
    ct_loss: Optional[torch.Tensor]         # rank-local; with global_ct under DDP the GLOBAL value (sum of the ranks' shares)
    logits: torch.Tensor
    skipped: Optional[torch.Tensor] = None     # skip_nonfinite: 1.0 if this step's optimizer update was skipped (non-finite gradient)
    grad_norm: Optional[torch.Tensor] = None   # pre-clip global gradient norm (what clip_grad_norm_ returns), when the step computed it


def linear_warmup_lr(base_lr: float, step: int, warmup: int, total: int) -> float:
    """transformers.get_linear_schedule_with_warmup: lambda of the step count AFTER `step` scheduler.step() calls."""
    if step < warmup:
        return base_lr * float(step) / float(max(1, warmup))
    return base_lr * max(0.0, float(total - step) / float(max(1, total - warmup)))


def _qkv_groups(model):
    """query/key/value Linears of every BERT-style attention block: their weights (and biases) go back to back in the
    arena so that the layer can run them as ONE [3D, D] GEMM (functional._bert_layer_fwd)."""
    groups = []
    for m in model.modules():
        q, k, v = (getattr(m, n, None) for n in ("query", "key", "value"))
        if all(isinstance(t, torch.nn.Module) and hasattr(t, "weight") for t in (q, k, v)) and q.weight.shape == k.weight.shape == v.weight.shape:
            groups.append((q.weight, k.weight, v.weight))
            if all(getattr(t, "bias", None) is not None for t in (q, k, v)):
                groups.append((q.bias, k.bias, v.bias))
    return groups


FDS_STATS_MODES = ("epoch_pass", "streaming")


def check_ema_decay(ema_decay, who="FineTuner"):
    """None (weight averaging off) or a finite decay with 0 < decay < 1 as a float; anything else is a ValueError.  Needs no device."""
    if ema_decay is None:
        return None
    try:
        d = float(ema_decay)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: ema_decay must be None or a number in (0, 1), got {ema_decay!r}") from None
    if not (math.isfinite(d) and 0.0 < d < 1.0):
        raise ValueError(f"{who}: ema_decay must be finite with 0 < ema_decay < 1, got {ema_decay!r}")
    return d


def ema_decay_at(t, decay, warmup=True):
    """The decay the averaging kernel applies at applied optimizer step t (1, 2, ...), in its own fp32 arithmetic:
    min(decay, (1 + t) / (10 + t)) with warmup, else decay.  -> numpy.float32; the kernel's weight is float32(1) - it."""
    import numpy as np
    f = np.float32
    d = f(decay)
    if warmup:
        tt = f(t)
        d = min(d, (f(1) + tt) / (f(10) + tt))
    return f(d)


class FineTuner:
    def __init__(self, model, task: str, learning_rate=1e-4, adam_eps=1e-6, warmup_ratio=0.03, total_steps=1000, alpha=1.0, beta=0.1,
                 max_norm: Optional[float] = 5.0, distributed: bool = False, bucket_bytes: int = 32 << 20, skip_nonfinite: bool = False,
                 loss_key: Optional[str] = None, deterministic: Optional[bool] = None, fds_stats: str = "epoch_pass",
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False, param_groups=None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, global_ct: Optional[bool] = None,
                 memory_bank: Optional[int] = None):
        """deterministic: True enters the process-wide deterministic mode (ops.set_deterministic: every cross-workgroup sum into a
        parameter gradient in a fixed order, one reduction workspace per launch stream); None follows MMDTI_DETERMINISTIC; False (and
        an unset environment) touches nothing.  Sites that have no fixed-order form yet raise in the mode (DESIGN.md lists them), and so
        does graphed_step: the mode covers step().
        skip_nonfinite: GradScaler.step's guard (tasks/trainer.py:268-282) -- a step whose gradient arena holds any inf / NaN element
        leaves the parameters, both Adam moments, Adam's step count and the 16-bit shadows as they were, while the learning-rate
        schedule advances.  The decision is taken on the device (no host synchronisation, captured inside graphed_step) from the
        all-reduced gradients under data parallelism, so every rank takes the same one.
        loss_key: the multilabel_classification loss table's key (models/nnmodel.py:28-32): None / 'bce' the BCE-with-logits kernel,
        'focal' / 'ghm' the kernels of ``losses.FocalLossWithLogits()`` / ``losses.GHMCLoss(10, 0.5)`` (kept as ``self.task_loss``).
        fds_stats: where the FDS epoch statistics come from.  "epoch_pass" (default): the reference's second forward over the training
        set, fds_epoch_pass (tasks/trainer.py:288-306).  "streaming": the training steps' own features feed per-bucket running moments on
        the device -- fds_epoch_begin(epoch) before an epoch's steps, fds_epoch_finish(epoch) after them, and fds_epoch_pass raises.  Each
        batch is then seen with the weights of its own step, not with the end-of-epoch weights (DESIGN.md "Streaming FDS statistics").
        The features are accumulated in the forward: a step that skip_nonfinite skips has still contributed its rows.
        weight_decay: Adam's weight decay (default 0, the reference's), added to the gradient as torch.optim.Adam does -- or, with
        decoupled_weight_decay=True, applied as p *= 1 - lr * wd (torch.optim.AdamW).  param_groups: a list of
        param_groups.ParamGroup (first match wins; unmatched parameters keep scale 1 and `weight_decay`), e.g.
        ``no_decay(model) + layerwise_decay(model, 0.8)``: each group's learning-rate scale and weight decay live in a small device table
        that the fused clip + Adam + shadow pass reads per block of 8 elements (DESIGN.md "Parameter groups"); set_group changes a row
        without a synchronisation or a re-capture.  Without groups and with coupled decay the pass is the ungrouped one.
        ema_decay: None (default: no buffer, no launch) or 0 < decay < 1 -- an exponential moving average of the arena's parameters,
        ``arena.ema``, updated by one launch right after every applied Adam pass (eager and captured; a step the guard skips leaves it
        alone): ema += (1 - d)(p - ema), d = decay or, with ema_warmup (default), min(decay, (1 + t) / (10 + t)) for the t-th applied
        step (ema_decay_at).  ``with engine.averaged():`` puts the average into the model -- parameters, state dict and both 16-bit
        shadows -- for validation and checkpoints, and takes it out again to the bit (DESIGN.md "Weight averaging (EMA)").
        global_ct: global ConR / SupCon negatives under data parallelism -- every rank's anchors meet the molecules of ALL ranks, so N
        ranks on a global batch optimise the single-process CT loss of that batch (DESIGN.md "Global ConR / SupCon negatives").  None
        follows MMDTI_GLOBAL_CT (unset / 0 = off).  Effective only with distributed=True and active collectives; otherwise, and when
        off, the CT term is the rank-local one and nothing about the step changes.
        memory_bank: Q > 0 gives the model's InfoNCE head a cross-batch memory of Q slots per side (InfoNCE.set_memory_bank): the last Q
        L2-normalised embeddings of each side stay on the device as extra negatives without a gradient, every training step reads them and
        then pushes its own (global) rows; ``StepOutput.infonce_loss`` is the banked value.  0 removes a bank the model has; None (default)
        leaves the model as it is.  Without a bank no launch, argument or allocation changes (DESIGN.md "Memory bank of InfoNCE negatives").
        net_input may carry ``sample_ids`` ([B] int64): a slot that holds the anchor's own molecule is skipped."""
        self.ema_decay, self.ema_warmup = check_ema_decay(ema_decay), bool(ema_warmup)
        self._averaged = False
        self._time_negatives = None                      # accumulate.TimeNegatives while an accumulated union step runs
        if fds_stats not in FDS_STATS_MODES:
            raise ValueError(f"FineTuner: fds_stats must be one of {FDS_STATS_MODES}, got {fds_stats!r}")
        self.fds_stats = fds_stats
        self.model, self.task = model, task
        if memory_bank is not None:
            from .models.infonce import check_memory_bank
            Q = check_memory_bank(memory_bank, "FineTuner")
            head = getattr(model, "infonce", None)
            if head is None or not hasattr(head, "set_memory_bank"):
                if Q:
                    raise ValueError("FineTuner: memory_bank needs a model with an InfoNCE head (model.infonce)")
            elif head.memory_bank != Q:
                head.set_memory_bank(Q)
        from . import ops
        self.deterministic = ops.deterministic_default() if deterministic is None else bool(deterministic)
        if self.deterministic:
            ops.set_deterministic(True)
        self.lr, self.eps, self.alpha, self.beta, self.max_norm = learning_rate, adam_eps, alpha, beta, max_norm
        self.total_steps = total_steps
        self.warmup = int(total_steps * warmup_ratio)
        self.sched_step = 0
        # the trainable set is what requires_grad says NOW (the reference's Adam(filter(lambda p: p.requires_grad, ...)), :160): frozen
        # parameters (freeze_layers) stay out of the arena and never change
        self.arena = ParamArena(model.parameters(), adjacent=_qkv_groups(model))
        self._outside = [p for p in model.parameters() if id(p) not in self.arena.offsets]
        self._warned_unfrozen = False
        self.weight_decay = float(weight_decay)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self.param_groups = None                         # the resolved ParamGroup list ([]: the default group alone), None: ungrouped pass
        if param_groups is not None or self.decoupled_weight_decay:
            self._set_param_groups(list(param_groups or ()))
        elif not (math.isfinite(self.weight_decay) and self.weight_decay >= 0.0):
            raise ValueError(f"FineTuner: weight_decay must be finite and >= 0, got {weight_decay!r}")
        self.skip_nonfinite = bool(skip_nonfinite)
        self.last_optimizer_outputs = (None, None)       # (skipped, grad_norm) of the latest optimizer_step
        self.guard = new_nonfinite_guard(self.arena.data.device) if self.skip_nonfinite else None
        self._graphs, self._state, self._salt, self._salted = {}, None, None, False
        self.world = 1
        self.reducer = None
        self._dropout_rank = None                        # the rank whose offset the dropout base carries (None: no offset, checkpoint.py)
        self.global_ct = False                           # (global ConR / SupCon negatives: only under distributed=True, see below)
        remove_grad_ready_hook(self)
        if distributed:
            self.negs = GlobalNegatives()
            self.world = self.negs.world
            if self.negs.active:
                from .parallel import host_group
                host_group()            # (the gloo side group of the host-side exchanges: created where every rank is -- ADVICE r03)
                # replicas must start identical: the cross-modal block, InfoNCE head and classification head are random-
                # initialised, so rank 0's arena is broadcast (no reliance on every rank seeding alike) ...
                torch.distributed.broadcast(self.arena.data, src=0)
                self.arena.refresh_shadow()
                # ... while dropout masks must DIFFER across ranks (each rank holds different molecules)
                from .checkpoint import dropout_base_for_rank
                self._dropout_rank = self.negs.rank
                dropout_state.reseed(dropout_base_for_rank(dropout_state.base, None, self._dropout_rank))
            self.reducer = ArenaReducer(self.arena, bucket_bytes)
            self._b_loc = None
            want = os.environ.get("MMDTI_GLOBAL_CT", "0") not in ("", "0") if global_ct is None else bool(global_ct)
            self.global_ct = bool(want and self.negs.active)
            # gradient buckets leave during backward (MMDTI_NO_REDUCE_OVERLAP=1: all of them after it)
            if os.environ.get("MMDTI_NO_REDUCE_OVERLAP") != "1":
                add_grad_ready_hook(self, self.reducer.on_grads_ready)
        if self.ema_decay is not None:
            # (after the broadcast: the average starts as a copy of the parameters every replica starts from; the update is elementwise on
            #  bit-identical replicas, so it needs no collective)
            self.arena.enable_ema()
        # built-in task-loss kernels (models/nnmodel.py:24-34): MSE, cross-entropy, and the multilabel table's three entries -- BCE-with-
        # logits ('bce', and the default here), focal and GHM by `loss_key`; every other task / loss (MAE-with-NaN ...) runs as the
        # callable the caller passes as `loss_func`
        if loss_key is not None and task != "multilabel_classification":
            raise ValueError(f"FineTuner: loss_key={loss_key!r} belongs to the multilabel_classification loss table, the task is {task!r}")
        if task == "regression":
            self.task_loss = lambda lg, y: MSELossFn.apply(lg, y.float())
        elif task in ("classification", "multiclass"):
            self.task_loss = lambda lg, y: CELossFn.apply(lg, y)
        elif task == "multilabel_classification" and loss_key in (None, "bce"):
            self.task_loss = lambda lg, y: BCELogitsLossFn.apply(lg, y)
        elif task == "multilabel_classification":
            from .losses import from_key
            self.task_loss = from_key(loss_key)
        else:
            self.task_loss = None

    # ------------------------------------------------------------------ parameter groups
    def _set_param_groups(self, groups):
        """Resolve the groups against the model, spread the indices over the arena's blocks of 8 and hand ids and table to the arena."""
        from .freeze import arena_group_ids
        from .param_groups import group_names, resolve
        index, table = resolve(self.model, groups, self.weight_decay)
        of = {id(p): g for (_, p), g in zip(self.model.named_parameters(), index)}
        a = self.arena
        per_param = [of[id(p)] for p in a.params]
        ids = arena_group_ids(per_param, [a.offsets[id(p)] for p in a.params], [p.numel() for p in a.params], a.numel)
        a.set_groups(ids, torch.tensor(table, dtype=torch.float32), self.decoupled_weight_decay)
        self.param_groups, self._group_names, self._group_table, self._group_of = groups, group_names(groups), table, per_param

    def set_group(self, index_or_name, lr_scale: Optional[float] = None, weight_decay: Optional[float] = None):
        """Change a group's learning-rate scale and / or weight decay: one small copy into the device table, enqueued on the current
        stream -- no synchronisation.  The next step honours it, and so does the next replay of every graph already captured (the
        table's address does not move; nothing is re-captured).  lr_scale = 0 freezes the group's parameters and shadows to the bit
        while its moments keep following the gradients; raising it again is gradual unfreezing.  index_or_name: the table row (0: the
        default group, j + 1: param_groups[j]) or the group's name (param_group_summary lists them)."""
        if self.param_groups is None:
            raise RuntimeError("FineTuner.set_group: this engine was built without parameter groups (pass param_groups=[...])")
        if isinstance(index_or_name, str):
            if index_or_name not in self._group_names:
                raise KeyError(f"FineTuner.set_group: no group named {index_or_name!r} (groups: {self._group_names})")
            i = self._group_names.index(index_or_name)
        else:
            i = int(index_or_name)
            if not 0 <= i < len(self._group_table):
                raise IndexError(f"FineTuner.set_group: group {i} out of range (0 .. {len(self._group_table) - 1})")
        row = list(self._group_table[i])
        for k, x, what in ((0, lr_scale, "lr_scale"), (1, weight_decay, "weight_decay")):
            if x is not None:
                if not (math.isfinite(float(x)) and float(x) >= 0.0):
                    raise ValueError(f"FineTuner.set_group: {what} must be finite and >= 0, got {x!r}")
                row[k] = float(x)
        self._group_table[i] = row
        from . import ops
        self.arena.group_table[i].copy_(ops.upload(torch.tensor(row, dtype=torch.float32), self.arena.data.device), non_blocking=True)

    def param_group_summary(self):
        """-> [(name, parameters, elements, lr_scale, weight_decay)], one row per group, over the parameters the optimizer holds."""
        params = self.arena.params
        if self.param_groups is None:
            return [("default", len(params), sum(p.numel() for p in params), 1.0, self.weight_decay)]
        rows = []
        for g, (name, (s, wd)) in enumerate(zip(self._group_names, self._group_table)):
            mine = [p for p, gid in zip(params, self._group_of) if gid == g]
            rows.append((name, len(mine), sum(p.numel() for p in mine), s, wd))
        return rows

    # ------------------------------------------------------------------ weight averaging
    @contextlib.contextmanager
    def averaged(self):
        """Inside the block the model holds the averaged weights: the arena's parameters, hence ``state_dict()``, and both 16-bit shadows
        the GEMMs read (one swap launch on entry, one on exit; afterwards parameters and shadows are what they were, bit for bit).
        Validate and checkpoint inside it.  Only the arena's parameters are averaged: parameters frozen when the engine was built and
        buffers (the FDS statistics) are the model's own.  step, graphed_step, optimizer_step and a nested averaged() raise inside."""
        if self.ema_decay is None:
            raise RuntimeError("FineTuner.averaged: this engine was built without weight averaging (pass ema_decay=...)")
        self._not_averaged("averaged")
        self.arena.swap_average()
        self._averaged = True
        try:
            yield self
        finally:
            self._averaged = False
            self.arena.swap_average()

    def _not_averaged(self, what):
        if self._averaged:
            raise RuntimeError(f"FineTuner.{what}: not inside averaged() -- the model holds the averaged weights, the raw ones sit in the "
                               "average's buffer until the block ends")

    # ------------------------------------------------------------------ resuming a run (DESIGN.md "Resuming a run")
    def _bank_state(self):
        """[(name, tensor)] of the InfoNCE memory bank's rings; [] without one"""
        head = getattr(self.model, "infonce", None)
        return head.memory_bank_state() if hasattr(head, "memory_bank_state") else []

    @property
    def memory_bank(self) -> int:
        """slots per side of the model's InfoNCE memory bank (0: none)"""
        return int(getattr(getattr(self.model, "infonce", None), "memory_bank", 0))

    def _arena_names(self):
        """the arena's parameters by their names in the model, in arena order"""
        of = {id(p): n for n, p in self.model.named_parameters()}
        return [of[id(p)] for p in self.arena.params]

    def state_dict(self):
        """Everything that defines where this engine stands between two optimizer steps (not in the middle of step_accumulated), as
        tensors on the host, numbers, strings, None, lists, tuples and dicts: ``torch.save`` it, ``checkpoint.load`` reads it back with
        weights_only=True.  The model's raw weights and buffers, the optimizer's moments and the parameter average by parameter name,
        the trainable flags, the schedule, the guard's and the graph's device counters, the group table, the dropout stream, the task
        loss's own state (GHM's bin history) and the streaming FDS accumulator.  Every copy is enqueued into pinned memory and the
        stream is synchronised once (a loss with state of its own reads its few words after that).  Raises inside averaged(): the
        model would hand out the averaged weights as the raw ones."""
        self._not_averaged("state_dict")
        from .checkpoint import STATE_VERSION
        from .runtime import host_copy
        names = self._arena_names()
        model_sd = {k: host_copy(v) for k, v in self.model.state_dict().items()}
        fds = getattr(self.model, "FDS", None)
        fds_acc = getattr(fds, "_stream_acc", None) if self.fds_stats == "streaming" else None
        sd = {
            "version": STATE_VERSION,
            "model": model_sd,
            "layout": [(n, p.numel()) for n, p in zip(names, self.arena.params)],
            "optimizer": self.arena.state_dict(names, sync=False),
            "trainable": {n: bool(p.requires_grad) for n, p in zip(names, self.arena.params)},
            "schedule": {"sched_step": int(self.sched_step), "total_steps": int(self.total_steps), "warmup": int(self.warmup), "lr": float(self.lr)},
            "guard": None if self.guard is None else host_copy(self.guard),
            "graph": None if self._state is None else {"state": host_copy(self._state), "salt": host_copy(self._salt), "salted": bool(self._salted)},
            "groups": None if self.param_groups is None else {"names": list(self._group_names), "table": [[float(x) for x in row] for row in self._group_table]},
            "ema": None if self.ema_decay is None else {"decay": float(self.ema_decay), "warmup": bool(self.ema_warmup)},
            "dropout": dict(dropout_state.state(), rank=self._dropout_rank),
            "task_loss": None,
            "fds_stream": None if fds_acc is None else {"acc": host_copy(fds_acc), "active": bool(getattr(self.model, "fds_streaming", False))},
            "deterministic": bool(self.deterministic),
        }
        bank = self._bank_state()
        if bank:                  # (a state written without a bank has no such key: those files stay as they were)
            sd["memory_bank"] = dict({"slots": self.memory_bank}, **{n: host_copy(t) for n, t in bank})
        torch.cuda.current_stream().synchronize()
        if hasattr(self.task_loss, "state_dict"):
            sd["task_loss"] = self.task_loss.state_dict()
        return sd

    def _check_state_dict(self, sd):
        """Everything load_state_dict refuses, before it writes anything.  -> the arena's names"""
        from .checkpoint import check_layout, check_version
        check_version(sd)
        names = self._arena_names()
        check_layout(sd["layout"], [(n, p.numel()) for n, p in zip(names, self.arena.params)])
        for what, saved, own in (("weight averaging (ema)", sd["ema"], self.ema_decay), ("parameter groups", sd["groups"], self.param_groups),
                                 ("the non-finite guard (skip_nonfinite)", sd["guard"], self.guard)):
            if (saved is None) != (own is None):
                raise ValueError(f"FineTuner.load_state_dict: the state was written {'without' if saved is None else 'with'} {what}, this "
                                 f"engine was built {'without' if own is None else 'with'} it")
        saved_bank = sd.get("memory_bank")
        if (saved_bank is None) != (self.memory_bank == 0):
            raise ValueError(f"FineTuner.load_state_dict: the state was written {'without' if saved_bank is None else 'with'} an InfoNCE memory "
                             f"bank, this engine was built {'without' if self.memory_bank == 0 else 'with'} one")
        if saved_bank is not None:
            own = dict(self._bank_state())
            if int(saved_bank["slots"]) != self.memory_bank or any(n not in saved_bank or tuple(saved_bank[n].shape) != tuple(t.shape)
                                                                   for n, t in own.items()):
                raise ValueError(f"FineTuner.load_state_dict: the state's InfoNCE memory bank has {int(saved_bank['slots'])} slots per side, "
                                 f"this engine's {self.memory_bank}")
        if sd["groups"] is not None and list(sd["groups"]["names"]) != list(self._group_names):
            raise ValueError(f"FineTuner.load_state_dict: the state's parameter groups are {list(sd['groups']['names'])}, this engine's "
                             f"{list(self._group_names)}")
        own = self.model.state_dict()
        odd = sorted(set(own) ^ set(sd["model"]))
        odd += [k for k, v in own.items() if k in sd["model"] and tuple(sd["model"][k].shape) != tuple(v.shape)]
        if odd:
            raise ValueError(f"FineTuner.load_state_dict: the model's state differs from the file's (missing, unexpected or of another shape): {odd[:5]}")
        self.arena.check_state_dict(sd["optimizer"], names)
        if set(sd["trainable"]) != set(names):
            raise ValueError("FineTuner.load_state_dict: the trainable flags do not name the optimizer's parameters")
        loss_sd = sd.get("task_loss")
        if loss_sd is not None and hasattr(self.task_loss, "bins") and int(loss_sd.get("bins", self.task_loss.bins)) != self.task_loss.bins:
            raise ValueError(f"FineTuner.load_state_dict: the task loss has {loss_sd['bins']} bins in the state, {self.task_loss.bins} here")
        fs = sd.get("fds_stream")
        if fs is not None:
            fds = getattr(self.model, "FDS", None)
            if self.fds_stats != "streaming" or fds is None or tuple(fs["acc"].shape) != tuple(fds.stream_state().shape):
                raise ValueError("FineTuner.load_state_dict: the state holds a streaming FDS accumulator this engine has no place for "
                                 "(fds_stats='streaming' and the same bucket range and feature width)")
        return names

    def load_state_dict(self, sd):
        """Put a state_dict() back: copies into the buffers this engine already has, so no address moves and graphs captured before
        stay valid (they are dropped only if the trainable set changed, as ever).  Raises ValueError, before anything is written, when
        the version, the optimizer's parameters (names, sizes, order), the presence of weight averaging, of parameter groups (or their
        names) or of the guard differ.  total_steps, warmup and lr stay the constructor's (one warning if the file's differ); the
        schedule continues at the saved step.  The process-wide dropout stream continues where the state left it, from this rank's
        base.  Under distributed=True every rank loads the same file: the replicas are bit-identical by construction.  Raises inside
        averaged()."""
        self._not_averaged("load_state_dict")
        from . import ops
        from .checkpoint import dropout_base_for_rank
        names = self._check_state_dict(sd)
        sch = sd["schedule"]
        differ = [f"{k}: {sch[k]!r} in the file, {own!r} here" for k, own in (("total_steps", self.total_steps), ("warmup", self.warmup), ("lr", self.lr))
                  if sch[k] != own]
        if differ:
            logger.warning("FineTuner.load_state_dict: the schedule differs (%s); this engine's values are kept, the step count is restored", "; ".join(differ))
        dev = self.arena.data.device
        put = lambda dst, src: dst.copy_(ops.upload(src.to(dst.dtype), dev), non_blocking=True)
        self.model.load_state_dict(sd["model"])             # (in-place copies: the arena-bound parameters keep their storage)
        self.arena.load_state_dict(sd["optimizer"], names)
        for n, p in zip(names, self.arena.params):
            p.requires_grad_(bool(sd["trainable"][n]))
        self._sync_trainable()
        self.sched_step = int(sch["sched_step"])
        if self.guard is not None:
            put(self.guard, sd["guard"])
        g = sd["graph"]
        if g is not None:
            if self._state is None:
                self._state = torch.zeros(4, device=dev, dtype=torch.float32)
                self._salt = torch.zeros(2, device=dev, dtype=torch.int64)
            put(self._state, g["state"])
            put(self._salt, g["salt"])
            self._salted = bool(g["salted"]) or self._salted    # (the next eager step resets the libraries' salt, as after a replay)
        if self.param_groups is not None:
            self._group_table = [[float(x) for x in row] for row in sd["groups"]["table"]]
            put(self.arena.group_table, torch.tensor(self._group_table, dtype=torch.float32))
        if sd.get("task_loss") is not None and hasattr(self.task_loss, "load_state_dict"):
            self.task_loss.load_state_dict(sd["task_loss"])
        fs = sd.get("fds_stream")
        if fs is not None:
            put(self.model.FDS.stream_state(), fs["acc"])
            self.model.fds_streaming = bool(fs["active"])
        for n, t in self._bank_state():
            put(t, sd["memory_bank"][n])
        d = sd["dropout"]
        dropout_state.load_state(dropout_base_for_rank(d["base"], d["rank"], self._dropout_rank), int(d["calls"]))

    # ------------------------------------------------------------------
    def _sync_trainable(self):
        """Follow requires_grad changes made after construction: a parameter frozen since gets no gradient, no update and no moment
        change from the next step on (masked Adam pass; captured graphs are re-captured); one unfrozen since is not in the optimizer
        -- as in the reference, where it is not in Adam's parameter list -- and is never updated (one warning)."""
        if self.arena.sync_trainable():
            self._graphs.clear()
            if self.reducer is not None:
                self.reducer.set_trainable(self.arena._flags)
        if not self._warned_unfrozen and self._outside and any(p.requires_grad for p in self._outside):
            self._warned_unfrozen = True
            logger.warning("FineTuner: a parameter that was frozen when the engine was built now requires grad; it is not in the "
                           "optimizer and will not be updated (build a new FineTuner to train it)")

    def _bind_global_negatives(self, b_loc: int):
        if self.negs.active and self._b_loc != b_loc:
            self.model.infonce.set_global_negatives(self.negs.gather, self.negs.reduce_scatter, self.negs.row0(b_loc))
            if self.global_ct:
                self.model.set_global_contrast(self.negs.gather, self.negs.reduce_scatter, self.negs.row0(b_loc))
            self._b_loc = b_loc

    def forward_backward(self, net_input: dict, net_target: torch.Tensor, epoch: int = 0, use_weight: bool = False,
                         return_infonce_loss: bool = True, return_ct_loss: bool = True, loss_func=None, *, zero_grad: bool = True,
                         reduce: bool = True, task_scale: Optional[float] = None, contrast_scale: Optional[float] = None) -> StepOutput:
        """optimizer.zero_grad(); model(...); loss; loss.backward()  (+ gradient all-reduce under DDP).  The two flags
        select the reference's four call forms (tasks/trainer.py:184-212); ``loss_func`` replaces the built-in task-loss
        kernel with any callable on (logits, target).
        Keyword-only, for accumulated steps (defaults: today's step): zero_grad=False adds this backward's gradients to what the arena
        holds; reduce=False keeps the gradient all-reduce from launching (the arena then holds this rank's sum; the call with
        reduce=True reduces every bucket once); task_scale / contrast_scale multiply the task term and the two contrastive terms
        (None: no multiplication is enqueued)."""
        model = self.model
        if not torch.cuda.is_current_stream_capturing():
            self._sync_trainable()
        if zero_grad:
            self.arena.zero_grad()
        if self.reducer is not None:
            if self._time_negatives is None:             # (an accumulated union step has bound its own provider)
                self._bind_global_negatives(net_target.shape[0])
            self.reducer.armed = bool(reduce)
            if reduce:
                self.reducer.begin_step()
        out = model(**net_input, **self._model_kwargs(net_target, epoch, use_weight, return_infonce_loss, return_ct_loss))
        out = out if isinstance(out, tuple) else (out,)
        logits = out[0]
        infonce = out[1] if return_infonce_loss else None
        ct = out[-1] if (return_ct_loss and len(out) > (2 if return_infonce_loss else 1)) else None
        lf = loss_func or self.task_loss
        if lf is None:
            raise ValueError(f"FineTuner: task {self.task!r} has no built-in loss kernel -- pass the task loss as `loss_func` "
                             "(any callable on (logits, target), e.g. the reference's LOSS_RREGISTER entry, models/nnmodel.py:24-34)")
        tl = lf(logits, net_target)
        # (accumulated steps: a micro-batch's terms enter the step's loss with their weights; the values returned are the weighted ones)
        if task_scale is not None:
            tl = tl * task_scale
        if contrast_scale is not None:
            infonce = None if infonce is None else infonce * contrast_scale
            ct = None if ct is None else ct * contrast_scale
        loss = self.alpha * tl
        if infonce is not None:
            # under DDP `infonce` is this rank's share of the GLOBAL loss: x world so that the rank-mean of gradients is exact
            loss = loss + self.beta * (infonce * self.world if self.world > 1 else infonce)
        if ct is not None:
            # (global_ct: `ct` is this rank's share of the union batch's loss, scaled like InfoNCE's; else a rank-local mean)
            loss = loss + self.beta * (ct * self.world if self.global_ct and self.world > 1 else ct)
        loss.backward()
        infonce_global = None if infonce is None else infonce.detach()
        ct_out = None if ct is None else ct.detach()
        if self.reducer is not None:
            if self.global_ct and ct is not None and self.world > 1:
                # the logged values are the GLOBAL ones: the ranks' shares of both terms summed in one message (8 bytes)
                shares = torch.stack([ct_out.reshape(())] + ([] if infonce is None else [infonce_global.reshape(())]))
                torch.distributed.all_reduce(shares, op=torch.distributed.ReduceOp.SUM)
                ct_out = shares[0]
                if infonce is not None:
                    infonce_global = shares[1]
            elif infonce is not None and self.negs.active and self.world > 1:
                infonce_global = infonce_global.clone()
                torch.distributed.all_reduce(infonce_global, op=torch.distributed.ReduceOp.SUM)      # 4 bytes, for logging
            if reduce:
                self.reducer.finish()
            self.reducer.armed = True
        return StepOutput(loss.detach(), tl.detach(), infonce_global, ct_out, logits.detach())

    def _model_kwargs(self, net_target, epoch, use_weight, return_infonce_loss, return_ct_loss):
        """the model call's keywords for the reference's four call forms (tasks/trainer.py:184-212)"""
        kw = dict(epoch=epoch)
        if return_infonce_loss:
            kw["return_infonce_loss"] = True
        if return_ct_loss:
            kw.update(return_ct_loss=True, use_weight=use_weight)
        if return_ct_loss or return_infonce_loss or getattr(self.model, "fds_streaming", False):
            kw["net_target"] = net_target
        return kw

    # ------------------------------------------------------------------ accumulated steps (DESIGN.md "Accumulated steps")
    def forward_backward_accumulated(self, micro_batches, epoch: int = 0, use_weight: bool = False, negatives: str = "union",
                                     return_infonce_loss: bool = True, return_ct_loss: bool = True, loss_func=None) -> StepOutput:
        """forward_backward over k micro-batches ``[(net_input, net_target), ...]``: the arena ends with the gradient of

            alpha * sum_i (b_i / B) task_loss(micro-batch i) + beta * (InfoNCE + ConR / SupCon),        B = sum_i b_i

        zeroed once before the first backward and, under data parallelism, all-reduced once, during and after the last.
        negatives="micro": each micro-batch's contrastive terms see its own rows (its micro-step's global rows under data parallelism),
        weighted b_i / B -- one forward + backward each, any sizes.  negatives="union": the contrastive terms are those of the
        concatenated batch (equal b_i, one rank) -- accumulate.TimeNegatives plays the other micro-batches' part as the other ranks
        play it under data parallelism: a no_grad forward of every micro-batch records the messages of the two loss functions, the
        row-block kernels turn the cached union into each virtual rank's contribution to every row, and the second pass runs forward +
        backward against the union with its own rows live.  Dropout: pass 2 draws pass 1's masks (DropoutState.mark / rewind), the
        counter ends advanced by k forwards.  k = 1 is forward_backward itself, launch for launch.
        -> StepOutput of the whole step: the four scalars summed with their weights, the logits concatenated."""
        from .accumulate import check_accumulation
        self._not_averaged("forward_backward_accumulated")
        micro_batches = list(micro_batches)
        k, B = check_accumulation([t.shape[0] for _, t in micro_batches], negatives, self.world)
        if negatives == "union" and self.memory_bank and return_infonce_loss:
            # (the union's recorded first pass and the bank would disagree on what "past" means)
            raise ValueError("step_accumulated: negatives='union' is not available with an InfoNCE memory bank (use negatives='micro': each "
                             "micro-batch reads the bank, then pushes)")
        fkw = dict(epoch=epoch, use_weight=use_weight, return_infonce_loss=return_infonce_loss, return_ct_loss=return_ct_loss,
                   loss_func=loss_func)
        if k == 1:
            return self.forward_backward(*micro_batches[0], **fkw)
        union = negatives == "union" and (return_infonce_loss or return_ct_loss)
        outs = []
        if not union:
            for i, (net_input, net_target) in enumerate(micro_batches):
                w = net_target.shape[0] / B
                # (negatives="union" without a contrastive term: only the task term is left, weighted like micro's)
                outs.append(self.forward_backward(net_input, net_target, zero_grad=i == 0, reduce=i == k - 1, task_scale=w,
                                                  contrast_scale=w, **fkw))
        else:
            marks, end = self._record_union(micro_batches, epoch, use_weight, return_infonce_loss, return_ct_loss)
            try:
                for i, (net_input, net_target) in enumerate(micro_batches):
                    self._bind_time_negatives(i)
                    dropout_state.rewind(marks[i])
                    outs.append(self.forward_backward(net_input, net_target, zero_grad=i == 0, reduce=i == k - 1,
                                                      task_scale=net_target.shape[0] / B, **fkw))
            finally:
                dropout_state.rewind(end)
                self._release_time_negatives()
        total = lambda name: None if getattr(outs[0], name) is None else torch.stack([getattr(o, name).reshape(()) for o in outs]).sum()
        return StepOutput(total("loss"), total("task_loss"), total("infonce_loss"), total("ct_loss"), torch.cat([o.logits for o in outs], dim=0))

    def _bind_time_negatives(self, i: int):
        """micro-batch i's view of the two channels (both setters read row0 when they are called: bound anew for every micro-batch)"""
        tn = self._time_negatives
        c = tn.infonce.at(i)
        self.model.infonce.set_global_negatives(c.gather, c.reduce_scatter, c.row0)
        c = tn.ct.at(i)
        self.model.set_global_contrast(c.gather, c.reduce_scatter, c.row0)

    def _release_time_negatives(self):
        """The providers the model had before the accumulated step: none, or -- under distributed=True -- GlobalNegatives, which the
        next forward_backward binds again."""
        self._time_negatives = None
        self.model.infonce.set_global_negatives(None, None, 0)
        self.model.set_global_contrast(None, None, 0)
        if self.reducer is not None:
            self._b_loc = None

    def _record_union(self, micro_batches, epoch, use_weight, return_infonce_loss, return_ct_loss):
        """Pass 1 and the work between the passes.  -> (dropout marks before each micro-batch's forward, the mark after the last)."""
        from .accumulate import TimeNegatives, UnionProbe
        from .functional import infonce_rows_grad
        model = self.model
        tn = self._time_negatives = TimeNegatives(len(micro_batches))
        marks, logits = [], []
        streaming, model.fds_streaming = getattr(model, "fds_streaming", False), False      # (pass 2's forwards feed the FDS statistics)
        try:
            with torch.no_grad():
                for i, (net_input, net_target) in enumerate(micro_batches):
                    self._bind_time_negatives(i)
                    marks.append(dropout_state.mark())
                    out = model(**net_input, **self._model_kwargs(net_target, epoch, use_weight, return_infonce_loss, return_ct_loss))
                    logits.append((out[0] if isinstance(out, tuple) else out).detach())
            end = dropout_state.mark()
            tn.seal()
            if tn.infonce.used:
                head = model.infonce
                tn.infonce.prepare(lambda c, j: infonce_rows_grad(c.union["f"], head.d_l, head.temperature, j * c.b, c.b))
            if tn.ct.used:
                def ct_sent(c, j):
                    # models.contrastive itself, with its own mode and constants, on the cached union: the probe's gather returns the
                    # union whatever it is handed, its reduce_scatter keeps rank j's contribution to every row
                    probe = UnionProbe(c, j)
                    net_input, net_target = micro_batches[j]
                    f = c.union["f"][j * c.b:(j + 1) * c.b, :c.union["f"].shape[1] - 3].clone().requires_grad_()
                    wkw = dict(weights=net_input.get("weights")) if use_weight else {}
                    with torch.enable_grad():
                        share = model.CT(f, net_target, logits[j], w=model.ct_w, negatives=probe, **wkw)
                    torch.autograd.grad(share, f)
                    return probe.sent
                tn.ct.prepare(ct_sent)
        except BaseException:
            self._release_time_negatives()
            raise
        finally:
            model.fds_streaming = streaming
        return marks, end

    def step_accumulated(self, micro_batches, epoch: int = 0, use_weight: bool = False, negatives: str = "union", **kw) -> StepOutput:
        """ONE optimizer step over k micro-batches (forward_backward_accumulated, then optimizer_step): the arena is zeroed once, the
        clip norm, the skip_nonfinite decision, Adam, the EMA update and the schedule see the summed gradients once."""
        self._not_averaged("step_accumulated")
        if getattr(self, "_salted", False):
            from . import ops
            ops.seed_salt_reset(sync=False)
            self._salted = False
        out = self.forward_backward_accumulated(micro_batches, epoch, use_weight, negatives, **kw)
        self.last_optimizer_outputs = (None, None)
        self.optimizer_step()
        out.skipped, out.grad_norm = self.last_optimizer_outputs
        return out

    def optimizer_step(self):
        """Clip + Adam with this step's learning rate; the schedule advances (also on a step the guard skips).
        -> (skipped, grad_norm) device scalars, each None when this engine does not compute it (see StepOutput).  They are also kept
        as ``last_optimizer_outputs``, which is where step() reads them: callers may wrap this method and drop its return value."""
        self._not_averaged("optimizer_step")
        lr = linear_warmup_lr(self.lr, self.sched_step, self.warmup, self.total_steps)
        norm, skipped = self.arena.adam_step(lr, eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm, guard=self.guard)
        if self.ema_decay is not None:
            self.arena.ema_step(self.ema_decay, self.ema_warmup, guard=self.guard)
        self.sched_step += 1
        self.last_optimizer_outputs = (skipped, norm)
        return skipped, norm

    @property
    def optimizer_steps(self) -> Optional[torch.Tensor]:
        """skip_nonfinite: optimizer updates actually applied (Adam's step count), a device scalar (fp32); None without the guard."""
        return None if self.guard is None else self.guard[0]

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        """skip_nonfinite: optimizer steps skipped for a non-finite gradient, a device scalar (fp32); None without the guard."""
        return None if self.guard is None else self.guard[1]

    # ------------------------------------------------------------------ the whole step as ONE HIP graph
    def graphed_step(self, net_input: dict, net_target: torch.Tensor, epoch: int = 0, use_weight: bool = False, **kw) -> StepOutput:
        """step() replayed from a captured HIP graph: ~900 kernel launches become one graph launch, which is what the step
        costs at the reference's real batch sizes (16-32: launch-bound, DESIGN.md "small batches").  One graph per input
        shape signature (keep the number of distinct padded shapes small: bucketed batches, lengths rounded up).
        What changes from step to step lives on the device: the optimizer-step counter, the learning rate of the HF schedule,
        Adam's bias corrections and the dropout salt (ops.step_state_advance is the first node of the graph); the inputs
        are copied into the graph's static buffers before each replay.  Returned tensors are the graph's static outputs --
        read them before the next call.  Not available under data parallelism (collectives are left out of graphs here)."""
        self._not_averaged("graphed_step")
        if self.reducer is not None:
            raise RuntimeError("graphed_step: not supported with distributed=True (use step())")
        from . import ops
        if self.deterministic or ops.is_deterministic():
            # (the mode is process-wide; a graph would bake in the addresses of the per-stream reduction workspaces)
            raise RuntimeError("graphed_step: not supported in the deterministic mode (use step())")
        # Host-side batch descriptors (atom_counts, token_counts, ...) select kernels and tile counts on the HOST at capture time;
        # a replay with another batch of the same padded shape would run with the captured batch's lengths.  The graph therefore
        # runs the padded layout: correct for any batch of the shape.
        from .collate import HOST_FIELDS
        self._sync_trainable()          # (before the graph look-up: a change of the trainable set drops the captured graphs)
        net_input = {k: v for k, v in net_input.items() if k not in HOST_FIELDS}
        key = (epoch >= getattr(getattr(self.model, "fds_cfg", None), "start_smooth", 1 << 30), bool(use_weight), tuple(sorted(kw.items())),
               tuple((k, tuple(v.shape), v.dtype) for k, v in sorted(net_input.items())), tuple(net_target.shape), net_target.dtype)
        if getattr(self.model, "fds_streaming", False):      # (the accumulate launch is in the graph from start_update on)
            key += (epoch >= self.model.fds_cfg.start_update,)
        ent = self._graphs.get(key)
        if ent is None:
            ent = self._capture(net_input, net_target, epoch, use_weight, kw)
            self._graphs[key] = ent
        static_in, static_tgt, graph, out = ent
        for k, v in net_input.items():
            static_in[k].copy_(v, non_blocking=True)
        static_tgt.copy_(net_target, non_blocking=True)
        # the device-resident step counter follows the host's: eager steps taken since the last replay (or another graph's replays)
        # have advanced the schedule too -- one 4-byte fill, enqueued
        self._state[0:1].fill_(float(self.sched_step))
        self._salted = True
        graph.replay()
        self.sched_step += 1
        self.arena.step_count += 1
        return out

    def _state_step(self, net_input, net_target, epoch, use_weight, kw):
        """The body that is captured: advance the device state, then forward / backward / clip + Adam reading it."""
        from . import ops
        ops.step_state_advance(self._state, self._salt, self.lr, self.warmup, self.total_steps)
        out = self.forward_backward(net_input, net_target, epoch, use_weight, **kw)
        out.grad_norm, out.skipped = self.arena.adam_step(0.0, eps=self.eps, weight_decay=self.weight_decay, max_norm=self.max_norm,
                                                          step_state=self._state, guard=self.guard)
        if self.ema_decay is not None:
            self.arena.ema_step(self.ema_decay, self.ema_warmup, guard=self.guard, step_state=self._state)
        self.arena.step_count -= 1                  # (the host-side counter is advanced by graphed_step, once per replay)
        return out

    def _capture(self, net_input, net_target, epoch, use_weight, kw):
        dev = net_target.device
        if self._state is None:
            self._state = torch.zeros(4, device=dev, dtype=torch.float32)
            self._salt = torch.zeros(2, device=dev, dtype=torch.int64)
            self._salt[0] = dropout_state.base & 0x7FFFFFFFFFFFFFFF
        # the device counter continues from wherever the eager path (or another graph) left the schedule
        self._state[0] = float(self.sched_step)
        if self.arena.adam_m is None:
            self.arena.adam_m = torch.zeros_like(self.arena.data)
            self.arena.adam_v = torch.zeros_like(self.arena.data)
        static_in = {k: v.clone() for k, v in net_input.items()}
        static_tgt = net_target.clone()
        # warm-up on a side stream (lazy stream / buffer creation must not happen inside the capture), with a throw-away copy of
        # the state this step mutates
        saved = (self.arena.data.clone(), self.arena.adam_m.clone(), self.arena.adam_v.clone(), self._state.clone(), self._salt.clone(),
                 self.arena.step_count, None if self.guard is None else self.guard.clone(),
                 None if self.arena.ema is None else self.arena.ema.clone())
        # a task loss with device state of its own (losses.GHMCLoss: the bin counts every call averages into) is part of that state
        lf = kw.get("loss_func") or self.task_loss
        loss_state = lf.device_state(dev) if hasattr(lf, "device_state") else None
        loss_saved = None if loss_state is None else loss_state.clone()
        # ... and so is the streaming FDS accumulator the forward feeds (allocated here, before the capture; its address stays put)
        fds_acc = self.model.FDS.stream_state() if getattr(self.model, "fds_streaming", False) else None
        fds_saved = None if fds_acc is None else fds_acc.clone()
        # ... and the InfoNCE memory bank the warm-up steps push into
        bank_saved = [(t, t.clone()) for _, t in self._bank_state()]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._state_step(static_in, static_tgt, epoch, use_weight, kw)
        torch.cuda.current_stream().wait_stream(s)
        self.arena.data.copy_(saved[0]); self.arena.adam_m.copy_(saved[1]); self.arena.adam_v.copy_(saved[2])
        self._state.copy_(saved[3]); self._salt.copy_(saved[4])
        self.arena.step_count = saved[5]
        if self.guard is not None:
            self.guard.copy_(saved[6])
        if saved[7] is not None:
            self.arena.ema.copy_(saved[7])
        if loss_state is not None:
            loss_state.copy_(loss_saved)
        if fds_acc is not None:
            fds_acc.copy_(fds_saved)
        for t, was in bank_saved:
            t.copy_(was)
        self.arena.refresh_shadow()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self._state_step(static_in, static_tgt, epoch, use_weight, kw)
        return static_in, static_tgt, graph, out

    def step(self, net_input: dict, net_target: torch.Tensor, epoch: int = 0, use_weight: bool = False, **kw) -> StepOutput:
        self._not_averaged("step")
        if getattr(self, "_salted", False):
            # graph replays left their dropout salt in the kernel libraries: an eager step draws its masks from the by-value
            # (seed, site) pairs alone, as every other engine in the process expects (enqueued, no synchronisation)
            from . import ops
            ops.seed_salt_reset(sync=False)
            self._salted = False
        out = self.forward_backward(net_input, net_target, epoch, use_weight, **kw)
        self.last_optimizer_outputs = (None, None)
        self.optimizer_step()
        out.skipped, out.grad_norm = self.last_optimizer_outputs
        return out

    # ------------------------------------------------------------------ tasks/trainer.py:288-306
    @torch.no_grad()
    def fds_epoch_pass(self, batches, epoch: int):
        """Full pass over the training batches (model left in train mode as in the reference) collecting pooled features,
        then FDS.update_last_epoch_stats / update_running_stats.  Under DDP the features are all-gathered so every rank
        ends with identical buffers."""
        if self.fds_stats == "streaming":
            raise RuntimeError("FineTuner.fds_epoch_pass: this engine collects the FDS statistics from the training steps "
                               "(fds_stats='streaming'): call fds_epoch_begin / fds_epoch_finish round the epoch's steps")
        model = self.model
        feats, labels = [], []
        for net_input, net_target in batches:
            _, f = model(**net_input, epoch=epoch, return_feature=True, net_target=net_target)
            feats.append(f)
            labels.append(net_target)
        f, y = torch.cat(feats), torch.cat(labels)
        if self.world > 1:
            f, y = gather_features(self.negs, f, y)
        model.FDS.update_last_epoch_stats(epoch)
        model.FDS.update_running_stats(f, y, epoch)

    # ------------------------------------------------------------------ fds_stats="streaming"
    def _fds_streaming(self, what):
        if self.fds_stats != "streaming":
            raise RuntimeError(f"FineTuner.{what}: this engine was built with fds_stats={self.fds_stats!r} (use fds_epoch_pass)")
        if getattr(self.model, "FDS", None) is None:
            raise RuntimeError(f"FineTuner.{what}: the model has no FDS module (regression task with fds=True)")
        return self.model.FDS

    def fds_epoch_begin(self, epoch: int):
        """Before the steps of ``epoch``: empty accumulator, and the model's training forwards feed it (from fds_cfg.start_update on)."""
        self._fds_streaming("fds_epoch_begin").stream_reset()
        self.model.fds_streaming = True

    @torch.no_grad()
    def fds_epoch_finish(self, epoch: int):
        """After the steps of ``epoch``, where fds_epoch_pass would run and in its order: update_last_epoch_stats, then the running
        statistics from what the steps accumulated.  Under DDP the ranks' accumulators are all-gathered in one collective and merged
        in rank order on every rank, so every rank ends with bit-identical buffers."""
        fds = self._fds_streaming("fds_epoch_finish")
        self.model.fds_streaming = False
        if self.reducer is not None and self.negs.active:        # (more than one rank, or the 1-rank rehearsal of MMDTI_FORCE_DDP=1)
            from . import ops
            from .parallel import gather_fds_accumulators
            acc = fds.stream_state()
            parts = gather_fds_accumulators(acc, self.negs.group)
            acc.zero_()
            for part in parts:
                ops.fds_stream_merge(acc, part)
        fds.update_last_epoch_stats(epoch)
        fds.stream_finish(epoch)
