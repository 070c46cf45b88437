"""Drop-in for the reference's ``tasks/trainer.py`` -- the caller of the hot path.

``Trainer`` keeps the reference's constructor keywords (/root/reference/tasks/trainer.py:29-70), ``fit_predict`` /
``predict`` signatures (:122, :387), ``decorate_batch`` / ``decorate_torch_batch`` (:72-120), ``set_seed`` (:529-537) and
``NNDataLoader`` (:540-556), so ``models/nnmodel.py`` (``NNModel.run`` / ``evaluate``) drives it unchanged.  Behaviour
reproduced, with the reference's own run frozen in tests/golden/g10_trainer_*.npz as the check:

  * the same ``DataLoader(shuffle=True, drop_last=True)`` over the training set and ``shuffle=False`` loaders for
    validation, so batch membership per step is the reference's for the same torch seed;
  * Adam(lr, eps=1e-6), HF linear warm-up/decay over ``len(loader) * epochs`` steps, warm-up ``int(steps*warmup_ratio)``;
  * ``loss = alpha*task + beta*infonce + beta*ct`` in the four call forms selected by return_infonce_loss/return_ct_loss;
  * gradient clipping at ``max_norm`` only in the AMP branch (``use_amp``), none otherwise (:270-281);
  * in the AMP branch also the GradScaler's skip of an optimizer step whose gradients hold an inf / NaN (:280; the schedule still
    advances, :282) -- ``skip_nonfinite`` (default: ``use_amp``); the epoch's skipped steps go to ``history`` and the epoch log;
  * the per-epoch FDS pass over the re-shuffled training loader in train mode under no_grad (:288-306);
  * validation each epoch, first metric decides; best checkpoint ``{'model_state_dict': ...}`` written to
    ``dump_dir/model_{fold}.pth`` (rank 0 only under data parallelism), early stopping with ``patience``, reload of the
    best checkpoint and the final prediction (:308-328).

What changes is where the work runs: the step goes through ``mmdti_hip.trainer.FineTuner`` (bf16 MFMA kernels with fp32
master weights in one flat arena, fused clip+Adam, no GradScaler -- bf16 needs no loss scaling); the four logged scalars
stay on the device and are fetched once per epoch instead of four ``float()`` synchronisations per step (:195-197,238);
FDS features never visit the host (:302-304 round-trips them through numpy and hard-codes ``.cuda()``).
There is no CPU path: ``use_cuda=False`` raises.
"""
from __future__ import annotations

import contextlib
import os
import time
import logging

import numpy as np
import torch
from torch.utils.data import DataLoader as TorchDataLoader

from ..trainer import FineTuner, FDS_STATS_MODES, check_ema_decay
from ..collate import HostCollate, device_payload, to_device, PAIR_INPUT_MODES

logger = logging.getLogger("mmdti_hip")


# ------------------------------------------------------------------------------------------------ epoch metric
def _auc(y, p):
    """ROC AUC by the rank statistic (ties get mid-ranks), one column."""
    y, p = np.asarray(y).ravel().astype(int), np.asarray(p).ravel().astype(np.float64)
    order = np.argsort(p, kind="mergesort")
    ranks = np.empty(len(p))
    sp = p[order]
    i = 0
    while i < len(sp):
        j = i
        while j + 1 < len(sp) and sp[j + 1] == sp[i]:
            j += 1
        ranks[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    npos, nneg = int(y.sum()), int(len(y) - y.sum())
    if npos == 0 or nneg == 0:
        raise ValueError("AUC needs both classes in the validation set")
    return float((ranks[y == 1].sum() - npos * (npos + 1) / 2.0) / (npos * nneg))


def _log_loss(y, p):
    """binary log loss of P(class 1), probabilities clipped to [eps, 1 - eps] (sklearn.metrics.log_loss).  eps follows the dtype the
    reference hands sklearn -- ``predict.astype(np.float32)`` (utils/metrics.py:168), so float32's eps: on saturated softmax outputs the
    float64 eps gives another number (y = [0,1,1,0,1], p = [1,1,.7,.2,0]: 6.49 vs 14.53 -- ADVICE r03)."""
    y, p = np.asarray(y).ravel().astype(np.float64), np.asarray(p).ravel().astype(np.float32)
    eps = np.finfo(np.float32).eps
    p = np.clip(p.astype(np.float64), eps, 1.0 - eps)
    return float(-np.mean(y * np.log(p) + (1.0 - y) * np.log(1.0 - p)))


def _auprc(y, p):
    """average precision: sum over the distinct score thresholds (descending) of (recall step) x precision"""
    y, p = np.asarray(y).ravel().astype(int), np.asarray(p).ravel().astype(np.float64)
    if y.sum() == 0:
        raise ValueError("average precision needs a positive in the validation set")
    order = np.argsort(-p, kind="mergesort")
    ys, ps = y[order], p[order]
    last = np.r_[np.nonzero(np.diff(ps))[0], len(ps) - 1]          # last index of every group of tied scores
    tp = np.cumsum(ys)[last]
    precision, recall = tp / (last + 1.0), tp / float(y.sum())
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def _confusion(y, p):
    y, q = np.asarray(y).ravel().astype(int), (np.asarray(p).ravel() > 0.5).astype(int)
    return float(((q == 1) & (y == 1)).sum()), float(((q == 1) & (y == 0)).sum()), float(((q == 0) & (y == 1)).sum()), float(((q == 0) & (y == 0)).sum())


def _f1(y, p):
    tp, fp, fn, _ = _confusion(y, p)
    return 0.0 if tp == 0 else float(2 * tp / (2 * tp + fp + fn))


def _mcc(y, p):
    tp, fp, fn, tn = _confusion(y, p)
    den = np.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    return 0.0 if den == 0 else float((tp * tn - fp * fn) / den)


def _pearson(y, p):
    y, p = np.asarray(y).ravel().astype(np.float64), np.asarray(p).ravel().astype(np.float64)
    return float(np.corrcoef(y, p)[0, 1])


def _midranks(v):
    order = np.argsort(v, kind="mergesort")
    r = np.empty(len(v))
    sv, i = v[order], 0
    while i < len(sv):
        j = i
        while j + 1 < len(sv) and sv[j + 1] == sv[i]:
            j += 1
        r[order[i:j + 1]] = 0.5 * (i + j) + 1.0
        i = j + 1
    return r


_METRIC_TABLE = {      # name -> (function(y_true, y_pred), larger_is_better)   (directions as utils/metrics.py:72-112)
    "mse": (lambda y, p: float(np.mean((y - p) ** 2)), False),
    "rmse": (lambda y, p: float(np.sqrt(np.mean((y - p) ** 2))), False),
    "mae": (lambda y, p: float(np.mean(np.abs(y - p))), False),
    "r2": (lambda y, p: float(1.0 - np.sum((y - p) ** 2) / np.sum((y - np.mean(y)) ** 2)), True),
    "pearsonr": (_pearson, True),
    "spearmanr": (lambda y, p: _pearson(_midranks(np.asarray(y).ravel().astype(np.float64)), _midranks(np.asarray(p).ravel().astype(np.float64))), True),
    "auc": (_auc, True),
    "auroc": (_auc, True),
    "auprc": (_auprc, True),
    "log_loss": (_log_loss, False),
    "acc": (lambda y, p: float(np.mean((np.asarray(p) > 0.5).astype(int) == np.asarray(y).astype(int))), True),
    "f1_score": (_f1, True),
    "mcc": (_mcc, True),
}
# the FIRST default metric of every task is the reference's (utils/metrics.py:114-120 DEFAULT_METRICS): it is the one logged and, with
# metrics other than 'loss' / 'none' / '', the one that drives early stopping
_DEFAULT_METRIC = {"regression": "mse", "classification": "log_loss", "multilabel_classification": "log_loss", "multilabel_regression": "mse"}


class EpochMetric:
    """The slice of ``utils.Metrics`` the trainer needs: ``cal_metric`` -> ordered dict whose FIRST entry drives early
    stopping, and that entry's direction.  Inside the reference's tree pass its own ``utils.Metrics`` object through the
    ``metrics_obj`` keyword instead (the full sklearn/scipy table lives there and is outside the hot path)."""

    def __init__(self, task, metrics_str):
        names = [m for m in (metrics_str or "").split(",") if m] if isinstance(metrics_str, str) and metrics_str not in ("none", "loss") else []
        if not names:
            names = [_DEFAULT_METRIC.get(task, "mse")]
        for n in names:
            if n not in _METRIC_TABLE:
                raise ValueError('Unknown metric: {}'.format(n))
        self.names = names
        self.task = task

    def cal_metric(self, label, predict, nan_value=-1.0, threshold=0.5, label_cnt=None):
        """Classification tasks (utils/metrics.py:30-56,156-170, ``cal_nan_metric(..., classification=True)``): every label column is
        scored over its entries with label 0 or 1 and ``!= nan_value`` only -- the unmeasured assays of Tox21 / ToxCast / SIDER / MUV
        (NaN or -1) do not enter; a column without such an entry is left out of the mean, and with no column left the mean of nothing
        is NaN, as the reference's ``np.mean([])``.  Regression metrics take every entry."""
        label, predict = np.asarray(label, dtype=np.float64), np.asarray(predict, dtype=np.float64)
        if self.task not in ("classification", "multilabel_classification"):
            return {n: float(np.mean([_METRIC_TABLE[n][0](label[:, c], predict[:, c]) for c in range(label.shape[1])])) for n in self.names}
        mask = (label == 0.0) | (label == 1.0)          # (false for NaN)
        if nan_value is not None:
            mask &= label != nan_value
        cols = [c for c in range(label.shape[1]) if mask[:, c].any()]
        out = {}
        for n in self.names:
            scores = [_METRIC_TABLE[n][0](label[mask[:, c], c], predict[mask[:, c], c]) for c in cols]
            out[n] = float(np.mean(scores)) if scores else float("nan")
        return out

    def is_increase(self, name):
        return _METRIC_TABLE[name][1]


def _is_increase(metrics, task, name):
    if isinstance(metrics, EpochMetric):
        return metrics.is_increase(name)
    return bool(metrics.METRICS_REGISTER[name][1])          # the reference's utils.Metrics


def normalise_target(task, net_target):
    """The target dtype rule of tasks/trainer.py:113-120 on a device tensor, without a host synchronisation.  For
    multilabel_classification a floating target marks a missing label with NaN: those become -1 BEFORE the integer cast (what a NaN
    converts to is left to the hardware, and 0 would train the missing label as a negative); integer targets pass through untouched."""
    if task == 'repr':
        return None
    if task == 'multilabel_classification':
        if net_target.is_floating_point():
            net_target = torch.where(torch.isnan(net_target), torch.full_like(net_target, -1.0), net_target)
        return net_target.long()
    if task in ('classification', 'multiclass'):
        return net_target.long()
    return net_target.float()


# ------------------------------------------------------------------------------------------------ the trainer
class Trainer(object):
    def __init__(self, save_path=None, **params):
        self.save_path = save_path
        self.task = params.get('task', None)
        if self.task != 'repr':
            self.metrics_str = params['metrics']
            self.metrics = params.get('metrics_obj') or EpochMetric(self.task, self.metrics_str)
        self._init_trainer(**params)

    def _init_trainer(self, **params):
        self.seed = params.get('seed', 42)
        self.set_seed(self.seed)
        self.logger_level = int(params.get('logger_level', 1))
        self.learning_rate = float(params.get('learning_rate', 1e-4))
        self.batch_size = params.get('batch_size', 32)
        self.max_epochs = params.get('epochs', 50)
        self.warmup_ratio = params.get('warmup_ratio', 0.1)
        self.patience = params.get('patience', 10)
        self.max_norm = params.get('max_norm', 1.0)
        self.cuda = params.get('use_cuda', False)
        self.amp = params.get('use_amp', False)
        # the skip-on-inf/NaN half of the reference's GradScaler (use_amp, :268-282): on exactly where the reference has a scaler
        self.skip_nonfinite = bool(params.get('skip_nonfinite', self.amp))
        # bit-identical parameter gradients run to run (FineTuner(deterministic=...)); None: MMDTI_DETERMINISTIC decides
        self.deterministic = params.get('deterministic', None)
        self.device = torch.device("cuda" if torch.cuda.is_available() and self.cuda else "cpu")
        self.scaler = None          # bf16 MFMA compute with fp32 master weights: no loss scaling (the reference: fp16 + GradScaler)
        self.alpha = params.get('alpha', 1)
        self.beta = params.get('beta', 0.1)
        self.fds = params.get('fds', False)
        # where the FDS epoch statistics come from (FineTuner(fds_stats=...)): "epoch_pass", the reference's second forward over the
        # training set (:288-306), or "streaming", the training steps' own features -- the loader is then iterated ONCE per epoch, so
        # the shuffle stream advances half as fast and the batch order of later epochs differs from the reference's
        self.fds_stats = params.get('fds_stats', 'epoch_pass')
        if self.fds_stats not in FDS_STATS_MODES:
            raise ValueError(f"Trainer: fds_stats must be one of {FDS_STATS_MODES}, got {self.fds_stats!r}")
        self.distributed = bool(params.get('distributed', False))
        # parameter groups of the fused Adam pass (not reference parameters; the defaults are the reference's one Adam(lr, eps=1e-6)):
        # weight_decay, coupled or decoupled (AdamW); param_groups, a list of param_groups.ParamGroup; layer_decay, the shorthand for
        # param_groups.layerwise_decay(model, layer_decay), appended behind the given groups
        self.weight_decay = float(params.get('weight_decay', 0.0))
        self.decoupled_weight_decay = bool(params.get('decoupled_weight_decay', False))
        self.param_groups = params.get('param_groups', None)
        self.layer_decay = params.get('layer_decay', None)
        # weight averaging (FineTuner(ema_decay=..., ema_warmup=...); not a reference parameter, off by default): when set, every epoch's
        # validation, the early-stop decision and the checkpoint see the moving average of the parameters, not the last step's weights
        self.ema_decay = check_ema_decay(params.get('ema_decay', None), "Trainer")
        self.ema_warmup = bool(params.get('ema_warmup', True))
        # global ConR / SupCon negatives under data parallelism (FineTuner(global_ct=...); not a reference parameter): None follows
        # MMDTI_GLOBAL_CT (unset = off, the rank-local term)
        gct = params.get('global_ct', None)
        self.global_ct = None if gct is None else bool(gct)
        # accumulated steps (FineTuner.step_accumulated; not reference parameters): accum_steps consecutive loader batches make ONE
        # optimizer step; accum_negatives says what the contrastive terms see -- "union": all of them, "micro": each batch itself.
        # 1 (default): engine.step on every batch, as ever
        self.accum_steps = int(params.get('accum_steps', 1))
        self.accum_negatives = params.get('accum_negatives', 'union')
        from ..accumulate import ACCUM_NEGATIVES, optimizer_steps_per_epoch
        optimizer_steps_per_epoch(0, self.accum_steps)          # (raises on accum_steps < 1)
        if self.accum_negatives not in ACCUM_NEGATIVES:
            raise ValueError(f"Trainer: accum_negatives must be one of {ACCUM_NEGATIVES}, got {self.accum_negatives!r}")
        # cross-batch memory of InfoNCE negatives (FineTuner(memory_bank=Q); not a reference parameter, 0 = off): Q slots per side of past
        # embeddings as extra negatives; every training sample then travels with its dataset index, so that a molecule's own stale
        # embedding is not its negative
        from ..models.infonce import check_memory_bank
        self.memory_bank = check_memory_bank(params.get('memory_bank', 0), "Trainer")
        if self.memory_bank and self.accum_steps > 1 and self.accum_negatives == 'union':
            raise ValueError("Trainer: memory_bank is not available with accum_negatives='union' (use accum_negatives='micro')")
        # LoRA adapters on the attention projections (lora.apply_lora; not reference parameters, lora_rank = 0: off, nothing changes):
        # the selected towers are frozen and train rank-r updates of their q / k / v projections; model_{fold}.pth is written MERGED,
        # under the reference's keys, and train_state_{fold}.pth carries the adapters through the engine's state
        self.lora_rank = int(params.get('lora_rank', 0))
        self.lora_config = None
        if self.lora_rank:
            from ..lora import LoRAConfig, TOWERS
            self.lora_config = LoRAConfig(rank=self.lora_rank, alpha=float(params.get('lora_alpha', 16.0)),
                                          targets=tuple(params.get('lora_targets', ("q", "v"))), towers=tuple(params.get('lora_towers', TOWERS)),
                                          seed=int(self.seed))
        # input pipeline (not reference parameters, defaults keep the reference's in-process loader):
        #   num_workers > 0 -> collate runs in DataLoader worker processes (HostCollate: no model copy in the workers) into
        #   pinned memory; narrow_inputs -> src_edge_type crosses PCIe as int16 and the never-read src_coord stays on the host
        self.num_workers = int(params.get('num_workers', 0))
        self.narrow_inputs = bool(params.get('narrow_inputs', True))
        #   pair_inputs="coords" -> the batches carry src_coord and no [B,N,N] plane: neither padded by the collate nor shipped, the
        #   pair-bias kernels derive every pair from its two atoms (the samples must carry src_coord; "planes": the reference's batches)
        self.pair_inputs = params.get('pair_inputs', 'planes')
        if self.pair_inputs not in PAIR_INPUT_MODES:
            raise ValueError(f"Trainer: pair_inputs must be one of {PAIR_INPUT_MODES}, got {self.pair_inputs!r}")
        self.rank = torch.distributed.get_rank() if (self.distributed and torch.distributed.is_initialized()) else 0
        if self.distributed and torch.distributed.is_initialized():
            from ..parallel import host_group
            host_group()            # (the gloo side group of _checkpoint_barrier / _agree: created here, where every rank is)
        self._loss_cache = {}       # id(loss_func) -> (loss_func, its kernel-backed loss): see _task_loss
        # resuming (not reference parameters, both off by default: nothing is written and no launch changes).  save_train_state: after
        # every epoch rank 0 writes train_state_{fold}.pth into dump_dir -- the engine's whole state, the epoch loop's bookkeeping and the
        # host RNG streams; resume: fit_predict continues from that file when it is there (and keeps writing it)
        self.resume = bool(params.get('resume', False))
        self.save_train_state = bool(params.get('save_train_state', False)) or self.resume

    # -------------------------------------------------------------- batches
    def decorate_batch(self, batch, feature_name=None):
        return self.decorate_torch_batch(batch)

    def decorate_torch_batch(self, batch):
        """Host -> device move of a collated batch and the target dtype rule (tasks/trainer.py:101-120)."""
        net_input, net_target = batch
        if isinstance(net_input, dict):
            if self.narrow_inputs or self.pair_inputs == "coords":
                net_input = device_payload(net_input, self._n_edge_types, self._pad_idx, self.pair_inputs)
            net_input = to_device(net_input, self.device)
            if self.distributed:
                from ..parallel import pad_to_global_lengths
                net_input = pad_to_global_lengths(net_input)        # the unmasked InfoNCE mean needs one padded length on all ranks
        else:
            net_input = {'net_input': net_input.to(self.device)}
        net_target = normalise_target(self.task, net_target.to(self.device, non_blocking=True))
        return net_input, net_target

    _n_edge_types = None
    _pad_idx = 0

    def device_batches(self, dataloader, feature_name=None):
        """(net_input, net_target) on the device for every batch of ``dataloader``, the host-to-device copies of batch i + 1 in flight
        on the copy stream while step i runs (data.DevicePrefetcher) -- the reference moves each batch with synchronous ``.cuda()``
        calls inside the step loop (tasks/trainer.py:181-183).  What decorate_torch_batch does to a batch happens here too, in the
        same order: narrowing, the move, the global padded length under data parallelism, the target dtype rule.  A loader whose
        batches are not the (dict, target) pairs of the model's collate goes through decorate_batch unchanged."""
        import itertools
        it = iter(dataloader)
        try:
            first = next(it)
        except StopIteration:
            return
        batches = itertools.chain([first], it)
        if self.device.type != "cuda" or not isinstance(first[0], dict):
            for batch in batches:
                yield self.decorate_batch(batch, feature_name)
            return
        from ..data import DevicePrefetcher
        for net_input, net_target in DevicePrefetcher(batches, self.device, narrow=self.narrow_inputs, n_edge_types=self._n_edge_types,
                                                      pad_idx=self._pad_idx, pair_inputs=self.pair_inputs):
            if self.distributed:
                from ..parallel import pad_to_global_lengths
                net_input = pad_to_global_lengths(net_input)        # the unmasked InfoNCE mean needs one padded length on all ranks
            yield net_input, normalise_target(self.task, net_target)

    def _collate_for(self, model):
        """The model's own ``batch_collate_fn`` in-process; with worker processes, the same collate as a small picklable
        object (the workers get the pad index and the tokenizer, not the model)."""
        d = getattr(model, 'dictionary', None)
        self._n_edge_types = len(d) * len(d) if d is not None else None
        self._pad_idx = getattr(model, 'padding_idx', 0)
        from ..models.mm_model import MM_Model
        if (self.num_workers > 0 or self.pair_inputs == "coords") and type(model).batch_collate_fn is MM_Model.batch_collate_fn:
            return HostCollate.of(model, narrow=self.narrow_inputs, pair_inputs=self.pair_inputs)    # (coords: the square pads are never built)
        return model.batch_collate_fn

    def _loader_kwargs(self):
        if self.num_workers <= 0:
            return {}
        # (not persistent: a persistent iterator skips the per-epoch base-seed draw, and the shuffle stream would then differ
        # from the in-process loader's -- the epoch order is part of what the G10 fixtures pin)
        # spawned workers, not forked ones: a child forked from a process that has initialised HIP inherits its driver state, and on this
        # stack the parent's GPU work then crawls (measured with bench.py's pipeline workload, 4 forked loader workers: 160-220 ms per step --
        # the host blocked for 0.1-0.35 s at a time in event waits and inside the backward -- against 42 ms with spawned ones and 31 ms of
        # kernels).  Costs a process start-up per loader; the dataset and collate.HostCollate are picklable by construction.
        kw = dict(num_workers=self.num_workers, pin_memory=self.device.type == "cuda")
        if self.device.type == "cuda":
            kw["multiprocessing_context"] = "spawn"
        return kw

    def _require_device(self):
        if self.device.type != "cuda":
            raise RuntimeError("mmdti_hip has no CPU path: construct the Trainer with use_cuda=True on a machine with an MI355X "
                               "(the reference's use_cuda=False plumbing run is the reference's own PyTorch-CPU code)")

    # -------------------------------------------------------------- fit
    def _ddp(self):
        """more than one rank behind this trainer"""
        return self.distributed and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1

    def train_loader(self, model, train_dataset, feature_name=None):
        """-> (loader, sampler | None).  Data parallel: each rank draws a disjoint, equally sized shard of every epoch's permutation
        (``DistributedSampler(drop_last=True)``; batch_size is per rank), so every rank takes the same number of steps -- a rank
        with one batch more would wait forever in that step's collectives.  Device-independent (covered by the 2-rank gloo tests)."""
        collate_fn = self._collate_for(model)
        if getattr(self, "memory_bank", 0):
            # (same length, same sampler draws, the same collate over the same samples: only ``sample_ids`` is added to the batch)
            from ..collate import IndexedCollate, IndexedDataset
            train_dataset, collate_fn = IndexedDataset(train_dataset), IndexedCollate(collate_fn)
        if self._ddp():
            from torch.utils.data.distributed import DistributedSampler
            sampler = DistributedSampler(train_dataset, shuffle=True, seed=self.seed, drop_last=True)
            return TorchDataLoader(dataset=train_dataset, batch_size=self.batch_size, sampler=sampler, collate_fn=collate_fn,
                                   drop_last=True, **self._loader_kwargs()), sampler
        return NNDataLoader(feature_name=feature_name, dataset=train_dataset, batch_size=self.batch_size, shuffle=True,
                            collate_fn=collate_fn, drop_last=True, **self._loader_kwargs()), None

    def total_optimizer_steps(self, batches_per_epoch):
        """What the schedule (and with it the warm-up) counts: optimizer steps -- (len(loader) // accum_steps) * max_epochs."""
        from ..accumulate import optimizer_steps_per_epoch
        return optimizer_steps_per_epoch(batches_per_epoch, self.accum_steps) * self.max_epochs

    def accumulation_groups(self, batches, pool="all"):
        """accum_steps consecutive (net_input, net_target) batches per optimizer step, a trailing incomplete group dropped (in the spirit
        of the loader's drop_last=True).  pool="all": the unmasked InfoNCE mean depends on the padded length, so a group is right-padded
        to its common atom / token lengths (parallel.pad_group_to_common_lengths); pool="real": batches stay as collated."""
        from ..accumulate import groups_of
        from ..parallel import pad_group_to_common_lengths
        for group in groups_of(batches, self.accum_steps):
            inputs = pad_group_to_common_lengths([net_input for net_input, _ in group], pool)
            yield [(net_input, net_target) for net_input, (_, net_target) in zip(inputs, group)]

    def fit_predict(self, model, train_dataset, valid_dataset, loss_func, activation_fn, dump_dir, fold, target_scaler, feature_name=None,
                    return_infonce_loss=False, return_ct_loss=False, use_weight=False):
        self._require_device()
        model = model.to(self.device)
        if self.lora_config is not None:
            from ..lora import apply_lora
            apply_lora(model, self.lora_config)        # (before the engine: its arena then holds the adapters and the heads only)
            logger.info('LoRA: rank {}, alpha {:g}, targets {}, towers {} -- {} adapter elements train beside the heads'.format(
                self.lora_config.rank, self.lora_config.alpha, ','.join(self.lora_config.targets), ','.join(self.lora_config.towers),
                sum(p.numel() for n, p in model.named_parameters() if '.lora_' in n)))
        train_dataloader, sampler = self.train_loader(model, train_dataset, feature_name)
        min_val_loss, max_score, wait = float("inf"), float("-inf"), 0
        num_training_steps = self.total_optimizer_steps(len(train_dataloader))
        if self.accum_steps > 1:
            from ..accumulate import check_accumulation
            world = torch.distributed.get_world_size() if self._ddp() else 1
            check_accumulation([self.batch_size] * self.accum_steps, self.accum_negatives, world)       # (before anything is built)
            logger.info('accumulated steps: {} x {} = {} molecules per optimizer step{}; contrastive terms see {}'.format(
                self.accum_steps, self.batch_size, self.accum_steps * self.batch_size, ' and rank' if world > 1 else '',
                'the union of the micro-batches' if self.accum_negatives == 'union' else 'each micro-batch on its own'))
        groups = self.param_groups
        if self.layer_decay is not None:
            from ..param_groups import layerwise_decay
            groups = list(groups or ()) + layerwise_decay(model, float(self.layer_decay))
        engine = FineTuner(model, self.task, learning_rate=self.learning_rate, adam_eps=1e-6, warmup_ratio=0.0,
                           total_steps=num_training_steps, alpha=self.alpha, beta=self.beta,
                           max_norm=self.max_norm if self.amp else None, distributed=self.distributed, skip_nonfinite=self.skip_nonfinite,
                           deterministic=self.deterministic, fds_stats=self.fds_stats, weight_decay=self.weight_decay,
                           decoupled_weight_decay=self.decoupled_weight_decay, param_groups=groups, ema_decay=self.ema_decay,
                           ema_warmup=self.ema_warmup, global_ct=self.global_ct, memory_bank=self.memory_bank or None)
        if engine.memory_bank:
            model.infonce.reset_memory_bank()            # (every fit starts from an empty bank; a resumed state then fills it)
            logger.info('InfoNCE memory bank: {} slots per side ({} steps of history)'.format(
                engine.memory_bank, engine.memory_bank // max(1, self.batch_size)))
        logger.info('ConR / SupCon keys: {}'.format(
            'global (every rank\'s molecules; the term is the union batch\'s)' if engine.global_ct else 'rank-local (this process\'s batch)'))
        if self.ema_decay is not None:
            logger.info('weight averaging: EMA decay {:g}{}; validation and checkpoints use the averaged weights'.format(
                self.ema_decay, ' with warm-up min(decay, (1 + t) / (10 + t))' if self.ema_warmup else ''))
        if engine.param_groups is not None or self.weight_decay:
            for name, count, elements, scale, wd in engine.param_group_summary():
                logger.info('param group {}: {} parameters, {} elements, lr_scale {:g}, weight_decay {:g}{}'.format(
                    name, count, elements, scale, wd, ' (decoupled)' if self.decoupled_weight_decay else ''))
        pool = getattr(model, "infonce_pool", "all")
        logger.info('InfoNCE pooling: {}'.format(
            'real tokens only (packed token rows without pad rows; the auto layout packs in training)' if pool == "real"
            else 'all positions, padding included (the reference)'))
        engine.warmup = int(num_training_steps * self.warmup_ratio)
        self._engine = engine
        task_loss = self._task_loss(loss_func)
        self.history = []
        epoch, start_epoch = 0, 0
        if self.resume:
            ts = self._load_train_state(engine, task_loss, dump_dir, fold)
            if ts is not None:
                epoch, min_val_loss, max_score, wait = ts["epoch"], ts["min_val_loss"], ts["max_score"], ts["wait"]
                start_epoch = self.max_epochs if ts["finished"] else epoch + 1
        for epoch in range(start_epoch, self.max_epochs):
            model = model.train()
            if sampler is not None:
                sampler.set_epoch(epoch)
            start_time = time.time()
            logged = []
            fds_epoch = self.fds and epoch >= model.fds_cfg.start_update
            if fds_epoch and self.fds_stats == "streaming":
                engine.fds_epoch_begin(epoch)
            skw = dict(epoch=epoch, use_weight=use_weight, return_infonce_loss=return_infonce_loss, return_ct_loss=return_ct_loss,
                       loss_func=task_loss)
            batches = self.device_batches(train_dataloader, feature_name)
            if self.accum_steps > 1:
                steps_of = (engine.step_accumulated(group, negatives=self.accum_negatives, **skw)
                            for group in self.accumulation_groups(batches, pool))
            else:
                steps_of = (engine.step(net_input, net_target, **skw) for net_input, net_target in batches)
            for out in steps_of:
                row = [out.loss, out.task_loss, out.infonce_loss if out.infonce_loss is not None else out.loss.new_zeros(()),
                       out.ct_loss if out.ct_loss is not None else out.loss.new_zeros(())]
                if out.skipped is not None:
                    row.append(out.skipped.reshape(()))          # (the guard's skip flag rides on the same read)
                logged.append(torch.stack(row))
            steps = torch.stack(logged).cpu().numpy() if logged else np.zeros((0, 4))        # the epoch's ONE device->host sync
            skipped = int(steps[:, 4].sum()) if steps.shape[1] > 4 else 0
            steps = steps[:, :4]
            if fds_epoch and self.fds_stats == "streaming":
                engine.fds_epoch_finish(epoch)
            elif fds_epoch:
                engine.fds_epoch_pass((self.decorate_batch(b, feature_name) for b in train_dataloader), epoch)
            # weight averaging: validation, the early-stop decision and the checkpoint it writes see the averaged weights (the FDS pass
            # above ran on the raw ones); the block's exit puts the raw weights back, bit for bit, for the next epoch's steps
            with (engine.averaged() if self.ema_decay is not None else contextlib.nullcontext()):
                y_preds, val_loss, metric_score = self.predict(model, valid_dataset, loss_func, activation_fn, dump_dir, fold, target_scaler,
                                                               epoch, load_model=False, feature_name=feature_name, return_infonce_loss=False)
                total_val_loss = float(np.mean(val_loss))
                _metric, _score = next(iter(metric_score.items()))
                self.history.append(dict(epoch=epoch, steps=steps, val_loss=total_val_loss, metric=_metric, score=_score, skipped=skipped))
                if steps.size:
                    logger.info('Epoch [{}/{}] train_loss: {:.4f}, train_m_loss: {:.4f}, train_infonce_loss: {:.4f}, train_ct_loss: {:.4f}, '
                                'val_loss: {:.4f}, val_{}: {:.4f}, {:.1f}s'.format(epoch + 1, self.max_epochs, *steps.mean(0), total_val_loss,
                                                                                    _metric, _score, time.time() - start_time)
                                + (', skipped steps: {}'.format(skipped) if self.skip_nonfinite else ''))
                is_early_stop, min_val_loss, wait, max_score = self._early_stop_choice(
                    wait, total_val_loss, min_val_loss, metric_score, max_score, model, dump_dir, fold, self.patience, epoch)
            if self.save_train_state:
                # (outside averaged(): the engine's state holds the raw weights and the average each in its own place)
                self._save_train_state(engine, task_loss, dump_dir, fold, epoch, min_val_loss, max_score, wait,
                                       finished=is_early_stop or epoch == self.max_epochs - 1)
            if is_early_stop:
                break
        self._checkpoint_barrier()          # rank 0's last write is complete before any rank reads the file
        if self.lora_config is not None:
            from ..lora import merge_lora
            merge_lora(model)               # (the checkpoint is merged: the closing prediction loads it into the reference-shaped model)
        y_preds, _, _ = self.predict(model, valid_dataset, loss_func, activation_fn, dump_dir, fold, target_scaler, epoch, load_model=True,
                                     feature_name=feature_name)
        return y_preds

    # -------------------------------------------------------------- early stopping / checkpoint (:330-385, utils/metrics.py:220-258)
    def _save(self, model, dump_dir, fold):
        """rank 0 only; written to a temporary name and renamed, so a reader never sees a half-written archive (torch.save is
        not atomic)"""
        if self.rank != 0:
            return
        os.makedirs(dump_dir, exist_ok=True)
        path = os.path.join(dump_dir, f'model_{fold}.pth')
        tmp = path + f'.tmp{os.getpid()}'
        sd = model.state_dict()
        if self.lora_config is not None:
            from ..lora import merged_state_dict
            sd = merged_state_dict(model)   # (W + s.B.A under the reference's keys; inside engine.averaged(): of the averaged weights)
        torch.save({'model_state_dict': sd}, tmp)
        os.replace(tmp, path)

    # -------------------------------------------------------------- resuming (DESIGN.md "Resuming a run")
    def _train_state_path(self, dump_dir, fold):
        return os.path.join(dump_dir, f'train_state_{fold}.pth')

    def _train_settings(self):
        """what decides the number of optimizer steps and the order of the batches: a resumed run must have been started alike"""
        s = dict(batch_size=int(self.batch_size), accum_steps=int(self.accum_steps), epochs=int(self.max_epochs), seed=int(self.seed))
        c = getattr(self, "lora_config", None)
        if c is not None:       # (absent without adapters: files written before, or without, LoRA compare as ever; alpha is not in the state)
            s["lora"] = "rank {} alpha {:g} targets {} towers {}".format(c.rank, c.alpha, ",".join(c.targets), ",".join(c.towers))
        return s

    def _save_train_state(self, engine, task_loss, dump_dir, fold, epoch, min_val_loss, max_score, wait, finished):
        """After an epoch's early-stop decision: everything the next epoch needs, written atomically by rank 0 (model_{fold}.pth stays
        what it is: the best epoch's weights under the reference's keys)."""
        if self.rank == 0:
            from ..checkpoint import atomic_save, pack_rng
            history = [dict(h, steps=torch.from_numpy(np.ascontiguousarray(h["steps"])), val_loss=float(h["val_loss"]), score=float(h["score"]),
                            metric=str(h["metric"])) for h in self.history]
            atomic_save({"engine": engine.state_dict(), "epoch": int(epoch), "min_val_loss": float(min_val_loss), "max_score": float(max_score),
                         "wait": int(wait), "history": history, "rng": pack_rng(), "finished": bool(finished),
                         "task_loss": task_loss.state_dict() if hasattr(task_loss, "state_dict") else None,
                         "settings": self._train_settings()}, self._train_state_path(dump_dir, fold))
        self._checkpoint_barrier()

    def _load_train_state(self, engine, task_loss, dump_dir, fold):
        """-> the file's bookkeeping after the engine, the loss, ``history`` and the RNG streams have been restored; None when there is
        no file (a run from epoch 0).  ValueError when the file was written under other settings."""
        path = self._train_state_path(dump_dir, fold)
        if not os.path.exists(path):
            logger.info('resume: no {} -- training starts at epoch 1'.format(path))
            return None
        from ..checkpoint import load, unpack_rng
        ts = load(path, map_location="cpu")
        own = self._train_settings()
        differ = ['{}: {!r} in the file, {!r} here'.format(k, ts["settings"].get(k), v) for k, v in own.items() if ts["settings"].get(k) != v]
        if differ:
            raise ValueError('Trainer: {} was written by a run with other settings ({})'.format(path, '; '.join(differ)))
        engine.load_state_dict(ts["engine"])
        if ts.get("task_loss") is not None and hasattr(task_loss, "load_state_dict"):
            task_loss.load_state_dict(ts["task_loss"])
        self.history = [dict(h, steps=h["steps"].numpy()) for h in ts["history"]]
        unpack_rng(ts["rng"])
        logger.info('resume: {} -- epoch {} of {} done{}'.format(path, ts["epoch"] + 1, self.max_epochs,
                                                                ', the run had finished' if ts["finished"] else ''))
        return ts

    def _checkpoint_barrier(self):
        if self._ddp():
            from ..parallel import host_group
            torch.distributed.barrier(group=host_group())

    def _agree(self, flag: bool) -> bool:
        """Data parallel: every rank follows RANK 0's reading of a per-epoch decision.  Each rank validates on its own device and the
        loss kernels add with atomics, so two ranks can differ in the last bit of a validation scalar; at a near-tie one rank
        would leave the epoch loop while the others enter the next step's collectives and wait forever."""
        if not self._ddp():
            return flag
        from ..parallel import host_broadcast_ints
        return bool(host_broadcast_ints([int(flag)], src=0)[0])

    def _early_stop_choice(self, wait, loss, min_loss, metric_score, max_score, model, dump_dir, fold, patience, epoch):
        by_loss = not isinstance(self.metrics_str, str) or self.metrics_str in ['loss', 'none', '']
        if by_loss:
            value, best, increase = loss, min_loss, False
        else:
            name, value = next(iter(metric_score.items()))
            increase = _is_increase(self.metrics, self.task, name)
            best = max_score if increase else min_loss
        improved = self._agree(value >= best if increase else value <= best)
        stop = False
        if improved:
            best, wait = value, 0
            self._save(model, dump_dir, fold)
        else:
            wait += 1
            if wait == patience:
                logger.warning(f'Early stopping at epoch: {epoch + 1}')
                stop = True
        if increase:
            return stop, min_loss, wait, best
        return stop, best, wait, max_score

    # -------------------------------------------------------------- predict
    def predict(self, model, dataset, loss_func, activation_fn, dump_dir, fold, target_scaler=None, epoch=1, load_model=False,
                feature_name=None, return_infonce_loss=False, return_ct_loss=False, return_feature=False):
        self._require_device()
        model = model.to(self.device)
        if load_model == True:      # noqa: E712  (the reference's spelling; callers pass bools)
            sd = torch.load(os.path.join(dump_dir, f'model_{fold}.pth'), map_location=self.device, weights_only=True)["model_state_dict"]
            model.load_state_dict(sd)           # (an arena-bound model re-casts its bf16 weight shadow on the next GEMM: runtime._fresh)
        dataloader = NNDataLoader(feature_name=feature_name, dataset=dataset, batch_size=self.batch_size, shuffle=False,
                                  collate_fn=self._collate_for(model), **self._loader_kwargs())
        model = model.eval()
        val_loss, y_preds, y_truths = [], [], []
        task_loss = self._task_loss(loss_func) or _builtin_loss(self.task)
        with torch.no_grad():
            for net_input, net_target in self.device_batches(dataloader, feature_name):
                outputs = model(**net_input)       # both auxiliary losses are force-disabled in the reference's predict (:427-428)
                if not load_model:
                    tl = task_loss(outputs, net_target)
                    val_loss.append(self.alpha * tl)
                y_preds.append(activation_fn(outputs))
                y_truths.append(net_target)
        y_preds = torch.cat(y_preds).float().cpu().numpy()
        y_truths = torch.cat(y_truths).cpu().numpy()
        val_loss = [float(v) for v in torch.stack(val_loss).cpu()] if val_loss else []
        label_cnt = getattr(model, "output_dim", None)
        metric_score = None
        if not load_model:
            if self.alpha != 0:
                if target_scaler is not None:
                    metric_score = self.metrics.cal_metric(target_scaler.inverse_transform(y_truths), target_scaler.inverse_transform(y_preds),
                                                           label_cnt=label_cnt)
                else:
                    metric_score = self.metrics.cal_metric(y_truths, y_preds, label_cnt=label_cnt)
            else:
                metric_score = {"ct_loss": float(np.mean(val_loss))}
        elif self.alpha == 0:
            metric_score = {"ct_loss": float(np.mean(val_loss)) if val_loss else float("nan")}
        return y_preds, val_loss, metric_score

    # -------------------------------------------------------------- attention maps
    def attention_maps(self, model, dataset, dump_dir, fold, feature_name=None, load_model=True, **kw):
        """Iterates ``dataset`` as ``predict`` does (same loader, same batches, eval mode, no_grad) and yields, per molecule, a dict of numpy
        arrays trimmed to the molecule's real lengths: ``prediction`` (the model's raw output row), ``atoms`` / ``tokens`` (the counts),
        ``text_to_graph`` {layer: [tokens, atoms]}, ``graph_to_text`` {layer: [atoms, tokens]}, ``unimol`` {layer: [atoms, atoms]},
        ``bert`` {layer: [tokens, tokens]} -- whichever ``which`` asks for (``**kw``: MM_Model.attention_maps' which / layers / head) --
        and, when the cross maps are there, ``atom_relevance`` [atoms] and ``token_relevance`` [tokens].  A generator: one batch's maps
        are alive at a time.  ``predict`` keeps the reference's signature; this is the read-out beside it."""
        self._require_device()
        model = model.to(self.device)
        if load_model == True:      # noqa: E712  (predict's spelling)
            sd = torch.load(os.path.join(dump_dir, f'model_{fold}.pth'), map_location=self.device, weights_only=True)["model_state_dict"]
            model.load_state_dict(sd)
        dataloader = NNDataLoader(feature_name=feature_name, dataset=dataset, batch_size=self.batch_size, shuffle=False,
                                  collate_fn=self._collate_for(model), **self._loader_kwargs())
        for net_input, _ in self.device_batches(dataloader, feature_name):
            yield from trim_attention_maps(model.attention_maps(**net_input, **kw))

    def _task_loss(self, loss_func):
        """What the step applies for ``loss_func``: None -- the engine's own kernel for the task (MSE / cross-entropy / BCE-with-
        logits); a kernel-backed object of ``mmdti_hip.losses`` for the reference's focal and GHM entries (one per Trainer and loss
        object, so that training and validation share GHM's bin history as they do in the reference); else the callable as given."""
        if not _is_builtin_loss(loss_func, self.task):
            return loss_func
        if self.task != "multilabel_classification" or loss_func is None or isinstance(loss_func, torch.nn.BCEWithLogitsLoss):
            return None
        if id(loss_func) not in self._loss_cache:       # (the entry keeps loss_func alive, so its id stays its own)
            self._loss_cache[id(loss_func)] = (loss_func, _builtin_loss(self.task, loss_func))
        return self._loss_cache[id(loss_func)][1]

    def set_seed(self, seed):
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)
        np.random.seed(seed)


def trim_attention_maps(am):
    """models.mm_model.AttentionMaps of one batch -> one dict of numpy arrays per molecule, every map cut to the molecule's real atoms /
    tokens (right-padded batches: the real positions are the first ones)."""
    out0 = am.outputs[0] if isinstance(am.outputs, (tuple, list)) else am.outputs
    pred = out0.detach().float().cpu().numpy()
    na, nt = am.atom_mask.sum(1).cpu().tolist(), am.token_mask.sum(1).cpu().tolist()
    host = {k: {l: m.detach().cpu().numpy() for l, m in getattr(am, k).items()} for k in ("text_to_graph", "graph_to_text", "unimol", "bert")}
    rel = (am.atom_relevance().cpu().numpy(), am.token_relevance().cpu().numpy()) if (am.text_to_graph and am.graph_to_text) else None
    cut = {"text_to_graph": lambda m, a, t: m[:t, :a], "graph_to_text": lambda m, a, t: m[:a, :t], "unimol": lambda m, a, t: m[:a, :a],
           "bert": lambda m, a, t: m[:t, :t]}
    for b, (a, t) in enumerate(zip(na, nt)):
        rec = {"prediction": pred[b], "atoms": int(a), "tokens": int(t)}
        for k, maps in host.items():
            if maps:
                rec[k] = {l: cut[k](m[b], a, t).copy() for l, m in maps.items()}
        if rel is not None:
            rec["atom_relevance"], rec["token_relevance"] = rel[0][b, :a].copy(), rel[1][b, :t].copy()
        yield rec


def _builtin_loss(task, loss_func=None):
    """The kernel-backed callable for a ``loss_func`` that _is_builtin_loss recognises (None: the task's default)."""
    from ..functional import CELossFn, MSELossFn, BCELogitsLossFn
    if task == "regression":
        return lambda o, t: MSELossFn.apply(o, t.float())
    if task == "multilabel_classification":
        kind = _multilabel_kind(loss_func)
        if kind == "self":
            return loss_func
        if kind == "focal":          # the function itself: called with its defaults alpha=0.25, gamma=2.0 (models/loss.py:257)
            from ..losses import FocalLossWithLogits
            return FocalLossWithLogits()
        if kind == "ghm":            # the table's single GHMC_Loss object: its bins / alpha and the history it has seen so far
            from ..losses import GHMCLoss
            loss = GHMCLoss(bins=loss_func._bins, alpha=loss_func._alpha)
            if loss_func._last_bin_count is not None:
                loss.load_state_dict({"last_bin_count": loss_func._last_bin_count})
            return loss
        return lambda o, t: BCELogitsLossFn.apply(o, t)
    return lambda o, t: CELossFn.apply(o, t)


def _multilabel_kind(loss_func):
    """Which entry of LOSS_RREGISTER['multilabel_classification'] (models/nnmodel.py:28-32) ``loss_func`` is, by what NNModel hands
    over: the FUNCTION ``FocalLossWithLogits`` ('focal'), the ``GHMC_Loss`` object ('ghm'), ``nn.BCEWithLogitsLoss()`` ('bce'); 'self'
    for the objects of ``mmdti_hip.losses``; None for anything else."""
    from ..losses import FocalLossWithLogits, GHMCLoss
    if isinstance(loss_func, (FocalLossWithLogits, GHMCLoss)):
        return "self"
    if loss_func is None:
        return "bce"
    if (isinstance(loss_func, torch.nn.BCEWithLogitsLoss) and loss_func.weight is None and loss_func.pos_weight is None
            and loss_func.reduction == "mean"):
        return "bce"
    import types
    if isinstance(loss_func, types.FunctionType) and loss_func.__name__ == "FocalLossWithLogits":
        return "focal"
    if type(loss_func).__name__ == "GHMC_Loss" and all(hasattr(loss_func, a) for a in ("_bins", "_alpha", "_last_bin_count")):
        return "ghm"
    return None


def _is_builtin_loss(loss_func, task):
    """True when ``loss_func`` is the reference's task loss for this task (models/nnmodel.py:24-34: ``nn.MSELoss()`` /
    ``myCrossEntropyLoss`` / the three multilabel entries) -- those run in kernels; any other callable is applied as given."""
    if loss_func is None:
        return task in ("regression", "classification", "multiclass", "multilabel_classification")
    if task == "regression":
        return isinstance(loss_func, torch.nn.MSELoss) and loss_func.reduction == "mean"
    if task in ("classification", "multiclass"):
        if getattr(loss_func, "__name__", "") == "myCrossEntropyLoss":
            return True
        # a configured nn.CrossEntropyLoss (class weights, label smoothing, another ignore_index / reduction) is NOT the plain kernel
        return (isinstance(loss_func, torch.nn.CrossEntropyLoss) and loss_func.weight is None and loss_func.label_smoothing == 0.0
                and loss_func.ignore_index == -100 and loss_func.reduction == "mean")
    if task == "multilabel_classification":
        return _multilabel_kind(loss_func) is not None
    return False


def NNDataLoader(feature_name=None, dataset=None, batch_size=None, shuffle=False, collate_fn=None, drop_last=False, **loader_kwargs):
    """tasks/trainer.py:540-556 (``loader_kwargs``: num_workers / pin_memory / persistent_workers, not in the reference)."""
    return TorchDataLoader(dataset=dataset, batch_size=batch_size, shuffle=shuffle, collate_fn=collate_fn, drop_last=drop_last, **loader_kwargs)
