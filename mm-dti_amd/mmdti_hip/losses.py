"""The multilabel_classification task losses of the reference's table (models/nnmodel.py:24-34) as device kernels.

``FocalLossWithLogits`` is the table's 'focal' entry -- the default of a multilabel model (models/nnmodel.py:90-93) -- and ``GHMCLoss``
its 'ghm' entry (``GHMC_Loss(bins=10, alpha=0.5)``).  Both are callables on ``(logits, target)`` like the reference's, take targets of
any dtype, and treat every target other than exactly 0 or 1 (NaN, -1) as a label that was not measured.  Neither reads anything back
to the host: a step that uses them enqueues without a synchronisation and can be captured in a HIP graph (``FineTuner.graphed_step``);
the reference's forms index with a boolean mask (a ``nonzero``) and, for GHM, call ``.item()`` eleven times per step.
"""
from __future__ import annotations

import torch

from .functional import FocalLogitsLossFn, GHMCLogitsLossFn


class FocalLossWithLogits:
    """models/loss.py:233-276: ``mean over the valid entries of -alpha (1 - q)^gamma log q``, q = clamp(y ? p : 1 - p, 1e-5, 1).  A batch
    without a single valid entry gives a NaN loss and zero gradients, as the reference's does (see mmdti_focal_logits_loss)."""

    def __init__(self, alpha: float = 0.25, gamma: float = 2.0):
        if not gamma > 0:
            raise ValueError(f"FocalLossWithLogits: gamma must be positive, got {gamma}")
        self.alpha, self.gamma = float(alpha), float(gamma)

    def __call__(self, logits, target):
        return FocalLogitsLossFn.apply(logits, target, self.alpha, self.gamma)

    def __repr__(self):
        return f"FocalLossWithLogits(alpha={self.alpha}, gamma={self.gamma})"


class GHMCLoss:
    """models/loss.py:19-132 (``GHMC_Loss``).  The moving average of the bin counts lives on the device and EVERY call updates it --
    training steps and validation batches alike, as the reference's single loss object sees both.  ``reset()`` forgets the history;
    ``state_dict()`` / ``load_state_dict()`` carry the counts (``last_bin_count``: None before the first call)."""

    def __init__(self, bins: int = 10, alpha: float = 0.5):
        if not 1 <= int(bins) <= 256:
            raise ValueError(f"GHMCLoss: bins must lie in 1..256, got {bins}")
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError(f"GHMCLoss: alpha must lie in [0, 1], got {alpha}")
        self.bins, self.alpha = int(bins), float(alpha)
        self._state = None          # [bins + 1] fp32 on the device: the last bin counts | the has-history flag
        self._pending = None        # counts loaded before the device is known

    def device_state(self, device):
        """The device buffer every call mutates (allocated on first use): ``FineTuner`` saves and restores it around the warm-up steps
        of a graph capture."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._state is None:
            self._state = torch.zeros(self.bins + 1, device=device, dtype=torch.float32)
            if self._pending is not None:
                self._state[:self.bins].copy_(self._pending)
                self._state[self.bins] = 1.0
                self._pending = None
        elif self._state.device != device:
            # the buffer never moves: a captured graph holds its address
            raise RuntimeError(f"GHMCLoss: the bin state lives on {self._state.device}, the call is on {device} (one loss object per device)")
        return self._state

    def __call__(self, logits, target):
        return GHMCLogitsLossFn.apply(logits, target, self.device_state(logits.device), self.bins, self.alpha)

    def reset(self):
        self._pending = None
        if self._state is not None:
            self._state.zero_()

    @property
    def last_bin_count(self):
        """The reference's ``_last_bin_count``: a [bins] device tensor, or None while there is no history.  (Reads the flag: a host
        synchronisation -- for checkpoints and tests, not for the step.)"""
        if self._state is None:
            return None if self._pending is None else self._pending.clone()
        return self._state[:self.bins].clone() if float(self._state[self.bins]) != 0.0 else None

    def state_dict(self):
        c = self.last_bin_count
        return {"bins": self.bins, "alpha": self.alpha, "last_bin_count": None if c is None else c.cpu()}

    def load_state_dict(self, sd):
        if int(sd.get("bins", self.bins)) != self.bins:
            raise ValueError(f"GHMCLoss.load_state_dict: {sd['bins']} bins in the state, {self.bins} here")
        c = sd.get("last_bin_count")
        self.reset()
        if c is None:
            return
        c = torch.as_tensor(c, dtype=torch.float32).reshape(-1)
        if c.numel() != self.bins:
            raise ValueError(f"GHMCLoss.load_state_dict: {c.numel()} bin counts, {self.bins} expected")
        if self._state is None:
            self._pending = c.clone()
        else:
            self._state[:self.bins].copy_(c)
            self._state[self.bins] = 1.0

    def __repr__(self):
        return f"GHMCLoss(bins={self.bins}, alpha={self.alpha})"


def from_key(loss_key):
    """'focal' / 'ghm' of LOSS_RREGISTER['multilabel_classification'] (models/nnmodel.py:28-32) with the reference's defaults."""
    if loss_key == "focal":
        return FocalLossWithLogits()
    if loss_key == "ghm":
        return GHMCLoss(bins=10, alpha=0.5)
    raise ValueError(f"unknown multilabel loss {loss_key!r}: 'bce', 'focal' or 'ghm'")
