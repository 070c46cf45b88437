"""Float64 statement of the banked InfoNCE direction (mmdti_infonce_bank_dir) and a host model of the ring (mmdti_infonce_bank_push).

One direction: anchor i (global row row0 + i) sees the Bg live keys followed by the bank slots that are valid and -- when ids are
given -- do not hold the anchor's own id; its label is live key row0 + i; cross_entropy(reduction="sum") over the anchors, autograd of
that sum / (2 Bg).  Written per anchor with concatenated key lists, not with masks: nothing here shares a formula with the kernels.
"""
import math

import torch


def bank_dir_ref(q, k, row0, Bl, bank, valid, bank_ids=None, ids=None, temperature=0.1, dtype=torch.float64):
    """-> (sum_i CE_i, dq [Bg, D], dk [Bg, D]) in `dtype`; the gradients are of sum / (2 Bg).  All arguments host tensors."""
    Bg = q.shape[0]
    qr, kr = q.to(dtype).clone().requires_grad_(), k.to(dtype).clone().requires_grad_()
    bank = bank.to(dtype)
    total = torch.zeros((), dtype=dtype)
    valid = valid.tolist()
    masked = ids is not None and bank_ids is not None
    bank_ids, ids = (bank_ids.tolist(), ids.tolist()) if masked else (None, None)
    for i in range(Bl):
        slots = [s for s in range(bank.shape[0]) if valid[s] != 0 and not (masked and bank_ids[s] == ids[row0 + i])]
        keys = torch.cat((kr, bank[slots]), dim=0) if slots else kr
        logits = (keys @ qr[row0 + i] / temperature).unsqueeze(0)
        total = total + torch.nn.functional.cross_entropy(logits, torch.tensor([row0 + i]), reduction="sum")
    (total / (2 * Bg)).backward()
    return total.detach(), qr.grad, kr.grad


class RingModel:
    """The ring on the host: row i of a push goes to slot (head + i) % cap, valid only if the whole row is finite (stored as zeros
    otherwise), id ids[i] or -1; then head advances by n modulo cap."""

    def __init__(self, cap, D):
        self.cap, self.rows, self.valid = cap, torch.zeros(cap, D), torch.zeros(cap, dtype=torch.uint8)
        self.ids, self.head = torch.full((cap,), -1, dtype=torch.int64), 0

    def push(self, rows, ids=None):
        assert rows.shape[0] <= self.cap
        for i, row in enumerate(rows):
            s, ok = (self.head + i) % self.cap, all(math.isfinite(float(x)) for x in row)
            self.rows[s], self.valid[s] = (row if ok else torch.zeros_like(row)), int(ok)
            self.ids[s] = -1 if ids is None else int(ids[i])
        self.head = (self.head + rows.shape[0]) % self.cap


def symmetric_ref(q, k, ring_q, ring_k, ids=None, temperature=0.1, dtype=torch.float64):
    """The banked symmetric loss of one process (row0 = 0, Bl = Bg): direction a reads the positive-side ring, direction b the
    query-side one.  ring_* are RingModels (or anything with rows / valid / ids).  -> the loss value (sum of both directions / 2 Bg)"""
    B = q.shape[0]
    a = bank_dir_ref(q, k, 0, B, ring_k.rows, ring_k.valid, ring_k.ids, ids, temperature, dtype)[0]
    b = bank_dir_ref(k, q, 0, B, ring_q.rows, ring_q.valid, ring_q.ids, ids, temperature, dtype)[0]
    return (a + b) / (2 * B)
