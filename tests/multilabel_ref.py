"""float64 NumPy restatements of the two multilabel task losses (models/loss.py:63-132, 233-276), shared by
test_multilabel_losses_cpu.py and test_multilabel_losses_gpu.py, and the cases of tests/golden/g11_multilabel_losses.npz."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_multilabel_losses.npz")


def load_fixture():
    return dict(np.load(FIXTURE, allow_pickle=False))


def sigmoid64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def focal_f64(x, t, alpha=0.25, gamma=2.0):
    """-> (value, gradient, per-element parts) of mean over the valid entries (target exactly 0 or 1) of -alpha (1 - q)^gamma log q,
    q = clamp(y ? p : 1 - p, 1e-5, 1).  Closed-form gradient; 0 at missing entries and where the clamp holds q at 1e-5."""
    t = np.asarray(t, dtype=np.float64)
    valid = (t == 0.0) | (t == 1.0)
    p = sigmoid64(x)
    qr = np.where(t == 1.0, p, 1.0 - p)
    q = np.clip(qr, 1e-5, 1.0)
    lq = np.log(q)
    li = np.where(valid, -alpha * (1.0 - q) ** gamma * lq, 0.0)
    s = np.where(t == 1.0, 1.0, -1.0)
    gi = np.where(valid & (qr >= 1e-5), -alpha * s * ((1.0 - q) ** (gamma + 1.0) - gamma * q * (1.0 - q) ** gamma * lq), 0.0)
    cnt = int(valid.sum())
    if cnt == 0:
        return float("nan"), np.zeros_like(gi), dict(valid=valid, q=q, li=li, gi=gi, cnt=0)
    return float(li.sum() / cnt), gi / cnt, dict(valid=valid, q=q, li=li, gi=gi, cnt=cnt)


def ghm_bin_position(x, t, bins):
    """g (bins - 1e-4), g = |sigmoid(x) - y|: its floor is the bin"""
    return np.abs(sigmoid64(x) - np.asarray(t, dtype=np.float64)) * (bins - 0.0001)


def ghmc_f64(x, t, last, bins=10, alpha=0.5):
    """One GHMC_Loss call -> (value, gradient, the bin counts it leaves).  last: the previous call's counts or None.  Entries whose
    target is not 0 or 1 stay out of the histogram and get zero weight and gradient; N counts every entry."""
    x = np.asarray(x, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    valid = (t == 0.0) | (t == 1.0)
    tz = np.where(valid, t, 0.0)
    p = sigmoid64(x)
    idx = np.minimum(np.floor(np.abs(p - tz) * (bins - 0.0001)).astype(np.int64), bins - 1)
    count = np.bincount(idx[valid], minlength=bins).astype(np.float64)
    if last is not None:
        count = alpha * np.asarray(last, dtype=np.float64) + (1.0 - alpha) * count
    nonempty = int((count > 0).sum())
    n = x.size
    beta = n / np.maximum(count * nonempty, 1e-4)
    w = np.where(valid, beta[idx], 0.0)
    bce = np.maximum(x, 0.0) - x * tz + np.log1p(np.exp(-np.abs(x)))
    return float((w * bce).sum() / n), w * (p - tz) / n, count


def focal_cases(fx):
    """-> [(name, logits fp32, targets (fp32 / int64 array), reference value fp32, reference gradient fp32)]: every focal case."""
    cases = []
    for tag in ("s", "w"):
        x, y, miss = fx[f"focal_{tag}_logits"], fx[f"focal_{tag}_y"], fx[f"focal_{tag}_miss"]
        t_int = y.astype(np.int64)
        targets = {"float": y.astype(np.float32), "int64": t_int, "neg1": np.where(miss, -1, t_int),
                   "nan": np.where(miss, np.float32("nan"), y.astype(np.float32)).astype(np.float32)}
        for kind, t in targets.items():
            cases.append((f"focal_{tag}_{kind}", x, t, fx[f"focal_{tag}_value_{kind}"], fx[f"focal_{tag}_grad_" + ("full" if kind in ("float", "int64") else "masked")]))
    x = fx["focal_allmissing_logits"]
    cases.append(("focal_allmissing", x, np.full(x.shape, -1, dtype=np.int64), fx["focal_allmissing_value"], fx["focal_allmissing_grad"]))
    return cases
