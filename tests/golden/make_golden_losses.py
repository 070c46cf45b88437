"""Generate tests/golden/g11_multilabel_losses.npz from the reference's own multilabel task losses.

Run ONCE where the reference tree is mounted read-only:

    python tests/golden/make_golden_losses.py

It imports the reference's models/loss.py (``FocalLossWithLogits``, ``GHMC_Loss``: the 'focal' and 'ghm' entries of
LOSS_RREGISTER['multilabel_classification'], models/nnmodel.py:28-32) at generation time, feeds them small seeded inputs in fp32
on the CPU and stores inputs, values, gradients and GHM's ``_last_bin_count`` trajectory.  Nothing from the reference is copied: the
fixture is data only, and the tests read only the .npz.

Focal, at (B, C) = (16, 12) and a ToxCast-like (8, 617): the same logits against
  * ``float``  the 0 / 1 labels as fp32,
  * ``int64``  the same labels as int64 (what the reference's trainer hands over),
  * ``neg1``   int64 labels with about 20 % replaced by -1,
  * ``nan``    fp32 labels with the same entries replaced by NaN,
and an all-missing batch.  float == int64 and neg1 == nan hold to the bit for value and gradient (asserted here), so one gradient
is stored per pair.

GHM: five consecutive calls of ONE ``GHMC_Loss(bins=10, alpha=0.5)`` on changing logits at (16, 12): value, gradient and
``_last_bin_count`` after each.  The logits are drawn so that no g * (bins - 1e-4), g = |sigmoid(x) - y|, lies within 1e-4 of an integer
(asserted): a one-ulp difference in ``sigmoid`` then cannot move an element to another bin.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("MMDTI_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))
BIN_EDGE_MARGIN = 1e-4
GHM_BINS, GHM_ALPHA, GHM_CALLS = 10, 0.5, 5


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def edge_distance(x, y, bins=GHM_BINS):
    """distance of g * (bins - 1e-4) to the nearest integer, per element, in float64 from the fp32 sigmoid"""
    g = (torch.sigmoid(x) - y).abs().double() * (bins - 0.0001)
    return (g - g.round()).abs()


def value_and_grad(fn, x, y):
    x = x.clone().requires_grad_()
    v = fn(x, y)
    (g,) = torch.autograd.grad(v, x, allow_unused=True)
    return v.detach(), torch.zeros_like(x) if g is None else g


def main():
    L = load_by_path("ref_loss", os.path.join(REF, "models/loss.py"))
    out = {}
    # ---------------------------------------------------------------- focal
    for tag, (B, C) in (("s", (16, 12)), ("w", (8, 617))):
        g = torch.Generator().manual_seed(1100 + C)
        x = 3.0 * torch.randn(B, C, generator=g)
        flat = x.view(-1)
        flat[::37] = 15.0            # saturated both ways: with the opposite label q = 1 - p falls below the 1e-5 clamp
        flat[5::41] = -15.0
        y = (torch.rand(B, C, generator=g) < 0.3).float()
        miss = torch.rand(B, C, generator=g) < 0.2
        t_float, t_int = y.clone(), y.long()
        t_neg1 = torch.where(miss, torch.full_like(t_int, -1), t_int)
        t_nan = torch.where(miss, torch.full_like(y, float("nan")), y)
        v_f, g_f = value_and_grad(L.FocalLossWithLogits, x, t_float)
        v_i, g_i = value_and_grad(L.FocalLossWithLogits, x, t_int)
        v_m, g_m = value_and_grad(L.FocalLossWithLogits, x, t_neg1)
        v_n, g_n = value_and_grad(L.FocalLossWithLogits, x, t_nan)
        assert torch.equal(v_f, v_i) and torch.equal(g_f, g_i), "focal: float and int64 targets differ"
        assert torch.equal(v_m, v_n) and torch.equal(g_m, g_n), "focal: -1 and NaN masks differ"
        assert float(g_m[miss].abs().max()) == 0.0, "focal: a masked entry has a gradient"
        assert int(((torch.sigmoid(x) < 1e-5) & (y == 1)).sum()) > 0, "focal: no entry reaches the clamp"
        out.update({f"focal_{tag}_logits": x, f"focal_{tag}_y": y.to(torch.int8), f"focal_{tag}_miss": miss,
                    f"focal_{tag}_value_float": v_f, f"focal_{tag}_value_int64": v_i, f"focal_{tag}_value_neg1": v_m, f"focal_{tag}_value_nan": v_n,
                    f"focal_{tag}_grad_full": g_f, f"focal_{tag}_grad_masked": g_m})
    g = torch.Generator().manual_seed(1177)
    x = torch.randn(16, 12, generator=g)
    v, gr = value_and_grad(L.FocalLossWithLogits, x, torch.full((16, 12), -1, dtype=torch.int64))
    assert torch.isnan(v)
    out.update(focal_allmissing_logits=x, focal_allmissing_value=v, focal_allmissing_grad=gr)
    # ---------------------------------------------------------------- GHM
    g = torch.Generator().manual_seed(1190)
    B, C = 16, 12
    loss = L.GHMC_Loss(bins=GHM_BINS, alpha=GHM_ALPHA)
    xs, ys, vals, grads, counts = [], [], [], [], []
    for call in range(GHM_CALLS):
        y = (torch.rand(B, C, generator=g) < 0.3).float()
        x = (1.0 + 0.5 * call) * torch.randn(B, C, generator=g) + 0.3 * call
        for _ in range(100):            # redraw the entries that sit near a bin edge
            near = edge_distance(x, y) <= 2 * BIN_EDGE_MARGIN
            if not near.any():
                break
            x = torch.where(near, (1.0 + 0.5 * call) * torch.randn(B, C, generator=g), x)
        assert float(edge_distance(x, y).min()) > BIN_EDGE_MARGIN, "GHM: an input sits within the margin of a bin edge"
        v, gr = value_and_grad(loss, x, y)
        xs.append(x); ys.append(y.to(torch.int8)); vals.append(v); grads.append(gr); counts.append(loss._last_bin_count.clone())
    out.update(ghm_logits=torch.stack(xs), ghm_y=torch.stack(ys), ghm_value=torch.stack(vals), ghm_grad=torch.stack(grads),
               ghm_last_bin_count=torch.stack(counts), ghm_bins=np.int64(GHM_BINS), ghm_alpha=np.float64(GHM_ALPHA),
               ghm_edge_margin=np.float64(BIN_EDGE_MARGIN))
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(OUT, "g11_multilabel_losses.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, len(arrays), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
