"""float64 references (plain torch on the CPU) for the fp32 kernels at the two ends of the step: ConR / SupCon, FDS, F.normalize,
the task losses, masked pooling and the embedding scatter.  Shared by test_head_refs_cpu.py (which pins these helpers to the
reference project's own numbers, tests/golden g3 / g4) and test_head_kernels_gpu.py (which holds the device kernels to them).

Every mask (positives / negatives, bucket ids, zero-variance columns) is decided on the float32 inputs exactly as the kernels
decide it; only the arithmetic behind the masks runs in float64."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from oracle import mmdti_oracle as O

F64 = torch.float64


def nerr(got, ref):
    """max|got - ref| / max|ref|: one band means the same thing whatever the magnitude of a gradient.  A reference that is zero
    everywhere admits only an exactly equal result (0.0), anything else is inf."""
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    num, den = float((got - ref).abs().max()), float(ref.abs().max())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


# ------------------------------------------------------------------------------------------------ ConR / SupCon
CT_MODES = ("regress", "single", "multi")


def ct_loss(mode, feature, labels, pred=None, weights=None, w=0.2, t=0.07, e=0.01, coef=1, dtype=F64):
    """-> (loss, d loss / d feature), both `dtype`, of oracle.ct_regress / ct_single / ct_multi on `feature` cast to `dtype`.
    labels: regress [B] / [B, k] float32 (+ pred alike); single [B] float32; multi [B, C] int64.  weights: [B] float32 or None."""
    f = feature.detach().to(dtype).clone().requires_grad_()
    if mode == "regress":
        lab, prd = labels.float().reshape(labels.shape[0], -1), pred.float().reshape(pred.shape[0], -1)
        loss = O.ct_regress(f, lab, prd, weights=weights, w=w, t=t, e=e)
    elif mode == "single":
        loss = O.ct_single(f, labels.float().reshape(-1), None, weights=weights, t=t)
    elif mode == "multi":
        loss = O.ct_multi(f, labels.long(), None, weights=weights, t=t, coef=coef)
    else:
        raise ValueError(mode)
    (df,) = torch.autograd.grad(loss, f, allow_unused=True)
    df = torch.zeros_like(f) if df is None else df
    return loss.detach().to(dtype), df.detach()


# The ConR / SupCon cases of test_head_kernels_gpu.py, built here so that test_head_refs_cpu.py can pin the fp32 oracle's own error on
# the very same inputs without a GPU.
CT_W = 0.3125          # labels and predictions are multiples of 1/8: no pair sits on the `<= w` threshold
CT_NCLS = 8
G = lambda s: torch.Generator().manual_seed(s)


def ct_features(kind, cls, D, g):
    """gauss: almost orthogonal rows at these widths (s / t in a narrow band round 0).  clustered: centre[label] + 0.3 noise with
    antipodal centre pairs -- same-label pairs near +1/t, opposite centres near -1/t, the rest round 0."""
    B = cls.numel()
    if kind == "gauss":
        return torch.randn(B, D, generator=g)
    half = torch.randn(CT_NCLS // 2, D, generator=g)
    centre = torch.cat((half, -half))
    return centre[cls] + 0.3 * torch.randn(B, D, generator=g)


@functools.lru_cache(maxsize=None)
def ct_case(mode, B, D, kind, use_w, variant=""):
    """-> namespace(mode, kind, f, labels, pred, weights, coef, loss, df, l32, o32): inputs (fp32 / int64, CPU), the float64 reference
    and the fp32 CPU oracle's own figures on this input (l32: its loss; o32: nerr of its gradient), computed once."""
    g = G(7 * B + D + 13 * len(kind) + 101 * CT_MODES.index(mode) + (1 if use_w else 0))
    cls = torch.randint(0, CT_NCLS, (B,), generator=g)
    if variant == "all_equal":
        cls = torch.full((B,), 3)
    f = ct_features(kind, cls, D, g)
    weights = (0.5 + torch.rand(B, generator=g)) if use_w else None
    pred, coef = None, 1
    if mode == "regress":
        labels = cls.float() / 8
        pred = labels + torch.randint(-3, 4, (B,), generator=g).float() / 8
        if variant == "isolated_row":        # row 0: no positive but itself, nobody's positive or negative
            labels[0], pred[0] = 100.0, 100.0
        if variant == "no_negative_row":     # row 1: positives, but its prediction is far from everyone's: flag 0
            pred[1] = 50.0
    elif mode == "single":
        labels = cls.float()
        if variant == "no_positive_row":     # row 2: a label nobody shares: SupCon denominator 1
            labels[2] = 77.0
    else:
        if variant == "c617_coef1":          # wide-valued assays: about half of the pairs share no column at all
            labels, coef = torch.randint(0, 1000, (B, 617), generator=g), 1
        elif variant == "c617_coef300":      # binary assays from class prototypes with 10% flips: same class ~500 matches, else ~308
            proto = torch.randint(0, 2, (CT_NCLS, 617), generator=g)
            labels, coef = proto[cls] ^ (torch.rand(B, 617, generator=g) < 0.1).long(), 300
        else:
            proto = torch.randint(0, 2, (CT_NCLS, 6), generator=g)
            labels, coef = proto[cls] ^ (torch.rand(B, 6, generator=g) < 0.15).long(), 4
    loss, df = ct_loss(mode, f, labels, pred=pred, weights=weights, w=CT_W, coef=coef)
    l32, df32 = ct_loss(mode, f, labels, pred=pred, weights=weights, w=CT_W, coef=coef, dtype=torch.float32)
    return SimpleNamespace(mode=mode, kind=kind, f=f, labels=labels, pred=pred, weights=weights, coef=coef, loss=loss, df=df,
                           l32=l32.to(F64), o32=nerr(df32, df))


# ------------------------------------------------------------------------------------------------ FDS
FDS_BUFFERS = ("running_mean", "running_var", "running_mean_last_epoch", "running_var_last_epoch", "smoothed_mean_last_epoch",
               "smoothed_var_last_epoch", "num_samples_tracked")


class FDS64(O.FDSOracle):
    """FDSOracle with its buffers in float64 and the smoothing window passed in explicitly (any odd length).  The bucket ids stay
    float32 arithmetic (fds_label_bins): they are integers and must be bit-exact."""

    def __init__(self, feature_dim, min_value, bin_width, window, bucket_num=100, bucket_start=0, start_update=0, start_smooth=1,
                 momentum=0.9):
        window = torch.as_tensor(window)
        assert window.dim() == 1 and window.numel() % 2 == 1
        super().__init__(feature_dim, min_value, bin_width, bucket_num=bucket_num, bucket_start=bucket_start, start_update=start_update,
                         start_smooth=start_smooth, ks=window.numel(), momentum=momentum)
        self.kernel_window = window.to(F64)          # (_smooth_stat takes the window's dtype: float64 conv1d)
        self.half_ks = (window.numel() - 1) // 2
        for k in FDS_BUFFERS:
            setattr(self, k, getattr(self, k).to(F64))

    def update_running_stats(self, features, labels, epoch):
        return super().update_running_stats(features.to(F64), labels, epoch)

    def smooth(self, features, labels, epoch):
        return super().smooth(features.to(F64), labels, epoch)

    def smooth_with_scale(self, features, labels, epoch):
        """-> (y, d y / d x): the per-element scale by autograd"""
        x = features.detach().to(F64).clone().requires_grad_()
        y = self.smooth(x, labels, epoch)
        if y is x:                                   # (epoch < start_smooth)
            return x.detach(), torch.ones_like(x)
        (sc,) = torch.autograd.grad(y.sum(), x)
        return y.detach(), sc


def smooth_stat(stat, window):
    """reflect-pad + conv1d across the bucket axis (fds.py:86-99) in float64"""
    window = torch.as_tensor(window).to(F64)
    half = (window.numel() - 1) // 2
    x = F.pad(stat.to(F64).unsqueeze(1).permute(2, 1, 0), pad=(half, half), mode="reflect")
    return F.conv1d(x, window.view(1, 1, -1), padding=0).permute(2, 1, 0).squeeze(1)


def calibrate(x, m1, v1, m2, v2):
    """calibrate_mean_var in float64 (the input is not written)"""
    return O.calibrate_mean_var(x.to(F64).clone(), m1.to(F64), v1.to(F64), m2.to(F64), v2.to(F64))


# ------------------------------------------------------------------------------------------------ small references
def l2norm(x, dxh=None):
    """F.normalize (eps 1e-12) -> xhat, and d x for an upstream d xhat by autograd"""
    xr = x.detach().to(F64).clone().requires_grad_()
    xh = F.normalize(xr, dim=1)
    if dxh is None:
        return xh.detach()
    (dx,) = torch.autograd.grad((xh * dxh.to(F64)).sum(), xr)
    return xh.detach(), dx


def _loss_and_grad(fn, x, *a):
    xr = x.detach().to(F64).clone().requires_grad_()
    loss = fn(xr, *a)
    (dx,) = torch.autograd.grad(loss, xr)
    return loss.detach().reshape(1), dx


def mse(pred, target):
    return _loss_and_grad(F.mse_loss, pred, target.to(F64))


def cross_entropy(logits, target):
    return _loss_and_grad(F.cross_entropy, logits, target.long())


def bce_logits(logits, target):
    return _loss_and_grad(F.binary_cross_entropy_with_logits, logits, target.to(F64))


def masked_pool(a, t, ma, mt, dp=None):
    """mm_model.py:572-576: sum of the unmasked rows of [a; t] / their count -> pooled [B, D] (+ d a, d t for an upstream d pooled).
    A molecule without any unmasked row is 0 / 0 = NaN in every column, as in the reference."""
    ar, tr = a.detach().to(F64).clone().requires_grad_(), t.detach().to(F64).clone().requires_grad_()
    out = torch.cat((ar * ma.unsqueeze(-1), tr * mt.unsqueeze(-1)), 1).sum(1) / (ma.sum(1) + mt.sum(1)).view(-1, 1)
    if dp is None:
        return out.detach()
    da, dt = torch.autograd.grad((out * dp.to(F64)).sum(), (ar, tr))
    return out.detach(), da, dt


def embedding_grad(ids, dout, vocab, padding_idx=-1):
    """d table of F.embedding(ids, table, padding_idx) for an upstream dout (padding_idx < 0: none)"""
    D = dout.shape[-1]
    table = torch.zeros(vocab, D, dtype=F64, requires_grad=True)
    out = F.embedding(ids, table, padding_idx=padding_idx if padding_idx >= 0 else None)
    (g,) = torch.autograd.grad((out * dout.to(F64).view(*ids.shape, D)).sum(), table)
    return g
