"""float64 restatement (plain torch on the CPU) of the ConR / SupCon terms for a ROW BLOCK of a batch: anchors [row0, row0 + rows) of a
Bg-row batch against all Bg keys -- what one rank computes under global negatives when the ranks' local batches, concatenated in rank
order, form the batch.  Written from the reference's models/contrastive.py (CT_Regress :3-59, CT_Single :62-112, CT_Multi :114-169)
with its [B, B] matrices cut to the block's rows; independent of the kernels.  Shared by test_ct_global_cpu.py (which pins it to
oracle.mmdti_oracle.ct_* on the union, summed over virtual ranks) and test_ct_global_gpu.py (which holds the kernels to it).

Every mask is decided on the float32 / int64 inputs as the reference decides it; the arithmetic behind the masks runs in float64.
The reference's quirks are kept: masked-out entries add exp(0) = 1 to the positive sum, ConR's denominator counts the anchor itself,
SupCon / Multi divide by max(#positives, 1), an anchor without any negative contributes 0, ConR's weight is the anchor's and
SupCon / Multi's the key's."""
import torch
import torch.nn.functional as F

F64 = torch.float64
MODES = ("regress", "single", "multi")
CT_W = 0.3125          # labels and predictions of ct_inputs are multiples of 1/8: no pair sits on the `<= w` threshold


def row_terms(mode, feature, labels, row0, rows, pred=None, weights=None, w=0.2, t=0.07, e=None, coef=1, normalize=True):
    """-> l [rows] float64: the per-anchor terms l_i of anchors row0 .. row0 + rows - 1 (their mean over ALL Bg anchors is the loss).
    feature [Bg, D] (any float dtype; differentiable -- pass a float64 leaf for the gradient); normalize=False takes it as the already
    L2-normalised f-hat, so that autograd yields d / d f-hat with f-hat as the free variable (the kernels' dfhat).
    labels: regress [Bg] / [Bg, k] float (+ pred alike), single [Bg] float, multi [Bg, C] int64; weights [Bg] float or None."""
    Bg = feature.shape[0]
    f = feature.to(F64).reshape(Bg, -1)
    q = F.normalize(f, dim=1) if normalize else f
    idx = torch.arange(row0, row0 + rows)
    prod = (q[idx] @ q.T) / t                                        # [rows, Bg]
    if mode == "regress":
        e = 0.01 if e is None else e
        l = labels.float().reshape(Bg, -1).mean(dim=1)
        p = pred.float().reshape(Bg, -1).mean(dim=1)
        l_dist = (l[idx].unsqueeze(1) - l.unsqueeze(0)).abs()        # float32, as the masks are decided
        p_dist = (p[idx].unsqueeze(1) - p.unsqueeze(0)).abs()
        le = l_dist.le(w)
        pos_i, neg_i = le.clone(), (~le) & p_dist.le(w)
        wa = torch.ones(rows, 1, dtype=F64) if weights is None else weights.float().reshape(Bg, -1).mean(dim=1)[idx].to(F64).unsqueeze(1)
        pushing_w = l_dist.to(F64) * wa * e                          # the ANCHOR's weight (:39-41)
        pos_i[torch.arange(rows), idx] = False
        denom = le.sum(1).to(F64)                                    # counts the anchor itself (:51)
    else:
        if mode == "single":
            lab = labels.float().reshape(Bg, 1)
            same = (lab[idx] - lab.T).abs().eq(0)
        elif mode == "multi":
            lab = labels.reshape(Bg, -1)
            C = lab.shape[1]
            sim = (lab[idx].unsqueeze(1) == lab.unsqueeze(0)).sum(-1).to(torch.float32) / C
            same = sim.ge(coef / C)
        else:
            raise ValueError(mode)
        pos_i, neg_i = same.clone(), ~same
        pushing_w = torch.ones(1, Bg, dtype=F64) if weights is None else weights.to(F64).reshape(1, Bg)      # the KEY's weight (:94, :150)
        pos_i[torch.arange(rows), idx] = False
        denom = pos_i.sum(1).to(F64)
        denom = torch.where(denom == 0, torch.ones_like(denom), denom)
    pos, neg = prod * pos_i, prod * neg_i
    neg_exp_dot = (pushing_w * torch.exp(neg) * neg_i).sum(1)
    no_neg_flag = neg_i.sum(1).bool()
    loss = (-torch.log(torch.exp(pos) / (torch.exp(pos).sum(1) + neg_exp_dot).unsqueeze(-1)) * pos_i).sum(1) / denom
    return loss * no_neg_flag


def share(mode, feature, labels, row0, rows, **kw):
    """the block's share of the loss: (1 / Bg) sum of its per-anchor terms; the shares of a partition of the rows add up to the loss"""
    return row_terms(mode, feature, labels, row0, rows, **kw).sum() / feature.shape[0]


def share_and_grad(mode, feature, labels, row0, rows, **kw):
    """-> (share, d share / d feature [Bg, D]) in float64: the block's contribution to EVERY row's gradient"""
    f = feature.detach().to(F64).clone().requires_grad_()
    s = share(mode, f, labels, row0, rows, **kw)
    (df,) = torch.autograd.grad(s, f, allow_unused=True)
    return s.detach(), (torch.zeros_like(f) if df is None else df.detach())


def nerr(got, ref):
    """max|got - ref| / max|ref| (0 / 0 -> 0, x / 0 -> inf)"""
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    num, den = float((got - ref).abs().max()), float(ref.abs().max())
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def ct_inputs(mode, B, D, seed, use_w=True, C=12, ncls=4):
    """-> dict(f [B, D] float32, labels, pred | None, weights | None, coef): seeded inputs on which every mask is non-trivial.
    regress: labels / predictions multiples of 1/8 (use w = CT_W); single: ncls classes; multi: [B, C] int64 assays from class
    prototypes with flips and some -1 (missing) entries, positives need coef = C // 2 + 1 matching columns."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, ncls, (B,), generator=g)
    f = torch.randn(B, D, generator=g) + 0.5 * torch.randn(ncls, D, generator=g)[cls]
    weights = (0.5 + torch.rand(B, generator=g)) if use_w else None
    pred, coef = None, 1
    if mode == "regress":
        labels = cls.float() / 4
        pred = labels + torch.randint(-3, 4, (B,), generator=g).float() / 8
    elif mode == "single":
        labels = cls.float()
    else:
        proto = torch.randint(0, 2, (ncls, C), generator=g)
        labels = proto[cls] ^ (torch.rand(B, C, generator=g) < 0.1).long()
        labels = torch.where(torch.rand(B, C, generator=g) < 0.05, torch.full_like(labels, -1), labels)
        coef = C // 2 + 1
    return dict(f=f, labels=labels, pred=pred, weights=weights, coef=coef)


def ref_kwargs(mode, c, w=CT_W):
    """keyword arguments of row_terms / share for a ct_inputs case"""
    kw = dict(pred=c["pred"], weights=c["weights"], coef=c["coef"])
    if mode == "regress":
        kw["w"] = w
    return kw
