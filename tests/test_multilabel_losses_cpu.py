"""Host-side checks of the multilabel focal / GHM task losses and of missing labels (no GPU): the fixture of the reference's own
losses against a float64 restatement, the bin-edge condition of the GHM inputs, EpochMetric on labels with -1 / NaN, the loss-selection
table of tasks.Trainer, the target normalisation, and the new C ABI symbols."""
import warnings

import numpy as np
import pytest
import torch

from mmdti_hip import _abi
from mmdti_hip.tasks import trainer as T

import multilabel_ref as R


def test_focal_fixture_equals_float64_restatement():
    """The reference's fp32 CPU values and gradients against the formula in float64.  The bound is the fp32 error budget of the
    reference's own evaluation, per element: it forms q = 1 - p from an fp32 p whose error is up to 2 ulp of a number below 1
    (dq = 2^-23), and l = -alpha (1 - q)^gamma log q answers that with |dl/dq| dq -- large where q is small (1/q); a handful of
    further fp32 roundings add 8 x 2^-24 relative.  The gradient answers dq with |dg/dq| dq, and the reference's autograd carries the
    factor (1 - p) p of sigmoid's backward, whose small factor has the relative error dq / q or dq / (1 - q)."""
    fx = R.load_fixture()
    alpha, gamma, dq, rnd = 0.25, 2.0, 2.0 ** -23, 8 * 2.0 ** -24
    for name, x, t, v_ref, g_ref in R.focal_cases(fx):
        v, g, parts = R.focal_f64(x, t, alpha, gamma)
        if name == "focal_allmissing":
            assert np.isnan(v_ref) and np.isnan(v) and not g_ref.any() and not g.any()
            continue
        q, valid, cnt = parts["q"], parts["valid"], parts["cnt"]
        dl_dq = alpha * np.abs((1 - q) ** gamma / q - gamma * (1 - q) ** (gamma - 1) * np.log(q))
        v_tol = float(np.where(valid, dl_dq * dq + rnd * np.abs(parts["li"]), 0.0).sum() / cnt)
        omq, lq = 1 - q, np.abs(np.log(q))
        dg_dq = alpha * ((gamma + 1) * omq ** gamma + gamma * omq ** gamma * lq + gamma ** 2 * q * omq ** (gamma - 1) * lq + gamma * omq ** gamma)
        g_tol = (dg_dq * dq + np.abs(parts["gi"]) * (dq / q + dq / np.maximum(omq, dq) + rnd) + 1e-12) / cnt
        assert abs(float(v_ref) - v) <= v_tol, (name, float(v_ref), v, v_tol)
        assert (np.abs(g_ref.astype(np.float64) - g) <= g_tol).all(), (name, float(np.abs(g_ref - g).max()))
        assert not g_ref[~valid].any() and not g[~valid].any()          # exactly 0 at missing entries
    # float == int64 and -1 == NaN, to the bit
    for tag in ("s", "w"):
        assert fx[f"focal_{tag}_value_float"] == fx[f"focal_{tag}_value_int64"] and fx[f"focal_{tag}_value_neg1"] == fx[f"focal_{tag}_value_nan"]
        assert fx[f"focal_{tag}_value_float"] != fx[f"focal_{tag}_value_neg1"]
    assert fx["focal_w_logits"].shape[1] == 617 and fx["focal_s_logits"].shape[1] == 12


def test_ghm_fixture_equals_float64_restatement_and_inputs_clear_the_bin_edges():
    fx = R.load_fixture()
    bins, alpha, margin = int(fx["ghm_bins"]), float(fx["ghm_alpha"]), float(fx["ghm_edge_margin"])
    assert fx["ghm_logits"].shape[0] >= 4 and margin == 1e-4
    last = None
    for k in range(fx["ghm_logits"].shape[0]):
        x, y = fx["ghm_logits"][k], fx["ghm_y"][k].astype(np.float32)
        # the generator's condition, on the stored inputs: no g (bins - 1e-4) within 1e-4 of an integer (so a one-ulp difference in
        # sigmoid cannot move an element to another bin); checked with the float64 sigmoid and with the fp32 one
        for pos in (R.ghm_bin_position(x, y, bins), np.abs(torch.sigmoid(torch.from_numpy(x)).numpy() - y).astype(np.float64) * (bins - 0.0001)):
            assert float(np.abs(pos - np.round(pos)).min()) > margin, k
        v, g, last = R.ghmc_f64(x, y, last, bins, alpha)
        # counts: integers and dyadic averages of integers -- exact in fp32 and float64 alike
        assert np.array_equal(last, fx["ghm_last_bin_count"][k].astype(np.float64)), k
        # value / gradient: about 16 fp32 roundings on the way (sigmoid, the BCE terms, the weight, the mean): 16 x 2^-24 relative; the
        # gradient's factor p - y is a difference of fp32 numbers near 1 (up to 2 ulp off: 2^-23), relative error 2^-23 / |p - y|
        rel, dq = 16 * 2.0 ** -24, 2.0 ** -23
        assert abs(float(fx["ghm_value"][k]) - v) <= rel * abs(v), (k, float(fx["ghm_value"][k]), v)
        g_tol = np.abs(g) * (rel + dq / np.maximum(np.abs(R.sigmoid64(x) - y), dq)) + 1e-12
        assert (np.abs(fx["ghm_grad"][k].astype(np.float64) - g) <= g_tol).all(), k
    assert not np.array_equal(fx["ghm_logits"][0], fx["ghm_logits"][1])


def test_epoch_metric_scores_the_valid_entries_only():
    """utils/metrics.py:30-56,156-170: label columns are scored over their 0 / 1 entries; -1 and NaN mark unmeasured assays."""
    rng = np.random.default_rng(5)
    n, C = 60, 4
    y = (rng.random((n, C)) < 0.4).astype(np.float64)
    p = rng.random((n, C))
    miss = rng.random((n, C)) < 0.25
    miss[:, 3] = True                                         # a column without a single measured entry: left out of the mean
    for sentinel in (-1.0, np.nan):
        lab = np.where(miss, sentinel, y)
        for name in ("log_loss", "auc", "auprc", "acc", "mcc"):
            m = T.EpochMetric("multilabel_classification", name)
            want = float(np.mean([T._METRIC_TABLE[name][0](y[~miss[:, c], c], p[~miss[:, c], c]) for c in range(3)]))
            got = m.cal_metric(lab, p)[name]
            assert got == pytest.approx(want, rel=1e-12, abs=0), (name, sentinel, got, want)
    # int64 labels with -1, as the trainer's validation pass collects them
    lab = np.where(miss, -1, y.astype(np.int64))
    assert T.EpochMetric("multilabel_classification", "none").cal_metric(lab, p)["log_loss"] == pytest.approx(
        float(np.mean([T._log_loss(y[~miss[:, c], c], p[~miss[:, c], c]) for c in range(3)])), rel=1e-12)
    # no measured entry anywhere: the mean of nothing, NaN (the reference's np.mean([]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert np.isnan(T.EpochMetric("multilabel_classification", "log_loss").cal_metric(np.full((5, 2), -1.0), rng.random((5, 2)))["log_loss"])
    # binary classification with complete labels and regression are what they were
    yb, pb = y[:, :1], p[:, :1]
    assert T.EpochMetric("classification", "auc").cal_metric(yb, pb)["auc"] == T._auc(yb, pb)
    yr = rng.normal(size=(n, 2))
    yr[0, 0] = -1.0                                           # a regression target of -1 is a value, not a sentinel
    assert T.EpochMetric("regression", "mse").cal_metric(yr, p[:, :2])["mse"] == pytest.approx(float(np.mean((yr - p[:, :2]) ** 2)), rel=1e-12)


class GHMC_Loss:                                              # the look-alike of models/loss.py:98 that NNModel's table holds
    def __init__(self, bins=10, alpha=0.5, last=None):
        self._bins, self._alpha, self._last_bin_count = bins, alpha, last

    def __call__(self, x, t):
        raise AssertionError("the look-alike must not be called: the kernel replaces it")


def FocalLossWithLogits(y_pred, y_true, alpha=0.25, gamma=2.0):      # the FUNCTION NNModel passes (models/loss.py:257)
    raise AssertionError("the function must not be called: the kernel replaces it")


def test_trainer_loss_selection_table():
    from mmdti_hip import losses
    task = "multilabel_classification"
    tr = T.Trainer(task=task, metrics="none", use_cuda=False)
    # 1. a function named FocalLossWithLogits -> the focal kernel with the reference's defaults
    assert T._is_builtin_loss(FocalLossWithLogits, task)
    lf = tr._task_loss(FocalLossWithLogits)
    assert isinstance(lf, losses.FocalLossWithLogits) and (lf.alpha, lf.gamma) == (0.25, 2.0)
    assert tr._task_loss(FocalLossWithLogits) is lf
    # 2. a GHMC_Loss look-alike -> ONE GHMCLoss per Trainer, with its bins / alpha, seeded from its history
    seen = GHMC_Loss(bins=6, alpha=0.25, last=torch.arange(6.0))
    assert T._is_builtin_loss(seen, task)
    lg = tr._task_loss(seen)
    assert isinstance(lg, losses.GHMCLoss) and (lg.bins, lg.alpha) == (6, 0.25) and tr._task_loss(seen) is lg
    assert torch.equal(lg.last_bin_count, torch.arange(6.0))
    fresh = tr._task_loss(GHMC_Loss())
    assert fresh is not lg and (fresh.bins, fresh.alpha) == (10, 0.5) and fresh.last_bin_count is None
    assert T.Trainer(task=task, metrics="none", use_cuda=False)._task_loss(seen) is not lg          # (per Trainer)
    # 3. nn.BCEWithLogitsLoss() -> the engine's own BCE kernel (None: FineTuner's default for the task); a configured one is not it
    assert T._is_builtin_loss(torch.nn.BCEWithLogitsLoss(), task) and tr._task_loss(torch.nn.BCEWithLogitsLoss()) is None
    weighted = torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(3))
    assert not T._is_builtin_loss(weighted, task) and tr._task_loss(weighted) is weighted
    # 4. anything else stays the callable it is -- also a lambda, a differently named function, a GHM-named object without the fields
    other = lambda o, t: (o - t).abs().mean()      # noqa: E731
    assert not T._is_builtin_loss(other, task) and tr._task_loss(other) is other

    class Bare:
        pass
    Bare.__name__ = "GHMC_Loss"
    bare = Bare()
    assert not T._is_builtin_loss(bare, task) and tr._task_loss(bare) is bare
    # the objects of mmdti_hip.losses are recognised as themselves
    mine = losses.GHMCLoss(bins=8, alpha=0.75)
    assert T._is_builtin_loss(mine, task) and tr._task_loss(mine) is mine
    mine_f = losses.FocalLossWithLogits(alpha=0.5, gamma=1.5)
    assert tr._task_loss(mine_f) is mine_f
    # other tasks: the function name means nothing there
    assert not T._is_builtin_loss(FocalLossWithLogits, "regression")
    # GHMCLoss: state_dict round trip and reset, before any device is involved
    sd = lg.state_dict()
    assert sd["bins"] == 6 and torch.equal(sd["last_bin_count"], torch.arange(6.0))
    twin = losses.GHMCLoss(bins=6, alpha=0.25)
    twin.load_state_dict(sd)
    assert torch.equal(twin.last_bin_count, torch.arange(6.0))
    twin.reset()
    assert twin.last_bin_count is None
    with pytest.raises(ValueError):
        losses.GHMCLoss(bins=10).load_state_dict(sd)
    with pytest.raises(ValueError):
        losses.FocalLossWithLogits(gamma=0.0)


def test_loss_table_keys_map_to_the_loss_objects():
    from mmdti_hip import losses
    with pytest.raises(ValueError):
        losses.from_key("hinge")
    assert isinstance(losses.from_key("focal"), losses.FocalLossWithLogits) and isinstance(losses.from_key("ghm"), losses.GHMCLoss)


def test_multilabel_target_normalisation():
    """NaN -> -1 BEFORE the integer cast for a floating multilabel target (no reliance on what NaN converts to); an int64 target passes
    through bit-identically; the other tasks keep their rule."""
    t = torch.tensor([[0.0, 1.0, float("nan")], [float("nan"), -1.0, 1.0]])
    out = T.normalise_target("multilabel_classification", t)
    assert out.dtype == torch.int64 and out.tolist() == [[0, 1, -1], [-1, -1, 1]]
    assert torch.isnan(t).sum() == 2                                   # (the caller's tensor is not written)
    ti = torch.tensor([[0, 1, -1], [1, 0, 1]], dtype=torch.int64)
    oi = T.normalise_target("multilabel_classification", ti)
    assert oi.dtype == torch.int64 and torch.equal(oi, ti)
    assert T.normalise_target("classification", torch.tensor([1.0, 0.0])).dtype == torch.int64
    assert T.normalise_target("regression", torch.tensor([1, 2])).dtype == torch.float32
    assert T.normalise_target("repr", t) is None
    # through the Trainer's own entry point
    tr = T.Trainer(task="multilabel_classification", metrics="none", use_cuda=False)
    _, tgt = tr.decorate_torch_batch((torch.zeros(2, 3), t))
    assert tgt.tolist() == [[0, 1, -1], [-1, -1, 1]]
    _, tgt = tr.decorate_torch_batch((torch.zeros(2, 3), ti))
    assert torch.equal(tgt, ti)


def test_new_symbols_are_in_the_header():
    protos = _abi.parse_header()
    assert protos["mmdti_focal_logits_loss"][2] == ["stream", "logits", "target", "n", "alpha", "gamma", "loss", "dlogits"]
    assert protos["mmdti_ghmc_logits_loss"][2] == ["stream", "logits", "target", "n", "bins", "alpha", "state", "loss", "dlogits"]
    src = open(_abi.HEADER).read()
    assert "models/loss.py:233-276" in src and "models/loss.py:63-132" in src          # each cites the reference call site it replaces
