"""GPU tests of the multilabel focal / GHM task-loss kernels (mmdti_focal_logits_loss, mmdti_ghmc_logits_loss) and of what they buy the
step: no host synchronisation, HIP-graph capture, missing labels end to end.  The reference's own values come from
tests/golden/g11_multilabel_losses.npz alone."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O

import multilabel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK, C = "multilabel_classification", 12
# the band of the existing BCE-kernel test against torch (test_multilabel_classification_trains_with_ct_multi_and_bce)
BAND_VALUE, BAND_GRAD = 1e-6, 1e-7


def _model(task=TASK, odim=C, **kw):
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 2, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1, attn_dropout=0.1)
    torch.manual_seed(0)
    return mm.MM_Model.from_configs(odim, task, mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16, **kw).cuda()


def _ocfg():
    return O.ModelCfg(unimol=O.UniMolCfg(layers=2, dim=64, ffn=128, heads=8, K=16, vocab=31), roberta=O.RobertaCfg(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40),
                      cross=O.CrossCfg(dim=64, heads=4, ffn=128), task=TASK, output_dim=C)


def _batch(seed, missing=0.2, ragged=False, B=8):
    """-> (device inputs, int64 device target with about `missing` of the labels set to -1)"""
    batch, label = O.synth_batch(B, 10, 14, _ocfg(), seed=seed, ragged=ragged, n_labels=C)
    g = torch.Generator().manual_seed(1000 + seed)
    label = torch.where(torch.rand(label.shape, generator=g) < missing, torch.full_like(label, -1), label)
    return {k: v.cuda() for k, v in batch.items()}, label.cuda()


def closed_form_focal(lg, t, alpha=0.25, gamma=2.0):
    """The focal loss over the valid entries as plain tensor arithmetic: no boolean indexing, differentiable by autograd."""
    t = t.to(lg.dtype)
    valid = (t == 0) | (t == 1)
    p = torch.sigmoid(lg)
    q = torch.where(t == 1, p, 1 - p).clamp(1e-5, 1.0)
    return (torch.where(valid, -alpha * (1 - q) ** gamma * torch.log(q), torch.zeros_like(q))).sum() / valid.sum()


def masked_focal(lg, t):
    """The reference's style: select the valid entries with a boolean mask (a nonzero: a device-to-host synchronisation)."""
    t = t.float()
    mask = ~torch.isnan(t) & ((t == 0) | (t == 1))
    p, y = torch.sigmoid(lg)[mask], t[mask]
    q = torch.where(y == 1, p, 1 - p).clamp(1e-5, 1.0)
    return (-0.25 * (1 - q) ** 2 * torch.log(q)).mean()


def test_kernels_match_the_reference_fixture():
    """Focal and GHM against the reference's fp32 CPU results, value and gradient, every case.  Tolerance per case: the larger of the
    BCE-kernel band (1e-6 value, 1e-7 gradient) and 4 x the distance between the fixture and the float64 restatement -- the
    reference's own fp32 error; the factor covers another summation order.  The measured distances go to
    profiles/multilabel_loss_parity.json."""
    from mmdti_hip.functional import FocalLogitsLossFn
    from mmdti_hip.losses import GHMCLoss
    fx = R.load_fixture()
    report = {}
    failures = []

    def check(name, v, g, v_ref, g_ref, v64, g64):
        v_tol = max(BAND_VALUE, 4 * abs(float(v_ref) - v64))
        g_tol = max(BAND_GRAD, 4 * float(np.abs(g_ref.astype(np.float64) - g64).max()))
        v_err, g_err = abs(v - float(v_ref)), float(np.abs(g - g_ref).max())
        report[name] = dict(value=v, value_ref=float(v_ref), value_err=v_err, value_tol=v_tol, grad_err=g_err, grad_tol=g_tol,
                            ref_vs_float64_value=abs(float(v_ref) - v64), ref_vs_float64_grad=float(np.abs(g_ref.astype(np.float64) - g64).max()))
        print(name, report[name])
        if not (v_err <= v_tol and g_err <= g_tol):
            failures.append((name, report[name]))

    for name, x, t, v_ref, g_ref in R.focal_cases(fx):
        lg = torch.from_numpy(x).cuda().requires_grad_()
        v = FocalLogitsLossFn.apply(lg, torch.from_numpy(np.ascontiguousarray(t)).cuda())
        v.backward()
        g = lg.grad.cpu().numpy()
        if name == "focal_allmissing":
            # a NaN loss (the mean of nothing) and what the reference's autograd leaves: a zero gradient
            assert np.isnan(float(v)) and np.isnan(float(v_ref)) and np.array_equal(g, g_ref) and not g.any()
            report[name] = dict(value="nan", grad_abs_max=float(np.abs(g).max()))
            continue
        v64, g64, parts = R.focal_f64(x, t)
        check(name, float(v), g, v_ref, g_ref, v64, g64)
        assert not g[~parts["valid"]].any(), name                                  # exactly 0 at missing entries
    # GHM: one loss object over the trajectory; the device state after each call equals the reference's _last_bin_count exactly
    bins, alpha = int(fx["ghm_bins"]), float(fx["ghm_alpha"])
    loss = GHMCLoss(bins=bins, alpha=alpha)
    assert loss.last_bin_count is None
    last = None
    for k in range(fx["ghm_logits"].shape[0]):
        x, y = fx["ghm_logits"][k], fx["ghm_y"][k].astype(np.float32)
        lg = torch.from_numpy(x).cuda().requires_grad_()
        v = loss(lg, torch.from_numpy(y).cuda())
        v.backward()
        v64, g64, last = R.ghmc_f64(x, y, last, bins, alpha)
        check(f"ghm_call{k}", float(v), lg.grad.cpu().numpy(), fx["ghm_value"][k], fx["ghm_grad"][k], v64, g64)
        assert np.array_equal(loss.last_bin_count.cpu().numpy(), fx["ghm_last_bin_count"][k]), (k, loss.last_bin_count)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "multilabel_loss_parity.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    assert not failures, failures
    # state_dict round trip on the device, reset
    twin = GHMCLoss(bins=bins, alpha=alpha)
    twin.device_state("cuda:0")
    twin.load_state_dict(loss.state_dict())
    assert torch.equal(twin.last_bin_count, loss.last_bin_count)
    loss.reset()
    assert loss.last_bin_count is None


def test_kernels_off_the_reference_path():
    """What the fixture cannot hold: another gamma (the powf path) and GHM with missing labels (the reference raises there)."""
    from mmdti_hip.functional import FocalLogitsLossFn
    from mmdti_hip.losses import GHMCLoss
    from mmdti_hip import ops
    from mmdti_hip._abi import MMDTIError
    fx = R.load_fixture()
    # focal, gamma 1.5, alpha 0.4 against the float64 closed form evaluated by torch on the device; logits within +-6 keep q above
    # 2.4e-3, so an ulp of the sigmoid (6e-8) moves a term by under alpha * 6e-8 / q / count = 5e-8: inside the BCE band
    x = torch.from_numpy(fx["focal_s_logits"]).cuda().clamp(-6, 6)
    t = torch.from_numpy(np.where(fx["focal_s_miss"], -1, fx["focal_s_y"].astype(np.int64))).cuda()
    lk = x.clone().requires_grad_()
    vk = FocalLogitsLossFn.apply(lk, t, 0.4, 1.5)
    vk.backward()
    l64 = x.double().requires_grad_()
    v64 = closed_form_focal(l64, t, 0.4, 1.5)
    v64.backward()
    assert abs(float(vk) - float(v64)) < BAND_VALUE and float((lk.grad.double() - l64.grad).abs().max()) < BAND_GRAD
    assert not lk.grad[t == -1].any()
    # run-to-run: the same bits (one workgroup, fixed summation order)
    xw, tw = torch.from_numpy(fx["focal_w_logits"]).cuda(), torch.from_numpy(fx["focal_w_y"].astype(np.float32)).cuda()
    a, b = ops.focal_logits_loss(xw, tw), ops.focal_logits_loss(xw, tw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # GHM with missing labels over the fixture's (edge-clear) inputs: out of the histogram, zero weight and gradient, N stays n.
    # Bound: a fixed-order fp32 sum of 192 terms and about 16 roundings per term, (192 + 16) x 2^-24 = 1.3e-5 relative worst case.
    bins, alpha = int(fx["ghm_bins"]), float(fx["ghm_alpha"])
    loss, last = GHMCLoss(bins=bins, alpha=alpha), None
    miss = fx["focal_s_miss"]
    for k in range(3):
        xk = fx["ghm_logits"][k]
        yk = np.where(miss, np.float32("nan") if k % 2 else np.float32(-1), fx["ghm_y"][k].astype(np.float32)).astype(np.float32)
        lg = torch.from_numpy(xk).cuda().requires_grad_()
        v = loss(lg, torch.from_numpy(yk).cuda())
        v.backward()
        v64, g64, last = R.ghmc_f64(xk, yk, last, bins, alpha)
        g = lg.grad.cpu().numpy()
        assert abs(float(v) - v64) <= 1.3e-5 * abs(v64), (k, float(v), v64)
        assert (np.abs(g - g64) <= 1.3e-5 * np.abs(g64) + 1e-9).all() and not g[miss].any()
        assert np.array_equal(loss.last_bin_count.cpu().numpy().astype(np.float64), last) and last.sum() < xk.size
    # argument checks come before any launch
    with pytest.raises(MMDTIError):
        ops.focal_logits_loss(xw, tw, gamma=0.0)
    with pytest.raises(MMDTIError):
        ops.ghmc_logits_loss(xw, tw, torch.zeros(5, device="cuda"), bins=10)
    with pytest.raises(MMDTIError):
        ops.focal_logits_loss(xw, tw[:, :5].contiguous())


def test_finetuner_focal_kernel_equals_the_closed_form_callable():
    """FineTuner(loss_key='focal') against the same step with the closed-form callable as loss_func, on a batch with about 20 % of the
    labels missing: the band of the existing BCE pair (1e-6 on the task loss, 1e-5 on the total)."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.losses import FocalLossWithLogits, GHMCLoss
    dev, y = _batch(9, ragged=True)
    frac = float((y == -1).float().mean())
    assert 0.1 < frac < 0.3, frac
    m1, m2 = _model().eval(), _model().eval()
    m2.load_state_dict(m1.state_dict())
    t1 = FineTuner(m1, TASK, total_steps=10, loss_key="focal")
    assert isinstance(t1.task_loss, FocalLossWithLogits)
    o1 = t1.step(dev, y)
    o2 = FineTuner(m2, TASK, total_steps=10).step(dev, y, loss_func=closed_form_focal)
    print("focal kernel vs callable: task", float(o1.task_loss), float(o2.task_loss), "total", float(o1.loss), float(o2.loss))
    assert abs(float(o1.task_loss) - float(o2.task_loss)) < 1e-6 and abs(float(o1.loss) - float(o2.loss)) < 1e-5
    assert isinstance(FineTuner(_model().eval(), TASK, total_steps=10, loss_key="ghm").task_loss, GHMCLoss)
    with pytest.raises(ValueError):
        FineTuner(_model().eval(), TASK, total_steps=10, loss_key="hinge")
    with pytest.raises(ValueError):
        FineTuner(_model("regression", 1).eval(), "regression", total_steps=10, loss_key="focal")


def test_multilabel_step_has_no_host_synchronisation():
    """The multilabel step with the focal and with the GHM kernel, on targets holding -1, enqueues without the host ever waiting for the
    device; the same step with the reference-style masked callable does not (boolean-mask indexing is a nonzero)."""
    from mmdti_hip.trainer import FineTuner
    dev, y = _batch(7, ragged=True)
    assert (y == -1).any()
    for key in ("focal", "ghm"):
        tuner = FineTuner(_model().train(), TASK, total_steps=10, loss_key=key)
        for _ in range(2):
            tuner.step(dev, y)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = tuner.step(dev, y)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.isfinite(out.loss).item() and torch.isfinite(out.task_loss).item(), key
    tuner = FineTuner(_model().train(), TASK, total_steps=10)
    for _ in range(2):
        tuner.step(dev, y, loss_func=masked_focal)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            tuner.step(dev, y, loss_func=masked_focal)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("key", ["focal", "ghm"])
def test_graphed_step_with_multilabel_kernels_matches_eager(key):
    """graphed_step with the focal / GHM kernel replays three different batches of one shape and matches three eager steps from the
    same start (the band of test_graphed_step_matches_eager_and_redraws_dropout); GHM's device bin state after the replays is the
    eager run's -- the capture's warm-up steps leave no trace in it."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip import ops
    m1, m2 = _model().eval(), _model().eval()
    m2.load_state_dict(m1.state_dict())
    t1 = FineTuner(m1, TASK, learning_rate=1e-3, warmup_ratio=0.5, total_steps=6, max_norm=5.0, loss_key=key)
    t2 = FineTuner(m2, TASK, learning_rate=1e-3, warmup_ratio=0.5, total_steps=6, max_norm=5.0, loss_key=key)
    batches = [_batch(20 + i) for i in range(3)]
    assert len({tuple(b["src_tokens"].shape) for b, _ in batches}) == 1 and not torch.equal(batches[0][1], batches[1][1])
    try:
        for dev, y in batches:
            o1 = t1.step(dev, y)
            o2 = t2.graphed_step(dev, y)
            assert abs(float(o1.loss) - float(o2.loss)) <= 2e-4 * abs(float(o1.loss)) + 1e-6, (float(o1.loss), float(o2.loss))
            assert abs(float(o1.task_loss) - float(o2.task_loss)) <= 2e-4 * abs(float(o1.task_loss)) + 1e-6
        assert len(t2._graphs) == 1 and t2.sched_step == 3
        if key == "ghm":
            s1, s2 = t1.task_loss.device_state("cuda:0"), t2.task_loss.device_state("cuda:0")
            assert float(s1[-1]) == 1.0 and float(s1[:-1].sum()) > 0
            assert torch.equal(s1, s2), (s1, s2)
    finally:
        ops.seed_salt_reset()


def FocalLossWithLogits(y_pred, y_true, alpha=0.25, gamma=2.0):
    """Stands for the function the reference's NNModel passes (recognised by its name): the kernel runs in its place."""
    raise AssertionError("the Trainer must run the focal kernel, not the callable")


def test_trainer_fits_with_missing_labels_and_scores_the_valid_entries(tmp_path):
    """tasks.Trainer.fit_predict on the 12-label toy with 20 % of the labels blanked to NaN (float targets), the loss a function named
    FocalLossWithLogits, metrics='log_loss': the loss goes down, predictions are finite, every epoch's early-stopping score is the log
    loss over the valid entries of that epoch's predictions, and no step was skipped."""
    from mmdti_hip.tasks import Trainer
    from mmdti_hip.tasks import trainer as T
    rng = np.random.default_rng(3)
    samples = []
    for _ in range(48):
        na = int(rng.integers(4, 10))
        atoms = rng.choice(np.arange(4, 30), size=na)
        d = O.coords2unimol(atoms, rng.normal(0, 3.0, size=(na, 3)), 31)
        d["smile"] = "C" * int(rng.integers(3, 10))
        lab = np.array([float((atoms == 4 + c).any()) for c in range(C)], dtype=np.float32)
        lab[rng.random(C) < 0.2] = np.nan
        samples.append((d, lab))
    assert 0.1 < np.mean([np.isnan(l).mean() for _, l in samples]) < 0.3

    class _Tok:
        pad_token_id = 1

        def __call__(self, smiles, padding=True, truncation=True, return_tensors="pt"):
            L = max(len(s) for s in smiles) + 2
            ids = torch.ones(len(smiles), L, dtype=torch.long)
            att = torch.zeros(len(smiles), L, dtype=torch.long)
            for r, s in enumerate(smiles):
                ids[r, :len(s) + 2] = torch.tensor([0] + [5 + (ord(c) % 7) for c in s] + [2])
                att[r, :len(s) + 2] = 1
            return {"input_ids": ids, "attention_mask": att}

    model = _model(_tokenizer=_Tok())
    trainer = Trainer(save_path=str(tmp_path), task=TASK, metrics="log_loss", learning_rate=1e-3, batch_size=8, epochs=4, warmup_ratio=0.1,
                      patience=20, max_norm=5.0, use_cuda=True, use_amp=True, alpha=1, beta=0.1, seed=1)
    seen = []
    inner = trainer.metrics.cal_metric

    def recording(label, predict, **kw):
        seen.append((np.array(label), np.array(predict)))
        return inner(label, predict, **kw)
    trainer.metrics.cal_metric = recording
    y_pred = trainer.fit_predict(model, samples[:40], samples[40:], FocalLossWithLogits, torch.sigmoid, str(tmp_path), 0, None,
                                 return_infonce_loss=True, return_ct_loss=True, use_weight=False)
    assert y_pred.shape == (8, C) and np.isfinite(y_pred).all() and (y_pred >= 0).all() and (y_pred <= 1).all()
    hist = trainer.history
    assert len(hist) == 4 and len(seen) == 4
    first, last = hist[0]["steps"][:, 1].mean(), hist[-1]["steps"][:, 1].mean()
    assert np.isfinite(hist[-1]["steps"]).all() and last < first, (first, last)
    assert all(h["skipped"] == 0 for h in hist) and all(np.isfinite(h["val_loss"]) for h in hist)
    truth = np.stack([l for _, l in samples[40:]])
    for h, (label, predict) in zip(hist, seen):
        assert label.dtype == np.int64 and np.array_equal(label == -1, np.isnan(truth)) and np.array_equal(label[label != -1], truth[~np.isnan(truth)].astype(np.int64))
        cols = []
        for c in range(C):
            ok = ~np.isnan(truth[:, c])
            if ok.any():
                cols.append(T._log_loss(truth[ok, c], predict[ok, c]))
        assert h["metric"] == "log_loss" and h["score"] == pytest.approx(float(np.mean(cols)), rel=1e-12), (h["score"], float(np.mean(cols)))
