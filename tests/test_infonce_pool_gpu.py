"""InfoNCE(pool="real") / MM_Model(infonce_pool="real") on the GPU: the head pools over the real tokens, so nothing in the model reads
a padded row -- the module against the oracle-composed restatement (tests/infonce_pool_ref.py); the packed step (pad-free packed rows)
against the padded step; the loss against the padded length; the automatic layout; training with dropout on; graphed_step; and the
unset switch, which must not move a bit.  Step tests run the reference's widths at reduced depth (test_packed_gpu._small_refarch)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import mmdti_oracle as O
from g9util import refarch_cfg, product_model, load_fixture_weights, rel_l2
from test_modules_gpu import M, T, check, compare_param_grads, grads_of          # noqa: F401  (fixture + helpers)
from test_packed_gpu import _small_refarch, _host_fields

import infonce_pool_ref as R

# analytically zero gradients (softmax shift invariance): rounding noise in every run -- the exclusions of
# test_packed_gpu.test_packed_step_equals_padded_step_at_dropout_zero
ZERO = ("pooler", "key.bias", "gbf_proj.linear2.bias")


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.parametrize("order", ["pool_then_project", "project_then_pool"])
def test_infonce_module_pools_over_real_tokens(M, golden, order, monkeypatch):
    """The G2 fixture's inputs under prefix masks against the restatement in the oracle's bf16 mode: the bands of
    test_infonce_module_golden for the same comparison.  Masked positions receive an input gradient of exactly 0."""
    from mmdti_hip import functional, ops
    monkeypatch.setattr(functional, "POOL_THEN_PROJECT", order == "pool_then_project")
    if order == "project_then_pool":
        # (this order's second GEMM multiplies the bf16 GELU outputs by the bf16 weight shadow in every precision mode, where the oracle's
        #  fp16 mode rounds both to fp16: the oracle states this order's arithmetic in its bf16 mode only -- so both sides run in it)
        monkeypatch.setattr(ops, "FWD_F16", False)
        O.set_forward_fp16(False)
    g = golden("g2_infonce_module_train_p0")
    mod = M.inf.InfoNCE(64, 64, pool="real").cuda()
    P = {"infonce." + k[2:]: T(v).clone().requires_grad_() for k, v in g.items() if k.startswith("w_")}
    mod.load_state_dict({k[len("infonce."):]: v.detach() for k, v in P.items()}, strict=True)
    mod.train(); mod.embed_dropout = 0.0
    xq, xk = T(g["xq"]).cuda().requires_grad_(), T(g["xk"]).cuda().requires_grad_()
    B, Sq, Sk = xq.shape[0], xq.shape[1], xk.shape[1]
    lq = torch.tensor([1 + (5 * b) % Sq for b in range(B)]); lq[-1] = Sq
    lk = torch.tensor([1 + (3 * b + 2) % Sk for b in range(B)]); lk[0] = Sk
    mq, mk = torch.arange(Sq).view(1, -1) < lq.view(-1, 1), torch.arange(Sk).view(1, -1) < lk.view(-1, 1)
    loss = mod(xq, xk, query_mask=mq.cuda(), key_mask=mk.cuda())
    loss.backward()
    xqo, xko = T(g["xq"]).requires_grad_(), T(g["xk"]).requires_grad_()
    lo = R.infonce_forward_real(xqo, xko, mq, mk, P, p=0.0, bf16=True)
    print("loss", order, float(loss.detach()), float(lo.detach()))
    assert abs(float(loss.detach()) - float(lo.detach())) <= 3e-4 * abs(float(lo.detach())) + 1e-5
    lo.backward()
    check(xq.grad, xqo.grad, 5e-2, "dxq"); check(xk.grad, xko.grad, 5e-2, "dxk")
    compare_param_grads(grads_of(mod, "infonce."), P, 6e-2)
    assert float(xq.grad[~mq.cuda()].abs().max()) == 0.0 and float(xk.grad[~mk.cuda()].abs().max()) == 0.0
    # the same sequences as pad-free packed rows: the same loss (pool-then-project: bit for bit, the pooled sums are)
    from mmdti_hip.packing import PackedRows
    pq, pk = PackedRows(lq, Sq, device="cuda", pad_row=False), PackedRows(lk, Sk, device="cuda", pad_row=False)
    packed = mod(pq.pack(xq.detach()), pk.pack(xk.detach()), packs=(pq, pk))
    assert abs(float(packed.detach()) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))
    with pytest.raises(ValueError):
        mod(xq, xk)                                                                  # pool="real" without masks
    with pytest.raises(ValueError):
        M.inf.InfoNCE(64, 64)(pq.pack(xq.detach()), pk.pack(xk.detach()), packs=(pq, pk))      # pool="all" on a pad-free pack


@pytest.mark.parametrize("form", ["all_padded", "real_packed"])
def test_infonce_project_then_pool_forms_no_other_test_reaches(M, form, monkeypatch):
    """The two forms of InfoNCEFn that no test above and no step test runs forward AND backward, both in the project-then-pool order:
    the mean over all positions of padded rows, and the mean over the real positions of pad-free packed rows.  3 sequences of 1, 5 and 9
    tokens in S = 9, width 16, hidden 24, d_l = 10 (ldp = 16); the references and bands of the module tests: O.infonce_forward
    (test_infonce_module_golden) / R.infonce_forward_real (above), both in the oracle's bf16 mode.  The order is chosen by the switch, as
    above: a hidden width that is no multiple of 8 (20, say) cannot run it -- mmdti_gemm_bf16 refuses its row stride ("lda/ldb must be
    multiples of 8 elements"), before and after InfoNCEFn's two projections became one."""
    from mmdti_hip import functional, ops
    from mmdti_hip.packing import PackedRows
    monkeypatch.setattr(functional, "POOL_THEN_PROJECT", False)
    monkeypatch.setattr(ops, "FWD_F16", False)               # (this order is stated in the oracle's bf16 mode only, see above)
    O.set_forward_fp16(False)
    B, S, D, Hd, d = 3, 9, 16, 24, 10
    mod = M.inf.InfoNCE(D, D, pool="real" if form == "real_packed" else "all")
    mod.d_l = mod.d_av = d
    torch.manual_seed(7)
    for name in ("info_proj_query", "info_proj_positive"):
        setattr(mod, name, torch.nn.Sequential(torch.nn.Linear(D, Hd), torch.nn.GELU(), torch.nn.Linear(Hd, d)))
    mod = mod.cuda()
    mod.train(); mod.embed_dropout = 0.0
    P = {"infonce." + k: v.detach().cpu().clone().requires_grad_() for k, v in mod.state_dict().items()}
    x = torch.randn(2, B, S, D)
    xq, xk = x[0].clone().cuda().requires_grad_(), x[1].clone().cuda().requires_grad_()
    xqo, xko = x[0].clone().requires_grad_(), x[1].clone().requires_grad_()
    lens = torch.tensor([1, 5, 9])
    mask = torch.arange(S).view(1, -1) < lens.view(-1, 1)
    if form == "real_packed":
        pq, pk = PackedRows(lens, S, device="cuda", pad_row=False), PackedRows(lens, S, device="cuda", pad_row=False)
        loss = mod(pq.pack(xq), pk.pack(xk), packs=(pq, pk))
        lo = R.infonce_forward_real(xqo, xko, mask, mask, P, p=0.0, bf16=True)
    else:
        loss = mod(xq, xk)
        lo = O.infonce_forward(xqo, xko, P, p=0.0, bf16=True)
    print("loss", form, float(loss.detach()), float(lo.detach()))
    assert abs(float(loss.detach()) - float(lo.detach())) <= 3e-4 * abs(float(lo.detach())) + 1e-5
    loss.backward()
    lo.backward()
    check(xq.grad, xqo.grad, 5e-2, "dxq"); check(xk.grad, xko.grad, 5e-2, "dxk")
    compare_param_grads(grads_of(mod, "infonce."), P, 6e-2)
    if form == "real_packed":
        assert float(xq.grad[~mask.cuda()].abs().max()) == 0.0 and float(xk.grad[~mask.cuda()].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ steps
def _loss_and_grads(model, d, host, tgt, task):
    from mmdti_hip.functional import CELossFn, MSELossFn
    model.zero_grad(set_to_none=True)
    logits, infonce, ct = model(**d, **host, return_infonce_loss=True, return_ct_loss=True, net_target=tgt)
    tl = MSELossFn.apply(logits, tgt) if task == "regression" else CELossFn.apply(logits, tgt)
    loss = tl + 0.1 * infonce + 0.1 * ct
    loss.backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), infonce=float(infonce), ct=float(ct), loss=float(loss),
                grads={n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})


def _assert_same_step(a, b, what):
    """the bands of test_packed_step_equals_padded_step_at_dropout_zero (a: the run compared against)"""
    for k in ("infonce", "ct", "loss"):
        rel = 3e-5 if k == "ct" else 1e-6
        print(what, k, a[k], b[k], abs(a[k] - b[k]) / max(abs(a[k]), 1e-30))
        assert abs(a[k] - b[k]) <= rel * abs(a[k]) + 1e-7, (what, k, a[k], b[k])
    r = rel_l2(b["logits"], a["logits"])
    print(what, "logits", r)
    assert r < 1e-6, (what, r)
    assert set(a["grads"]) == set(b["grads"])
    worst = ("", 0.0)
    for n in a["grads"]:
        if float(a["grads"][n].abs().max()) < 1e-9 or any(z in n for z in ZERO):
            continue
        r = rel_l2(b["grads"][n], a["grads"][n])
        worst = max(worst, (n, r), key=lambda t: t[1])
        assert r < (4e-2 if n.startswith(("gbf.", "gbf_proj.")) else 6e-3), (what, n, r)
    print(what, "worst gradient", worst)


def _setup(task, **params):
    ocfg, model = _small_refarch(task, **params)
    load_fixture_weights(model, O.init_params(ocfg, seed=5, std=0.05))
    model.train()                                                                    # every dropout probability is 0
    batch, label = O.synth_batch(7, 40, 48, ocfg, seed=11, ragged=True)
    tgt = label.cuda().float() if task == "regression" else label.cuda().long()
    return ocfg, model, batch, tgt


@pytest.mark.parametrize("task", ["classification", "regression"])
def test_packed_step_is_the_padded_step_and_has_no_pad_rows(task):
    """(a) same weights, same mixed-length batch, dropout 0, infonce_pool="real": packed rows against padded rows."""
    ocfg, model, batch, tgt = _setup(task, infonce_pool="real")
    host = _host_fields(batch)
    d = {k: v.cuda() for k, v in batch.items()}
    res = {}
    for layout in ("padded", "packed"):
        model.strict_reference = layout == "padded"
        res[layout] = _loss_and_grads(model, d, host, tgt, task)
        assert model.last_layout == layout
    pk1, pk2 = model._pack_cache[3]
    assert not pk1.pad_row and not pk2.pad_row and pk1.n_pad_rows == 0 and pk2.n_pad_rows == 0
    assert pk1.M == int(host["atom_counts"].sum()) and pk2.M == int(host["token_counts"].sum())
    assert pk1.M < batch["src_tokens"].numel() and pk2.M < batch["input_ids"].numel()
    _assert_same_step(res["padded"], res["packed"], f"{task}: packed vs padded")


def _pad_further(batch, ocfg, extra=16):
    """the same molecules collated `extra` positions further, each field with the value the collate function pads it with"""
    u, r = ocfg.unimol, ocfg.roberta
    return {"src_tokens": F.pad(batch["src_tokens"], (0, extra), value=u.pad_idx),
            "src_distance": F.pad(batch["src_distance"], (0, extra, 0, extra), value=0.0),
            "src_edge_type": F.pad(batch["src_edge_type"], (0, extra, 0, extra), value=u.pad_idx),
            "input_ids": F.pad(batch["input_ids"], (0, extra), value=r.pad_idx),
            "attention_mask": F.pad(batch["attention_mask"], (0, extra), value=0)}


def test_loss_does_not_depend_on_the_padded_length():
    """(b) the same molecules collated to N and N + 16 atoms, L and L + 16 tokens, dropout 0: under "real" losses and gradients agree
    in both layouts; under "all" the InfoNCE loss moves (the quirk of infonce.py:32-33), far above the band -- so the test bites."""
    task = "classification"
    ocfg, model, batch, tgt = _setup(task, infonce_pool="real")
    wide = _pad_further(batch, ocfg)
    assert wide["src_tokens"].shape[1] == batch["src_tokens"].shape[1] + 16 and wide["input_ids"].shape[1] == batch["input_ids"].shape[1] + 16
    assert torch.equal(_host_fields(wide)["atom_counts"], _host_fields(batch)["atom_counts"])
    for layout in ("padded", "packed"):
        model.strict_reference = layout == "padded"
        res = []
        for b in (batch, wide):
            res.append(_loss_and_grads(model, {k: v.cuda() for k, v in b.items()}, _host_fields(b), tgt, task))
            assert model.last_layout == layout
        _assert_same_step(res[0], res[1], f"{layout}: N + 16 vs N")
    ocfg, every, _, _ = _setup(task, infonce_pool="all")
    every.strict_reference = True
    a, b = (_loss_and_grads(every, {k: v.cuda() for k, v in bt.items()}, _host_fields(bt), tgt, task) for bt in (batch, wide))
    print("pool=all: infonce", a["infonce"], b["infonce"])
    assert abs(a["infonce"] - b["infonce"]) > 100 * (1e-6 * abs(a["infonce"]) + 1e-7)


def test_auto_layout_packs_in_training_only_under_real():
    """(c) the reference's dropout on, strict_reference=None: packed rows under "real" (nothing reads a padded row), padded rows under
    "all" (today's behaviour: the padded rows keep their own dropout masks)."""
    ocfg = refarch_cfg("classification", 600)
    ocfg.unimol.layers, ocfg.roberta.layers = 2, 2
    batch, label = O.synth_batch(7, 40, 48, ocfg, seed=11, ragged=True)
    d, host = {k: v.cuda() for k, v in batch.items()}, _host_fields(batch)
    for pool, layout in (("real", "packed"), ("all", "padded")):
        model = product_model(ocfg, dropout=True, infonce_pool=pool).cuda().train()
        assert model.strict_reference is None and model.pad_row_dropout_live() == (pool == "all")
        out = model(**d, **host, return_infonce_loss=True, return_ct_loss=True, net_target=label.cuda().long())
        assert model.last_layout == layout and all(bool(torch.isfinite(o).all()) for o in out)
        model.eval()
        with torch.no_grad():
            model(**d, **host)
        assert model.last_layout == "packed"


def test_real_pool_trains_with_dropout_on_in_both_layouts():
    """(d) six optimizer steps with the reference's dropout, "real": padded rows against packed rows (the automatic layout).  The
    two layouts share a distribution; the draws differ (the masks are indexed by row), so the bands are those of
    test_packed_step_trains_with_dropout_on."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.runtime import dropout_state
    ocfg = refarch_cfg("classification", 600)
    ocfg.unimol.layers, ocfg.roberta.layers = 2, 2
    batch, label = O.synth_batch(8, 40, 48, ocfg, seed=21, ragged=True)
    d = dict({k: v.cuda() for k, v in batch.items()}, **_host_fields(batch))
    traj = {}
    for layout in ("padded", "packed"):
        dropout_state.reseed(20240607)
        model = product_model(ocfg, dropout=True, infonce_pool="real", strict_reference=True if layout == "padded" else None).cuda().train()
        load_fixture_weights(model, O.init_params(ocfg, seed=5, std=0.05))
        tuner = FineTuner(model, "classification", learning_rate=2e-4, total_steps=100)
        outs = [tuner.step(d, label.cuda()) for _ in range(6)]
        assert model.last_layout == layout
        traj[layout] = [(float(o.loss), float(o.infonce_loss)) for o in outs]
        assert all(math.isfinite(x) for t in traj[layout] for x in t)
    mean = {k: np.mean(np.array(v), axis=0) for k, v in traj.items()}
    print("trajectories", traj)
    assert np.all(np.abs(mean["padded"] - mean["packed"]) < 0.12 * np.abs(mean["padded"])), (mean, traj)
    for (la, ia), (lb, ib) in zip(traj["padded"], traj["packed"]):
        assert abs(la - lb) < 0.4 * abs(la) and abs(ia - ib) < 0.4 * abs(ia), traj


def test_graphed_step_captures_and_replays_under_real():
    """(e) graphed_step keeps the padded layout and takes the masked mean from the device masks (no host value): it captures, replays
    two different ragged batches of one shape, and matches the eager padded step within the band of
    test_graphed_step_runs_any_ragged_batch_of_the_captured_shape_and_mixes_with_eager_steps."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.collate import device_payload, to_device
    from mmdti_hip import ops
    ocfg = refarch_cfg("classification", 600)
    ocfg.unimol.layers, ocfg.roberta.layers = 2, 2
    m1 = product_model(ocfg, infonce_pool="real").cuda().train()
    m2 = product_model(ocfg, infonce_pool="real", strict_reference=True).cuda().train()
    load_fixture_weights(m1, O.init_params(ocfg, seed=5, std=0.05))
    m2.load_state_dict(m1.state_dict())
    b1, y1 = O.synth_batch(7, 40, 48, ocfg, seed=31, ragged=True)
    b2, y2 = {k: v.flip(0).contiguous() for k, v in b1.items()}, y1.flip(0).contiguous()
    t1 = FineTuner(m1, "classification", learning_rate=1e-3, warmup_ratio=0.5, total_steps=8, max_norm=5.0)
    t2 = FineTuner(m2, "classification", learning_rate=1e-3, warmup_ratio=0.5, total_steps=8, max_norm=5.0)
    try:
        for i, (b, y) in enumerate(((b1, y1), (b2, y2), (b1, y1))):
            dev = to_device(device_payload(b), "cuda")
            o1 = t1.graphed_step(dev, y.cuda())
            assert m1.last_layout == "padded"
            o2 = t2.step(dev, y.cuda())
            print("graphed vs eager", i, float(o1.loss), float(o2.loss), float(o1.infonce_loss), float(o2.infonce_loss))
            assert abs(float(o1.loss) - float(o2.loss)) <= 3e-4 * abs(float(o2.loss)) + 1e-6, (i, float(o1.loss), float(o2.loss))
            assert abs(float(o1.infonce_loss) - float(o2.infonce_loss)) <= 3e-4 * abs(float(o2.infonce_loss)) + 1e-6
        assert len(t1._graphs) == 1
    finally:
        ops.seed_salt_reset()


def test_unset_switch_moves_no_bit_and_never_reaches_the_new_entry_points(monkeypatch):
    """(f) a model built with the switch unset against one built with infonce_pool="all", deterministic mode: loss, logits and every
    gradient are torch.equal, in both layouts; ops.seq_mean_real_* are never called."""
    from mmdti_hip import ops
    monkeypatch.delenv("MMDTI_INFONCE_POOL", raising=False)
    calls = []
    for name in ("seq_mean_real_fwd", "seq_mean_real_bwd"):
        orig = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _o=orig, _n=name, **k: (calls.append(_n), _o(*a, **k))[1])
    task = "classification"
    ocfg, unset, batch, tgt = _setup(task)
    _, named, _, _ = _setup(task, infonce_pool="all")
    assert unset.infonce_pool == named.infonce_pool == "all"
    d, host = {k: v.cuda() for k, v in batch.items()}, _host_fields(batch)
    ops.set_deterministic(True)
    try:
        for strict in (True, False):
            unset.strict_reference = named.strict_reference = strict
            a, b = _loss_and_grads(unset, d, host, tgt, task), _loss_and_grads(named, d, host, tgt, task)
            assert unset.last_layout == named.last_layout == ("padded" if strict else "packed")
            assert a["loss"] == b["loss"] and a["infonce"] == b["infonce"] and a["ct"] == b["ct"] and torch.equal(a["logits"], b["logits"])
            assert set(a["grads"]) == set(b["grads"]) and all(torch.equal(a["grads"][n], b["grads"][n]) for n in a["grads"])
    finally:
        ops.set_deterministic(False)
    assert calls == []
    # ... and the spy does see them under "real"
    real = _setup(task, infonce_pool="real")[1]
    real.strict_reference = True
    _loss_and_grads(real, d, host, tgt, task)
    assert calls.count("seq_mean_real_fwd") == 2 and calls.count("seq_mean_real_bwd") == 2
