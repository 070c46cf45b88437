"""pair_inputs="coords" on the GPU: the materialising kernel against the host statement of the pair rule, the fused coords kernels
bit for bit against "materialise, then the planes kernel", the hot-path model, the reference fixtures run from their stored
coordinates, the Trainer and a captured step."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from g9util import (T, samples_from, tiny_cfg, zero_dropout_cfg, tokenizer_from, product_model, load_fixture_weights, rel_l2, cosine, host_fields,
                    REF_U, REF_C)

V, PAD, E = 31, 0, 31 * 31
PLANES = ("src_distance", "src_edge_type")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mmdti_hip import ops as _ops
    return _ops


def G(seed):
    return torch.Generator().manual_seed(seed)


def _molecules(N, seed, nan_pads=True):
    """B = 3 ragged molecules padded to N: one of 2 tokens (bos + eos only, the reference's failed-conformer case), one of full length,
    one in between; coordinates ~ N(0, 3 A) centred, one pair of coincident atoms in the longest; pad slots hold NaN coordinates."""
    gen = G(seed)
    lens = [2, N, max(3, (N + 1) // 2)]
    coord = torch.full((3, N, 3), float("nan") if nan_pads else 0.0)
    tok = torch.full((3, N), PAD, dtype=torch.int64)
    for b, n in enumerate(lens):
        c = torch.randn(n, 3, generator=gen) * 3.0
        c = c - c.mean(0)
        if n >= 4:
            c[n - 2] = c[1]                          # coincident atoms
        if n == 2:
            c[:] = 0.0                               # the two specials sit at the origin (data/conformer.py)
        coord[b, :n] = c
        tok[b, :n] = torch.randint(4, V, (n,), generator=gen)
        tok[b, 0], tok[b, n - 1] = 1, 2
    return coord, tok, lens


@pytest.mark.parametrize("N", [5, 16, 17, 130, 272])
def test_materialiser_matches_the_host_rule(ops, N):
    from mmdti_hip.collate import pair_inputs_from_coords
    coord, tok, lens = _molecules(N, 100 + N)
    ref_d, ref_e = pair_inputs_from_coords(coord, tok, V, PAD)
    c64 = coord.double()
    diff = c64.unsqueeze(-2) - c64.unsqueeze(-3)
    d64 = (diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2).sqrt()
    padp = tok.eq(PAD).unsqueeze(-1) | tok.eq(PAD).unsqueeze(-2)
    d64 = d64.masked_fill(padp, 0.0)
    for edt in (torch.int16, torch.int64):
        d, e = ops.pair_inputs_from_coords(coord.cuda(), tok.cuda(), V, PAD, edt)
        assert e.dtype == edt and d.dtype == torch.float32 and d.shape == (3, N, N)
        assert torch.equal(e.cpu().long(), ref_e)                                    # exact, both widths
        d = d.cpu()
        assert bool(torch.isfinite(d).all())                                         # NaN coordinates of pad slots do not leak
        # within 4 ulp of the float64 value: the chain (3 subtractions, dx * dx, 2 fma, sqrt) rounds at most to 3 * 2^-24 relative,
        # one ulp is at most 2^-23 relative
        pos = d64 > 0
        ulp = torch.exp2(torch.floor(torch.log2(d64[pos])) - 23)
        worst = float(((d.double()[pos] - d64[pos]).abs() / ulp).max())
        print(f"N={N} {edt}: worst distance error {worst:.3f} ulp; {int((d != ref_d).sum())} of {d.numel()} differ from the once-rounded float64 value")
        assert worst <= 4.0, worst
        # exact zeros: diagonal, the coincident pair, every pad slot
        assert bool((d[~pos] == 0).all())
        assert bool((torch.diagonal(d, dim1=1, dim2=2) == 0).all())
        n = lens[1]
        assert float(d[1, n - 2, 1]) == 0.0 and float(d[1, 1, n - 2]) == 0.0 and float(d[0, 0, 1]) == 0.0
        assert bool((d[padp] == 0).all()) and bool((e.cpu().long()[padp] == PAD).all())


def _gbf_params(seed):
    K, Fh, H = 128, 128, 64
    gen = G(seed)
    mul, bias = 1 + 0.1 * torch.randn(E, generator=gen), 0.1 * torch.randn(E, generator=gen)
    means, stds = torch.rand(K, generator=gen) * 3, torch.rand(K, generator=gen) * 3 - 1.5
    w1, b1 = (torch.randn(Fh, K, generator=gen) * 0.2).bfloat16(), torch.randn(Fh, generator=gen) * 0.1
    w2, b2 = (torch.randn(H, Fh, generator=gen) * 0.2).bfloat16(), torch.randn(H, generator=gen) * 0.1
    return [t.cuda() for t in (mul, bias, means, stds)], w1.cuda(), b1.cuda(), w2.cuda(), b2.cuda()


def _prefixes(ops, lens, N, packed):
    kt = torch.tensor([(n + 15) // 16 for n in lens])
    if packed:
        rows = torch.tensor([min(n + 1, N) for n in lens])          # real tokens + one representative pad row (packing.PackedRows.rows_host)
        return ops.gbf_tile_prefixes(kt, N, "cuda", rows)
    pf, pb = ops.gbf_tile_prefixes(kt, N, "cuda")
    return pf, pb, None, None


LAYOUTS = [("rowmajor", False, False, None), ("tiled", True, False, None), ("compact", True, True, None), ("tiled_prefix", True, False, "prefix"),
           ("compact_prefix", True, True, "prefix"), ("compact_rows", True, True, "rows")]


@pytest.fixture
def zeroed_planes(ops, monkeypatch):
    """Pair tensors start as zeros: with tile_prefix the kernels leave the all-padding tiles unwritten, and torch.equal reads every slot."""
    real = ops.pair_empty
    monkeypatch.setattr(ops, "pair_empty", lambda *a, **k: real(*a, **dict(k, zero=True)))


@pytest.mark.parametrize("name,tiled,compact,rag", LAYOUTS, ids=[l[0] for l in LAYOUTS])
@pytest.mark.parametrize("N", [17, 130])
def test_fused_forward_coords_is_the_planes_kernel_on_materialised_planes(ops, zeroed_planes, N, name, tiled, compact, rag):
    coord, tok, lens = _molecules(N, 200 + N)
    tabs, w1, b1, w2, b2 = _gbf_params(31)
    ld = ops.pair_ld(N)
    rec = ops.pair_records(coord.cuda(), tok.cuda())
    pf = rb = None
    if rag:
        pf, _, rb, _ = _prefixes(ops, lens, N, rag == "rows")
    out_c = ops.gbf_bias_fwd_coords(rec, V, PAD, *tabs, w1, b1, w2, b2, ld, tiled=tiled, compact=compact, tile_prefix=pf, row_blocks=rb)
    for edt in (torch.int16, torch.int64):
        dist, et = ops.pair_inputs_from_records(rec, V, PAD, edt)
        out_p, _ = ops.gbf_bias_fwd(dist, et, *tabs, w1, b1, w2, b2, ld, save=False, tiled=tiled, compact=compact, tile_prefix=pf, row_blocks=rb)
        assert out_c.dtype == out_p.dtype == (torch.float16 if compact else torch.float32)
        assert torch.equal(out_c, out_p), (name, N, edt)
    assert bool(torch.isfinite(out_c.float()[out_c.float() != float("-inf")]).all())          # (NaN pad coordinates reach nothing)


GRADS = ("dw1", "db1", "dw2", "db2", "dmul", "dbias", "dmeans", "dstds")
GSHAPES = ((128, 128), (128,), (64, 128), (64,), (E,), (E,), (128,), (128,))
BWD_LAYOUTS = [l for l in LAYOUTS if l[0] != "compact_prefix"]


@pytest.mark.parametrize("det", [True, False], ids=["deterministic", "default"])
@pytest.mark.parametrize("name,tiled,compact,rag", BWD_LAYOUTS, ids=[l[0] for l in BWD_LAYOUTS])
@pytest.mark.parametrize("N", [17, 130])
def test_complete_backward_coords_against_planes(ops, N, name, tiled, compact, rag, det):
    coord, tok, lens = _molecules(N, 300 + N)
    tabs, w1, b1, w2, b2 = _gbf_params(37)
    ld, H = ops.pair_ld(N), 64
    gen = G(41)
    g_std = torch.zeros(3, H, N, ld); g_std[..., :N] = torch.randn(3, H, N, N, generator=gen)
    g = ops.pair_tile(g_std.cuda(), N, 0.0) if tiled else g_std.cuda()
    if compact:
        g = g.to(torch.bfloat16)
    pb = rbb = None
    if rag:
        _, pb, _, rbb = _prefixes(ops, lens, N, rag == "rows")
    rec = ops.pair_records(coord.cuda(), tok.cuda())
    dist, et = ops.pair_inputs_from_records(rec, V, PAD, torch.int16)
    ops.set_deterministic(det)
    try:
        got_c = {n: torch.full(sh, 0.5, device="cuda") for n, sh in zip(GRADS, GSHAPES)}       # (non-zero: the kernels accumulate)
        got_p = {n: torch.full(sh, 0.5, device="cuda") for n, sh in zip(GRADS, GSHAPES)}
        ops.gbf_bias_bwd_full_coords(g, rec, V, PAD, *tabs, w1, b1, w2, ld, *[got_c[n].view(-1) for n in GRADS], tile_prefix=pb, row_blocks=rbb)
        ops.gbf_bias_bwd_full(g, dist, et, *tabs, w1, b1, w2, ld, *[got_p[n].view(-1) for n in GRADS], tile_prefix=pb, row_blocks=rbb)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    for n in GRADS:
        a, b_ = got_c[n] - 0.5, got_p[n] - 0.5
        assert bool(torch.isfinite(a).all()) and float(b_.abs().max()) > 0, n
        if det:
            assert torch.equal(got_c[n], got_p[n]), (n, name, N)
        else:
            # the band test_gbf_bias_complete_backward_matches_chain_and_autograd holds this kernel to (its LDS histogram atomics scatter at 1e-7)
            r = float((a - b_).norm() / (b_.norm() + 1e-12))
            print(f"{name} N={N} {n}: coords vs planes rel l2 {r:.2e}")
            assert r < (2e-2 if n in ("dmul", "dbias", "dmeans", "dstds") else 6e-3), (n, r)


# ------------------------------------------------------------------------------------------------ the hot-path model
def _hot_cfg(task="classification"):
    return zero_dropout_cfg(dict(REF_U, layers=2), dict(layers=1, dim=512, heads=8, ffn=1024, vocab=40, max_pos=40), REF_C, task, 2)


class _Spy:
    """Counts the launches of the pair-bias entry points of ops and remembers every [B,N,N] tensor handed to one of them."""

    NAMES = ("gbf_bias_fwd", "gbf_bias_bwd_full", "gbf_bias_bwd", "gbf_features_fwd", "gbf_bias_fwd_coords", "gbf_bias_bwd_full_coords",
             "pair_inputs_from_records")

    def __init__(self, ops, monkeypatch):
        self.calls = {n: 0 for n in self.NAMES}
        self.squares = 0
        for n in self.NAMES:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.calls[name] += 1
            self.squares += sum(1 for t in a if torch.is_tensor(t) and t.dim() == 3 and t.shape[1] == t.shape[2] and t.dtype != torch.int32)
            return fn(*a, **k)
        return f

    def reset(self):
        self.calls = {n: 0 for n in self.NAMES}
        self.squares = 0


def _step(model, batch, tgt):
    from mmdti_hip.functional import CELossFn
    for p in model.parameters():
        p.grad = None
    logits, infonce, ct = model(**batch, return_infonce_loss=True, return_ct_loss=True, net_target=tgt, use_weight=False)
    task = CELossFn.apply(logits, tgt)
    loss = task + 0.1 * infonce + 0.1 * ct
    loss.backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), task=task.detach().clone(), infonce=infonce.detach().clone(), ct=ct.detach().clone(),
                loss=loss.detach().clone()), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layout", ["padded", "packed"])
def test_hot_path_model_coords_step_is_the_planes_step(ops, monkeypatch, layout):
    from mmdti_hip.synth import synth_batch
    torch.manual_seed(7)
    model = product_model(_hot_cfg(), strict_reference=layout == "padded").cuda().train()
    cpu, label = synth_batch(4, 32, 14, seed=77, ragged=True, smiles_vocab=40, with_coord=True)
    B, N = cpu["src_tokens"].shape
    assert B == 4 and N <= 34 and int(cpu["src_tokens"].eq(PAD).sum()) > 0
    host = host_fields(cpu) if layout == "packed" else {}
    tgt = label.cuda().long()
    coords = {k: v.cuda() for k, v in cpu.items() if k not in PLANES}
    d, e = ops.pair_inputs_from_coords(coords["src_coord"], coords["src_tokens"], V, PAD)
    planes = {k: v for k, v in coords.items() if k != "src_coord"}
    planes.update(src_distance=d, src_edge_type=e)
    spy = _Spy(ops, monkeypatch)
    ops.set_deterministic(True)
    try:
        out_p, grad_p = _step(model, dict(planes, **host), tgt)
        assert model.last_layout == layout
        assert spy.calls["gbf_bias_fwd"] == 1 and spy.calls["gbf_bias_bwd_full"] == 1 and spy.calls["gbf_bias_fwd_coords"] == 0
        spy.reset()
        assert not any(torch.is_tensor(v) and v.dim() == 3 and v.shape[1] == v.shape[2] == N for v in coords.values())
        out_c, grad_c = _step(model, dict(coords, **host), tgt)
        assert model.last_layout == layout
    finally:
        ops.set_deterministic(False)
    # the coords kernels were the ones launched, and no [B,N,N] input tensor existed anywhere on the way
    assert spy.calls["gbf_bias_fwd_coords"] == 1 and spy.calls["gbf_bias_bwd_full_coords"] == 1, spy.calls
    assert all(spy.calls[n] == 0 for n in ("gbf_bias_fwd", "gbf_bias_bwd_full", "gbf_bias_bwd", "gbf_features_fwd", "pair_inputs_from_records")), spy.calls
    assert spy.squares == 0
    for k in out_p:
        assert torch.equal(out_p[k], out_c[k]), (k, out_p[k], out_c[k])
    assert grad_p.keys() == grad_c.keys() and len(grad_p) > 50
    for n in grad_p:
        assert torch.equal(grad_p[n], grad_c[n]), n


# ------------------------------------------------------------------------------------------------ reference parity from the stored coordinates
@pytest.mark.parametrize("tag", ["cls", "reg_fds"])
def test_g9_model_tiny_from_stored_coordinates(ops, golden, monkeypatch, tag):
    """test_g9_gpu.test_g9_model_tiny_hip with the two planes taken out of every batch: H = 8, so every pair bias goes through the
    fallback (planes materialised once on the device, unfused kernels).  Same bands as the planes run; the coords-versus-planes
    difference is printed for DESIGN.md."""
    from mmdti_hip.functional import CELossFn, MSELossFn
    g = golden("g9_model_tiny_" + tag)
    task = str(g["task"])
    sd = {k[2:]: T(v) for k, v in g.items() if k.startswith("w_")}
    ocfg = tiny_cfg(task, sd["bert.embeddings.word_embeddings.weight"].shape[0])
    kw = dict(fds=True, fds_num=10, _fds_raw_values=g["fds_raw"], use_scaler=False) if task == "regression" else {}
    tok = tokenizer_from(str(golden("g9_collate")["tok_json"]), 38)
    model = product_model(ocfg, tok, **kw).cuda()
    load_fixture_weights(model, sd)
    store = {}
    real = model.encoder.encode
    model.encoder.encode = lambda *a, **k: (lambda out: (store.__setitem__("enc", out[0].detach()), out)[1])(real(*a, **k))
    model.bert.register_forward_hook(lambda m, i, o: store.__setitem__("bert", o[0].detach()))
    full = {k[2:]: T(v).cuda() for k, v in g.items() if k.startswith("b_") and k != "b_label"}
    batch = {k: v for k, v in full.items() if k not in PLANES}
    assert "src_coord" in batch
    label = T(g["b_label"]).cuda()
    tgt = label.float() if task == "regression" else label.long()
    model.train()
    spy = _Spy(ops, monkeypatch)
    epoch = 0
    if task == "regression":
        samples = samples_from(g)
        batches = [model.batch_collate_fn(samples[i:i + 6]) for i in (0, 6)]
        for ep in (0, 1):
            feats, labs = [], []
            with torch.no_grad():
                for b, y in batches:
                    _, f = model(**{k: v.cuda() for k, v in b.items() if k not in PLANES}, epoch=ep, return_feature=True, net_target=y.cuda().float())
                    feats.append(f); labs.append(y.cuda().float())
            assert rel_l2(torch.cat(feats), g[f"fds_feats_ep{ep}"]) < 1e-2
            model.FDS.update_last_epoch_stats(ep)
            model.FDS.update_running_stats(torch.cat(feats), torch.cat(labs), ep)
            for k, v in model.FDS.state_dict().items():
                ref = T(g[f"fds_ep{ep}_{k}"])
                if k in ("epoch", "num_samples_tracked"):
                    assert torch.equal(v.cpu(), ref), (k, ep)
                else:
                    assert rel_l2(v, ref) < 3e-2, (k, ep, rel_l2(v, ref))
        model.FDS.update_last_epoch_stats(2)
        model.FDS.load_state_dict({k[len("fds_ep2_"):]: T(v) for k, v in g.items() if k.startswith("fds_ep2_")}, strict=False)
        epoch = 2
    spy.reset()
    logits, infonce, ct = model(**batch, return_infonce_loss=True, return_ct_loss=True, net_target=tgt, use_weight=False, epoch=epoch)
    assert spy.calls["pair_inputs_from_records"] == 1 and spy.calls["gbf_features_fwd"] == 1 and spy.calls["gbf_bias_fwd_coords"] == 0, spy.calls
    r = dict(enc=rel_l2(store["enc"], g["o_enc"]), bert=rel_l2(store["bert"], g["o_bert"]), logits=rel_l2(logits, g["o_logits"]),
             infonce=abs(float(infonce) - float(g["o_infonce"])) / abs(float(g["o_infonce"])),
             ct=abs(float(ct) - float(g["o_ct"])) / max(abs(float(g["o_ct"])), 1e-6))
    tl = MSELossFn.apply(logits, tgt) if task == "regression" else CELossFn.apply(logits, tgt)
    loss = 1.0 * tl + 0.1 * infonce + 0.1 * ct
    r["loss"] = abs(float(loss) - float(g["o_loss"])) / abs(float(g["o_loss"]))
    print("g9_model_tiny_" + tag + " from coordinates:", json.dumps(r))
    assert r["enc"] < 1e-2 and r["bert"] < 1e-2 and r["logits"] < 2e-2, r
    assert r["infonce"] < 1e-3 and r["loss"] < 1e-3, r
    assert r["ct"] < 5e-3 or abs(float(ct) - float(g["o_ct"])) < 2e-4, r
    loss.backward()
    worst, cos_min = ("", 0.0), 1.0
    for n, p in model.named_parameters():
        key = "hasgrad_" + n
        if key not in g:
            continue
        if not bool(g[key]):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        assert p.grad is not None, n
        ref = T(g["g_" + n])
        if any(z in n for z in ("self_attn.k_proj.bias", "key.bias", "gbf_proj.linear2.bias")) or float(ref.abs().max()) < 1e-7:
            continue
        rr = rel_l2(p.grad, ref)
        worst = max(worst, (n, rr), key=lambda t: t[1])
        cos_min = min(cos_min, cosine(p.grad, ref))
    print("g9_model_tiny_" + tag + " from coordinates: worst gradient", worst, "cos_min", cos_min)
    assert worst[1] < 3.6e-2 and cos_min > 0.9995, (worst, cos_min)
    # coords versus planes on the same weights: the device-derived planes against the stored ones, and what it does to the outputs
    with torch.no_grad():
        d, e = ops.pair_inputs_from_coords(full["src_coord"], full["src_tokens"], V, PAD, torch.int64)
        assert torch.equal(e, full["src_edge_type"])
        nd = int((d != full["src_distance"]).sum())
        ulps = int((d.view(torch.int32) - full["src_distance"].view(torch.int32)).abs().max())
        nt = dict(net_target=tgt) if task == "regression" else {}
        lp = model(**{k: v for k, v in full.items() if k != "src_coord"}, epoch=epoch, **nt)
        lc = model(**batch, epoch=epoch, **nt)
    print(f"g9_model_tiny_{tag}: device distances differ from the stored planes in {nd} of {d.numel()} slots (max {ulps} ulp); logits coords vs planes rel l2 {rel_l2(lc, lp):.3e}")
    assert ulps <= 4


# ------------------------------------------------------------------------------------------------ Trainer
def test_g10_trainer_cls_in_coords_mode(golden, tmp_path):
    """test_g9_gpu.test_g10_trainer_hip (cls, packed rows) through Trainer(pair_inputs="coords"): the existing G10 bands, and -- Trainer(**params)
    ignores unknown keys -- proof that the mode was on: no batch that reached the model carried a plane."""
    from mmdti_hip.tasks import Trainer
    g = golden("g10_trainer_cls")
    task = str(g["task"])
    hp = json.loads(str(g["hp_json"]))
    sd = {k[3:]: T(v) for k, v in g.items() if k.startswith("w0_")}
    tok = tokenizer_from(str(g["tok_json"]), 38)
    model = product_model(tiny_cfg(task, sd["bert.embeddings.word_embeddings.weight"].shape[0]), tok)
    load_fixture_weights(model, sd)
    train, valid = samples_from(g, "train_"), samples_from(g, "valid_")
    seen = []
    model.register_forward_pre_hook(lambda m, a, k: seen.append((len(a), sorted(k))), with_kwargs=True)
    trainer = Trainer(save_path=str(tmp_path), **dict(hp, use_cuda=True, pair_inputs="coords"))
    assert trainer.pair_inputs == "coords"
    torch.manual_seed(1234)
    y_pred = trainer.fit_predict(model, train, valid, None, lambda x: torch.softmax(x, dim=-1)[:, 1:], str(tmp_path), 0, None, return_infonce_loss=True,
                                 return_ct_loss=True, use_weight=False)
    assert len(seen) >= 20 and all(n == 0 and "src_coord" in ks and "src_tokens" in ks and not set(PLANES) & set(ks) for n, ks in seen), seen[:2]
    steps = np.concatenate([h["steps"] for h in trainer.history])
    err = dict(task=float(np.max(np.abs(steps[:, 1] - g["step_task_loss"]) / (np.abs(g["step_task_loss"]) + 1e-2))),
               infonce=float(np.max(np.abs(steps[:, 2] - g["step_infonce"]) / np.abs(g["step_infonce"]))),
               ct=float(np.max(np.abs(steps[:, 3] - g["step_ct"]))),
               y_pred=float(np.max(np.abs(y_pred - g["y_pred"]))), first_step_task=abs(float(steps[0, 1] - g["step_task_loss"][0])))
    ck = torch.load(os.path.join(str(tmp_path), "model_0.pth"), map_location="cpu", weights_only=True)["model_state_dict"]
    per = [rel_l2(ck[k], g["ck_" + k]) for k in ck if ck[k].is_floating_point() and float(np.abs(g["ck_" + k]).max()) > 0 and not k.startswith("FDS.")]
    err["ckpt"], err["ckpt_median"] = max(per), float(np.median(per))
    print("g10_trainer_cls in coords mode:", json.dumps(err))
    assert err["first_step_task"] < 2e-3 and err["task"] < 5e-2 and err["infonce"] < 1e-2 and err["ct"] < 5e-2, err
    assert err["y_pred"] < 3e-2 and err["ckpt"] < 6e-2 and err["ckpt_median"] < 5e-3, err


# ------------------------------------------------------------------------------------------------ captured step
def test_graphed_step_captures_and_replays_a_coords_step(ops):
    """One capture and two replays of a coords-mode step (default mode, tiny model), held to eager coords steps at the tolerance of
    test_trainer_gpu.test_graphed_step_matches_eager_and_redraws_dropout."""
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.synth import synth_batch
    ocfg = tiny_cfg("classification", 40)
    m1, m2 = product_model(ocfg).cuda().train(), product_model(ocfg).cuda().train()
    m2.load_state_dict(m1.state_dict())
    batches = [synth_batch(8, 10, 14, seed=20 + i, ragged=False, smiles_vocab=40, with_coord=True) for i in range(3)]
    t1 = FineTuner(m1, "classification", learning_rate=1e-3, warmup_ratio=0.5, total_steps=6, max_norm=5.0)
    t2 = FineTuner(m2, "classification", learning_rate=1e-3, warmup_ratio=0.5, total_steps=6, max_norm=5.0)
    try:
        for b, y in batches:
            dev = {k: v.cuda() for k, v in b.items() if k not in PLANES}
            o1 = t1.step(dev, y.cuda())
            o2 = t2.graphed_step(dev, y.cuda())
            assert abs(float(o1.loss) - float(o2.loss)) <= 2e-4 * abs(float(o1.loss)) + 1e-6, (float(o1.loss), float(o2.loss))
            assert abs(float(o1.infonce_loss) - float(o2.infonce_loss)) <= 2e-4 * abs(float(o1.infonce_loss))
        assert len(t2._graphs) == 1 and t2.sched_step == 3 and float(t2._state[0]) == 3.0          # one capture, replayed for every batch
        errs = [float((p1 - p2).norm() / (p1.norm() + 1e-12)) for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters())
                if p1.requires_grad and not any(z in n for z in ("key.bias", "gbf_proj.linear2.bias", "pooler"))]
        assert float(np.median(errs)) < 1e-4 and max(errs) < 5e-2, (float(np.median(errs)), max(errs))
    finally:
        ops.seed_salt_reset()


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_are_raised_before_any_launch(ops):
    from mmdti_hip import _abi
    coord, tok, _ = _molecules(8, 5, nan_pads=False)
    rec = ops.pair_records(coord.cuda(), tok.cuda())
    tabs, w1, b1, w2, b2 = _gbf_params(3)
    with pytest.raises(_abi.MMDTIError, match="V \\* V must be the edge-table size"):
        ops.gbf_bias_fwd_coords(rec, 30, PAD, *tabs, w1, b1, w2, b2, 8)
    with pytest.raises(_abi.MMDTIError, match="V \\* V must be the edge-table size"):
        ops.pair_inputs_from_records(rec, 200, PAD)
    with pytest.raises(_abi.MMDTIError, match="N too large"):
        ops.lib().mmdti_pair_inputs_from_coords(0, rec.data_ptr(), 1, 40000, V, PAD, rec.data_ptr(), rec.data_ptr(), 2)
    with pytest.raises(_abi.MMDTIError, match="null atom records"):
        ops.lib().mmdti_gbf_bias_fwd_coords(0, 0, V, PAD, *[t.data_ptr() for t in tabs], w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), 3, 8, 8,
                                            128, 128, 64, E, rec.data_ptr(), 0, 0, 0)
    model = product_model(tiny_cfg("classification", 40)).cuda()
    ids = torch.ones(3, 6, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="src_coord"):
        model(src_tokens=tok.cuda(), input_ids=ids, attention_mask=ids)                     # missing coordinates (and no planes)
    model.dictionary.add_symbol("[EXTRA]")                                                   # V * V is no longer the edge-table size
    with pytest.raises(ValueError, match="edge-table size"):
        model(src_tokens=tok.cuda(), src_coord=coord.cuda(), input_ids=ids, attention_mask=ids)
    torch.cuda.synchronize()
