"""Global ConR / SupCon negatives under data parallelism, without a GPU: the float64 row-block reference (tests/ct_rows_ref.py) against
the oracle on the union batch, the case that motivates the mode, the payload / adjoint / whole-step semantics on two gloo ranks, and
the host-side refusals of the two row-block entry points (which return before any launch)."""
import os
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ct_rows_ref as R
from oracle import mmdti_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x10000            # fake, 16-byte aligned device address: nothing here dereferences it


def _oracle(mode, f, c, w=R.CT_W):
    """oracle.mmdti_oracle.ct_* on the whole batch, float64 -> (loss, d loss / d feature)"""
    f = f.detach().to(R.F64).clone().requires_grad_()
    if mode == "regress":
        # (labels / predictions are multiples of 1/8: exact in either precision, so the masks are the float32 ones; in float64 the
        #  oracle's pushing weight l_dist * weight * e is not rounded to float32 on the way)
        wt = None if c["weights"] is None else c["weights"].double()
        loss = O.ct_regress(f, c["labels"].double().reshape(-1, 1), c["pred"].double().reshape(-1, 1), weights=wt, w=w)
    elif mode == "single":
        loss = O.ct_single(f, c["labels"], None, weights=c["weights"])
    else:
        loss = O.ct_multi(f, c["labels"], None, weights=c["weights"], coef=c["coef"])
    (df,) = torch.autograd.grad(loss, f, allow_unused=True)
    return loss.detach(), (torch.zeros_like(f) if df is None else df)


# ------------------------------------------------------------------------------------------------ 1. reference against oracle
@pytest.mark.parametrize("use_w", [False, True], ids=["now", "w"])
@pytest.mark.parametrize("world,Bl", [(2, 5), (4, 3), (2, 1), (4, 1)])
@pytest.mark.parametrize("mode", R.MODES)
def test_rows_reference_summed_over_virtual_ranks_is_the_oracle_on_the_union(mode, world, Bl, use_w):
    Bg = world * Bl
    c = R.ct_inputs(mode, Bg, 24, seed=100 + 7 * Bg + R.MODES.index(mode), use_w=use_w)
    if mode == "regress" and Bg >= 6:
        c["pred"][1] = 50.0                   # anchor 1: positives, but its prediction is far from everyone's -> no negative, flag 0
    kw = R.ref_kwargs(mode, c)
    ref_loss, ref_df = _oracle(mode, c["f"], c)
    tot, dtot = 0.0, torch.zeros_like(ref_df)
    for r in range(world):
        s, df = R.share_and_grad(mode, c["f"], c["labels"], r * Bl, Bl, **kw)
        tot, dtot = tot + s, dtot + df
    torch.testing.assert_close(tot, ref_loss, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(dtot, ref_df, rtol=1e-10, atol=1e-14)
    if mode == "regress" and Bg >= 6:
        terms = R.row_terms(mode, c["f"], c["labels"], 0, Bg, **kw)
        assert float(terms[1]) == 0.0 and float(terms.abs().max()) > 0.0
        assert float(ref_loss) > 0.0
    if Bg >= 10:
        assert float(ref_loss) > 0.0 and float(ref_df.abs().max()) > 0.0          # (not degenerate: there is a loss to get wrong)


def test_all_labels_equal_has_no_negative_anywhere():
    c = R.ct_inputs("single", 6, 8, seed=3)
    c["labels"] = torch.full((6,), 2.0)
    for r in range(2):
        s, df = R.share_and_grad("single", c["f"], c["labels"], 3 * r, 3, weights=c["weights"])
        assert float(s) == 0.0 and float(df.abs().max()) == 0.0
    assert float(_oracle("single", c["f"], c)[0]) == 0.0


# ------------------------------------------------------------------------------------------------ 2. the motivating case
def test_positives_in_one_shard_rank_local_mean_differs_global_form_is_the_union():
    """An imbalanced classification batch of 8 on 2 ranks whose 2 positives (label 1) both sit in shard 1: on rank 0 every label is
    equal (no negative: the shard's loss is 0); on the union every label-0 anchor has negatives.  The rank mean of shard-local SupCon
    is not the union's loss; the sum of the ranks' global shares is."""
    g = torch.Generator().manual_seed(5)
    f = torch.randn(8, 16, generator=g)
    lab = torch.tensor([0., 0., 0., 0., 0., 1., 0., 1.])
    union = O.ct_single(f.double(), lab, None)
    local = sum(O.ct_single(f[4 * r:4 * r + 4].double(), lab[4 * r:4 * r + 4], None) for r in range(2)) / 2
    assert float(O.ct_single(f[:4].double(), lab[:4], None)) == 0.0
    assert abs(float(local) - float(union)) > 0.1 * float(union) > 0.0
    glob = sum(R.share("single", f, lab, 4 * r, 4) for r in range(2))
    torch.testing.assert_close(glob, union, rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------------ 3. two gloo ranks
def _init(rank, world, initfile):
    for p in (ROOT, os.path.join(ROOT, "mm-dti_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"file://{initfile}")


class _AllGatherFn(torch.autograd.Function):
    """forward = GlobalNegatives.gather, backward = its reduce_scatter (the pair functional.CTLossFn drives on the device)"""

    @staticmethod
    def forward(ctx, x, negs):
        ctx.negs = negs
        return negs.gather(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.negs.reduce_scatter(g.clone()), None


def _worker_payload_and_adjoint(rank, world, initfile, out):
    _init(rank, world, initfile)
    from mmdti_hip.parallel import CTPayload, GlobalNegatives
    Bl, D, C = 3, 5, 4
    g = torch.Generator().manual_seed(1)                                  # (the same stream on both ranks: each cuts its own rows)
    f_all, lab_all, pred_all, w_all = torch.randn(world * Bl, D, generator=g), torch.randn(world * Bl, generator=g), \
        torch.randn(world * Bl, generator=g), torch.rand(world * Bl, generator=g)
    li_all = torch.randint(-1, 3, (world * Bl, C), generator=g)          # int64 assays with -1 = missing
    li_all[0, 0], li_all[-1, -1] = -1, -1
    sl = slice(rank * Bl, (rank + 1) * Bl)
    negs = GlobalNegatives()
    calls = []
    real = negs.gather
    negs.gather = lambda x: (calls.append(tuple(x.shape)), real(x))[1]
    # ConR: one fp32 message f-hat | label | pred | weight
    fa, la, lia, pa, wa = CTPayload.gather(negs, f_all[sl], labels_f=lab_all[sl], pred=pred_all[sl], weights=w_all[sl])
    assert calls == [(Bl, D + 3)] and lia is None
    assert torch.equal(fa, f_all) and torch.equal(la, lab_all) and torch.equal(pa, pred_all) and torch.equal(wa, w_all)
    assert all(t.is_contiguous() for t in (fa, la, pa, wa))
    # SupCon without weights: the unused columns come back as None (a host-side decision, the same on every rank)
    fa, la, lia, pa, wa = CTPayload.gather(negs, f_all[sl], labels_f=lab_all[sl])
    assert torch.equal(fa, f_all) and torch.equal(la, lab_all) and lia is None and pa is None and wa is None
    # Multi: the int64 labels travel as a second message of their own dtype, -1 included
    del calls[:]
    fa, la, lia, pa, wa = CTPayload.gather(negs, f_all[sl], labels_i=li_all[sl], weights=w_all[sl])
    assert calls == [(Bl, D + 3), (Bl, C)] and lia.dtype == torch.int64
    assert torch.equal(fa, f_all) and torch.equal(lia, li_all) and torch.equal(wa, w_all) and la is None and pa is None
    assert bool((lia == -1).any())
    with pytest.raises(ValueError, match="message width"):
        CTPayload.unpack(torch.zeros(4, D + 2), D)
    # the adjoint: sum over ranks of the [Bg, D] contributions, own rows
    mine = torch.arange(world * Bl * D, dtype=torch.float32).view(world * Bl, D) * (rank + 1)
    got = negs.reduce_scatter(mine.clone())
    expect = torch.arange(world * Bl * D, dtype=torch.float32).view(world * Bl, D)[sl] * sum(r + 1 for r in range(world))
    assert torch.equal(got, expect)
    if rank == 0:
        torch.save({"ok": True}, out)
    dist.destroy_process_group()


def _worker_step_equivalence_global_ct(rank, world, initfile, out):
    """The oracle's tiny model: rank-local steps with global InfoNCE AND global CT (each rank's share x world, gradients averaged) ==
    one single-process step on the union batch with the union's InfoNCE and the union's SupCon."""
    _init(rank, world, initfile)
    import ct_rows_ref as Rr
    from mmdti_hip.parallel import CTPayload, GlobalNegatives, shard_batch
    cfg = O.ModelCfg(unimol=O.UniMolCfg(layers=1, dim=32, ffn=64, heads=4, K=8, vocab=31),
                     roberta=O.RobertaCfg(layers=1, dim=32, heads=2, ffn=64, vocab=40, max_pos=40),
                     cross=O.CrossCfg(dim=32, heads=2, ffn=64), task="classification", output_dim=2)
    P = {k: v.requires_grad_() for k, v in O.init_params(cfg, seed=3, std=0.1).items()}
    batch, label = O.synth_batch(4, 6, 9, cfg, seed=11, ragged=True)      # GLOBAL batch, padded to global max lengths
    label = torch.tensor([0, 0, 0, 1]).view(label.shape).to(label.dtype)  # the only positive class member sits in shard 1
    negs = GlobalNegatives()
    sh, lab = shard_batch(batch, label, rank, world)
    enc, bert, pooled = O.mm_features(sh, P, cfg)
    a, b = O.infonce_embed(enc, bert, P, p=0.0)
    both = _AllGatherFn.apply(torch.cat((a, b), 1), negs)
    d = a.shape[1]
    Bg, bl = both.shape[0], a.shape[0]
    qh, kh = torch.nn.functional.normalize(both[:, :d], dim=-1), torch.nn.functional.normalize(both[:, d:], dim=-1)
    logits = qh @ kh.T / 0.1
    r0 = negs.row0(bl)
    rows = slice(r0, r0 + bl)
    nce = ((torch.logsumexp(logits[rows], 1) - logits[rows].diagonal(offset=r0)).sum()
           + (torch.logsumexp(logits.T[rows], 1) - logits.T[rows].diagonal(offset=r0)).sum()) / (2 * Bg)
    logits_head = O.classification_head(pooled, P)
    # global CT as functional.CTLossFn runs it: local normalisation, ONE payload message, rows of this rank against all keys
    fh = torch.nn.functional.normalize(pooled, dim=1)
    D = fh.shape[1]
    msg_all = _AllGatherFn.apply(CTPayload.pack(fh, labels_f=lab.float().reshape(-1)), negs)
    fa, la, _, _ = CTPayload.unpack(msg_all, D, labels_f=True)
    ct = Rr.share("single", fa, la, r0, bl, normalize=False).to(torch.float32)
    loss = O.task_loss(logits_head, lab, cfg.task) + 0.1 * nce * world + 0.1 * ct * world
    loss.backward()
    flat = torch.cat([p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel()) for p in P.values()])
    dist.all_reduce(flat)
    flat /= world
    ct_global = ct.detach().clone()
    dist.all_reduce(ct_global)
    # single process on the union
    Pr = {k: v.detach().clone().requires_grad_() for k, v in P.items()}
    enc, bert, pooled = O.mm_features(batch, Pr, cfg)
    infonce = O.infonce_forward(enc, bert, Pr, p=0.0)
    lh = O.classification_head(pooled, Pr)
    ctr = O.ct_single(pooled, label, None)
    (O.task_loss(lh, label, cfg.task) + 0.1 * infonce + 0.1 * ctr).backward()      # (equal shards: the mean of shard means IS the mean)
    ref = torch.cat([p.grad.reshape(-1) if p.grad is not None else torch.zeros(p.numel()) for p in Pr.values()])
    torch.testing.assert_close(ct_global, ctr.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(flat, ref, rtol=2e-3, atol=2e-6)
    # ... which the rank-local form does not reproduce on this batch: shard 0 holds one class only, its local SupCon is 0
    half = label.shape[0] // world
    local = sum(O.ct_single(pooled[i * half:(i + 1) * half], label[i * half:(i + 1) * half], None) for i in range(world)) / world
    assert abs(float(local) - float(ctr)) > 0.05 * abs(float(ctr)) > 0.0
    if rank == 0:
        torch.save({"ok": True}, out)
    dist.destroy_process_group()


@pytest.mark.parametrize("worker", [_worker_payload_and_adjoint, _worker_step_equivalence_global_ct])
def test_two_ranks_gloo(worker):
    with tempfile.TemporaryDirectory() as td:
        initfile, out = os.path.join(td, "init"), os.path.join(td, "out.pt")
        mp.spawn(worker, args=(2, initfile, out), nprocs=2, join=True)
        assert torch.load(out)["ok"]


# ------------------------------------------------------------------------------------------------ 4. refusals
def _fwd(lib, mode=1, fhat=PTR, Bg=8, D=64, row0=0, rows=8, lab_f=PTR, lab_i=0, C=0, pred=0, wts=0, t=0.07, loss=PTR, G=PTR, row_ws=PTR):
    lib.mmdti_ct_loss_rows_fwd(0, mode, fhat, Bg, D, row0, rows, lab_f, lab_i, C, pred, wts, 0.2, t, 0.01, 1.0, loss, G, row_ws)


def _bwd(lib, fhat=PTR, G=PTR, Bg=8, D=64, row0=0, rows=8, t=0.07, dfhat=PTR):
    lib.mmdti_ct_loss_rows_bwd(0, fhat, G, Bg, D, row0, rows, t, dfhat)


def test_rows_entry_points_refuse_bad_arguments_before_any_launch():
    from mmdti_hip import _abi
    lib = _abi.lib()
    E = _abi.MMDTIError
    protos = _abi.parse_header()
    assert protos["mmdti_ct_loss_rows_fwd"][2] == ["stream", "mode", "fhat_all", "Bg", "D", "row0", "rows", "labels_f_all", "labels_i_all", "C",
                                                   "pred_all", "weights_all", "w", "t", "e", "coef", "loss", "G", "row_ws"]
    assert protos["mmdti_ct_loss_rows_bwd"][2] == ["stream", "fhat_all", "G", "Bg", "D", "row0", "rows", "t", "dfhat_all"]
    # forward: the row block
    for kw in (dict(row0=-1), dict(rows=0), dict(rows=-3), dict(row0=1, rows=8), dict(row0=8, rows=1), dict(row0=2 ** 31 - 1, rows=2 ** 31 - 1)):
        with pytest.raises(E, match="ct_loss_rows_fwd: bad row block"):
            _fwd(lib, **kw)
    with pytest.raises(E, match="ct_loss_rows_fwd: bad sizes"):
        _fwd(lib, Bg=0, rows=1)
    with pytest.raises(E, match="ct_loss_rows_fwd: bad sizes"):
        _fwd(lib, D=0)
    # forward: null pointers, each named
    for kw, name in ((dict(fhat=0), "fhat_all"), (dict(loss=0), "loss"), (dict(G=0), "G")):
        with pytest.raises(E, match=f"ct_loss_rows_fwd: {name} is null"):
            _fwd(lib, **kw)
    # forward: what a mode needs
    with pytest.raises(E, match="ct_loss_rows_fwd: bad mode 3"):
        _fwd(lib, mode=3)
    for mode in (0, 1):
        with pytest.raises(E, match="ct_loss_rows_fwd: labels missing"):
            _fwd(lib, mode=mode, lab_f=0, pred=PTR)
    with pytest.raises(E, match="ct_loss_rows_fwd: labels missing"):
        _fwd(lib, mode=2, lab_f=PTR, lab_i=0, C=4)
    with pytest.raises(E, match="ct_loss_rows_fwd: labels missing"):
        _fwd(lib, mode=2, lab_i=PTR, C=0)
    with pytest.raises(E, match="ct_loss_rows_fwd: regress needs predictions"):
        _fwd(lib, mode=0, pred=0)
    for t in (0.0, -0.07):
        with pytest.raises(E, match="ct_loss_rows_fwd: t must be positive"):
            _fwd(lib, t=t)
    with pytest.raises(E, match="ct_loss_rows_fwd: .*too large for LDS"):
        _fwd(lib, Bg=16000, D=512, rows=4)                         # D + Bg + 4 floats > 64 KiB
    # forward: the deterministic mode needs the per-row terms' buffer, as the square entry does
    lib.mmdti_set_deterministic(1)
    try:
        with pytest.raises(E, match="ct_loss_rows_fwd: deterministic mode needs row_ws"):
            _fwd(lib, row_ws=0)
    finally:
        lib.mmdti_set_deterministic(0)
    # backward
    for kw in (dict(row0=-1), dict(rows=0), dict(row0=1, rows=8), dict(row0=8, rows=1), dict(row0=2 ** 31 - 1, rows=2 ** 31 - 1)):
        with pytest.raises(E, match="ct_loss_rows_bwd: bad row block"):
            _bwd(lib, **kw)
    with pytest.raises(E, match="ct_loss_rows_bwd: bad sizes"):
        _bwd(lib, Bg=-1)
    for kw, name in ((dict(fhat=0), "fhat_all"), (dict(G=0), "G"), (dict(dfhat=0), "dfhat_all")):
        with pytest.raises(E, match=f"ct_loss_rows_bwd: {name} is null"):
            _bwd(lib, **kw)
    with pytest.raises(E, match="ct_loss_rows_bwd: t must be positive"):
        _bwd(lib, t=0.0)
    with pytest.raises(E, match="ct_loss_rows_bwd: Bg too large"):
        _bwd(lib, Bg=16385, rows=4)
