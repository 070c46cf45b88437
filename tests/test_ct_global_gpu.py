"""Global ConR / SupCon negatives on the device, inside ONE process: the row-block kernels (mmdti_ct_loss_rows_fwd / _bwd) against the
square kernels they share their body with (bit for bit) and against the float64 reference of tests/ct_rows_ref.py; functional.CTLossFn
with a loop-back stand-in that plays every virtual rank; the wiring through MM_Model and FineTuner on a 1-rank group.

Bands.  Square case and the rows / G of every virtual rank: torch.equal with the square kernels.  Sums over virtual ranks (loss, dfhat,
d loss / d feature): the distance from the float64 reference may be at most 2 x the square path's own distance from the same reference
on the same inputs, plus 1e-7 x max|reference| -- the two differ only in how fp32 partial sums are associated, and the square kernels
are the parent's code, not the code under test."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import ct_rows_ref as R
from oracle import mmdti_oracle as O
from test_kernels_gpu import ops, dev          # noqa: F401  (fixture + helper)

T = 0.07
MODE_ID = {"regress": 0, "single": 1, "multi": 2}


def _case(mode, B, D, use_w=True):
    # (seeds at which even the 5- and 6-row cases have anchors with positives and negatives in every mode: the tests assert loss > 0)
    return R.ct_inputs(mode, B, D, seed=2000 + 11 * B + D + 3 * R.MODES.index(mode), use_w=use_w, C=12)


def _kw(mode, c, rows=slice(None)):
    """keyword arguments of ops.ct_loss_fwd / ops.ct_loss_rows_fwd for (the rows of) a case, on the device"""
    kw = dict(weights=None if c["weights"] is None else dev(c["weights"][rows].contiguous()), t=T)
    if mode == "regress":
        kw.update(labels_f=dev(c["labels"][rows].contiguous()), pred=dev(c["pred"][rows].contiguous()), w=R.CT_W, e=0.01)
    elif mode == "single":
        kw.update(labels_f=dev(c["labels"][rows].contiguous()))
    else:
        kw.update(labels_i=dev(c["labels"][rows].contiguous()), coef=float(c["coef"]))
    return kw


def _square(ops, mode, fh, kw):
    """the square entry points through the library, with the per-row terms kept: -> (loss [1], G [B, B], row_terms [B], dfhat [B, D])"""
    B, D = fh.shape
    buf = torch.empty(1 + B, device="cuda")
    Gm = torch.empty(B, B, device="cuda")
    li = kw.get("labels_i")
    p = lambda k: 0 if kw.get(k) is None else kw[k].data_ptr()
    ops.lib().mmdti_ct_loss_fwd(torch.cuda.current_stream().cuda_stream, MODE_ID[mode], fh.data_ptr(), B, D, p("labels_f"), p("labels_i"),
                                0 if li is None else li.shape[1], p("pred"), p("weights"), kw.get("w", 0.2), T, kw.get("e", 0.01),
                                kw.get("coef", 1.0), buf.data_ptr(), Gm.data_ptr(), buf.data_ptr() + 4)
    return buf[:1], Gm, buf[1:], ops.ct_loss_bwd(fh, Gm, T)


def _ref_fhat(mode, c, fh):
    """float64 loss and d loss / d fhat (fhat the free variable) of the whole batch, on the device's own fhat"""
    return R.share_and_grad(mode, fh.cpu(), c["labels"], 0, fh.shape[0], normalize=False, t=T, **R.ref_kwargs(mode, c))


def _dist(got, ref):
    return float((got.detach().cpu().double() - ref).abs().max())


def _within_band(what, d_rows, d_square, ref):
    floor = 1e-7 * float(ref.abs().max())
    print(f"{what}: rows {d_rows:.3e}  square {d_square:.3e}  allowed {2 * d_square + floor:.3e}")
    assert d_rows <= 2 * d_square + floor, f"{what}: {d_rows:.3e} > 2 x {d_square:.3e} + {floor:.3e}"


# ------------------------------------------------------------------------------------------------ 5. the square case, bit for bit
@pytest.mark.parametrize("B,D", [(5, 24), (260, 512)])      # 260: past one pass of the 256-thread key loop; 512: two passes of the column loop
@pytest.mark.parametrize("mode", R.MODES)
def test_rows_at_row0_0_over_the_whole_batch_are_the_square_kernels(ops, mode, B, D):
    c = _case(mode, B, D)
    fh, _ = ops.l2norm_fwd(dev(c["f"]))
    kw = _kw(mode, c)
    loss, Gm, terms, df = _square(ops, mode, fh, kw)
    loss2, Gm2 = ops.ct_loss_fwd(MODE_ID[mode], fh, **kw)
    assert torch.equal(loss, loss2) and torch.equal(Gm, Gm2)
    loss_r, G_r, terms_r = ops.ct_loss_rows_fwd(MODE_ID[mode], fh, 0, B, **kw)
    df_r = ops.ct_loss_rows_bwd(fh, G_r, 0, T)
    assert float(loss) > 0.0 and float(Gm.abs().max()) > 0.0 and float(df.abs().max()) > 0.0
    assert torch.equal(loss_r, loss) and torch.equal(G_r, Gm) and torch.equal(terms_r, terms) and torch.equal(df_r, df)


# ------------------------------------------------------------------------------------------------ 6. virtual ranks partition the square
def virtual_rank_distances(ops, mode, world, Bl, D):
    """-> dict of the four distances from the float64 reference (loss / dfhat, rows summed over virtual ranks / square), after
    asserting that every rank's rows are the square kernel's rows"""
    Bg = world * Bl
    c = _case(mode, Bg, D)
    fh, _ = ops.l2norm_fwd(dev(c["f"]))
    kw = _kw(mode, c)
    loss, Gm, terms, df = _square(ops, mode, fh, kw)
    tot, dtot = torch.zeros(1, device="cuda"), torch.zeros_like(fh)
    for r in range(world):
        loss_r, G_r, terms_r = ops.ct_loss_rows_fwd(MODE_ID[mode], fh, r * Bl, Bl, **kw)
        assert G_r.shape == (Bl, Bg) and terms_r.shape == (Bl,)
        assert torch.equal(terms_r, terms[r * Bl:(r + 1) * Bl]), (mode, r)
        assert torch.equal(G_r, Gm[r * Bl:(r + 1) * Bl]), (mode, r)
        tot += loss_r                                           # (rank order, as the all-reduce of the shares adds them)
        dtot += ops.ct_loss_rows_bwd(fh, G_r, r * Bl, T)
    ref_loss, ref_df = _ref_fhat(mode, c, fh)
    assert float(ref_loss) > 0.0 and float(ref_df.abs().max()) > 0.0
    return dict(loss_rows=_dist(tot, ref_loss.reshape(1)), loss_square=_dist(loss, ref_loss.reshape(1)), dfhat_rows=_dist(dtot, ref_df),
                dfhat_square=_dist(df, ref_df), ref_loss=ref_loss, ref_df=ref_df)


@pytest.mark.parametrize("world,Bl,D", [(2, 3, 24), (4, 65, 512)])
@pytest.mark.parametrize("mode", R.MODES)
def test_virtual_ranks_partition_the_square_result(ops, mode, world, Bl, D):
    d = virtual_rank_distances(ops, mode, world, Bl, D)
    _within_band(f"{mode} {world}x{Bl}x{D} loss", d["loss_rows"], d["loss_square"], d["ref_loss"])
    _within_band(f"{mode} {world}x{Bl}x{D} dfhat", d["dfhat_rows"], d["dfhat_square"], d["ref_df"])


# ------------------------------------------------------------------------------------------------ 7. CTLossFn, every virtual rank in one process
class Loopback:
    """Stand-in for the two collectives of one virtual rank.  ``messages`` holds what every rank sends (built by the test with the same
    public helper, parallel.CTPayload.pack): gather checks that this rank sent its own and returns all of them in rank order.
    reduce_scatter records this rank's [Bg, D] contribution and returns the rows of ``total`` (the sum over ranks, from a first pass)
    or, while there is none yet, of its own contribution."""

    def __init__(self, rank, world, messages, contrib, total=None):
        self.rank, self.world, self.messages, self.contrib, self.total = rank, world, messages, contrib, total
        self.gathers = 0

    def row0(self, b_loc):
        return self.rank * b_loc

    def gather(self, x):
        sent = self.messages[x.dtype]
        assert torch.equal(x, sent[self.rank]), "the rank's message is not what CTPayload.pack builds from its rows"
        self.gathers += 1
        return torch.cat(sent, 0)

    def reduce_scatter(self, g):
        self.contrib[self.rank] = g.clone()
        b = g.shape[0] // self.world
        src = g if self.total is None else self.total
        return src[self.rank * b:(self.rank + 1) * b]


def _ct_fn_args(mode, c, rows=slice(None)):
    kw = _kw(mode, c, rows)
    return (MODE_ID[mode], kw.get("labels_f"), kw.get("labels_i"), kw.get("pred"), kw["weights"], kw.get("w", 0.2), T, kw.get("e", 0.01),
            kw.get("coef", 1.0))


@pytest.mark.parametrize("world,Bl,D", [(2, 3, 24), (4, 65, 512)])
@pytest.mark.parametrize("mode", R.MODES)
def test_ct_loss_fn_with_loopback_negatives_is_the_union_through_the_square_fn(ops, mode, world, Bl, D):
    from mmdti_hip.functional import CTLossFn
    from mmdti_hip.parallel import CTPayload
    Bg = world * Bl
    c = _case(mode, Bg, D)                       # (ConR: per-anchor weights and predictions)
    # the union through the existing square function
    fu = dev(c["f"]).requires_grad_()
    loss_u = CTLossFn.apply(fu, *_ct_fn_args(mode, c))
    loss_u.backward()
    # what every virtual rank sends
    sl = [slice(r * Bl, (r + 1) * Bl) for r in range(world)]
    messages = {torch.float32: [], torch.int64: []}
    for r in range(world):
        kw = _kw(mode, c, sl[r])
        messages[torch.float32].append(CTPayload.pack(ops.l2norm_fwd(dev(c["f"][sl[r]].contiguous()))[0], kw.get("labels_f"), kw.get("pred"), kw["weights"]))
        if mode == "multi":
            messages[torch.int64].append(kw["labels_i"])
    contrib, total, grads, shares = [None] * world, None, None, None
    for _ in range(2):                           # first pass: every rank's contribution; second: the adjoint returns their sum
        grads, shares = [], []
        for r in range(world):
            neg = Loopback(r, world, messages, contrib, total)
            f = dev(c["f"][sl[r]].contiguous()).requires_grad_()
            share = CTLossFn.apply(f, *_ct_fn_args(mode, c, sl[r]), neg)
            share.backward()
            assert neg.gathers == (2 if mode == "multi" else 1)
            grads.append(f.grad)
            shares.append(share.detach())
        total = torch.zeros_like(contrib[0])
        for g in contrib:                        # (rank order, as the all-reduce adds them)
            total += g
    ref_loss, ref_df = R.share_and_grad(mode, c["f"], c["labels"], 0, Bg, t=T, **R.ref_kwargs(mode, c))      # d / d raw feature
    assert float(ref_loss) > 0.0 and float(ref_df.abs().max()) > 0.0
    got_loss = torch.stack(shares).sum().reshape(1)
    what = f"CTLossFn {mode} {world}x{Bl}x{D}"
    _within_band(what + " loss", _dist(got_loss, ref_loss.reshape(1)), _dist(loss_u.reshape(1), ref_loss.reshape(1)), ref_loss)
    _within_band(what + " d loss / d feature", _dist(torch.cat(grads, 0), ref_df), _dist(fu.grad, ref_df), ref_df)


# ------------------------------------------------------------------------------------------------ 8. / 9. model and engine, 1-rank group
def _spy(monkeypatch, calls):
    """count the calls of the two row-block entry points and of the payload gather"""
    from mmdti_hip import ops as _ops
    from mmdti_hip.parallel import CTPayload
    lib = _ops.lib()
    for name in ("mmdti_ct_loss_rows_fwd", "mmdti_ct_loss_rows_bwd"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _r=real, _n=name: (calls.append(_n), _r(*a))[1])
    real_gather = CTPayload.gather
    monkeypatch.setattr(CTPayload, "gather", staticmethod(lambda *a, **k: (calls.append("payload"), real_gather(*a, **k))[1]))


@pytest.fixture
def one_rank_group(monkeypatch):
    import torch.distributed as dist
    import mmdti_hip.parallel as par
    from mmdti_hip import ops as _ops
    monkeypatch.setenv("MMDTI_FORCE_DDP", "1")
    monkeypatch.setenv("MASTER_PORT", "29577")
    for k, v in (("RANK", "0"), ("LOCAL_RANK", "0"), ("WORLD_SIZE", "1")):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("MMDTI_GLOBAL_CT", raising=False)
    par.init_from_env(force=True)
    try:
        yield
    finally:
        _ops.set_deterministic(False)
        par._HOST_GROUP = None
        dist.destroy_process_group()


def _batch(task, odim):
    from test_trainer_gpu import _ocfg
    batch, label = O.synth_batch(8, 10, 14, _ocfg(task, odim), seed=7, ragged=True)
    if task == "classification":          # (both classes present: SupCon has positives and negatives, its value is not 0)
        label = torch.tensor([0, 1, 0, 0, 1, 0, 1, 0], dtype=label.dtype).view(label.shape)
    return batch, label


def _two_steps(task, odim, global_ct, dev_batch, lab, state, sync_debug):
    from mmdti_hip.runtime import dropout_state
    from mmdti_hip.trainer import FineTuner
    from test_trainer_gpu import _model
    model = _model(task, odim).eval()
    if state is not None:
        model.load_state_dict(state)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tuner = FineTuner(model, task, learning_rate=1e-3, total_steps=8, distributed=True, deterministic=True, global_ct=global_ct)
    dropout_state.reseed(77)
    outs = [tuner.step(dev_batch, lab)]
    torch.cuda.synchronize()
    if sync_debug:
        torch.cuda.set_sync_debug_mode("error")
    try:
        outs.append(tuner.step(dev_batch, lab))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    a = tuner.arena
    return tuner, state, outs, (a.data.clone(), a.adam_m.clone(), a.adam_v.clone())


@pytest.mark.parametrize("task,odim", [("regression", 1), ("classification", 2)])
def test_model_and_engine_on_a_one_rank_group(task, odim, one_rank_group, monkeypatch):
    """global_ct=True on a 1-rank group runs the row-block kernels at row0 = 0 over the whole batch -- the square kernels' bits -- and
    the factor `world` is 1: two deterministic steps end in the same parameters and Adam moments as global_ct=False"""
    calls = []
    _spy(monkeypatch, calls)
    batch, label = _batch(task, odim)
    dev_batch, lab = {k: v.cuda() for k, v in batch.items()}, label.cuda()
    t_on, state, out_on, end_on = _two_steps(task, odim, True, dev_batch, lab, None, sync_debug=True)
    assert t_on.global_ct and t_on.negs.active and t_on.model._ct_negatives is not None
    assert calls.count("mmdti_ct_loss_rows_fwd") == 2 and calls.count("mmdti_ct_loss_rows_bwd") == 2 and calls.count("payload") == 2
    del calls[:]
    t_off, _, out_off, end_off = _two_steps(task, odim, False, dev_batch, lab, state, sync_debug=False)
    assert not t_off.global_ct and t_off.model._ct_negatives is None and calls == []
    for a, b, what in zip(end_on, end_off, ("parameters", "adam_m", "adam_v")):
        assert torch.equal(a, b), what
    for o_on, o_off in zip(out_on, out_off):
        assert torch.equal(o_on.ct_loss, o_off.ct_loss) and float(o_on.ct_loss) > 0.0        # the logged value is the local one
        assert torch.equal(o_on.loss, o_off.loss)


def test_off_by_default(one_rank_group, monkeypatch):
    """MMDTI_GLOBAL_CT unset, distributed=True: neither row-block entry point is called and the CT payload is never gathered"""
    from mmdti_hip.trainer import FineTuner
    from test_trainer_gpu import _model
    calls, gathered = [], []
    _spy(monkeypatch, calls)
    batch, label = _batch("classification", 2)
    model = _model("classification", 2).eval()
    tuner = FineTuner(model, "classification", distributed=True)
    assert tuner.negs.active and not tuner.global_ct
    real = tuner.negs.gather
    tuner.negs.gather = lambda x: (gathered.append(tuple(x.shape)), real(x))[1]
    out = tuner.step({k: v.cuda() for k, v in batch.items()}, label.cuda())
    torch.cuda.synchronize()
    assert calls == [] and model._ct_negatives is None and float(out.ct_loss) > 0.0
    assert gathered == [(8, 100)]                      # InfoNCE's fused message alone
    monkeypatch.setenv("MMDTI_GLOBAL_CT", "0")
    assert not FineTuner(_model("classification", 2).eval(), "classification", distributed=True).global_ct
    monkeypatch.setenv("MMDTI_GLOBAL_CT", "1")
    assert FineTuner(_model("classification", 2).eval(), "classification", distributed=True).global_ct
    assert not FineTuner(_model("classification", 2).eval(), "classification", distributed=True, global_ct=False).global_ct
    assert not FineTuner(_model("classification", 2).eval(), "classification", distributed=False, global_ct=True).global_ct
