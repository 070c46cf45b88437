"""The fp32 kernels at the two ends of the step -- ConR / SupCon, FDS, l2norm, the task losses, masked pooling, the embedding
scatter -- against the float64 references of tests/head_refs.py, at the smallest shapes where every loop of the kernels takes a
second, ragged iteration (B > 256 keys, D > 256 / > 64 columns, more than one workgroup of the flat grids, more than 16 row groups).

Bands
  integer outputs, exact zeros, untouched entries, a second call of the same kernel: bit-exact
  ConR / SupCon loss                       rtol 2e-4, atol 1e-6   (the band of test_kernels_gpu.test_ct_losses_golden)
  FDS statistics, smoothed features        rtol 1e-4, atol 1e-5   (test_fds_golden)
  task-loss values, pooled rows, xhat      rtol 1e-5, atol 1e-6   (test_head_and_losses, test_masked_pool)
  every gradient-like output               nerr = max|got - ref| / max|ref| <= 2e-5
The gradient band: the ConR kernels use __expf / __logf on arguments up to 1/t = 14.3 (relative error near 1e-6 per term) and sum
300 keys and 520 columns in another order than torch; on Gaussian features the fp32 CPU oracle sits at <= 7.2e-7 by the same
measure, on clustered features at <= 1.9e-6 but for SupCon, where it misses the band itself (below, and
test_head_refs_cpu.test_ct_cases_float32_oracle_error)."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_refs as R
from oracle import mmdti_oracle as O
from test_kernels_gpu import ops, dev, G          # noqa: F401  (fixture + helpers)

GRAD_NERR = 2e-5


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().cpu().double(), b.detach().cpu().double(), rtol=rtol, atol=atol)


def rt(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ================================================================================================ ConR / SupCon
CT_SHAPES = [(1, 64), (2, 50), (33, 1000), (256, 512), (257, 512), (300, 520)]
CT_W, NCLS, ct_case = R.CT_W, R.CT_NCLS, R.ct_case          # (the cases are built in head_refs: the CPU file pins their oracle figures)
# SupCon (single) on clustered features is the one ill-conditioned family: the clusters ARE the classes, every positive pair sits near
# s / t = +13, the loss is almost at its minimum and d loss / d feature (max 1e-5 .. 3e-5, ten times below every other case) is what
# is left after the positive and the negative terms cancel.  The fp32 CPU oracle itself misses 2e-5 there: its nerr against float64 on
# these very inputs is 1.3e-5 .. 5.5e-5 (every other case: 1.9e-7 .. 1.9e-6); test_head_refs_cpu.test_ct_cases_float32_oracle_error
# pins both ranges without a GPU.  The rule for this family: band = 16 x the oracle's nerr on the same input (head_refs.ct_case
# computes it), at most CT_BAND_CAP.  The margin: the kernel sums the D products of a similarity one after the other in fp32 where the
# oracle's matmul sums in blocks, and evaluates exp / log as exp2 / log2 of an fp32-rounded x log2(e): a factor of a few on an error
# that is all cancellation; 16 is a quarter of the largest margin the band rule allows.  The cap is a hundred times the ordinary band
# and still far below the nerr of 0.1 .. 1 that a dropped partial or a wrong stride leaves; it keeps a change of the generators or of
# the oracle from widening the band unseen.
# Measured on an MI355X (ct_check prints nerr, oracle figure and band per case): the kernels sit at 1.4 .. 3.7 times the oracle's figure
# on this family (2.1e-5 .. 1.4e-4) and at <= 3.9e-6 on every other case.
CT_ILL, CT_ILL_MARGIN, CT_BAND_CAP = ("single", "clustered"), 16, 2e-3


def ct_band(c):
    """the gradient band of a case: 2e-5, or CT_ILL_MARGIN x the fp32 CPU oracle's own nerr on the ill-conditioned family"""
    band = CT_ILL_MARGIN * c.o32 if (c.mode, c.kind) == CT_ILL else GRAD_NERR
    assert band <= CT_BAND_CAP, f"band {band:.3g}: the generators or the oracle changed"
    return band


def ct_device(ops, c):
    fh, inv = ops.l2norm_fwd(dev(c.f))
    wts = dev(c.weights) if c.weights is not None else None
    if c.mode == "regress":
        loss, Gm = ops.ct_loss_fwd(ops.CT_REGRESS, fh, labels_f=dev(c.labels), pred=dev(c.pred), weights=wts, w=CT_W, e=0.01)
    elif c.mode == "single":
        loss, Gm = ops.ct_loss_fwd(ops.CT_SINGLE, fh, labels_f=dev(c.labels), weights=wts)
    else:
        loss, Gm = ops.ct_loss_fwd(ops.CT_MULTI, fh, labels_i=dev(c.labels.contiguous()), weights=wts, coef=float(c.coef))
    df = ops.l2norm_bwd(ops.ct_loss_bwd(fh, Gm), fh, inv)
    return loss, Gm, df


def ct_check(ops, c):
    loss, Gm, df = ct_device(ops, c)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(df).all())
    e, band = R.nerr(df, c.df), ct_band(c)
    print(f"ct {c.mode} {c.kind} B={c.f.shape[0]} D={c.f.shape[1]}: loss {float(loss):.8g} ref {float(c.loss):.8g} grad nerr {e:.3g} "
          f"(fp32 oracle {c.o32:.3g}, band {band:.3g})")
    close(loss, c.loss.reshape(1), 2e-4, 1e-6)
    assert e <= band, f"d loss / d feature: nerr {e:.3g} > {band:.3g}"
    loss2, Gm2, df2 = ct_device(ops, c)          # the row-ordered sum: the same bits on a second call
    assert torch.equal(loss, loss2) and torch.equal(Gm, Gm2) and torch.equal(df, df2)
    return loss, Gm, df


@pytest.mark.parametrize("use_w", [False, True], ids=["now", "w"])
@pytest.mark.parametrize("kind", ["gauss", "clustered"])
@pytest.mark.parametrize("B,D", CT_SHAPES)
@pytest.mark.parametrize("mode", R.CT_MODES)
def test_ct_loss_and_gradient(ops, mode, B, D, kind, use_w):
    c = ct_case(mode, B, D, kind, use_w)
    loss, Gm, df = ct_check(ops, c)
    if B == 1:          # no pair at all
        assert float(loss) == 0.0 and float(df.abs().max()) == 0.0
    elif B >= 33:       # (the case is not degenerate: there is a loss to get wrong)
        assert float(c.loss) > 0.1 and float(c.df.abs().max()) > 0


@pytest.mark.parametrize("kind", ["gauss", "clustered"])
@pytest.mark.parametrize("B,D", [(40, 64), (257, 512)])
def test_ct_edge_rows(ops, B, D, kind):
    # a row outside every mask: zero loss term, zero row and column of G, zero gradient row
    c = ct_case("regress", B, D, kind, True, "isolated_row")
    loss, Gm, df = ct_check(ops, c)
    assert float(Gm[0].abs().max()) == 0.0 and float(Gm[:, 0].abs().max()) == 0.0 and float(df[0].abs().max()) == 0.0
    assert float(c.df[0].abs().max()) == 0.0 and float(c.loss) > 0.1
    # a row with positives and no negative (flag 0): its row of G is zero, its gradient is not (it is other rows' positive)
    c = ct_case("regress", B, D, kind, True, "no_negative_row")
    loss, Gm, df = ct_check(ops, c)
    assert float(Gm[1].abs().max()) == 0.0 and float(df[1].abs().max()) > 0.0
    # a row without a positive: SupCon divides by 1
    c = ct_case("single", B, D, kind, True, "no_positive_row")
    loss, Gm, df = ct_check(ops, c)
    assert float(Gm[2].abs().max()) == 0.0 and float(df[2].abs().max()) > 0.0
    # all labels equal: no negative anywhere
    for mode in ("regress", "single"):
        c = ct_case(mode, B, D, kind, False, "all_equal")
        loss, Gm, df = ct_check(ops, c)
        assert float(c.loss) == 0.0 and float(loss) == 0.0 and float(df.abs().max()) == 0.0


@pytest.mark.parametrize("use_w", [False, True], ids=["now", "w"])
@pytest.mark.parametrize("variant", ["c617_coef1", "c617_coef300"])
@pytest.mark.parametrize("B,D", [(33, 1000), (257, 512)])
def test_ct_multi_many_assays(ops, B, D, variant, use_w):
    c = ct_case("multi", B, D, "clustered", use_w, variant)
    assert float(c.loss) > 0.1
    ct_check(ops, c)


def test_ct_lds_bound_is_a_host_side_rejection(ops):
    """the anchor row, the B products and the reduction scratch share 64 KiB of LDS: D + B + 4 > 16384 floats is refused before
    anything is launched -- every output buffer of a direct library call keeps its sentinel"""
    B, D = 8, 16380
    fh = torch.zeros(B, D, device="cuda")
    lab = torch.zeros(B, device="cuda")
    with pytest.raises(ops.MMDTIError):
        ops.ct_loss_fwd(ops.CT_SINGLE, fh, labels_f=lab)
    buf, Gm = torch.full((1 + B,), -7.0, device="cuda"), torch.full((B, B), -7.0, device="cuda")
    with pytest.raises(ops.MMDTIError, match="too large for LDS"):
        ops.lib().mmdti_ct_loss_fwd(torch.cuda.current_stream().cuda_stream, ops.CT_SINGLE, fh.data_ptr(), B, D, lab.data_ptr(), 0, 0, 0, 0,
                                    0.2, 0.07, 0.01, 1.0, buf.data_ptr(), Gm.data_ptr(), buf.data_ptr() + 4)
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()) and bool((Gm == -7.0).all())


# ================================================================================================ FDS
def _labels_for_bins(b, mn, bw):
    return (mn + (b.double() + 0.5) * bw).float()


@pytest.mark.parametrize("mn,bw", [(-1.0, 0.25), (0.3, 0.1), (-2.7, 0.37)])
def test_fds_bins_edges(ops, mn, bw):
    """n = 1000 (four workgroups, the last ragged): labels exactly on bin edges, one ulp to either side, below min_value (negative
    quotients) and beyond the last bucket -- bit-exact against fds_label_bins, and the two end-bucket flags."""
    bs, bn = 2, 20
    g = G(5)
    edges = (mn + torch.arange(-6, 27).double() * bw).float()
    up, down = torch.nextafter(edges, torch.tensor(float("inf"))), torch.nextafter(edges, torch.tensor(float("-inf")))
    rnd = (mn - 2.0) + torch.rand(1000 - 3 * edges.numel(), generator=g) * (28 * bw + 2.0)
    labels = torch.cat((edges, up, down, rnd))
    assert labels.numel() == 1000
    ref = O.fds_label_bins(labels, mn, bw)
    assert int(ref.min()) < 0 and int(ref.max()) > bn
    bins, flags = ops.fds_bins(dev(labels), mn, bw, bs, bn)
    assert torch.equal(bins.cpu().long(), ref)
    assert flags.cpu().tolist() == [1, 1]
    inner = labels[(ref != bs) & (ref != bn - 1)].contiguous()          # without a sample exactly in an end bucket
    bins, flags = ops.fds_bins(dev(inner), mn, bw, bs, bn)
    assert torch.equal(bins.cpu().long(), O.fds_label_bins(inner, mn, bw)) and flags.cpu().tolist() == [0, 0]


@pytest.mark.parametrize("ends", [True, False], ids=["ends", "noends"])
@pytest.mark.parametrize("bs,bn", [(0, 20), (3, 20), (0, 100), (3, 100)])
@pytest.mark.parametrize("D", [16, 300, 512])
def test_fds_update_stats(ops, D, bs, bn, ends):
    n, mn, bw, nb = 1500, 0.0, 0.5, bn - bs
    g = G(31 * D + bn + bs)
    b = torch.randint(bs - 3, bn + 3, (n,), generator=g)          # rows below bucket_start and above bucket_num - 1 included
    empty, single = [bs + 2, bs + 5], bs + 4
    for e in empty + [single]:
        b[b == e] = bs + 1
    b[17] = single                                               # a one-sample bucket
    if ends:
        b[3], b[4] = bs, bn - 1
    else:                                                        # no sample exactly in an end bucket: the rows beyond stay out
        b[(b == bs) | (b == bn - 1)] = bs + 1
    labels = _labels_for_bins(b, mn, bw)
    assert torch.equal(O.fds_label_bins(labels, mn, bw), b)
    feats = torch.randn(n, D, generator=g) * 2 + 1
    feats[:, 5], feats[:, D - 1] = 1.5, -0.25                   # constant columns: variance EXACTLY 0 (calibrate_mean_var tests == 0)
    feats2 = feats * 0.7 + 0.1
    rm0, rv0 = torch.randn(nb, D, generator=g), torch.rand(nb, D, generator=g) + 0.5
    ref = R.FDS64(D, mn, bw, torch.ones(1), bucket_num=bn, bucket_start=bs)
    ref.running_mean, ref.running_var = rm0.double(), rv0.double()
    rm, rv, tr = dev(rm0), dev(rv0), torch.zeros(nb, device="cuda")
    bins, flags = ops.fds_bins(dev(labels), mn, bw, bs, bn)
    assert torch.equal(bins.cpu().long(), b) and flags.cpu().tolist() == [int(ends), int(ends)]
    untouched = [e - bs for e in empty] + ([] if ends else [0, nb - 1])
    touched = [i for i in range(nb) if i not in untouched]
    for epoch, (x, factor) in enumerate(((feats, 0.0), (feats2, 0.9))):
        ref.update_running_stats(x, labels, epoch)              # (epoch == start_update: factor 0; later: momentum 0.9)
        ops.fds_update_stats(dev(x), bins, flags, bs, bn, factor, rm, rv, tr)
        close(rm, ref.running_mean, 1e-4, 1e-5)
        close(rv, ref.running_var, 1e-4, 1e-5)
        assert torch.equal(tr.cpu().double(), ref.num_samples_tracked)
        assert torch.equal(rm.cpu()[untouched], rm0[untouched]) and torch.equal(rv.cpu()[untouched], rv0[untouched])
        assert float(tr[untouched].abs().max()) == 0.0 and float(tr[touched].min()) >= 1.0
        assert float(rv[single - bs].abs().max()) == 0.0        # one sample: variance exactly 0
        for col in (5, D - 1):
            assert float(rv[touched, col].abs().max()) == 0.0 and float(ref.running_var[touched, col].abs().max()) == 0.0
    cnt = int(((b >= bs) & (b <= bn - 1)).sum()) if not ends else n
    assert float(tr.sum()) == 2.0 * cnt


def _windows(ks):
    g = G(ks)
    asym = torch.rand(ks, generator=g) + 0.1          # (asymmetric: a flipped window would show)
    return [O.fds_kernel_window("gaussian", ks, 2), asym / asym.sum()]


@pytest.mark.parametrize("nb,D,ks", [(3, 16, 5), (20, 512, 5), (20, 512, 9), (100, 520, 5), (100, 520, 9)])
def test_fds_smooth_stats(ops, nb, D, ks):
    """(3, 16, 5): the reflection applies on both sides of one output at once.  (20, 512) and (100, 520): 40 and 204 workgroups of
    the flat grid, D not a power of two in the second: the bucket / column split of a flat index beyond the first workgroup."""
    stat = torch.randn(nb, D, generator=G(nb + D))
    for win in _windows(ks):
        out = ops.fds_smooth_stats(dev(stat), dev(win.float().contiguous()))
        close(out, R.smooth_stat(stat, win.float()), 1e-4, 1e-5)


@pytest.mark.parametrize("ends", [True, False], ids=["ends", "noends"])
@pytest.mark.parametrize("D", [16, 512, 520])
@pytest.mark.parametrize("n", [5, 257])
def test_fds_smooth(ops, n, D, ends):
    bs, bn, mn, bw = 3, 12, 0.0, 0.5
    nb = bn - bs
    g = G(3 * n + D)
    m1, m2 = torch.randn(nb, D, generator=g), torch.randn(nb, D, generator=g)
    v1 = torch.rand(nb, D, generator=g) + 0.5
    ratio = torch.tensor([0.01, 0.5, 2.0, 50.0])[torch.arange(D) % 4]          # both clamp ends (0.1 and 10) and two values between
    v2 = v1 * ratio
    v1[2, ::3] = 0.0                    # bucket bs + 2: zero-variance columns stay untouched
    v1[4, :] = 1e-13                    # bucket bs + 4: sum(v1) < 1e-10, the whole bucket stays untouched
    if ends:
        pattern = [bs - 2, bs + 2, bs + 4, bn - 1, bs, bn + 3, bs + 1]          # (n = 5 takes the first five: every edge is in them)
    else:                               # no sample exactly in an end bucket: rows below / above are inactive
        pattern = [bs - 2, bs + 2, bs + 4, bn + 3, bs + 1, bs + 6, bs + 3]
    b = torch.tensor(pattern)[torch.arange(n) % len(pattern)]
    labels = _labels_for_bins(b, mn, bw)
    x = torch.randn(n, D, generator=g) * 2
    ref = R.FDS64(D, mn, bw, torch.ones(1), bucket_num=bn, bucket_start=bs)
    ref.running_mean_last_epoch, ref.running_var_last_epoch = m1.double(), v1.double()
    ref.smoothed_mean_last_epoch, ref.smoothed_var_last_epoch = m2.double(), v2.double()
    y_ref, sc_ref = ref.smooth_with_scale(x, labels, 1)
    bins, flags = ops.fds_bins(dev(labels), mn, bw, bs, bn)
    assert torch.equal(bins.cpu().long(), b)
    y, sc = ops.fds_smooth(dev(x), bins, flags, bs, bn, dev(m1), dev(v1), dev(m2), dev(v2))
    close(y, y_ref, 1e-4, 1e-5)
    close(sc, sc_ref, 1e-4, 1e-5)
    lo, hi = float(sc_ref.min()), float(sc_ref.max())
    assert abs(lo - 0.1 ** 0.5) < 1e-12 and abs(hi - 10 ** 0.5) < 1e-12          # both clamp ends are reached
    inactive = (b == bs + 4) if ends else ((b < bs) | (b > bn - 1) | (b == bs + 4))
    assert bool(inactive.any())
    assert torch.equal(y.cpu()[inactive], x[inactive]) and bool((sc.cpu()[inactive] == 1).all())
    zrows = b == bs + 2
    assert bool(zrows.any())
    assert torch.equal(y.cpu()[zrows][:, ::3], x[zrows][:, ::3]) and bool((sc.cpu()[zrows][:, ::3] == 1).all())
    y2, _ = ops.fds_smooth(dev(x), bins, flags, bs, bn, dev(m1), dev(v1), dev(m2), dev(v2), want_scale=False)
    assert torch.equal(y, y2)


# ================================================================================================ l2norm
@pytest.mark.parametrize("layout", ["contiguous", "left_half", "right_half"])
@pytest.mark.parametrize("D", [50, 64, 65, 512])
@pytest.mark.parametrize("B", [1, 257])
def test_l2norm(ops, B, D, layout):
    g = G(B + D)
    buf = torch.randn(B, 2 * D, generator=g) * 3
    zero_row = 100 if B > 1 else None
    if zero_row is not None:
        buf[zero_row] = 0.0
    bd = dev(buf)
    if layout == "contiguous":
        x, xd = buf[:, :D].contiguous(), bd[:, :D].contiguous()
    elif layout == "left_half":
        x, xd = buf[:, :D], bd[:, :D]                 # ldx = 2 D
    else:
        x, xd = buf[:, D:], bd[:, D:]
    assert layout == "contiguous" or xd.stride(0) == 2 * D
    dxh = torch.randn(B, D, generator=g)
    xh_ref, dx_ref = R.l2norm(x, dxh)
    xh, inv = ops.l2norm_fwd(xd)
    close(xh, xh_ref, 1e-5, 1e-6)
    dx = ops.l2norm_bwd(dev(dxh), xh, inv)
    assert bool(torch.isfinite(dx).all())
    rows = torch.ones(B, dtype=torch.bool)
    if zero_row is not None:                          # eps clamp: xhat = 0, d x = d xhat / eps
        rows[zero_row] = False
        assert float(xh[zero_row].abs().max()) == 0.0
        close(dx[zero_row], dx_ref[zero_row], 1e-5, 0.0)
    e = R.nerr(dx.cpu()[rows], dx_ref[rows])
    assert e <= GRAD_NERR, f"l2norm_bwd nerr {e:.3g}"
    assert torch.equal(bd, dev(buf))                  # the other half of the buffer is only read


def test_l2norm_single_zero_row(ops):
    xh, inv = ops.l2norm_fwd(torch.zeros(1, 65, device="cuda"))
    assert float(xh.abs().max()) == 0.0
    dxh = torch.randn(1, 65, generator=G(1))
    dx = ops.l2norm_bwd(dev(dxh), xh, inv)
    assert bool(torch.isfinite(dx).all())
    close(dx, R.l2norm(torch.zeros(1, 65), dxh)[1], 1e-5, 0.0)


# ================================================================================================ task losses
NS = [1, 255, 256, 257, 1000]


def _loss_check(got, ref, what):
    (l, d), (l_ref, d_ref) = got, ref
    assert bool(torch.isfinite(l).all()) and bool(torch.isfinite(d).all())
    close(l, l_ref, 1e-5, 1e-6)
    e = R.nerr(d, d_ref.view_as(d))
    assert e <= GRAD_NERR, f"{what}: gradient nerr {e:.3g}"


@pytest.mark.parametrize("n", NS)
def test_mse_loss(ops, n):
    g = G(n)
    pred, tg = torch.randn(n, 1, generator=g) * 3, torch.randn(n, 1, generator=g)
    _loss_check(ops.mse_loss(dev(pred), dev(tg)), R.mse(pred, tg), "mse")


@pytest.mark.parametrize("C", [2, 3, 10])
@pytest.mark.parametrize("B", NS)
def test_ce_loss(ops, B, C):
    g = G(B + C)
    lg = torch.randn(B, C, generator=g) * 3
    lg[::5, 0] = 80.0                      # logits of +-80: the stable forms, no inf / NaN
    lg[2::5, C - 1] = -80.0
    lg[4::5, :] = 80.0
    lg[4::5, 1] = -80.0
    tg = torch.randint(0, C, (B,), generator=g)
    _loss_check(ops.ce_loss(dev(lg), dev(tg)), R.cross_entropy(lg, tg), "ce")


@pytest.mark.parametrize("targets", ["hard", "soft"])
@pytest.mark.parametrize("n", NS)
def test_bce_logits_loss(ops, n, targets):
    g = G(n + len(targets))
    x = torch.randn(n, generator=g) * 3
    x[::7], x[3::7] = 80.0, -80.0
    t = torch.randint(0, 2, (n,), generator=g).float() if targets == "hard" else torch.rand(n, generator=g)
    _loss_check(ops.bce_logits_loss(dev(x), dev(t)), R.bce_logits(x, t), "bce")
    if n == 1000:          # the [B, C] form the multilabel head passes
        _loss_check(ops.bce_logits_loss(dev(x.view(40, 25)), dev(t.view(40, 25))), R.bce_logits(x.view(40, 25), t.view(40, 25)), "bce 2-d")


# ================================================================================================ masked pooling
POOL_SHAPES = [(7, 11, 68), (130, 258, 512), (258, 512, 512)]


def _packing(counts, S):
    """the layout of mmdti_hip.packing.PackedRows (n real rows, then one representative pad row iff n < S) for counts that may be 0"""
    c = torch.as_tensor(counts, dtype=torch.int64)
    B = c.numel()
    rows = c + (c < S).long()
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(rows, 0)
    seq = torch.repeat_interleave(torch.arange(B), rows)
    local = torch.arange(int(off[-1])) - off[:-1][seq]
    i32 = lambda t: t.to(torch.int32).cuda()
    return SimpleNamespace(B=B, S=S, M=int(off[-1]), off=i32(off), n_real=i32(c), row_seq=i32(seq), gather=seq * S + local,
                           real=local < c[seq])


def _pool_counts(Na, Nt):
    # ragged | every atom row masked, tokens present | the converse | nothing masked
    return [Na // 2 + 1, 0, Na, Na], [Nt - 3, Nt // 3, 0, Nt]


@pytest.mark.parametrize("Na,Nt,D", POOL_SHAPES)
def test_masked_pool_padded(ops, Na, Nt, D):
    g = G(Na + Nt + D)
    ca, ct = _pool_counts(Na, Nt)
    B = len(ca) + 1
    ma = torch.arange(Na).view(1, -1) < torch.tensor(ca + [0]).view(-1, 1)
    mt = torch.arange(Nt).view(1, -1) < torch.tensor(ct + [0]).view(-1, 1)
    ma[-1], mt[-1] = torch.rand(Na, generator=g) < 0.5, torch.rand(Nt, generator=g) < 0.5          # scattered holes
    a, t, dp = torch.randn(B, Na, D, generator=g), torch.randn(B, Nt, D, generator=g), torch.randn(B, D, generator=g)
    out_ref, da_ref, dt_ref = R.masked_pool(a, t, ma, mt, dp)
    mad, mtd = dev(ma).view(torch.uint8), dev(mt).view(torch.uint8)
    out = ops.masked_pool_fwd(dev(a), dev(t), mad, mtd)
    close(out, out_ref, 1e-5, 1e-6)
    da, dt = ops.masked_pool_bwd(dev(dp), mad, mtd, Na, Nt)
    assert R.nerr(da, da_ref) <= GRAD_NERR and R.nerr(dt, dt_ref) <= GRAD_NERR
    assert float(da.cpu()[~ma].abs().max()) == 0.0 and float(dt.cpu()[~mt].abs().max()) == 0.0          # masked rows: exactly 0
    assert float(da[1].abs().max()) == 0.0 and float(dt[2].abs().max()) == 0.0


@pytest.mark.parametrize("Na,Nt,D", POOL_SHAPES)
def test_masked_pool_packed(ops, Na, Nt, D):
    g = G(Na + Nt + D + 1)
    ca, ct = _pool_counts(Na, Nt)
    B = len(ca)
    pa, pt = _packing(ca, Na), _packing(ct, Nt)
    ma = torch.arange(Na).view(1, -1) < torch.tensor(ca).view(-1, 1)
    mt = torch.arange(Nt).view(1, -1) < torch.tensor(ct).view(-1, 1)
    a, t, dp = torch.randn(B, Na, D, generator=g), torch.randn(B, Nt, D, generator=g), torch.randn(B, D, generator=g)
    out_ref, da_ref, dt_ref = R.masked_pool(a, t, ma, mt, dp)
    ap, tp = a.view(B * Na, D)[pa.gather].contiguous(), t.view(B * Nt, D)[pt.gather].contiguous()
    out = ops.masked_pool_packed_fwd(dev(ap), dev(tp), pa, pt)
    close(out, out_ref, 1e-5, 1e-6)
    padded = ops.masked_pool_fwd(dev(a), dev(t), dev(ma).view(torch.uint8), dev(mt).view(torch.uint8))
    close(out, padded, 1e-6, 1e-6)                                     # (the band of test_packed_gpu: the rows fall into other row groups)
    da, dt = ops.masked_pool_packed_bwd(dev(dp), pa, pt)
    da_d, dt_d = ops.masked_pool_bwd(dev(dp), dev(ma).view(torch.uint8), dev(mt).view(torch.uint8), Na, Nt)
    assert torch.equal(da.cpu(), da_d.cpu().view(B * Na, D)[pa.gather]) and torch.equal(dt.cpu(), dt_d.cpu().view(B * Nt, D)[pt.gather])
    assert R.nerr(da, da_ref.view(B * Na, D)[pa.gather]) <= GRAD_NERR and R.nerr(dt, dt_ref.view(B * Nt, D)[pt.gather]) <= GRAD_NERR
    assert float(da.cpu()[~pa.real].abs().max()) == 0.0 and float(dt.cpu()[~pt.real].abs().max()) == 0.0      # representative pad rows


def test_masked_pool_molecule_without_any_row(ops):
    """The reference divides the (zero) sum by the (zero) count: NaN in every column of that molecule, which the forward kernels
    reproduce; the other molecules are not affected.  The backward kernels write exact zeros to the masked rows (every row of that
    molecule), where autograd would carry the NaN on."""
    Na, Nt, D = 7, 11, 68
    g = G(2)
    ca, ct = [3, 0, 7], [5, 0, 11]
    ma = torch.arange(Na).view(1, -1) < torch.tensor(ca).view(-1, 1)
    mt = torch.arange(Nt).view(1, -1) < torch.tensor(ct).view(-1, 1)
    a, t, dp = torch.randn(3, Na, D, generator=g), torch.randn(3, Nt, D, generator=g), torch.randn(3, D, generator=g)
    ref = R.masked_pool(a, t, ma, mt)
    assert bool(torch.isnan(ref[1]).all()) and bool(torch.isfinite(ref[[0, 2]]).all())
    mad, mtd = dev(ma).view(torch.uint8), dev(mt).view(torch.uint8)
    pa, pt = _packing(ca, Na), _packing(ct, Nt)
    ap, tp = a.view(3 * Na, D)[pa.gather].contiguous(), t.view(3 * Nt, D)[pt.gather].contiguous()
    for out in (ops.masked_pool_fwd(dev(a), dev(t), mad, mtd), ops.masked_pool_packed_fwd(dev(ap), dev(tp), pa, pt)):
        assert bool(torch.isnan(out[1]).all())
        close(out[[0, 2]], ref[[0, 2]], 1e-5, 1e-6)
    da, dt = ops.masked_pool_bwd(dev(dp), mad, mtd, Na, Nt)
    assert float(da[1].abs().max()) == 0.0 and float(dt[1].abs().max()) == 0.0 and bool(torch.isfinite(da).all() & torch.isfinite(dt).all())
    dap, dtp = ops.masked_pool_packed_bwd(dev(dp), pa, pt)
    assert torch.equal(dap.cpu(), da.cpu().view(3 * Na, D)[pa.gather]) and torch.equal(dtp.cpu(), dt.cpu().view(3 * Nt, D)[pt.gather])


# ================================================================================================ embeddings
def _ids(vocab, shape, g):
    if vocab == 31:                                   # heavy duplication, not a multiple of 8
        return torch.randint(0, vocab, shape, generator=g)
    return (vocab * torch.rand(shape, generator=g) ** 4).long().clamp_(max=vocab - 1)          # skewed: some ids repeat hundreds of times


@pytest.mark.parametrize("padding_idx", [1, -1])
@pytest.mark.parametrize("vocab", [31, 600])
def test_embedding_bwd_scatter_and_gemm(ops, vocab, padding_idx):
    D, shape = 512, (8, 512)
    g = G(vocab)
    ids = _ids(vocab, shape, g)
    counts = torch.bincount(ids.reshape(-1), minlength=vocab)
    assert int(counts.max()) >= 100 and int(counts[1]) > 0
    dout = rt(torch.randn(*shape, D, generator=g))          # (bf16-representable: the GEMM path takes dout in bf16)
    ref = R.embedding_grad(ids, dout, vocab, padding_idx)
    dt = torch.zeros(vocab, D, device="cuda")
    ops.embedding_bwd(dev(ids), dev(dout), dt, padding_idx=padding_idx)
    dt2 = torch.zeros(vocab, D, device="cuda")
    ops.embedding_bwd_gemm(dev(ids), dev(dout.to(torch.bfloat16)).view(-1, D), dt2, padding_idx=padding_idx)
    for name, got in (("scatter", dt), ("gemm", dt2)):
        e = R.nerr(got, ref)
        assert e <= GRAD_NERR, f"{name}: nerr {e:.3g}"
        if padding_idx >= 0:
            assert float(got[padding_idx].abs().max()) == 0.0
        else:
            assert float(got[1].abs().max()) > 0.0
        assert float(got.cpu()[counts == 0].abs().max() if bool((counts == 0).any()) else 0.0) == 0.0


def test_roberta_position_ids_long_rows(ops):
    L, pad = 512, 1
    ids = torch.randint(2, 600, (5, L), generator=G(9))
    ids[0, :37] = pad                                  # leading
    ids[1, -100:] = pad                                # trailing
    ids[2, 63:66] = pad; ids[2, 200:264] = pad; ids[2, 300] = pad; ids[2, 511] = pad          # interior, across the 64-wide chunks
    ids[4, :] = pad                                    # nothing but pads
    got = ops.roberta_position_ids(dev(ids), pad)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), O.roberta_position_ids(ids, pad))
