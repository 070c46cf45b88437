"""InfoNCE memory bank, kernel level: mmdti_infonce_bank_dir against the float64 reference (tests/infonce_bank_ref.py) and
mmdti_infonce_bank_push against the host model of the ring.

Inputs are L2-normalised randn as in test_kernels_gpu.test_infonce_matrix_pipe_kernels_vs_autograd, and the tolerances are that test's:
the row sum of the loss rtol 2e-5 / atol 1e-4, gradients rtol 1e-4 / atol 1e-7.
"""
import pytest
import torch

from infonce_bank_ref import RingModel, bank_dir_ref

pytestmark = pytest.mark.gpu

G = lambda s: torch.Generator().manual_seed(s)
unit = lambda n, D, seed: torch.nn.functional.normalize(torch.randn(n, D, generator=G(seed)), dim=-1)
LOSS_TOL, GRAD_TOL = dict(rtol=2e-5, atol=1e-4), dict(rtol=1e-4, atol=1e-7)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from mmdti_hip import ops as _ops
    return _ops


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol)


def make_case(Bg, D, cap, valid_slots, ids=False):
    """host tensors: q, k, bank, valid, bank_ids, ids_all (the last two None without ids).  valid_slots: 'all' | 'none' | a count of
    scattered slots."""
    q, k, bank = unit(Bg, D, 5), unit(Bg, D, 6), unit(cap, D, 7)
    valid = torch.zeros(cap, dtype=torch.uint8)
    if valid_slots == "all":
        valid.fill_(1)
    elif valid_slots != "none":
        valid[torch.randperm(cap, generator=G(8))[:valid_slots]] = 1
    # (an invalid slot may hold anything, a non-finite row included: it must not be read into the sums)
    bank[valid == 0] = float("nan")
    bank_ids = ids_all = None
    if ids:
        ids_all = torch.arange(1000, 1000 + Bg, dtype=torch.int64)
        bank_ids = torch.arange(5000, 5000 + cap, dtype=torch.int64)
    return q, k, bank, valid, bank_ids, ids_all


def run_dir(ops, case, row0, Bl):
    q, k, bank, valid, bank_ids, ids_all = case
    Bg, D = q.shape
    c = lambda t: None if t is None else t.cuda()
    loss = torch.zeros(1, device="cuda")
    dq, dk = torch.zeros(Bg, D, device="cuda"), torch.zeros(Bg, D, device="cuda")
    ops.infonce_bank_dir(c(q), c(k), row0, Bl, 0.1, loss, dq, dk, c(bank), c(valid), c(bank_ids), c(ids_all))
    return loss, dq, dk


def check_case(ops, case, row0, Bl):
    q, k, bank, valid, bank_ids, ids_all = case
    want = bank_dir_ref(q, k, row0, Bl, torch.nan_to_num(bank), valid, bank_ids, ids_all)
    loss, dq, dk = run_dir(ops, case, row0, Bl)
    print(f"loss {float(loss):.6f} ref {float(want[0]):.6f}  max|dq - ref| {float((dq.double().cpu() - want[1]).abs().max()):.3e}  "
          f"max|dk - ref| {float((dk.double().cpu() - want[2]).abs().max()):.3e}")
    close(loss, want[0].reshape(1), **LOSS_TOL)
    close(dq, want[1], **GRAD_TOL)
    close(dk, want[2], **GRAD_TOL)
    return loss, dq, dk


@pytest.mark.parametrize("Bg,Bl,row0,D,cap,valid_slots", [
    (2, 2, 0, 50, 16, "none"),           # the smallest batch, nothing valid
    (32, 32, 0, 50, 4096, "all"),        # the shape the feature is for: 128 splits
    (77, 30, 40, 64, 100, 37),           # ragged anchor and key tiles, the widest D, a cap that is no multiple of 16
    (300, 300, 0, 50, 16, "all"),        # one split
])
def test_bank_dir_against_float64_reference(ops, Bg, Bl, row0, D, cap, valid_slots):
    check_case(ops, make_case(Bg, D, cap, valid_slots), row0, Bl)


def test_empty_bank_equals_the_bankless_kernel_within_tolerance(ops):
    """(case 1's other face) nothing valid: the value and gradients of mmdti_infonce_dir, up to the summation order"""
    q, k, bank, valid, _, _ = make_case(77, 50, 64, "none")
    loss, dq, dk = run_dir(ops, (q, k, bank, valid, None, None), 16, 32)
    l0 = torch.zeros(1, device="cuda")
    dq0, dk0 = torch.zeros_like(dq), torch.zeros_like(dk)
    ops.infonce_dir(q.cuda(), k.cuda(), 16, 32, 0.1, l0, dq0, dk0)
    close(loss, l0, **LOSS_TOL)
    close(dq, dq0, **GRAD_TOL)
    close(dk, dk0, **GRAD_TOL)


def test_ids_mask_exactly_the_anchors_own_slots(ops):
    """(256, 64, 128, 50, 1000, all, with ids): the ids of anchors 128..131 sit in five slots each -- those anchors ignore exactly those
    slots, every other anchor sees them (the reference builds each anchor's key list by hand)."""
    Bg, Bl, row0, D, cap = 256, 64, 128, 50, 1000
    case = list(make_case(Bg, D, cap, "all", ids=True))
    slots = torch.randperm(cap, generator=G(9))[:20]
    for a in range(4):
        case[4][slots[5 * a:5 * a + 5]] = case[5][row0 + a]
    loss, dq, _ = check_case(ops, tuple(case), row0, Bl)
    # and the mask matters: without ids the four anchors' rows of dq differ, the other sixty are the same bits
    _, dq_all, _ = run_dir(ops, (*case[:4], None, None), row0, Bl)
    same = (dq == dq_all).all(dim=1).cpu()
    assert not same[row0:row0 + 4].any() and same[row0 + 4:row0 + Bl].all()


def test_dq_outside_the_anchor_rows_is_zero_and_the_bank_is_only_read(ops):
    Bg, Bl, row0, D, cap = 77, 30, 40, 64, 100
    q, k, bank, valid, bank_ids, ids_all = make_case(Bg, D, cap, 37, ids=True)
    dev = [t.cuda() for t in (bank, valid, bank_ids)]
    before = [t.clone() for t in dev]
    loss = torch.zeros(1, device="cuda")
    dq, dk = torch.zeros(Bg, D, device="cuda"), torch.zeros(Bg, D, device="cuda")
    ops.infonce_bank_dir(q.cuda(), k.cuda(), row0, Bl, 0.1, loss, dq, dk, dev[0], dev[1], dev[2], ids_all.cuda())
    assert float(dq[:row0].abs().max()) == 0.0 and float(dq[row0 + Bl:].abs().max()) == 0.0 and float(dq.abs().max()) > 0.0
    for was, now in zip(before, dev):
        assert torch.equal(was.view(torch.uint8), now.view(torch.uint8))          # (bytes: the NaN rows of invalid slots compare too)


def test_two_calls_give_the_same_bits(ops):
    case = make_case(32, 50, 4096, "all")
    a, b = run_dir(ops, case, 0, 32), run_dir(ops, case, 0, 32)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def ring_on_device(cap, D):
    return (torch.zeros(cap, D, device="cuda"), torch.zeros(cap, device="cuda", dtype=torch.uint8),
            torch.full((cap,), -1, device="cuda", dtype=torch.int64), torch.zeros(1, device="cuda", dtype=torch.int32))


def assert_ring(dev, model):
    rows, valid, ids, head = dev
    assert int(head) == model.head
    assert torch.equal(valid.cpu(), model.valid) and torch.equal(ids.cpu(), model.ids) and torch.equal(rows.cpu(), model.rows)


def test_push_wraps_and_drops_non_finite_rows(ops):
    cap, D = 10, 50
    dev, model = ring_on_device(cap, D), RingModel(cap, D)
    a, b, c = unit(7, D, 1), unit(7, D, 2), unit(cap, D, 3)
    b[2, 49] = float("inf")
    b[5, 0] = float("nan")
    for rows, ids in ((a, torch.arange(7)), (b, None), (c, torch.arange(100, 100 + cap))):      # n < cap twice across the wrap, then n == cap
        ops.infonce_bank_push(*dev, rows.cuda(), None if ids is None else ids.cuda())
        model.push(rows, ids)
        assert_ring(dev, model)
        if rows is b:
            assert model.valid.tolist() == [1, 1, 0, 1, 1, 1, 1, 1, 1, 0] and model.head == 4      # (the neighbours are kept)
    from mmdti_hip._abi import MMDTIError
    with pytest.raises(MMDTIError, match="at most cap"):
        ops.infonce_bank_push(*dev, unit(cap + 1, D, 4).cuda())


def test_push_replays_from_a_captured_graph(ops):
    cap, D, n = 10, 50, 4
    static_rows, static_ids = torch.zeros(n, D, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.int64)
    eager, graphed = ring_on_device(cap, D), ring_on_device(cap, D)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                     # (warm-up outside the capture, on a throw-away ring)
        ops.infonce_bank_push(*ring_on_device(cap, D), static_rows, static_ids)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.infonce_bank_push(*graphed, static_rows, static_ids)
    for step in range(3):                          # (the capture itself ran nothing: both rings start empty)
        rows, ids = unit(n, D, 20 + step).cuda(), torch.arange(10 * step, 10 * step + n, device="cuda")
        ops.infonce_bank_push(*eager, rows, ids)
        static_rows.copy_(rows)
        static_ids.copy_(ids)
        graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager, graphed):
        assert torch.equal(x, y)
    assert int(eager[3]) == (3 * n) % cap
