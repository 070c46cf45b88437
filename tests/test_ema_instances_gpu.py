"""ema_update_kernel and ema_swap_kernel of csrc/elementwise.hip on the device, through ops.ema_update / ops.ema_swap, against the float64
reference and the derived bound of tests/ema_cases.py: every size x decay x warm-up x t x source of t for the update; the exchange as bit
patterns and the shadows against the library's own casts for the swap.  Every device buffer is a view cut from an arena whose two guard
zones hold a sentinel: after the launches no sentinel has moved (tests/test_ema_cpu.py checks the table and the reference on the CPU)."""
import pytest
import torch

from mmdti_hip import _abi, ops

import ema_cases as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, BF16, F16 = E.F64, E.F32, E.BF16, E.F16
PAD = 64                                   # elements on both sides of a view: a multiple of 8, so every view stays 16-byte aligned


class Guarded:
    """a device copy of x (or n sentinel elements of dtype) between two guard zones"""

    def __init__(self, x=None, n=None, dtype=F32):
        n = x.numel() if x is not None else n
        dtype = x.dtype if x is not None else dtype
        self.buf = torch.full((n + 2 * PAD,), E.SENT32, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + n]
        if x is not None:
            self.view.copy_(x)
        self.sent = self.buf[:PAD].clone()
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        ibits = torch.int32 if self.buf.dtype == F32 else torch.int16
        s = self.sent.view(ibits)
        return torch.equal(self.buf[:PAD].view(ibits), s) and torch.equal(self.buf[self.buf.numel() - PAD:].view(ibits), s)


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == F32 else torch.int16).cpu()


def _t_args(source, t):
    """-> (step by value, guard, step state): exactly one of them carries t, the others carry values the kernel must not read"""
    if source == "value":
        return t, None, None
    if source == "state":
        return 7, None, torch.tensor([t, 123.0, 0.5, 0.5], dtype=F32, device=DEV)
    guard = torch.tensor([t, 3.0, 0.0, 0.5, 0.5, 0.0, 0.0, 0.0], dtype=F32, device=DEV)
    state = torch.tensor([t + 11.0, 123.0, 0.5, 0.5], dtype=F32, device=DEV)          # (given too: the guard comes first)
    return 7, guard, state


@pytest.mark.parametrize("source", E.SOURCES)
@pytest.mark.parametrize("n", E.SIZES)
def test_update_instance(n, source):
    p, e0 = E.make_inputs(n, 1)
    E.assert_declared_plan(_abi.lib(), False, n, source=source)          # (host only: the launches below are the declared ones)
    P = Guarded(p)
    worst = 0.0
    for c in (c for c in E.update_cases() if c["n"] == n and c["source"] == source):
        A = Guarded(e0)
        step, guard, state = _t_args(source, c["t"])
        ops.ema_update(P.view, A.view, c["decay"], c["warmup"], step, guard, state)
        torch.cuda.synchronize()
        assert A.intact() and P.intact(), (c, "a store outside the buffer")
        assert torch.equal(_bits(P.view), _bits(p)), (c, "p was written")
        ref, bound = E.reference(p, e0, E.weight32(c["t"], c["decay"], c["warmup"]))
        got = A.view.cpu().to(F64)
        assert torch.isfinite(got).all()
        err = (got - ref).abs()
        ratio = float((err / bound.clamp(min=1e-300)).max())
        assert bool((err <= bound).all()), (c, "worst |got - ref| / bound", ratio)
        exact = (p == e0)
        assert torch.equal(_bits(A.view)[exact], _bits(e0)[exact]), (c, "p == ema must leave ema as it is")
        worst = max(worst, ratio)
    print(f"ema_update n={n} t from {source}: worst |got - ref| / (3 * 2^-24 * M) = {worst:.3f}")


@pytest.mark.parametrize("n", (7, 4099))
def test_a_set_guard_flag_leaves_the_average_and_reads_no_t(n):
    p, e0 = E.make_inputs(n, 2)
    P, A = Guarded(p), Guarded(e0)
    guard = torch.tensor([float("nan"), 0.0, 1.0, 0.5, 0.5, 0.0, 0.0, 0.0], dtype=F32, device=DEV)       # t = NaN would poison every element
    state = torch.tensor([float("nan"), 0.0, 0.0, 0.0], dtype=F32, device=DEV)
    ops.ema_update(P.view, A.view, 0.9, True, 0, guard, state)
    torch.cuda.synchronize()
    assert torch.equal(_bits(A.view), _bits(e0)) and A.intact()
    guard[E.NF_FLAG], guard[E.NF_T] = 0.0, 4.0
    ops.ema_update(P.view, A.view, 0.9, True, 0, guard, state)
    torch.cuda.synchronize()
    ref, bound = E.reference(p, e0, E.weight32(4, 0.9, True))
    assert bool(((A.view.cpu().to(F64) - ref).abs() <= bound).all()) and not torch.equal(_bits(A.view), _bits(e0))


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _abi.lib()
    x, y = torch.zeros(64, dtype=F32, device=DEV), torch.ones(64, dtype=F32, device=DEV)
    b, h = torch.zeros(64, dtype=BF16, device=DEV), torch.zeros(64, dtype=F16, device=DEV)
    s = ops._stream()
    bad_update = ((x.data_ptr() + 4, y.data_ptr(), 8, 0.9, 1, 1, 0, 0), (x.data_ptr(), y.data_ptr() + 8, 8, 0.9, 1, 1, 0, 0),       # misaligned
                  (0, y.data_ptr(), 8, 0.9, 1, 1, 0, 0), (x.data_ptr(), x.data_ptr(), 8, 0.9, 1, 1, 0, 0), (x.data_ptr(), y.data_ptr(), -1, 0.9, 1, 1, 0, 0),
                  (x.data_ptr(), y.data_ptr(), 8, 0.9, 1, 0, 0, 0),                                                                     # no source of t
                  (x.data_ptr(), y.data_ptr(), 8, 1.0, 1, 1, 0, 0), (x.data_ptr(), y.data_ptr(), 8, 0.0, 1, 1, 0, 0),
                  (x.data_ptr(), y.data_ptr(), 8, float("nan"), 1, 1, 0, 0))
    for a in bad_update:
        assert lib._dll.mmdti_ema_update(s, *a) == lib.const["MMDTI_ERR_INVALID"], a
        with pytest.raises(_abi.MMDTIError, match="ema_update"):
            lib.mmdti_ema_update(s, *a)
    bad_swap = ((x.data_ptr() + 4, y.data_ptr(), b.data_ptr(), h.data_ptr(), 8), (x.data_ptr(), y.data_ptr() + 4, b.data_ptr(), 0, 8),
                (x.data_ptr(), y.data_ptr(), b.data_ptr() + 2, 0, 8), (x.data_ptr(), y.data_ptr(), b.data_ptr(), h.data_ptr() + 2, 8),
                (x.data_ptr(), y.data_ptr(), 0, 0, 8), (x.data_ptr(), x.data_ptr(), b.data_ptr(), 0, 8), (x.data_ptr(), y.data_ptr(), b.data_ptr(), 0, -1))
    for a in bad_swap:
        assert lib._dll.mmdti_ema_swap(s, *a) == lib.const["MMDTI_ERR_INVALID"], a
        with pytest.raises(_abi.MMDTIError, match="ema_swap"):
            lib.mmdti_ema_swap(s, *a)
    lib.mmdti_ema_update(s, x.data_ptr(), y.data_ptr(), 0, 0.9, 1, 1, 0, 0)            # n = 0: nothing to do, no launch
    lib.mmdti_ema_swap(s, x.data_ptr(), y.data_ptr(), b.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0 and float((y - 1).abs().sum()) == 0.0 and float(b.float().abs().sum()) == 0.0


def _casts(x):
    """the library's own roundings of a device fp32 tensor: mmdti_cast_f32_bf16 / mmdti_cast_f32_f16 (no dropout)"""
    n = x.numel()
    src = torch.empty(n + 8, dtype=F32, device=DEV)[:n].copy_(x)
    yb, yh = torch.empty(n + 8, dtype=BF16, device=DEV)[:n], torch.empty(n + 8, dtype=F16, device=DEV)[:n]
    lib = _abi.lib()
    lib.mmdti_cast_f32_bf16(ops._stream(), src.data_ptr(), yb.data_ptr(), n, 0.0, 0, 0)
    lib.mmdti_cast_f32_f16(ops._stream(), src.data_ptr(), yh.data_ptr(), n, 0.0, 0, 0)
    return yb, yh


@pytest.mark.parametrize("with_f16", [True, False])
@pytest.mark.parametrize("n", E.SIZES)
def test_swap_instance(n, with_f16):
    p, e = E.make_inputs(n, 3)
    if n >= 1023:                              # bit patterns a float move must not touch, and values past the fp16 range
        p[9], e[10], p[n - 2], e[n - 3] = float("nan"), float("inf"), -0.0, 1e5
    E.assert_declared_plan(_abi.lib(), True, n, with_f16=with_f16)
    P, A = Guarded(p), Guarded(e)
    B, H = Guarded(n=n, dtype=BF16), Guarded(n=n, dtype=F16)
    sent16 = _bits(H.view).clone()
    ops.ema_swap(P.view, A.view, B.view, H.view if with_f16 else None)
    torch.cuda.synchronize()
    assert all(g.intact() for g in (P, A, B, H)), "a store outside a buffer"
    assert torch.equal(_bits(P.view), _bits(e)) and torch.equal(_bits(A.view), _bits(p)), "the exchange is not bit-exact"
    yb, yh = _casts(P.view)
    assert torch.equal(_bits(B.view), _bits(yb)), "bf16 shadow != mmdti_cast_f32_bf16 of the swapped-in values"
    if with_f16:
        assert torch.equal(_bits(H.view), _bits(yh)), "fp16 shadow != mmdti_cast_f32_f16 of the swapped-in values"
    else:
        assert torch.equal(_bits(H.view), sent16), "the fp16 shadow was written although it was not given"
    # twice is the identity, and the shadows follow
    ops.ema_swap(P.view, A.view, B.view, H.view if with_f16 else None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(P.view), _bits(p)) and torch.equal(_bits(A.view), _bits(e)) and all(g.intact() for g in (P, A, B, H))
    yb, yh = _casts(P.view)
    assert torch.equal(_bits(B.view), _bits(yb)) and (not with_f16 or torch.equal(_bits(H.view), _bits(yh)))
