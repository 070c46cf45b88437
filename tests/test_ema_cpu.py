"""Weight averaging without a GPU: the two entry points are declared and exported and the ABI constant has not moved; ema_decay_at is the
kernel's fp32 schedule; the float64 reference of tests/ema_cases.py obeys the closed form of the recurrence; the case table reaches every
size, decay, warm-up setting, step and source of t; the declared instance and grid of both kernels are the library's own plan
(mmdti_stream_plan) at every size of the table and on both sides of the grid cap; and tasks.Trainer refuses a bad ema_decay at construction."""
import ctypes
import math

import numpy as np
import pytest
import torch

from mmdti_hip import _abi
from mmdti_hip.trainer import check_ema_decay, ema_decay_at

import ema_cases as E


def test_header_and_library_export_both_symbols_and_the_abi_constant_stays():
    protos = _abi.parse_header()
    dll = ctypes.CDLL(_abi.LIB_PATH)
    for name, nargs in (("mmdti_ema_update", 9), ("mmdti_ema_swap", 6)):
        assert name in protos and len(protos[name][1]) == nargs, name
        assert hasattr(dll, name), f"{name} not exported"
    assert protos["mmdti_ema_update"][2] == ["stream", "p", "ema", "n", "decay", "warmup", "step", "guard", "step_state"]
    assert protos["mmdti_ema_swap"][2] == ["stream", "p", "ema", "p_bf16", "p_f16", "n"]
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2 and dll.mmdti_abi_version() == 2
    src = open(_abi.HEADER).read()
    doc = src[src.index("weight averaging"):src.index("int mmdti_ema_swap(")]
    assert doc.count("Purely additive: MMDTI_ABI_VERSION does not move") == 2


def test_the_declared_plan_is_the_librarys_for_both_kernels():
    """instance() and launch() of ema_cases.py against mmdti_stream_plan, called as ops.ema_update / ops.ema_swap call the entry points:
    every size of the table with t from each source, the sizes round the 4096-workgroup cap (1024 elements a workgroup for the update,
    2048 for the swap), an empty arena (no launch), and the launchers' own refusals"""
    lib = _abi.lib()
    for n in E.SIZES + (0,):
        for source in E.SOURCES:
            got = E.assert_declared_plan(lib, False, n, source=source)
            assert n == 0 or got["launches"][0][:2] == ("ema_update_kernel", -(-n // 1024))
        for with_f16 in (True, False):
            got = E.assert_declared_plan(lib, True, n, with_f16=with_f16)
            assert n == 0 or got["launches"][0][:2] == ("ema_swap_kernel", -(-n // 2048))
    for swap, per in ((False, 1024), (True, 2048)):
        for n in (E.CAP * per - 1, E.CAP * per, E.CAP * per + 1, 3 * E.CAP * per + 7):
            assert E.assert_declared_plan(lib, swap, n)["launches"][0][1] == min(E.CAP, -(-n // per))
    import stream_cases as S
    with pytest.raises(_abi.MMDTIError, match="ema_update: no source of t"):
        S.stream_plan(lib, "ema_update", [S.PTR, S.PTR + 64, 0, 0], 8, a=0, f=0.9)
    with pytest.raises(_abi.MMDTIError, match="ema_swap: 16-byte alignment required"):
        S.stream_plan(lib, "ema_swap", [S.PTR, S.PTR + 64, S.PTR + 2, 0], 8)


def test_ema_decay_at_is_the_fp32_schedule_and_never_decreases():
    f = np.float32
    for decay in E.DECAYS + (0.5, 0.9999):
        for t in (1, 2, 9, 100, 10 ** 5):
            want = min(f(decay), (f(1) + f(t)) / (f(10) + f(t)))
            got = ema_decay_at(t, decay, True)
            assert isinstance(got, np.float32) and got == want, (decay, t, got, want)
            assert ema_decay_at(t, decay, False) == f(decay)
        seq = [ema_decay_at(t, decay, True) for t in range(1, 3000)]
        assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[0] == f(2) / f(11) and ema_decay_at(10 ** 5, decay, True) == f(decay)
    # the first steps follow (1 + t) / (10 + t), the cap takes over where it is smaller: 0.9 from t = 80 on
    assert ema_decay_at(79, 0.9, True) < f(0.9) and ema_decay_at(80, 0.9, True) == f(0.9)


def test_reference_obeys_the_closed_form_for_a_constant_p():
    """for constant p: e_n - p == (e_0 - p) prod d_t, within float64 rounding"""
    g = torch.Generator().manual_seed(3)
    p, e0 = torch.randn(257, generator=g), torch.randn(257, generator=g)
    for decay, warmup in ((0.9, True), (0.999, True), (0.9, False)):
        n = 40
        ws = [E.weight32(t, decay, warmup) for t in range(1, n + 1)]
        e, bound = E.recurrence(e0, [p] * n, ws)
        prod = math.prod(1.0 - float(w) for w in ws)
        want = (e0.to(E.F64) - p.to(E.F64)) * prod
        assert float(((e - p.to(E.F64)) - want).abs().max()) <= 64 * n * 2.0 ** -53 * 8.0
        assert bound.shape == e.shape and float(bound.min()) > 0
    # a skipped step (None) leaves the average and consumes no weight
    a, _ = E.recurrence(e0, [p, None, p], ws[:2])
    b, _ = E.recurrence(e0, [p, p], ws[:2])
    assert torch.equal(a, b)
    # one update is the single-step reference
    one, bnd = E.reference(p, e0, ws[0])
    assert torch.equal(one, E.recurrence(e0, [p], ws[:1])[0]) and torch.equal(bnd, E.recurrence(e0, [p], ws[:1])[1])


def test_the_case_table_reaches_every_setting_and_the_inputs_hold_the_specials():
    cases = E.update_cases()
    assert len(cases) == 7 * 3 * 2 * 2 * 3
    for key, want in (("n", {1, 7, 8, 1023, 1024, 4099, 262147}), ("decay", {0.9, 0.999}), ("warmup", {True, False}), ("t", {1, 5, 1000}),
                      ("source", {"value", "state", "guard"})):
        assert {c[key] for c in cases} == want
    assert any(n % 4 for n in E.SIZES) and any(n % 8 == 0 for n in E.SIZES) and max(E.SIZES) > 2048 * 2
    for n in E.SIZES:
        p, e = E.make_inputs(n, 0)
        assert p.shape == e.shape == (n,) and torch.isfinite(p).all() and torch.isfinite(e).all()
        assert torch.isfinite((p - e)).all()                       # fp32: no difference overflows
        d = (p - e)[(p - e) != 0].abs()
        assert d.numel() == 0 or float(d.min()) >= 2.0 ** -126     # ... and none is subnormal
        if n >= 1023:
            both = torch.cat([p, e]).abs()
            assert bool((both == 0).any()) and bool((both == 1e30).any()) and bool((both == torch.tensor(1e-30)).any())
            assert bool((p[-8:].abs() == 0).any() or (e[-8:].abs() == 0).any())         # a special inside the last block of 8


def test_trainer_refuses_a_bad_ema_decay_without_a_device():
    from mmdti_hip.tasks import Trainer
    base = dict(task="regression", metrics="mse", use_cuda=False)
    for bad in (1.0, 0, -0.1, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="ema_decay"):
            Trainer(**base, ema_decay=bad)
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema_decay(bad)
    t = Trainer(**base)
    assert t.ema_decay is None and t.ema_warmup is True
    t = Trainer(**base, ema_decay=0.99, ema_warmup=False)
    assert t.ema_decay == 0.99 and t.ema_warmup is False
    assert check_ema_decay(None) is None and check_ema_decay(0.5) == 0.5
