"""The eight adam_group_kernel<GUARD, MASK, DECOUPLED> instantiations of csrc/elementwise.hip against the float64 reference of
tests/adam_group_cases.py, through mmdti_adam_step_grouped with explicit pointers, over three steps, at n = 1, 5, 8, 8 x 125 + 5 and the
size that passes the grid cap once with a ragged tail.  tests/test_adam_group_cases_cpu.py proves on the CPU that the table reaches every
instantiation, size, layout and table entry, that the fp32 emulation stays inside the bounds and that four wrong emulations do not.

Operands are cut from NaN-filled arenas, p / m / v and the shadows from sentinel-filled ones with guards on both sides: after the steps no
sentinel outside a view has moved.  p, m, v: worst |got - ref| / bound <= 1 and |gain| <= 6.  The shadows EQUAL the rounding of the
device's own p (fp16 saturating) wherever the pass stores them; masked blocks keep their bits in all five buffers; blocks of a group
whose lr_scale is 0 keep p and both shadows to the bit (the shadows: the sentinel) while m and v advance; a step under a set guard flag
leaves every buffer untouched.  With one group (1, wd) the coupled form EQUALS ops.adam_step, ops.adam_step_guarded and
ops.adam_step_masked as bit patterns in p, m, v and both shadows: the operations are the same, so this is a condition, not a tolerance."""
import pytest
import torch

from mmdti_hip import _abi, ops

import adam_group_cases as G
import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, BF16, F16 = S.F64, S.F32, S.BF16, S.F16
B1, B2, EPS = 0.9, 0.999, 1e-8
Bufs = lambda: S.Bufs(DEV)


def _inout(b, name, x):
    ptr = b.out(name, 1, x.numel(), x.dtype)
    b.outs[name].view[0, 0, 0].copy_(x.to(DEV))
    return ptr


def _launch(c, t):
    lib, b, n = _abi.lib(), Bufs(), c["n"]
    ptr = {k: _inout(b, k, t[k]) for k in ("p", "m", "v")}
    pb = b.out("pb", 1, n, BF16, on="bf16" in c["shadows"])
    ph = b.out("ph", 1, n, F16, on="f16" in c["shadows"])
    skip = t["skip"].to(DEV) if c["mask"] else None
    group = t["ids"].to(torch.uint8).to(DEV)
    table = t["table"].to(DEV)
    gs = torch.tensor([c["gs"]], dtype=F32, device=DEV) if c["gs"] is not None else None
    names = [k for k in ("p", "m", "v", "pb", "ph") if k in b.outs]
    snap = lambda: {k: b.outs[k].buf.view(b.outs[k].ibits).clone() for k in names}
    for st, g in zip(t["steps"], t["g"]):
        by_ptr = c["state"] or c["guard"]
        state = torch.tensor([st["step"], st["lr"], st["bc1"], st["bc2"]], dtype=F32, device=DEV) if c["state"] else None
        guard = torch.tensor([st["step"], 0.0, float(st["flag"]), st["bc1"], st["bc2"]], dtype=F32, device=DEV) if c["guard"] else None
        lr = 123.0 if c["state"] else st["lr"]                          # (with a step state the by-value rate must not be read)
        step = st["step"] if not by_ptr else 7
        before = snap() if st["flag"] else None
        lib.mmdti_adam_step_grouped(ops._stream(), ptr["p"], b.put(g), ptr["m"], ptr["v"], pb, n, lr, B1, B2, EPS, step, ops._p(gs), ops._p(state), ph,
                                    ops._p(guard), ops._p(skip), group.data_ptr(), table.data_ptr(), table.shape[0], int(c["decoupled"]))
        torch.cuda.synchronize()
        if before is not None:
            after = snap()
            assert all(torch.equal(before[k], after[k]) for k in names), "a step under a set guard flag wrote to a buffer"
    for k in names:
        assert b.outs[k].outside_untouched() == 0, (k, "a store outside the buffer")
    got = {k: b.outs[k].view[0, 0, 0].cpu() for k in names}
    assert not any(bool(torch.isnan(got[k]).any()) for k in ("p", "m", "v"))
    live = torch.ones(n, dtype=torch.bool) if not c["mask"] else ~t["skip"].bool().repeat_interleave(8)[:n]
    frozen = G.frozen_elements(c, t)
    for k in ("p", "m", "v"):
        assert torch.equal(got[k][~live].view(torch.int32), t[k][~live].view(torch.int32)), f"{k}: a masked element changed"
    assert torch.equal(got["p"][frozen].view(torch.int32), t["p"][frozen].view(torch.int32)), "p of a group with lr_scale 0 changed"
    if not c["zero"] and bool((live & frozen).any()) and not all(st["flag"] for st in t["steps"]):
        assert not torch.equal(got["m"][live & frozen], t["m"][live & frozen]), "m of a group with lr_scale 0 did not advance"
    written = live & ~frozen
    for k, dt in (("pb", BF16), ("ph", F16)):
        if k in got:
            bits = S.bits16(got[k])
            assert bool((bits[~written] == S.SENT16).all()), f"{k}: the shadow of a masked or frozen block was written"
            assert torch.equal(bits[written], S.bits16(S.round16(got["p"].to(F64), dt))[written]), f"{k}: not the rounding of the device's own fp32 p"
    if c["zero"] and c["layout"] == "one":
        for k in ("p", "m", "v"):
            assert torch.equal(got[k].view(torch.int32), t[k].view(torch.int32)), f"{k} moved with g = 0, m = v = 0 and no weight decay"
    return {k: got[k] for k in ("p", "m", "v")}


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_instance(c):
    t, ref = G.prepared(c["i"])
    G.assert_declared_plan(_abi.lib(), c)          # (host only: the launches below are the ones the case declares)
    got = _launch(c, t)
    res = G.evaluate(c, ref, got)
    assert set(res) == set(ref)
    for k, (ratio, z) in res.items():
        print(f"{G.case_id(c)} {k}: ratio {ratio:.4g} z {z:.3g}")
    for k, (ratio, z) in res.items():
        assert ratio <= 1.0 and abs(z) <= S.Z_MAX, f"{G.instance(c)} {G.case_id(c)} {k}: worst ratio {ratio:.4g}, gain {z:.3g}"


# ------------------------------------------------------------------------------------------------ against the existing kernels, bit for bit
N_EQ = 8 * 1000 + 5


def _operands(seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(N_EQ, generator=g)
    t = dict(p=rn(), m=0.1 * rn(), v=(0.1 * rn()) ** 2, g=[0.3 * rn() for _ in range(3)])
    t["p"][3], t["p"][N_EQ - 2], t["v"][5] = 1e5, -1e5, 0.0
    t["skip"] = (torch.rand((N_EQ + 7) // 8, generator=g) < 0.3).to(torch.uint8)
    t["skip"][-1] = 0                                                  # the ragged last block is taken
    return t


def _run(t, step_fn):
    """three steps on fresh device copies -> the five buffers as bit patterns"""
    d = {k: t[k].to(DEV).clone() for k in ("p", "m", "v")}
    pb = torch.full((N_EQ,), float("nan"), dtype=BF16, device=DEV)
    ph = torch.full((N_EQ,), float("nan"), dtype=F16, device=DEV)
    gs = torch.tensor([0.37], dtype=F32, device=DEV)
    for s, g in enumerate(t["g"]):
        step_fn(d["p"], g.to(DEV), d["m"], d["v"], pb, ph, gs, s + 1, 1e-3 * (1.0 - 0.2 * s))
    torch.cuda.synchronize()
    return dict(p=d["p"].view(torch.int32).cpu(), m=d["m"].view(torch.int32).cpu(), v=d["v"].view(torch.int32).cpu(), pb=pb.view(torch.int16).cpu(),
                ph=ph.view(torch.int16).cpu())


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("form", ["plain", "guarded", "masked", "masked_guarded", "state"])
def test_one_group_equals_the_existing_kernels_bit_for_bit(form, wd):
    t = _operands(11)
    group = torch.zeros((N_EQ + 7) // 8, dtype=torch.uint8, device=DEV)
    table = torch.tensor([[1.0, wd]], dtype=F32, device=DEV)
    skip = t["skip"].to(DEV) if form.startswith("masked") else None
    guard_of = lambda step: torch.tensor([step, 0.0, 0.0, 1.0 - 0.9 ** step, (1.0 - 0.999 ** step) ** 0.5], dtype=F32, device=DEV)
    state_of = lambda step, lr: torch.tensor([step, lr, 1.0 - 0.9 ** step, (1.0 - 0.999 ** step) ** 0.5], dtype=F32, device=DEV)

    def old(p, g, m, v, pb, ph, gs, step, lr):
        if form == "plain":
            ops.adam_step(p, g, m, v, pb, lr, B1, B2, EPS, wd, step, gs, None, p_f16=ph)
        elif form == "state":
            ops.adam_step(p, g, m, v, pb, 123.0, B1, B2, EPS, wd, step, gs, state_of(step, lr), p_f16=ph)
        elif form == "guarded":
            ops.adam_step_guarded(p, g, m, v, pb, lr, B1, B2, EPS, wd, guard_of(step), gs, None, p_f16=ph)
        else:
            ops.adam_step_masked(p, g, m, v, pb, lr, B1, B2, EPS, wd, step, skip, guard_of(step) if form == "masked_guarded" else None, gs, None, p_f16=ph)

    def new(p, g, m, v, pb, ph, gs, step, lr):
        guard = guard_of(step) if form in ("guarded", "masked_guarded") else None
        state = state_of(step, lr) if form == "state" else None
        ops.adam_step_grouped(p, g, m, v, pb, 123.0 if form == "state" else lr, B1, B2, EPS, step, group, table, False, skip, guard, gs, state, p_f16=ph)

    a, b = _run(t, old), _run(t, new)
    for k in ("p", "m", "v", "pb", "ph"):
        bad = (a[k] != b[k]).nonzero().flatten()
        assert bad.numel() == 0, f"{form} wd {wd}: {k} differs from the existing kernel in {bad.numel()} elements, the first at {int(bad[0])}"


def test_a_zero_scale_freezes_p_and_the_shadows_while_the_moments_follow_the_plain_update():
    """blocks alternate between (1, 0) and (0, 0): the frozen blocks keep p and both shadows to the bit, m and v EQUAL ops.adam_step's
    everywhere, and the live blocks' p and shadows EQUAL ops.adam_step's too"""
    t = _operands(12)
    nb = (N_EQ + 7) // 8
    group = (torch.arange(nb) % 2).to(torch.uint8).to(DEV)
    table = torch.tensor([[1.0, 0.0], [0.0, 0.0]], dtype=F32, device=DEV)
    frozen = (torch.arange(nb) % 2 == 1).repeat_interleave(8)[:N_EQ]
    plain = _run(t, lambda p, g, m, v, pb, ph, gs, step, lr: ops.adam_step(p, g, m, v, pb, lr, B1, B2, EPS, 0.0, step, gs, None, p_f16=ph))
    got = _run(t, lambda p, g, m, v, pb, ph, gs, step, lr: ops.adam_step_grouped(p, g, m, v, pb, lr, B1, B2, EPS, step, group, table, False, None, None, gs, None, p_f16=ph))
    nan16 = lambda dt: torch.full((1,), float("nan"), dtype=dt).view(torch.int16)
    assert torch.equal(got["m"], plain["m"]) and torch.equal(got["v"], plain["v"])
    assert torch.equal(got["p"][frozen], t["p"].view(torch.int32)[frozen]), "p of a frozen block changed"
    assert bool((got["pb"][frozen] == nan16(BF16)).all()) and bool((got["ph"][frozen] == nan16(F16)).all()), "a shadow of a frozen block was written"
    # (the first step's update is the plain one; from the second on the plain pass has moved the frozen blocks' p, the live ones agree throughout)
    for k in ("p", "pb", "ph"):
        assert torch.equal(got[k][~frozen], plain[k][~frozen]), k


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    lib = _abi.lib()
    x = torch.zeros(16, dtype=F32, device=DEV)
    group, table = torch.zeros(2, dtype=torch.uint8, device=DEV), torch.ones(1, 2, dtype=F32, device=DEV)
    call = lambda n, group_ptr, table_ptr, ng: lib.mmdti_adam_step_grouped(ops._stream(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, n, 1e-3, B1, B2,
                                                                        EPS, 1, 0, 0, 0, 0, 0, group_ptr, table_ptr, ng, 0)
    for bad in ((16, 0, table.data_ptr(), 1), (16, group.data_ptr(), 0, 1), (16, group.data_ptr(), table.data_ptr(), 0), (16, group.data_ptr(), table.data_ptr(), 257),
                (-1, group.data_ptr(), table.data_ptr(), 1)):
        with pytest.raises(_abi.MMDTIError):
            call(*bad)
    call(0, group.data_ptr(), table.data_ptr(), 1)                      # n = 0: nothing to do, no launch
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0
