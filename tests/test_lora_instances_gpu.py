"""Every instance of the LoRA kernels (mmdti_lora_fwd / _bwd / _dx: the 27 rows of MMDTI_PLAN_LORA) against the float64 reference of
tests/lora_cases.py, each product within the bound derived there from its accumulation length and operand magnitudes; B = 0 leaves y
unchanged to the bit; the deterministic backward repeats to the bit, never uses atomics and refuses a workspace that is too small;
refused shapes return the error before a launch."""
import pytest
import torch

import lora_cases as L

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from mmdti_hip import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    _ops.set_deterministic(False)


def dev(t):
    return t.cuda()


def within(got, ref, bnd, what):
    err = (got.detach().cpu().to(F64) - ref).abs()
    worst = (err - bnd).max().item()
    print(f"{what}: max |err| {err.max().item():.3e}, max bound {bnd.max().item():.3e}, worst (err - bound) {worst:.3e}")
    assert torch.isfinite(got).all(), what
    assert worst <= 0, f"{what}: error exceeds the bound by {worst:.3e}"


@pytest.mark.parametrize("c", L.FWD_CASES, ids=L.case_id)
def test_forward(ops, c):
    o = L.operands(c)
    ybuf = dev(o["ybuf"])
    y = L.view(c, ybuf, c["n_out"])
    t = ops.lora_fwd(dev(o["x"]), dev(o["A"]), dev(o["B"]), y, o["scale"])
    torch.cuda.synchronize()
    ref, bnd = L.ref_t(o)
    within(t, ref, bnd, "t")
    ref, bnd = L.ref_y(c, o, t.cpu())
    within(y, ref, bnd, "y")
    if c["sliced"]:   # the columns beside the slice are untouched
        n = c["n_out"]
        assert torch.equal(ybuf[:, :n].cpu(), o["ybuf"][:, :n]) and torch.equal(ybuf[:, 2 * n:].cpu(), o["ybuf"][:, 2 * n:])


@pytest.mark.parametrize("c", L.FWD_CASES, ids=L.case_id)
def test_forward_with_zero_B_keeps_y_to_the_bit(ops, c):
    o = L.operands(c)
    o["ybuf"][0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0]).to(o["ybuf"].dtype)   # (a negative zero must stay one)
    ybuf = dev(o["ybuf"])
    ops.lora_fwd(dev(o["x"]), dev(o["A"]), dev(torch.zeros_like(o["B"])), L.view(c, ybuf, c["n_out"]), o["scale"])
    torch.cuda.synchronize()
    assert torch.equal(ybuf.cpu().view(torch.int16), o["ybuf"].view(torch.int16))


def run_bwd(ops, c, o):
    dA, dB = dev(o["dA"]), dev(o["dB"])
    dy = L.view(c, dev(o["dybuf"]), c["n_out"])
    u = ops.lora_bwd(dev(o["x"]), dy, dev(o["t"]), dev(o["B"]), dA, dB, o["scale"])
    torch.cuda.synchronize()
    return u, dA, dB


@pytest.mark.parametrize("c", L.BWD_CASES, ids=L.case_id)
def test_backward(ops, c):
    o = L.operands(c)
    ops.set_deterministic(c["det"])
    try:
        u, dA, dB = run_bwd(ops, c, o)
        ref, bnd = L.ref_u(c, o)
        within(u, ref, bnd, "u")
        ref, bnd = L.ref_dB(c, o)
        within(dB, ref, bnd, "dB")
        ref, bnd = L.ref_dA(c, o, u.cpu())
        within(dA, ref, bnd, "dA")
        if c["det"]:
            u2, dA2, dB2 = run_bwd(ops, c, o)
            assert torch.equal(dA, dA2) and torch.equal(dB, dB2) and torch.equal(u, u2)
    finally:
        ops.set_deterministic(False)


def test_deterministic_backward_refuses_a_small_workspace(ops, monkeypatch):
    from mmdti_hip._abi import MMDTIError
    c = L.C("bwd", 4161, 512, 1536, 32, det=True)
    need = L.det_workspace_bytes(c["T"], c["n_in"], c["n_out"], c["r"])
    assert need > (1 << 20)
    monkeypatch.setenv("MMDTI_DET_WORKSPACE_MB", "1")
    o = L.operands(c)
    ops.set_deterministic(False)      # (forgets the workspaces registered so far: the next one is sized from the environment)
    ops.set_deterministic(True)
    try:
        with pytest.raises(MMDTIError, match="lora_bwd: deterministic mode: the workspace"):
            run_bwd(ops, c, o)
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("c", L.DX_CASES, ids=L.case_id)
def test_dx(ops, c):
    o = L.operands(c)
    dxbuf = dev(o["dxbuf"])
    dx = L.view(c, dxbuf, c["n_in"])
    ops.lora_dx(dev(o["u"]), dev(o["A"]), dx)
    torch.cuda.synchronize()
    ref, bnd = L.ref_dx(c, o)
    within(dx, ref, bnd, "dx")
    if c["sliced"]:
        n = c["n_in"]
        assert torch.equal(dxbuf[:, :64].cpu(), o["dxbuf"][:, :64]) and torch.equal(dxbuf[:, 64 + n:].cpu(), o["dxbuf"][:, 64 + n:])


@pytest.mark.parametrize("r, n_in, n_out, words", L.REFUSED)
def test_refused_shapes_launch_nothing(ops, r, n_in, n_out, words):
    from mmdti_hip._abi import MMDTIError
    T = 16
    x, A, B = (torch.ones(T, n_in), torch.ones(r, n_in), torch.ones(n_out, r))
    x, A, B = (dev(v.to(torch.bfloat16)) for v in (x, A, B))
    y = dev(torch.ones(T, n_out).to(torch.bfloat16))
    y0 = y.clone()
    with pytest.raises(MMDTIError, match=words):
        ops.lora_fwd(x, A, B, y, 2.0)
    dA, dB = dev(torch.ones(r, n_in)), dev(torch.ones(n_out, r))
    with pytest.raises(MMDTIError, match=words):
        ops.lora_bwd(x, y, dev(torch.ones(T, r).to(torch.bfloat16)), B, dA, dB, 2.0)
    if n_out == 64:                                     # (lora_dx has no `out`: the rank and `in` cases)
        dx = dev(torch.ones(T, n_in))
        with pytest.raises(MMDTIError, match=words):
            ops.lora_dx(dev(torch.ones(T, r).to(torch.bfloat16)), A, dx)
        assert bool((dx == 1).all())
    torch.cuda.synchronize()
    assert torch.equal(y, y0) and bool((dA == 1).all()) and bool((dB == 1).all())


@pytest.mark.parametrize("T, n_in, n_out, r, f16", [(130, 512, 1536, 32, False), (257, 64, 512, 8, True), (63, 512, 512, 16, True)])
def test_adapted_projection_against_float64_autograd(ops, T, n_in, n_out, r, f16):
    """The three kernels chained as functional.py chains them, against float64 AUTOGRAD of the un-merged function
    y = y0 + s.(x.A^T).B^T under the loss sum(y * dy): the backward formulas are autograd's here, not the ones the kernels were written
    from.  Operand values are exact in bf16 AND fp16 (bf16 values of at least 2^-10), so the forward's fp16 shadows, the backward's bf16
    shadows and the kernel's fp16 -> bf16 conversion of x all read the float64 leaves' own values.  Bounds: each product's
    (K + 8) 2^-23 sum of magnitudes, plus the stored bf16 t / u (2^-8 relative, and their own accumulation error) carried through the
    product that reads them, plus the rounding of a 16-bit output."""
    bf16, dt = torch.bfloat16, (torch.float16 if f16 else torch.bfloat16)
    g = torch.Generator().manual_seed(97 * T + r)

    def exact(*shape, scale=1.0):
        v = (torch.randn(*shape, generator=g) * scale).to(bf16).float()
        return torch.where(v.abs() < 2.0 ** -10, torch.full_like(v, 2.0 ** -10), v)
    x, A, B, dy, y0 = exact(T, n_in), exact(r, n_in, scale=n_in ** -0.5), exact(n_out, r, scale=0.2), exact(T, n_out, scale=0.1), exact(T, n_out)
    s = 16.0 / r
    xd, Ad, Bd = (v.double().requires_grad_() for v in (x, A, B))
    yd = y0.double() + s * (xd @ Ad.T) @ Bd.T
    (yd * dy.double()).sum().backward()
    # the device, as functional.py chains it
    y = dev(y0.to(dt))
    t = ops.lora_fwd(dev(x.to(dt)), dev(A.to(dt)), dev(B.to(dt)), y, s)
    dA, dB, dx = dev(torch.zeros(r, n_in)), dev(torch.zeros(n_out, r)), dev(torch.zeros(T, n_in))
    u = ops.lora_bwd(dev(x.to(dt)), dev(dy.to(bf16)), t, dev(B.to(bf16)), dA, dB, s)
    ops.lora_dx(u, dev(A.to(bf16)), dx)
    torch.cuda.synchronize()
    ax, aA, aB, ady = (v.double().abs() for v in (x, A, B, dy))
    t_ex, u_ex = (xd @ Ad.T).detach(), (s * dy.double() @ Bd).detach()
    d_t = L.unit(n_in) * (ax @ aA.T) + L.rounding_term(t_ex, bf16)
    d_u = L.unit(n_out) * s * (ady @ aB) + L.rounding_term(u_ex, bf16)
    within(t, t_ex, d_t, "t")
    within(u, u_ex, d_u, "u")
    to_f16 = 2.0 ** -25 if f16 else 0.0            # a bf16 t below fp16's normal range loses bits on its way into the second product
    y_ex = yd.detach()
    within(y, y_ex, s * (d_t + to_f16) @ aB.T + L.unit(r) * (s * (t_ex.abs() + d_t) @ aB.T + y0.double().abs()) + L.rounding_term(y_ex, dt), "y")
    within(dB, Bd.grad, s * ady.T @ d_t + L.unit(T) * s * ady.T @ (t_ex.abs() + d_t), "dB")
    within(dA, Ad.grad, d_u.T @ ax + L.unit(T) * (u_ex.abs() + d_u).T @ ax, "dA")
    within(dx, xd.grad, d_u @ aA + L.unit(r) * (u_ex.abs() + d_u) @ aA, "dx")
