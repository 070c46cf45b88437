"""The case table, input builder and float64 reference of the weight-averaging kernels (ema_update_kernel and ema_swap_kernel of
csrc/elementwise.hip), shared by test_ema_cpu.py, test_ema_instances_gpu.py and test_ema_gpu.py.

UPDATE.  ema <- fma(w, p - ema, ema) in fp32, w = 1 - d, d = ema_decay_at(t, decay, warmup).  The reference is the same statement in
float64 with the kernel's OWN fp32 weight: e + w32 (p - e).  The bound is derived, not measured: with M = max(|p|, |ema|),
    the difference p - ema rounds once:            <= 2^-24 |p - ema| <= 2^-24 2M, and is then scaled by w <= 1
    the fma rounds once, to a value between p and ema: <= 2^-24 M
so |ema_gpu - ema_f64| <= 3 * 2^-24 * M per update; over k updates the errors add (each later update scales the earlier error by d < 1).

SIZES.  1, 7, 8: below and at one 16-byte vector pair; 1023, 1024: one workgroup's round of the update kernel with and without a ragged
tail; 4099: several workgroups and a tail of 3; 262147: more than one workgroup of the swap kernel (2048 elements each) with a tail of 3.
Every size is far below the grid cap (4096 workgroups): the grid-stride loops take one round, and the cap itself is the Adam pass's."""
import numpy as np
import torch

from mmdti_hip.trainer import ema_decay_at

F64, F32, BF16, F16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
U = 2.0 ** -24
SIZES = (1, 7, 8, 1023, 1024, 4099, 262147)
DECAYS = (0.9, 0.999)
WARMUPS = (True, False)
STEPS = (1, 5, 1000)
SOURCES = ("value", "state", "guard")
NF_T, NF_SKIPPED, NF_FLAG = 0, 1, 2
SENT32 = -7.0e-33                       # guard value round every device buffer of the instance tests (no input takes it)


ALL_KERNELS = ("ema_update_kernel", "ema_swap_kernel")
CAP = 4096


def grid_for(n, per):
    return max(1, min(CAP, -(-n // per)))


def instance(swap):
    return ALL_KERNELS[int(bool(swap))]


def launch(swap, n):
    """(workgroups, elements per workgroup and round): the update takes one 16-byte vector per thread, the swap one block of 8"""
    per = 256 * 8 if swap else 256 * 4
    return grid_for(n, per), per


def library_plan(lib, swap, n, source="value", with_f16=True):
    """mmdti_stream_plan's answer for mmdti_ema_update (t from `source`) or mmdti_ema_swap (stream_cases.stream_plan)"""
    import stream_cases as S
    if swap:
        return S.stream_plan(lib, "ema_swap", [S.PTR, S.PTR + 0x1000, S.PTR, S.PTR if with_f16 else 0], n)
    ptrs = [S.PTR, S.PTR + 0x1000, S.PTR if source == "guard" else 0, S.PTR if source in ("guard", "state") else 0]
    return S.stream_plan(lib, "ema_update", ptrs, n, a=1 if source == "value" else 7, f=0.9)


def declared_plan(swap, n):
    """one launch; none for an empty arena"""
    return dict(launches=[(instance(swap), launch(swap, n)[0], 1, 256, 0)] if n else [], wgs=0)


def assert_declared_plan(lib, swap, n, **kw):
    got, want = library_plan(lib, swap, n, **kw), declared_plan(swap, n)
    assert got == want, (swap, n, kw, got, want)
    return got


def update_cases():
    """one row per launch: every size x decay x warm-up x t x source of t"""
    return [dict(n=n, decay=d, warmup=w, t=t, source=s) for n in SIZES for s in SOURCES for d in DECAYS for w in WARMUPS for t in STEPS]


def make_inputs(n, seed):
    """p, ema: N(0, 1) with exact zeros (in p, in ema, in both), +-1e-30 and +-1e30 in one or both (the largest difference, 2e30, is
    finite in fp32; equal tiny values cancel exactly, so no difference is subnormal)"""
    g = torch.Generator().manual_seed(7919 * n + seed)
    p, e = torch.randn(n, generator=g), torch.randn(n, generator=g)
    specials = ((0.0, None), (None, 0.0), (0.0, 0.0), (1e-30, None), (None, -1e-30), (1e-30, 1e-30), (1e30, None), (None, -1e30), (1e30, -1e30),
                (1e30, 1e-30), (-0.0, 1.0))
    if n >= 64:
        for k, (a, b) in enumerate(specials):
            for i in (3 + 5 * k, n - 1 - 5 * k):                   # near the front and inside the ragged tail / the last workgroup
                if a is not None:
                    p[i] = a
                if b is not None:
                    e[i] = b
    elif n >= 7:
        p[1], e[2], p[4], e[5] = 0.0, 1e-30, 1e30, -1e30
    else:
        p[0], e[0] = 1e30, -1e-30
    return p, e


def weight32(t, decay, warmup):
    """the kernel's weight: float32(1) - ema_decay_at(t, decay, warmup)"""
    return np.float32(1) - ema_decay_at(t, decay, warmup)


def reference(p, e, w32):
    """float64 e + w32 (p - e) -> (value, bound)"""
    p64, e64 = p.to(F64), e.to(F64)
    return e64 + float(w32) * (p64 - e64), 3 * U * torch.maximum(p64.abs(), e64.abs())


def recurrence(e0, ps, weights):
    """the float64 recurrence over a sequence of parameter snapshots ps (None: a skipped step, the average stays) with the fp32 weights
    of the applied steps -> (value, bound): 3 * k * 2^-24 * M for k applied updates, M the largest |p| or |average| any of them saw"""
    e = e0.to(F64)
    M = torch.zeros_like(e)
    ws = iter(weights)
    k = 0
    for p in ps:
        if p is None:
            continue
        p64 = p.to(F64)
        M = torch.maximum(M, torch.maximum(p64.abs(), e.abs()))
        e = e + float(next(ws)) * (p64 - e)
        k += 1
    return e, 3 * k * U * M
