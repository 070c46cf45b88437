"""The case table of the grouped Adam pass (adam_group_kernel<GUARD, MASK, DECOUPLED> of csrc/elementwise.hip, entry point
mmdti_adam_step_grouped), its input builder, float64 reference, bound and fp32 emulation, shared by test_adam_group_cases_cpu.py (which
proves that the table reaches all eight instantiations, every size, layout and table entry, that the emulation stays inside the bound
and that four wrong emulations do not) and test_adam_group_instances_gpu.py (which holds the kernels to the reference on the device).
The pattern, the helpers and the Adam bound are those of stream_cases.py.

SIZES.  One thread takes one aligned block of 8 elements, a workgroup of 256 at most 2048 elements a round, grid_for caps a launch at
4096 workgroups: n = 1, 5 (one ragged block), 8 (one full block), 8 x 125 + 5 (full blocks and a ragged tail) and 8388608 + 8 x 129 + 5,
which passes the cap once (two rounds) with a ragged tail.  The large size runs in two of the eight instantiations (a float64 chain over
8.4 M elements takes seconds on the host); the other six take 8 x 125 + 5 in its place.

LAYOUTS of the group ids (one byte per block of 8): `one` group; ids `alternate` from block to block over a table of four; a `single`
block of a frozen group between two long runs; the `last`, ragged block in a group of its own; `clamped`: ids >= ngroups, which the kernel
takes as ngroups - 1.  TABLE4 holds the scales 1, 0.37 and 0 and the decays 0 and 0.01.

WHAT IS HELD.  A float64 statement of the kernel's update over three steps, the errors of p, m, v carried from step to step, as
stream_cases.adam_chain does, with per-element lr_i = lr s and wd_i.  The bound extends adam_chain's by the new rounding points:
    lr_i = lr s: one rounding, so the step's relative error grows from 3 U to 4 U:
                step = (lr_i / bc1) m / den: |step| (4 U + E_bc1 / bc1 + L_den / den) + (lr_i / bc1) L_m / den
    coupled     g' = g gs + wd_i p: 3 U (|g gs| + |wd_i p|) + wd_i L_p                       (adam_chain's, wd per element)
    decoupled   three roundings on p before the update -- lw = lr_i wd_i (with lr_i's own: 2 U lw), keep = 1 - lw (U |keep|), p' = p keep (U |p'|):
                L_p' = |keep| L_p + |p| (2 U lw + U |keep|) + U |p keep|;   g' = g gs: 3 U |g gs| (adam_chain's form at wd = 0)
    m, v, r, den as in adam_chain;   p: L_p' + L_step + U |p|
The kernel spells m, v and g' as fused multiply-adds (one rounding where the bound allows two): inside the bound.  lr_scale = 0: the step is
0 and keep is 1, so the reference keeps p exactly; the kernel does not store p or the shadows of such a block at all.  Masked blocks keep
their bits in all five buffers; a set guard flag leaves every buffer untouched; the shadows EQUAL the rounding of the device's own p."""
import functools
import math

import numpy as np
import torch

import stream_cases as S
from stream_cases import BF16, F16, F32, F64, U, CAP, NF_FLAG, SENT16, bits16, case_id, evaluate, grid_for  # noqa: F401

BIGG = 8388608 + 8 * 129 + 5
MID = 8 * 125 + 5
SIZES = (1, 5, 8, MID, BIGG)
LAYOUTS = ("one", "alternate", "single", "last", "clamped")
TABLE4 = ((1.0, 0.01), (0.37, 0.0), (0.0, 0.01), (0.37, 0.01))
CLAMPED_ID = 200
ALL_KERNELS = tuple(f"adam_group_kernel<{g}, {m}, {d}>" for g in ("false", "true") for m in ("false", "true") for d in ("false", "true"))
BIG_IN = ((False, False, False), (True, True, True))            # (guard, mask, decoupled) of the two instantiations that run BIGG
#        n     layout       wd1    gs    state  shadows         zero       (wd1: the decay of layout `one`'s only group)
OPTS = ((BIGG, "alternate", None, None, False, ("bf16",), False),
        (MID, "single", None, 0.37, True, ("f16",), False),
        (MID, "clamped", None, None, True, ("bf16", "f16"), False),
        (MID, "last", None, 0.37, False, ("bf16",), False),
        (1, "one", 0.01, None, True, ("bf16", "f16"), False),
        (5, "clamped", None, 0.37, False, (), False),
        (8, "last", None, None, False, ("bf16", "f16"), False),
        (MID, "one", 0.0, None, False, ("bf16", "f16"), True),
        (MID, "alternate", None, 0.37, True, ("bf16",), True))

CASES = []


def _build():
    for guard in (False, True):
        for mask in (False, True):
            for dec in (False, True):
                for n, layout, wd1, gs, state, shadows, zero in OPTS:
                    if n == BIGG and (guard, mask, dec) not in BIG_IN:
                        n = MID
                    CASES.append(dict(kind="adam_group", i=len(CASES), guard=guard, mask=mask, decoupled=dec, n=n, layout=layout, wd1=wd1, gs=gs,
                                      state=state, shadows=shadows, zero=zero))


_build()


def instance(c):
    b = lambda x: "true" if x else "false"
    return (f"adam_group_kernel<{b(c['guard'])}, {b(c['mask'])}, {b(c['decoupled'])}>",)


def launch(c):
    """(workgroups, elements per workgroup and round, elements)"""
    return grid_for(c["n"], 256 * 8), 256 * 8, c["n"]


def rounds(c):
    g, per, items = launch(c)
    return -(-items // (g * per))


def library_plan(lib, c):
    """mmdti_stream_plan's answer for mmdti_adam_step_grouped with the addresses the case gives (stream_cases.stream_plan)"""
    on = lambda x: S.PTR if x else 0
    ptrs = [S.PTR] * 4 + [on("bf16" in c["shadows"]), on("f16" in c["shadows"]), on(c["state"]), on(c["guard"]), on(c["mask"]), S.PTR, S.PTR]
    return S.stream_plan(lib, "adam_step_grouped", ptrs, c["n"], a=7 if c["state"] or c["guard"] else 1, b=len(table_of(c)), c=int(c["decoupled"]))


def declared_plan(c):
    return dict(launches=S.flat(instance(c)[0], launch(c)[0]), wgs=0)


def assert_declared_plan(lib, c):
    got, want = library_plan(lib, c), declared_plan(c)
    assert got == want, (case_id(c), got, want)
    return got


def table_of(c):
    return ((1.0, c["wd1"]),) if c["layout"] == "one" else TABLE4


def group_ids(c):
    """one id per block of 8 (int64; the device gets them as bytes)"""
    nb, lay = (c["n"] + 7) // 8, c["layout"]
    if lay == "one":
        return torch.zeros(nb, dtype=torch.int64)
    if lay == "alternate":
        return torch.arange(nb) % 4
    if lay == "single":
        ids = torch.full((nb,), 3, dtype=torch.int64)
        ids[:nb // 2] = 1
        ids[nb // 2] = 2                                    # one frozen block (lr_scale 0) between two long runs
        return ids
    if lay == "last":
        ids = torch.zeros(nb, dtype=torch.int64)
        ids[-1] = 1 + c["i"] % 2                            # (0.37, 0) in one case, the frozen (0, 0.01) in the next
        return ids
    assert lay == "clamped"
    ids = torch.randint(0, 4, (nb,), generator=torch.Generator().manual_seed(977 * c["i"] + 1))
    ids[::3] = CLAMPED_ID                                   # >= ngroups: the kernel takes ngroups - 1
    return ids


def make_inputs(c):
    """stream_cases' Adam operands, steps and skip mask for the same options, plus the ids and the table"""
    t = S.make_inputs(dict(kind="adam", i=1000 + c["i"], n=c["n"], guard=c["guard"], mask=c["mask"], state=c["state"], zero=c["zero"]))
    t["ids"] = group_ids(c)
    t["table"] = torch.tensor(table_of(c), dtype=F32)
    return t


MUTATIONS = ("swap_decay", "gid_shift", "decay_no_lr", "cols_swapped")


def group_chain(c, t, dt=F64, mut=None):
    """three steps -> {p, m, v: (value, bound)} after the last (masked elements and flagged steps keep what they held)"""
    f = lambda x: x.to(dt)
    T = lambda x: torch.tensor(float(x), dtype=dt)
    n = c["n"]
    p, m, v = f(t["p"]), f(t["m"]), f(t["v"])
    Lp, Lm, Lv = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    b1, b2, eps = np.float32(0.9), np.float32(0.999), np.float32(1e-8)
    ob1, ob2 = T(np.float32(1) - b1), T(np.float32(1) - b2)
    b1, b2, eps = T(b1), T(b2), T(eps)
    gs = T(np.float32(c["gs"] if c["gs"] is not None else 1.0))
    ng = t["table"].shape[0]
    ids = t["ids"].clamp(max=ng - 1)                        # (an id >= ngroups counts as the last group)
    if mut == "gid_shift":                                  # the id of element i read at i >> 2 instead of i >> 3
        gid = ids[(torch.arange(n) >> 2).clamp(max=ids.numel() - 1)]
    else:
        gid = ids.repeat_interleave(8)[:n]
    tab = f(t["table"])
    s, wd = (tab[gid, 1], tab[gid, 0]) if mut == "cols_swapped" else (tab[gid, 0], tab[gid, 1])
    decoupled = c["decoupled"] != (mut == "swap_decay")
    live = torch.ones(n, dtype=torch.bool) if not c["mask"] else ~t["skip"].bool().repeat_interleave(8)[:n]
    for st, g in zip(t["steps"], t["g"]):
        if st["flag"]:
            continue
        lr, bc1, bc2 = T(np.float32(st["lr"])), T(st["bc1"]), T(st["bc2"])
        if dt == F32 and not st["E1"] == 0.0:
            bc1, bc2 = T(np.float32(1) - np.power(np.float32(0.9), np.float32(st["step"]))), T(np.sqrt(np.float32(1) - np.power(np.float32(0.999), np.float32(st["step"]))))
        lri = lr * s
        gsc = f(g) * gs
        if decoupled:
            lw = wd if mut == "decay_no_lr" else lri * wd
            keep = 1 - lw
            pd = p * keep
            gi = gsc
        else:
            pd = p
            gi = gsc + wd * p
        mi = b1 * m + ob1 * gi
        vi = b2 * v + ob2 * gi * gi
        r = torch.sqrt(vi)
        den = r / bc2 + eps
        step = (lri / bc1) * mi / den
        pn = pd - step
        if dt == F64:
            if decoupled:
                Lpd = keep.abs() * Lp + p.abs() * (2 * U * lw + U * keep.abs()) + U * pd.abs()
                Lg = 3 * U * gsc.abs()
            else:
                Lpd = Lp
                Lg = 3 * U * (gsc.abs() + (wd * p).abs()) + wd * Lp
            Lmn = 3 * U * ((b1 * m).abs() + (ob1 * gi).abs()) + b1 * Lm + ob1 * Lg
            Lvn = 3 * U * (b2 * v + ob2 * gi * gi) + b2 * Lv + 2 * ob2 * gi.abs() * Lg
            Lr = torch.where(vi > 0, Lvn / (2 * r.clamp(min=1e-300)), torch.sqrt(Lvn)) + U * r
            Lden = Lr / bc2 + 2 * U * den + den * st["E2"] / bc2
            Lstep = step.abs() * (4 * U + st["E1"] / bc1 + Lden / den) + (lri / bc1) * Lmn / den
            Lpn = Lpd + Lstep + U * pn.abs()
            Lp, Lm, Lv = torch.where(live, Lpn, Lp), torch.where(live, Lmn, Lm), torch.where(live, Lvn, Lv)
        p, m, v = torch.where(live, pn, p), torch.where(live, mi, m), torch.where(live, vi, v)
    return dict(p=(p, Lp), m=(m, Lm), v=(v, Lv))


def reference(c, t):
    return group_chain(c, t, F64)


def emulate(c, t, mut=None):
    return {k: v[0] for k, v in group_chain(c, t, F32, mut).items()}


def frozen_elements(c, t):
    """elements whose group has lr_scale 0: the kernel stores neither p nor the shadows there"""
    ng = t["table"].shape[0]
    return (t["table"][t["ids"].clamp(max=ng - 1), 0] == 0).repeat_interleave(8)[:c["n"]]


@functools.lru_cache(maxsize=2)
def prepared(i):
    c = CASES[i]
    t = make_inputs(c)
    return t, reference(c, t)
