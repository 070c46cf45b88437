"""Case table and float64 references of the mean over REAL positions (mmdti_seq_mean_real_fwd / _bwd, InfoNCE(pool="real")).

Shapes: the smallest at which the kernels can go wrong.  B = 3 sequences; S walks round the 32 row phases of the wide forward kernel
(1, 31, 32, 33, 70: one phase, the last phase empty, every phase once, phase 0 twice, three rounds with a partial one) and the 32-row
slabs of the padded backward; D covers the wide form (D % 8 == 0: 8 = one piece of one slice, 64 = one full slice, 72 = a second,
partial slice, 512 = the head's width) and the scalar form the project-then-pool order needs (D = 50 in rows of ld = 56), plus rows of
ld = 50 that are not 8-column aligned at all (the scalar backward).  Masks: the three prefix lengths 1, S - 1, S; and a plane with a
hole in the middle of one sequence, one all-masked sequence and one full sequence.  Packed rows: lengths (5, 1, 33) under S = 33.
"""
import math

import torch

B = 3
SEQ_LENS = (1, 31, 32, 33, 70)
WIDTHS = ((8, 8), (64, 64), (72, 72), (512, 512), (50, 56), (50, 50))          # (D, ld)
AUX_MODES = (0, 1, 2)                                                          # none, a saved gelu', gelu' of the saved pre-activation
MASK_KINDS = ("prefix", "hole")
PACKED_LENS = (5, 1, 33)
PACKED_S = 33

FWD_BAND = (1e-5, 1e-6)                       # rtol, atol: the bands of the kernels these sit beside (test_packed_gpu.py)
BWD_BAND = {0: (1e-2, 1e-6), 1: (1e-2, 1e-5), 2: (1e-2, 1e-5)}


def wide_fwd(D, ld):
    """the 16-byte forward form (else the scalar kernel)"""
    return D % 8 == 0 and ld % 8 == 0


def wide_bwd(D, ld):
    """the 8-column backward form (else the scalar kernel, which takes no aux factor)"""
    return ld % 8 == 0


def mask_plane(kind, S):
    """[B, S] bool, True = real."""
    m = torch.zeros(B, S, dtype=torch.bool)
    if kind == "prefix":
        for b, n in enumerate((1, S - 1, S)):
            m[b, :n] = True
    elif kind == "hole":
        m[0] = True
        m[0, S // 2] = False                  # (S = 1: the sequence is then empty, like sequence 1)
        m[2] = True                           # sequence 1 stays all-masked
    else:
        raise ValueError(kind)
    return m


def cases():
    """every (S, D, ld, mask kind) of the padded form"""
    return [(S, D, ld, kind) for S in SEQ_LENS for D, ld in WIDTHS for kind in MASK_KINDS]


def inputs(S, D, ld, seed):
    """x [B*S, ld] fp32 holding bf16 values, dout [B, D] fp32, aux [B*S, ld] fp32 holding bf16 values"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * S, ld, generator=g).to(torch.bfloat16).float()
    dout = torch.randn(B, D, generator=g)
    aux = torch.randn(B * S, ld, generator=g).to(torch.bfloat16).float()
    return x, dout, aux


def gelu_grad64(a):
    return 0.5 * (1.0 + torch.erf(a / math.sqrt(2.0))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)


def ref_fwd(x, mask, D):
    """float64: out[b] = sum over real rows / their number; an empty sequence gives zeros.  x [B*S, ld], mask [B, S]."""
    Bn, S = mask.shape
    x = x.double().view(Bn, S, -1)[..., :D]
    out = torch.zeros(Bn, D, dtype=torch.float64)
    for b in range(Bn):
        n = int(mask[b].sum())
        if n:
            out[b] = x[b][mask[b]].sum(0) / n
    return out


def ref_bwd(dout, mask, D, ld, aux=None, aux_mode=0):
    """float64: dx[b, s] = dout[b] / count_b * f(aux[b, s]) at real positions, 0 elsewhere and in the columns D..ld."""
    Bn, S = mask.shape
    dx = torch.zeros(Bn, S, ld, dtype=torch.float64)
    for b in range(Bn):
        n = int(mask[b].sum())
        if n:
            dx[b, mask[b], :D] = dout[b].double() / n
    if aux_mode:
        a = aux.double().view(Bn, S, ld)
        f = a if aux_mode == 1 else gelu_grad64(a)
        dx = torch.where(dx != 0, dx * f, dx)
    return dx.view(Bn * S, ld)
