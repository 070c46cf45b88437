"""mmdti_seq_mean_real_fwd / _bwd -- the mean over the REAL positions of every sequence (InfoNCE(pool="real")) -- against float64 on
the bf16-rounded inputs, over the table of seq_mean_real_cases.py: both layouts (mask plane over padded rows, pad-free packed rows),
both code shapes (16-byte and scalar), the three aux modes, masked rows holding NaN (they must be skipped, not multiplied by 0)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import seq_mean_real_cases as C
from test_kernels_gpu import ops, dev, bf, close          # noqa: F401  (fixture + helpers)


def _poisoned(x, mask, ld):
    """x with NaN in every masked row: the kernels must not read them into a sum"""
    x = x.clone().view(mask.shape[0], mask.shape[1], ld)
    x[~mask] = float("nan")
    return x.view(-1, ld)


@pytest.mark.parametrize("S,D,ld,kind", C.cases())
def test_padded_form_against_float64(ops, S, D, ld, kind):
    mask = C.mask_plane(kind, S)
    x, dout, aux = C.inputs(S, D, ld, seed=1000 * S + D + ld)
    got = ops.seq_mean_real_fwd(dev(bf(_poisoned(x, mask, ld))), C.B, S, D, ld, mask=dev(mask))
    want = C.ref_fwd(x, mask, D)
    print("fwd", S, D, ld, kind, float((got.double().cpu() - want).abs().max()))
    close(got, want, *C.FWD_BAND)
    empty = mask.sum(1) == 0
    assert bool(empty.any()) == (kind == "hole" or S == 1)
    assert float(got[dev(empty)].abs().max() if bool(empty.any()) else 0.0) == 0.0          # an empty sequence: zeros, not NaN
    rows = mask.view(-1)
    for mode in C.AUX_MODES:
        if mode and not C.wide_bwd(D, ld):
            with pytest.raises(ops.MMDTIError):                                               # the aux factor needs 8-column aligned rows
                ops.seq_mean_real_bwd(dev(dout), C.B, S, D, ld, mask=dev(mask), aux=dev(bf(aux)), aux_mode=mode)
            continue
        a = dev(bf(_poisoned(aux, mask, ld))) if mode else None
        dx = ops.seq_mean_real_bwd(dev(dout), C.B, S, D, ld, mask=dev(mask), aux=a, aux_mode=mode).float().cpu()
        want = C.ref_bwd(dout, mask, D, ld, aux, mode)
        print("bwd", S, D, ld, kind, mode, float((dx.double() - want).abs().max()))
        close(dx, want, *C.BWD_BAND[mode])
        assert float(dx[~rows].abs().max() if bool((~rows).any()) else 0.0) == 0.0           # exact zeros in masked rows
        assert ld == D or float(dx[:, D:].abs().max()) == 0.0                                # ... and in the pad columns


@pytest.mark.parametrize("D,ld", C.WIDTHS)
def test_packed_form_against_float64_and_bit_identical_to_the_padded_form(ops, D, ld):
    from mmdti_hip.packing import PackedRows
    S, lens = C.PACKED_S, C.PACKED_LENS
    pk = PackedRows(torch.tensor(lens), S, device="cuda", pad_row=False)
    assert pk.M == sum(lens)
    mask = torch.arange(S).view(1, -1) < torch.tensor(lens).view(-1, 1)
    x, dout, aux = C.inputs(S, D, ld, seed=77 + D + ld)
    real = mask.view(-1)
    xp = dev(bf(x[real]))
    got = ops.seq_mean_real_fwd(xp, C.B, S, D, ld, pack=pk)
    close(got, C.ref_fwd(x, mask, D), *C.FWD_BAND)
    padded = ops.seq_mean_real_fwd(dev(bf(_poisoned(x, mask, ld))), C.B, S, D, ld, mask=dev(mask))
    assert torch.equal(got, padded)                                                          # same phase order, masked rows skipped
    for mode in C.AUX_MODES:
        if mode and not C.wide_bwd(D, ld):
            with pytest.raises(ops.MMDTIError):
                ops.seq_mean_real_bwd(dev(dout), C.B, S, D, ld, pack=pk, aux=dev(bf(aux[real])), aux_mode=mode)
            continue
        a = dev(bf(aux[real])) if mode else None
        dx = ops.seq_mean_real_bwd(dev(dout), C.B, S, D, ld, pack=pk, aux=a, aux_mode=mode).float().cpu()
        assert dx.shape == (pk.M, ld)
        close(dx, C.ref_bwd(dout, mask, D, ld, aux, mode)[real], *C.BWD_BAND[mode])
        assert ld == D or float(dx[:, D:].abs().max()) == 0.0


def test_bad_arguments_are_refused_before_a_launch(ops):
    from mmdti_hip.packing import PackedRows
    from mmdti_hip import _abi
    S, D = 9, 64
    pk = PackedRows(torch.tensor([5, 9, 1]), S, device="cuda", pad_row=False)
    with_pad = PackedRows(torch.tensor([5, 9, 1]), S, device="cuda")
    x = torch.zeros(C.B * S, D, device="cuda", dtype=torch.bfloat16)
    mask = torch.ones(C.B, S, device="cuda", dtype=torch.bool)
    d = torch.zeros(C.B, D, device="cuda")
    with pytest.raises(ops.MMDTIError):
        ops.seq_mean_real_fwd(x, C.B, S, D, D)                                               # neither layout
    with pytest.raises(ops.MMDTIError):
        ops.seq_mean_real_fwd(x[:pk.M], C.B, S, D, D, mask=mask, pack=pk)                    # both
    with pytest.raises(ops.MMDTIError):
        ops.seq_mean_real_fwd(x[:with_pad.M], C.B, S, D, D, pack=with_pad)                   # a pack that carries pad rows
    with pytest.raises(ops.MMDTIError):
        ops.seq_mean_packed_fwd(x[:pk.M], pk, D, D)                                          # the unmasked mean needs the pad row
    with pytest.raises(ops.MMDTIError):
        ops.seq_mean_packed_bwd(d, pk, D, D)
    # the library itself: MMDTI_ERR_INVALID, no launch
    lib, st = _abi.lib(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, dx = torch.zeros(C.B, D, device="cuda"), torch.zeros(C.B * S, D, device="cuda", dtype=torch.bfloat16)
    m8 = mask.view(torch.uint8)
    for m, off in ((0, 0), (m8.data_ptr(), pk.off.data_ptr())):
        with pytest.raises(ops.MMDTIError):
            lib.mmdti_seq_mean_real_fwd(st, x.data_ptr(), C.B, S, D, D, m, off, out.data_ptr())
        with pytest.raises(ops.MMDTIError):
            lib.mmdti_seq_mean_real_bwd(st, d.data_ptr(), C.B * S, C.B, S, D, D, m, off, pk.row_seq.data_ptr(), dx.data_ptr(), 0, 0, 0)
    with pytest.raises(ops.MMDTIError):                                                      # packed rows without row_seq
        lib.mmdti_seq_mean_real_bwd(st, d.data_ptr(), pk.M, C.B, S, D, D, 0, pk.off.data_ptr(), 0, dx.data_ptr(), 0, 0, 0)
    with pytest.raises(ops.MMDTIError):                                                      # rows that are not B * S under a mask
        lib.mmdti_seq_mean_real_bwd(st, d.data_ptr(), C.B * S - 1, C.B, S, D, D, m8.data_ptr(), 0, 0, dx.data_ptr(), 0, 0, 0)
    with pytest.raises(ops.MMDTIError):                                                      # an aux factor on rows of 50 columns
        lib.mmdti_seq_mean_real_bwd(st, d.data_ptr(), C.B * S, C.B, S, 50, 50, m8.data_ptr(), 0, 0, dx.data_ptr(), x.data_ptr(), 50, 1)
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(dx.float().abs().max()) == 0.0            # nothing was written
