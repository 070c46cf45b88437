"""InfoNCE pooling over the real tokens (InfoNCE(pool="real"), MM_Model(infonce_pool=...), MMDTI_INFONCE_POOL), checked without a
GPU: the pad-free packed layout's index arithmetic, the two new C ABI symbols, the switch's validation, the float64 restatement the
GPU tests compare against (tests/infonce_pool_ref.py) -- and the quirk of the reference the feature removes, pinned on the oracle --
and the self-consistency of the kernel case table (tests/seq_mean_real_cases.py)."""
import ctypes

import pytest
import torch

from oracle import mmdti_oracle as O
from mmdti_hip import _abi
from mmdti_hip.packing import PackedRows

import infonce_pool_ref as R
import seq_mean_real_cases as C


# ------------------------------------------------------------------------------------------------ packing
def test_pad_free_packed_rows_index_arithmetic():
    pk = PackedRows(torch.tensor([5, 9, 1, 9]), 9, pad_row=False)
    assert pk.pad_row is False and PackedRows(torch.tensor([5, 9]), 9).pad_row is True
    assert (pk.B, pk.S, pk.M, pk.max_rows, pk.n_pad_rows) == (4, 9, 24, 9, 0)
    assert pk.off_host.tolist() == [0, 5, 14, 15, 24] and pk.rows_host.tolist() == [5, 9, 1, 9]
    assert pk.gather_host.tolist() == [0, 1, 2, 3, 4] + list(range(9, 18)) + [18] + list(range(27, 36))
    assert pk.seq_host.tolist() == [0] * 5 + [1] * 9 + [2] + [3] * 9
    assert pk.pad_weights().tolist() == [1.0] * 24
    x = torch.arange(1, 37).view(4, 9)
    pk.gather = pk.gather_host
    back = pk.unpack(pk.pack(x))
    real = torch.arange(9).view(1, -1) < pk.counts_host.view(-1, 1)
    assert torch.equal(back[real], x[real])                                       # round trip on the real positions
    assert back[0].tolist() == [1, 2, 3, 4, 5, 0, 0, 0, 0] and back[2].tolist() == [19] + [0] * 8      # zeros, not the next sequence's row
    wide = pk.unpack(torch.ones(24, 3))
    assert wide.shape == (4, 9, 3) and float(wide.sum()) == 24 * 3
    with pytest.raises(ValueError):
        PackedRows(torch.tensor([0, 3]), 5, pad_row=False)


# ------------------------------------------------------------------------------------------------ C ABI
def test_header_and_library_export_both_entry_points_and_the_abi_constant_stays():
    protos = _abi.parse_header()
    dll = ctypes.CDLL(_abi.LIB_PATH)
    assert protos["mmdti_seq_mean_real_fwd"][2] == ["stream", "x_bf16", "B", "S", "D", "ld", "mask", "row_off", "out"]
    assert protos["mmdti_seq_mean_real_bwd"][2] == ["stream", "dout", "rows", "B", "S", "D", "ld", "mask", "row_off", "row_seq", "dx_bf16",
                                                    "aux_bf16", "ld_aux", "aux_mode"]
    for name in ("mmdti_seq_mean_real_fwd", "mmdti_seq_mean_real_bwd"):
        assert hasattr(dll, name), f"{name} not exported"
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2 and dll.mmdti_abi_version() == 2
    src = open(_abi.HEADER).read()
    doc = src[src.index("The mean over the REAL positions"):src.index("int mmdti_seq_mean_real_bwd(")]
    assert doc.count("infonce.py:32-33") >= 2 and "Purely additive: MMDTI_ABI_VERSION does not move" in doc


def test_the_library_refuses_both_or_neither_layout_without_a_gpu():
    """MMDTI_ERR_INVALID before any launch: the argument check needs no device."""
    lib = _abi.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    for mask, off in ((0, 0), (p, p)):
        with pytest.raises(_abi.MMDTIError, match="exactly one of mask"):
            lib.mmdti_seq_mean_real_fwd(0, p, 1, 1, 8, 8, mask, off, p)
        with pytest.raises(_abi.MMDTIError, match="exactly one of mask"):
            lib.mmdti_seq_mean_real_bwd(0, p, 1, 1, 1, 8, 8, mask, off, p, p, 0, 0, 0)
    with pytest.raises(_abi.MMDTIError, match="8-column aligned"):
        lib.mmdti_seq_mean_real_bwd(0, p, 1, 1, 1, 50, 50, p, 0, 0, p, p, 50, 1)


# ------------------------------------------------------------------------------------------------ the switch
def test_constructor_and_environment_reject_unknown_values(monkeypatch):
    from mmdti_hip.models.infonce import InfoNCE, pool_from_env
    assert InfoNCE(64, 64).pool == "all" and InfoNCE(64, 64, pool="real").pool == "real"
    with pytest.raises(ValueError):
        InfoNCE(64, 64, pool="mean")
    monkeypatch.delenv("MMDTI_INFONCE_POOL", raising=False)
    assert pool_from_env() == "all"
    monkeypatch.setenv("MMDTI_INFONCE_POOL", "real")
    assert pool_from_env() == "real" and pool_from_env("all") == "all"
    monkeypatch.setenv("MMDTI_INFONCE_POOL", "tokens")
    with pytest.raises(ValueError):
        pool_from_env()
    with pytest.raises(ValueError):
        pool_from_env("1")


def _tiny_model(**params):
    from types import SimpleNamespace
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 1, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=1, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12,
                           hidden_dropout=0.1, attn_dropout=0.1)
    return mm.MM_Model.from_configs(2, "classification", mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16, **params)


def test_model_follows_the_argument_then_the_environment_and_adds_no_state(monkeypatch):
    monkeypatch.delenv("MMDTI_INFONCE_POOL", raising=False)
    base = _tiny_model()
    assert base.infonce_pool == "all" and base.infonce.pool == "all" and base.train().pad_row_dropout_live()
    real = _tiny_model(infonce_pool="real")
    assert real.infonce_pool == "real" and real.infonce.pool == "real"
    assert not real.train().pad_row_dropout_live()                                # nothing reads a padded row
    assert list(real.state_dict()) == list(base.state_dict())                     # no parameter, no buffer
    monkeypatch.setenv("MMDTI_INFONCE_POOL", "real")
    assert _tiny_model().infonce_pool == "real" and _tiny_model(infonce_pool="all").infonce_pool == "all"
    monkeypatch.setenv("MMDTI_INFONCE_POOL", "REAL")
    with pytest.raises(ValueError):
        _tiny_model()
    with pytest.raises(ValueError):
        _tiny_model(infonce_pool="none")


def test_module_argument_rules_hold_before_any_launch():
    from mmdti_hip.models.infonce import InfoNCE
    x = torch.zeros(2, 5, 64)
    m = torch.ones(2, 5, dtype=torch.bool)
    real, every = InfoNCE(64, 64, pool="real"), InfoNCE(64, 64)
    with pytest.raises(ValueError, match="query_mask and key_mask"):
        real(x, x)
    with pytest.raises(ValueError, match="query_mask and key_mask"):
        real(x, x, query_mask=m)
    with pytest.raises(ValueError, match="bool / uint8"):
        real(x, x, query_mask=m.float(), key_mask=m)
    with pytest.raises(ValueError, match="bool / uint8"):
        real(x, x, query_mask=m[:, :4], key_mask=m)
    with_pad, pad_free = PackedRows(torch.tensor([3, 5]), 5), PackedRows(torch.tensor([3, 5]), 5, pad_row=False)
    with pytest.raises(ValueError, match="pad-free"):
        real(torch.zeros(with_pad.M, 64), torch.zeros(with_pad.M, 64), packs=(with_pad, with_pad))
    with pytest.raises(ValueError, match="no pad row"):
        every(torch.zeros(pad_free.M, 64), torch.zeros(pad_free.M, 64), packs=(pad_free, pad_free))


# ------------------------------------------------------------------------------------------------ the reference helper
def _head(seed, B=5, Sq=7, Sk=9, D=64):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name in ("info_proj_query", "info_proj_positive"):
        P[f"infonce.{name}.0.weight"] = torch.randn(D, D, generator=g, dtype=torch.float64) * 0.2
        P[f"infonce.{name}.0.bias"] = torch.randn(D, generator=g, dtype=torch.float64) * 0.1
        P[f"infonce.{name}.2.weight"] = torch.randn(50, D, generator=g, dtype=torch.float64) * 0.2
        P[f"infonce.{name}.2.bias"] = torch.randn(50, generator=g, dtype=torch.float64) * 0.1
    xq = torch.randn(B, Sq, D, generator=g, dtype=torch.float64)
    xk = torch.randn(B, Sk, D, generator=g, dtype=torch.float64)
    return P, xq, xk, g


def test_restatement_is_the_oracle_when_nothing_is_padded():
    P, xq, xk, _ = _head(1)
    mq, mk = torch.ones(xq.shape[:2], dtype=torch.bool), torch.ones(xk.shape[:2], dtype=torch.bool)
    a = R.infonce_forward_real(xq, xk, mq, mk, P)
    b = O.infonce_forward(xq, xk, P, p=0.0)
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))


def test_restatement_ignores_the_padded_length_and_the_oracle_does_not():
    """The same sequences padded 16 positions further (whatever the padded rows hold): the mean over real tokens does not move, the
    reference's mean over all positions does -- the quirk of infonce.py:32-33 that pool="real" removes."""
    P, xq, xk, g = _head(2)
    B = xq.shape[0]
    lq, lk = torch.tensor([7, 3, 5, 1, 6]), torch.tensor([4, 9, 2, 8, 5])
    mq = torch.arange(xq.shape[1]).view(1, -1) < lq.view(-1, 1)
    mk = torch.arange(xk.shape[1]).view(1, -1) < lk.view(-1, 1)

    def further(x, m):
        pad = torch.randn(B, 16, x.shape[2], generator=g, dtype=torch.float64)
        return torch.cat((x, pad), 1), torch.cat((m, torch.zeros(B, 16, dtype=torch.bool)), 1)

    xq2, mq2 = further(xq, mq)
    xk2, mk2 = further(xk, mk)
    a, a2 = R.infonce_forward_real(xq, xk, mq, mk, P), R.infonce_forward_real(xq2, xk2, mq2, mk2, P)
    assert abs(float(a) - float(a2)) <= 1e-12 * abs(float(a))
    ea, ea2 = R.infonce_embed_real(xq, xk, mq, mk, P), R.infonce_embed_real(xq2, xk2, mq2, mk2, P)
    assert all(torch.allclose(u, v, rtol=1e-12, atol=1e-14) for u, v in zip(ea, ea2))
    b, b2 = O.infonce_forward(xq, xk, P, p=0.0), O.infonce_forward(xq2, xk2, P, p=0.0)
    assert abs(float(b) - float(b2)) > 1e-3 * abs(float(b))
    # NaN in a masked row is skipped, an empty sequence pools to zeros
    xq3 = xq.clone()
    xq3[~mq] = float("nan")
    assert torch.equal(R.infonce_embed_real(xq3, xk, mq, mk, P)[0], ea[0])
    assert float(R.masked_mean(xq, torch.zeros_like(mq)).abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_is_self_consistent():
    cs = C.cases()
    assert len(cs) == len(set(cs)) == len(C.SEQ_LENS) * len(C.WIDTHS) * len(C.MASK_KINDS)
    assert {S % 32 for S in C.SEQ_LENS} >= {0, 1, 31} and max(C.SEQ_LENS) > 64 and min(C.SEQ_LENS) == 1       # the phase wrap at 32
    assert {D for D, ld in C.WIDTHS if C.wide_fwd(D, ld)} == {8, 64, 72, 512}
    assert (50, 56) in C.WIDTHS and not C.wide_fwd(50, 56) and C.wide_bwd(50, 56) and not C.wide_bwd(50, 50)
    assert all(ld >= D for D, ld in C.WIDTHS) and C.AUX_MODES == (0, 1, 2)
    for S in C.SEQ_LENS:
        pre, hole = C.mask_plane("prefix", S), C.mask_plane("hole", S)
        assert pre.sum(1).tolist() == [1, S - 1, S]
        assert hole.sum(1).tolist() == [S - 1, 0, S] and (S < 3 or (bool(hole[0, 0]) and bool(hole[0, -1]) and not bool(hole[0, S // 2])))
    assert len(C.PACKED_LENS) == C.B and max(C.PACKED_LENS) == C.PACKED_S and min(C.PACKED_LENS) == 1 and C.PACKED_S % 32 == 1
    # the references agree with autograd: ref_bwd is the adjoint of ref_fwd, times the aux factor
    S, D, ld = 33, 8, 8
    x, dout, aux = C.inputs(S, D, ld, seed=3)
    for kind in C.MASK_KINDS:
        mask = C.mask_plane(kind, S)
        xd = x.double().requires_grad_()
        (C.ref_fwd(xd, mask, D) * dout.double()).sum().backward()
        assert torch.allclose(C.ref_bwd(dout, mask, D, ld), xd.grad, rtol=1e-12, atol=0)
        a = aux.double().requires_grad_()
        torch.nn.functional.gelu(a).sum().backward()
        assert torch.allclose(C.gelu_grad64(aux.double()), a.grad, rtol=1e-10, atol=1e-12)
        assert torch.allclose(C.ref_bwd(dout, mask, D, ld, aux, 1), xd.grad * aux.double(), rtol=1e-12, atol=0)
        assert torch.allclose(C.ref_bwd(dout, mask, D, ld, aux, 2), xd.grad * C.gelu_grad64(aux.double()), rtol=1e-12, atol=0)
