"""InfoNCE memory bank, host side (no GPU): the three symbols, the launch plan held to an independent statement over a sweep, the ring
model against the float64 reference at wrap-around, the empty bank against the oracle's info_nce, and the ValueErrors that need no
device."""
import ctypes

import pytest
import torch

from infonce_bank_ref import RingModel, bank_dir_ref, symmetric_ref
from mmdti_hip import _abi
from oracle import mmdti_oracle as O

SYMBOLS = ("mmdti_infonce_bank_dir", "mmdti_infonce_bank_plan", "mmdti_infonce_bank_push")
G = lambda s: torch.Generator().manual_seed(s)
unit = lambda n, D, seed: torch.nn.functional.normalize(torch.randn(n, D, generator=G(seed)), dim=-1)


def test_symbols_in_header_and_library():
    protos = _abi.parse_header()
    dll = ctypes.CDLL(_abi.LIB_PATH)
    for name in SYMBOLS:
        assert name in protos and hasattr(dll, name), name
    assert protos["mmdti_infonce_bank_dir"][2] == ["stream", "qh_all", "kh_all", "Bg", "D", "row0", "Bl", "bank", "bank_valid", "bank_ids",
                                                  "ids_all", "cap", "temperature", "loss_sum", "dq_all", "dk_all", "scratch"]
    assert protos["mmdti_infonce_bank_push"][2] == ["stream", "bank", "bank_valid", "bank_ids", "head", "rows", "ids", "n", "D", "cap"]
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2          # (purely additive)


WAVE_SLOTS = 256 * 4          # CUs x SIMDs of an MI355X: a workgroup of the rows pass is one wave


def expected_scratch(Bl, Bg, splits):
    """what the kernels index: gl [Bl, Bg] | Bl loss terms | (max, sum) per (split, anchor of a 16-block) | a 64-float dQ row per the same"""
    rows = 16 * ((Bl + 15) // 16)
    terms = Bl * Bg
    stats = terms + Bl
    slabs = stats + 2 * splits * rows
    return terms, stats, slabs, slabs + 64 * splits * rows


def test_plan_against_independent_statement():
    from mmdti_hip import ops
    for cap in (16, 100, 4096, 65536):
        bank_tiles = (cap + 15) // 16
        for Bl in range(1, 301):
            for Bg in (Bl, 8 * Bl):
                p = ops.infonce_bank_plan(Bg, Bl, cap)
                ab, live = (Bl + 15) // 16, (Bg + 15) // 16
                s = p["splits"]
                assert (p["anchor_blocks"], p["live_tiles"], p["tiles"], p["block"]) == (ab, live, live + bank_tiles, 64)
                assert p["grid"] == ab * s and p["cols_grid"] == live and p["fold_grid"] * 256 >= 16 * ab * 64 > (p["fold_grid"] - 1) * 256
                # a split never holds fewer than two bank tiles' worth of keys, and never no tile at all
                assert 1 <= s <= max(1, bank_tiles // 2) and s <= p["tiles"]
                # as many splits as fill the chip's wave slots and no more -- or as many as the bank allows
                assert (s - 1) * ab < WAVE_SLOTS
                assert p["grid"] >= WAVE_SLOTS or s == max(1, bank_tiles // 2)
                assert (p["off_terms"], p["off_stats"], p["off_slabs"], p["scratch_floats"]) == expected_scratch(Bl, Bg, s)
                assert p == ops.infonce_bank_plan(Bg, Bl, cap, D=64) == ops.infonce_bank_plan(Bg, Bl, cap, D=7)      # (Bl, Bg, cap only)
    # the shape the feature is for: at least one workgroup per CU
    assert ops.infonce_bank_plan(32, 32, 4096)["grid"] >= 256
    # one split where the anchor blocks alone fill the chip, and where the bank is a tile or two
    assert ops.infonce_bank_plan(16 * WAVE_SLOTS, 16 * WAVE_SLOTS, 65536)["splits"] == 1
    assert ops.infonce_bank_plan(300, 300, 16)["splits"] == 1
    assert ops.infonce_bank_plan(2048, 256, 16384)["splits"] == 64


def test_plan_and_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _abi.lib()
    words = (ctypes.c_longlong * 12)()
    with pytest.raises(_abi.MMDTIError, match="feature width"):
        lib.mmdti_infonce_bank_plan(32, 32, 64, 65, ctypes.addressof(words))
    with pytest.raises(_abi.MMDTIError, match="bad sizes"):
        lib.mmdti_infonce_bank_plan(32, 33, 64, 50, ctypes.addressof(words))
    with pytest.raises(_abi.MMDTIError, match="capacity"):
        lib.mmdti_infonce_bank_plan(32, 32, 0, 50, ctypes.addressof(words))
    with pytest.raises(_abi.MMDTIError, match="feature width"):
        lib.mmdti_infonce_bank_dir(0, 16, 16, 4, 96, 0, 4, 16, 16, 0, 0, 8, 0.1, 16, 16, 16, 16)
    with pytest.raises(_abi.MMDTIError, match="temperature"):
        lib.mmdti_infonce_bank_dir(0, 16, 16, 4, 50, 0, 4, 16, 16, 0, 0, 8, 0.0, 16, 16, 16, 16)
    with pytest.raises(_abi.MMDTIError, match="at most cap"):
        lib.mmdti_infonce_bank_push(0, 16, 16, 16, 16, 16, 0, 9, 50, 8)


def test_ring_model_wraps_and_feeds_the_reference():
    D, cap = 6, 5
    ring = RingModel(cap, D)
    a, b = unit(3, D, 1), unit(4, D, 2)
    ring.push(a, torch.tensor([10, 11, 12]))
    assert ring.head == 3 and ring.valid.tolist() == [1, 1, 1, 0, 0] and ring.ids.tolist() == [10, 11, 12, -1, -1]
    b[1, 2] = float("inf")
    ring.push(b, torch.tensor([20, 21, 22, 23]))            # slots 3, 4, 0, 1
    assert ring.head == 2 and ring.valid.tolist() == [1, 1, 1, 1, 0] and ring.ids.tolist() == [22, 23, 12, 20, 21]
    assert torch.equal(ring.rows[0], b[2]) and torch.equal(ring.rows[2], a[2]) and float(ring.rows[4].abs().max()) == 0.0
    # the reference over this ring = the reference over the four valid rows laid out densely
    q, k = unit(3, D, 3), unit(3, D, 4)
    dense = torch.stack([ring.rows[s] for s in (0, 1, 2, 3)])
    got = bank_dir_ref(q, k, 0, 3, ring.rows, ring.valid)
    want = bank_dir_ref(q, k, 0, 3, dense, torch.ones(4, dtype=torch.uint8))
    for g, w in zip(got, want):
        torch.testing.assert_close(g, w, rtol=1e-14, atol=1e-14)
    # ids: the anchor whose id sits in a slot loses exactly that key -- the others keep it
    ids = torch.tensor([12, 77, 78])
    with_ids = bank_dir_ref(q, k, 0, 3, ring.rows, ring.valid, ring.ids, ids)
    lg0 = torch.cat((k, dense[[0, 1, 3]])).double() @ q[0].double() / 0.1          # (id 12 sits in slot 2)
    term0 = torch.logsumexp(lg0, 0) - lg0[0]
    rest = bank_dir_ref(q, k, 1, 2, dense, torch.ones(4, dtype=torch.uint8))[0]
    torch.testing.assert_close(with_ids[0], term0 + rest, rtol=1e-13, atol=1e-13)


def test_empty_bank_is_the_oracles_info_nce():
    B, D = 16, 50
    q, k = unit(B, D, 5), unit(B, D, 6)
    empty = RingModel(8, D)
    got = symmetric_ref(q, k, empty, empty)
    torch.testing.assert_close(got.float(), O.info_nce(q, k).reshape(()), rtol=1e-6, atol=1e-7)


def test_value_errors_without_a_device():
    from mmdti_hip.models.infonce import InfoNCE, check_memory_bank
    from mmdti_hip.tasks.trainer import Trainer
    for bad in (-1, 1.5, "8", True, (1 << 24) + 1):
        with pytest.raises(ValueError, match="memory_bank"):
            InfoNCE(64, 64, memory_bank=bad)
    assert check_memory_bank(0) == 0 and check_memory_bank(4096) == 4096
    head = InfoNCE(64, 64)
    assert head.memory_bank == 0 and head.bank_q is None and head.memory_bank_state() == []
    keys = set(head.state_dict())
    head.set_memory_bank(8)
    assert set(head.state_dict()) == keys                    # (checkpoints keep the reference's keys)
    assert [n for n, _ in head.memory_bank_state()] == ["q.rows", "q.valid", "q.ids", "q.head", "k.rows", "k.valid", "k.ids", "k.head"]
    assert head.bank_q.rows.shape == (8, 50) and int(head.bank_k.valid.sum()) == 0
    head.bank_q.valid.fill_(1); head.bank_q.head.fill_(3)
    head.reset_memory_bank()
    assert int(head.bank_q.valid.sum()) == 0 and int(head.bank_q.head) == 0
    head.set_memory_bank(0)
    assert head.bank_q is None and head.bank_k is None
    with pytest.raises(ValueError, match="memory_bank"):
        Trainer(task="regression", metrics="mse", memory_bank=-4)
    with pytest.raises(ValueError, match="union"):
        Trainer(task="regression", metrics="mse", memory_bank=64, accum_steps=2, accum_negatives="union")
    assert Trainer(task="regression", metrics="mse", memory_bank=64, accum_steps=2, accum_negatives="micro").memory_bank == 64
    assert Trainer(task="regression", metrics="mse").memory_bank == 0


def test_indexed_dataset_leaves_the_collate_alone():
    from mmdti_hip.collate import IndexedCollate, IndexedDataset
    data = [dict(x=float(i)) for i in range(7)]

    def collate(samples):
        return {"x": torch.tensor([s["x"] for s in samples])}, torch.tensor([s["x"] * 2 for s in samples])

    ds = IndexedDataset(data)
    assert len(ds) == 7 and ds[3] == (data[3], 3)
    order = [5, 0, 3]
    plain_in, plain_t = collate([data[i] for i in order])
    got_in, got_t = IndexedCollate(collate)([ds[i] for i in order])
    assert torch.equal(got_in["x"], plain_in["x"]) and torch.equal(got_t, plain_t)
    assert got_in["sample_ids"].tolist() == order and got_in["sample_ids"].dtype == torch.int64
    assert set(got_in) == set(plain_in) | {"sample_ids"}
