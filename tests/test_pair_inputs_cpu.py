"""pair_inputs="coords" on the host (no GPU): the pair rule against every golden fixture that carries coordinates, the payload /
collate switches, the global padded length of a coords batch, and the C boundary of the new entry points."""
import ctypes
import glob
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mmdti_hip import _abi, collate
from mmdti_hip.collate import HOST_FIELDS, HostCollate, collate_batch, device_payload, pair_inputs_from_coords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
V, PAD = 31, 0
NEW_SYMBOLS = ("mmdti_pair_records_pack", "mmdti_pair_inputs_from_coords", "mmdti_gbf_bias_fwd_coords", "mmdti_gbf_bias_bwd_full_coords")


def _fixture_samples():
    """(fixture, key prefix) of every stored sample with coordinates: g9_collate, g9_model_tiny_*, g10_trainer_*."""
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "g9_collate.npz")) + glob.glob(os.path.join(GOLDEN, "g9_model_tiny_*.npz")) +
                       glob.glob(os.path.join(GOLDEN, "g10_trainer_*.npz"))):
        g = np.load(path, allow_pickle=True)
        for k in g.files:
            if k.endswith("_src_coord") and not k.startswith("b_"):
                out.append((g, k[:-len("src_coord")], os.path.basename(path)))
    return out


def test_host_rule_reproduces_every_stored_sample_bit_for_bit():
    samples = _fixture_samples()
    assert len(samples) == 87, len(samples)
    for g, pre, name in samples:
        d, e = pair_inputs_from_coords(g[pre + "src_coord"], g[pre + "src_tokens"], V, PAD)
        ref_d, ref_e = torch.from_numpy(g[pre + "src_distance"]), torch.from_numpy(g[pre + "src_edge_type"]).long()
        assert torch.from_numpy(g[pre + "src_coord"]).dtype == torch.float32 and ref_d.dtype == torch.float32
        assert torch.equal(e, ref_e), (name, pre)
        assert d.dtype == torch.float32 and torch.equal(d.view(torch.int32), ref_d.view(torch.int32)), (name, pre)


def test_host_rule_reproduces_the_padded_batch_of_g9_collate():
    g = np.load(os.path.join(GOLDEN, "g9_collate.npz"), allow_pickle=True)
    d, e = pair_inputs_from_coords(g["b_src_coord"], g["b_src_tokens"], V, PAD)
    assert torch.equal(e, torch.from_numpy(g["b_src_edge_type"]).long())
    assert torch.equal(d.view(torch.int32), torch.from_numpy(g["b_src_distance"]).view(torch.int32))
    # the rule in words: either atom pad -> (pad index, 0.0), whatever the pad slot's coordinates hold
    c = torch.from_numpy(g["b_src_coord"]).clone()
    tok = torch.from_numpy(g["b_src_tokens"])
    assert bool(tok.eq(PAD).any())
    c[tok.eq(PAD)] = float("nan")
    d2, e2 = pair_inputs_from_coords(c, tok, V, PAD)
    assert torch.equal(d2.view(torch.int32), d.view(torch.int32)) and torch.equal(e2, e)


def _g9_samples():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import g9util
    g = np.load(os.path.join(GOLDEN, "g9_collate.npz"), allow_pickle=True)
    return g9util.samples_from(g), g9util.tokenizer_from(str(g["tok_json"]), 64)


def test_payload_and_collate_modes():
    samples, tok = _g9_samples()
    full, label = collate_batch(samples, PAD, tok)
    # default mode: as ever -- planes kept (edge types int16), src_coord dropped, host fields attached
    plain = device_payload(full, V * V, PAD)
    assert plain.keys() == device_payload(full, V * V, PAD, pair_inputs="planes").keys()
    assert "src_coord" not in plain and plain["src_edge_type"].dtype == torch.int16 and plain["src_distance"].dtype == torch.float32
    assert torch.equal(plain["src_edge_type"].long(), full["src_edge_type"]) and torch.equal(plain["src_distance"], full["src_distance"])
    assert set(plain) == (set(full) - {"src_coord"}) | set(HOST_FIELDS)
    # coords mode: no plane keys, src_coord kept, every other field (host fields included) identical
    co = device_payload(full, V * V, PAD, pair_inputs="coords")
    assert "src_distance" not in co and "src_edge_type" not in co
    assert torch.equal(co["src_coord"], full["src_coord"]) and co["src_coord"].dtype == torch.float32
    assert set(co) == (set(plain) - {"src_distance", "src_edge_type"}) | {"src_coord"}
    for k in set(co) - {"src_coord"}:
        a, b = co[k], plain[k]
        assert (torch.equal(a, b) and a.dtype == b.dtype) if torch.is_tensor(a) else a == b, k
    # the collate itself never builds the square pads in that mode, and what it builds is what the planes collate builds
    lean, label2 = collate_batch(samples, PAD, tok, pair_inputs="coords")
    assert list(lean) == [k for k in full if k not in ("src_distance", "src_edge_type")] and torch.equal(label, label2)
    assert all(torch.equal(lean[k], full[k]) for k in lean)
    # HostCollate: default = the parent's output; coords = the lean payload (also with narrow=False: the mode implies the payload step)
    a, _ = HostCollate(PAD, tok, V * V)(samples)
    assert a.keys() == plain.keys() and all((torch.equal(a[k], plain[k]) and a[k].dtype == plain[k].dtype) if torch.is_tensor(a[k]) else a[k] == plain[k] for k in a)
    for narrow in (True, False):
        b, _ = HostCollate(PAD, tok, V * V, narrow=narrow, pair_inputs="coords")(samples)
        assert b.keys() == co.keys() and all(torch.equal(b[k], co[k]) if torch.is_tensor(b[k]) else b[k] == co[k] for k in b)
    # the planes the kernels will derive are the ones that were dropped
    d, e = pair_inputs_from_coords(co["src_coord"], co["src_tokens"], V, PAD)
    assert torch.equal(e, full["src_edge_type"]) and torch.equal(d.view(torch.int32), full["src_distance"].view(torch.int32))
    with pytest.raises(ValueError, match="pair_inputs"):
        device_payload(full, V * V, PAD, pair_inputs="coordinates")
    with pytest.raises(KeyError, match="src_coord"):
        device_payload(plain, V * V, PAD, pair_inputs="coords")


def test_synth_batch_returns_the_coordinates_it_draws():
    from mmdti_hip.synth import synth_batch
    plain, _ = synth_batch(4, 12, 10, seed=3, ragged=True)
    full, _ = synth_batch(4, 12, 10, seed=3, ragged=True, with_coord=True)
    assert "src_coord" not in plain and all(torch.equal(plain[k], full[k]) for k in plain)
    assert full["src_coord"].shape == (*full["src_tokens"].shape, 3) and full["src_coord"].dtype == torch.float32
    d, e = pair_inputs_from_coords(full["src_coord"], full["src_tokens"], V, PAD)
    assert torch.equal(e, full["src_edge_type"]) and torch.equal(d.view(torch.int32), full["src_distance"].view(torch.int32))


def _worker_pad_round_trip(rank, world, initfile, out):
    for p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"file://{initfile}")
    from mmdti_hip.parallel import pad_to_global_lengths
    from mmdti_hip.synth import synth_batch
    from mmdti_hip.collate import device_payload, pair_inputs_from_coords
    full, _ = synth_batch(3, 12 + 28 * rank, 9 + 2 * rank, seed=11 + rank, ragged=True, with_coord=True)
    n_loc = full["src_tokens"].shape[1]
    batch = device_payload(full, 31 * 31, 0, pair_inputs="coords")
    glob_b = pad_to_global_lengths(batch)
    lens = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(lens, torch.tensor([n_loc]))
    n_glob = int(max(lens))
    ok = "src_distance" not in glob_b and "src_edge_type" not in glob_b
    ok &= glob_b["src_tokens"].shape == (3, n_glob) and glob_b["src_coord"].shape == (3, n_glob, 3)
    ok &= torch.equal(glob_b["src_tokens"][:, :n_loc], batch["src_tokens"]) and torch.equal(glob_b["src_coord"][:, :n_loc], batch["src_coord"])
    ok &= bool(glob_b["src_tokens"][:, n_loc:].eq(0).all()) and bool(glob_b["src_coord"][:, n_loc:].eq(0).all())
    ok &= all(glob_b[k] is batch[k] for k in ("atom_counts", "token_counts", "token_pad_id", "packable"))
    # the planes of the grown batch = the planes-mode batch grown the same way (0.0 / pad index in the new slots)
    planes = pad_to_global_lengths(device_payload(full, None, 0))
    d, e = pair_inputs_from_coords(glob_b["src_coord"], glob_b["src_tokens"], 31, 0)
    ok &= torch.equal(e, planes["src_edge_type"].long()) and torch.equal(d.view(torch.int32), planes["src_distance"].view(torch.int32))
    oks = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(oks, torch.tensor([int(bool(ok))]))
    if rank == 0:
        torch.save({"ok": all(int(o) for o in oks) and n_glob > int(min(lens))}, out)       # (some rank did grow)
    dist.destroy_process_group()


def test_pad_to_global_lengths_round_trip_of_a_coords_batch():
    with tempfile.TemporaryDirectory() as td:
        initfile, out = os.path.join(td, "init"), os.path.join(td, "out.pt")
        mp.spawn(_worker_pad_round_trip, args=(2, initfile, out), nprocs=2, join=True)
        assert torch.load(out)["ok"]


def test_header_declares_and_library_exports_the_coords_entry_points():
    protos = _abi.parse_header()
    dll = ctypes.CDLL(_abi.LIB_PATH)
    src = open(_abi.HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert hasattr(dll, name), f"{name} not exported"
        decl = src[:src.index(f"int {name}(")]
        comment = decl[decl.rindex("/*"):]            # the comment right above the declaration cites the reference
        assert "data/conformer.py:204-212" in comment and "mm_model.py:553-556" in comment, name
    # purely additive: the version stays, and the existing signatures are the parent's
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2 and dll.mmdti_abi_version() == 2
    assert len(protos["mmdti_gbf_bias_fwd"][1]) == 26 and len(protos["mmdti_gbf_bias_bwd_full"][1]) == 32
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"exporting exactly the {len(protos)} symbols" in doc and all(n in doc for n in NEW_SYMBOLS)


def test_coords_arguments_are_refused_before_any_launch():
    lib = _abi.lib()
    buf = (ctypes.c_char * 256)()
    rec = (ctypes.addressof(buf) + 15) & ~15                     # (host memory: nothing below may reach a launch)
    one = rec                                                     # any non-null pointer serves where only "non-null" is asked
    fwd = lambda records, Vv, pad, N, E: lib.mmdti_gbf_bias_fwd_coords(0, records, Vv, pad, one, one, one, one, one, one, one, one, 1, N, (N + 3) // 4 * 4,
                                                                       128, 128, 64, E, one, 0, 0, 0)
    bwd = lambda records, Vv, pad, N, E: lib.mmdti_gbf_bias_bwd_full_coords(0, one, records, Vv, pad, one, one, one, one, one, one, one, 1, N, (N + 3) // 4 * 4,
                                                                            128, 128, 64, E, 0, one, one, one, one, one, one, one, one, 0, 0, 0, 0)
    mat = lambda records, Vv, pad, N: lib.mmdti_pair_inputs_from_coords(0, records, 1, N, Vv, pad, one, one, 2)
    for call in (fwd, bwd):
        with pytest.raises(_abi.MMDTIError, match="V \\* V must be the edge-table size"):
            call(rec, 30, 0, 8, 961)
        with pytest.raises(_abi.MMDTIError, match="N too large"):
            call(rec, 31, 0, 40000, 961)
        with pytest.raises(_abi.MMDTIError, match="null atom records"):
            call(0, 31, 0, 8, 961)
        with pytest.raises(_abi.MMDTIError, match="16-byte aligned"):
            call(rec + 4, 31, 0, 8, 961)
        with pytest.raises(_abi.MMDTIError, match="pad index"):
            call(rec, 31, 31, 8, 961)
    with pytest.raises(_abi.MMDTIError, match="N too large"):
        mat(rec, 31, 0, 40000)
    with pytest.raises(_abi.MMDTIError, match="null atom records"):
        mat(0, 31, 0, 8)
    with pytest.raises(_abi.MMDTIError, match="V <= 181"):
        mat(rec, 200, 0, 8)
    with pytest.raises(_abi.MMDTIError, match="16-byte aligned"):
        lib.mmdti_pair_records_pack(0, one, one, 8, 1, 8, rec + 8)
    with pytest.raises(_abi.MMDTIError, match="int64 or int32"):
        lib.mmdti_pair_records_pack(0, one, one, 2, 1, 8, rec)


def test_model_without_planes_or_coordinates_is_a_clear_error():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import g9util
    model = g9util.product_model(g9util.tiny_cfg("classification", 40))
    tok = torch.zeros(2, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="src_coord"):
        model(src_tokens=tok, input_ids=tok, attention_mask=tok)
    with pytest.raises(ValueError, match="src_coord"):
        model(tok, torch.zeros(2, 5, 5), None, tok, tok)
