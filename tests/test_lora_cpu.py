"""LoRA on the host, without a GPU: the library's launch plans (mmdti_lora_plan) against the independent statement of
tests/lora_cases.py; apply_lora / merge_lora / the state helpers on a small reference-shaped model; the `adapters` argument of
paths.py; the Trainer's parameter plumbing."""
import ctypes
import os
from types import SimpleNamespace

import pytest
import torch

import lora_cases as L
from mmdti_hip import _abi, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ plans
def test_the_table_holds_the_declared_instances():
    lib = _abi.lib()
    assert lib.const["MMDTI_PLAN_LORA"] == L.LORA_FAMILY
    n = ctypes.c_int(0)
    lib.mmdti_plan_table_size(L.LORA_FAMILY, ctypes.byref(n))
    assert n.value == L.LORA_KERNELS
    lib._dll.mmdti_plan_kernel_name.restype = ctypes.c_char_p
    names = [lib._dll.mmdti_plan_kernel_name(L.LORA_FAMILY, i).decode() for i in range(n.value)]
    want = {}
    for r in L.RANKS:
        for mode in (0, 1, 2):
            want[L.kernel_key("fwd", r, mode)] = L.kernel_name("fwd", r, mode)
        for flag in (False, True):
            want[L.kernel_key("dx", r, flag)] = L.kernel_name("dx", r, flag)
            for det in (False, True):
                want[L.kernel_key("bwd", r, flag, det)] = L.kernel_name("bwd", r, flag, det)
    assert names == [want[i] for i in range(L.LORA_KERNELS)]
    # and the case table reaches every row of the library's table
    assert {L.kernel_key(c["entry"], c["r"], c["flag"], c["det"]) for c in L.CASES} == set(range(n.value))


@pytest.mark.parametrize("c", L.CASES, ids=L.case_id)
def test_plan_of_every_case(c):
    got = ops.lora_plan(c["entry"], c["T"], c["n_in"], c["n_out"], c["r"], c["flag"], c["det"])
    assert got == L.expected_plan(c["entry"], c["T"], c["n_in"], c["n_out"], c["r"], c["flag"], c["det"])


def test_plan_sweep():
    Ts = [1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 4096, 4097, 16384, 16385, 32768, 32769, 65536, 65537, 200000]
    for entry in ("fwd", "bwd", "dx"):
        for T in Ts:
            for r in L.RANKS:
                for n_in, n_out in ((64, 64), (512, 1536), (320, 512), (768, 768)):
                    for flag in ((0, 1, 2) if entry == "fwd" else (False, True)):
                        for det in (False, True):
                            assert ops.lora_plan(entry, T, n_in, n_out, r, flag, det) == L.expected_plan(entry, T, n_in, n_out, r, flag, det), \
                                (entry, T, r, n_in, n_out, flag, det)


def test_the_deterministic_workspace_of_the_bench_shape_fits_the_default():
    """the library's own plan: slabs = workgroups of the slab kernel, each slab_floats floats"""
    for n_in, n_out in ((512, 1536), (512, 512)):
        p = ops.lora_plan("bwd", 65536, n_in, n_out, 32, deterministic=True)
        need = p["launches"][0]["gx"] * p["slab_floats"] * 4
        assert need == L.det_workspace_bytes(65536, n_in, n_out, 32) and need <= ops.DET_DEFAULT_MB << 20


@pytest.mark.parametrize("r, n_in, n_out, words", L.REFUSED)
def test_plan_refuses_what_the_entry_points_refuse(r, n_in, n_out, words):
    for entry in ("fwd", "bwd"):
        with pytest.raises(_abi.MMDTIError, match=words):
            ops.lora_plan(entry, 16, n_in, n_out, r)
    with pytest.raises(_abi.MMDTIError, match="T must be at least 1"):
        ops.lora_plan("fwd", 0, 64, 64, 8)


def test_the_entry_points_are_in_the_header_and_the_documents():
    protos = _abi.parse_header()
    assert {"mmdti_lora_fwd", "mmdti_lora_bwd", "mmdti_lora_dx", "mmdti_lora_plan"} <= set(protos)
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert f"exporting exactly the {len(protos)} symbols" in doc and "mmdti_lora_fwd" in doc


# ------------------------------------------------------------------------------------------------ apply / merge / state helpers
def _cpu_model():
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 2, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1,
                           attn_dropout=0.1)
    torch.manual_seed(0)
    return mm.MM_Model.from_configs(2, "classification", mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16)


def test_config_refuses_what_the_kernels_refuse():
    from mmdti_hip.lora import LoRAConfig
    cfg = LoRAConfig()
    assert (cfg.rank, cfg.alpha, cfg.targets, cfg.towers, cfg.seed, cfg.scale) == (8, 16.0, ("q", "v"), ("bert", "cross", "unimol"), 0, 2.0)
    for kw in (dict(rank=12), dict(rank=0), dict(targets=("o",)), dict(targets=()), dict(towers=("head",)), dict(alpha=0.0), dict(targets=("q", "q"))):
        with pytest.raises(ValueError, match="LoRAConfig"):
            LoRAConfig(**kw)


def test_apply_lora_flags_names_shapes_and_init():
    from mmdti_hip import lora
    model = _cpu_model()
    reference = {n: p.requires_grad for n, p in model.named_parameters()}
    lora.apply_lora(model, lora.LoRAConfig(rank=16, alpha=8.0, targets=("q", "v"), towers=("bert", "unimol"), seed=3))
    named = dict(model.named_parameters())
    frozen = lora.TOWER_PREFIXES["bert"] + lora.TOWER_PREFIXES["unimol"]
    for n, flag in reference.items():                                      # the selected towers freeze, everything else keeps its flag
        assert named[n].requires_grad == (flag and not n.startswith(frozen)), n
    adapters = sorted(n for n in named if n not in reference)
    want = [f"encoder.layers.{i}.self_attn.lora_{m}" for i in range(2) for m in "AB"]
    want += [f"bert.encoder.layer.{i}.attention.self.lora_{m}_{t}" for i in range(2) for m in "AB" for t in "qv"]
    assert adapters == sorted(want)
    assert all(named[n].requires_grad for n in adapters)
    assert not any("cross_modal_module" in n for n in adapters) and any(p.requires_grad for n, p in named.items() if n.startswith("cross_modal_module."))
    assert tuple(named["encoder.layers.0.self_attn.lora_A"].shape) == (16, 64) and tuple(named["encoder.layers.0.self_attn.lora_B"].shape) == (192, 16)
    assert tuple(named["bert.encoder.layer.1.attention.self.lora_A_q"].shape) == (16, 64)
    assert tuple(named["bert.encoder.layer.1.attention.self.lora_B_v"].shape) == (64, 16)
    for n in adapters:
        p = named[n]
        if ".lora_B" in n:
            assert float(p.abs().max()) == 0.0
        else:                                                               # Kaiming-uniform: inside +- 1 / sqrt(fan_in), not degenerate
            assert float(p.abs().max()) <= 64 ** -0.5 and float(p.std()) > 0.5 * 64 ** -0.5 / 3 ** 0.5
    att = model.encoder.layers[0].self_attn
    assert att.lora_scale == 0.5 and att.lora_targets == ("",) and model.bert.encoder.layer[0].attention.self.lora_targets == ("q", "v")
    again = lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=16, alpha=8.0, targets=("q", "v"), towers=("bert", "unimol"), seed=3))
    other = lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=16, alpha=8.0, targets=("q", "v"), towers=("bert", "unimol"), seed=4))
    assert all(torch.equal(named[n], dict(again.named_parameters())[n]) for n in adapters)                 # seeded
    assert not torch.equal(named[adapters[0]], dict(other.named_parameters())[adapters[0]])
    with pytest.raises(ValueError, match="already has adapters"):
        lora.apply_lora(model)


def test_state_helpers_and_merge_are_exact():
    from mmdti_hip import lora
    model = lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=8, targets=("q", "k", "v")))
    reference_keys = set(_cpu_model().state_dict())
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".lora_B" in n:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    sd = lora.lora_state_dict(model)
    assert set(sd) == set(model.state_dict()) - reference_keys and len(sd) == 2 * (2 + 3 * 4)
    twin = lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=8, targets=("q", "k", "v"), seed=9))
    lora.load_lora_state_dict(twin, sd)
    assert all(torch.equal(v, twin.state_dict()[k]) for k, v in sd.items())
    with pytest.raises(KeyError, match="adapter names differ"):
        lora.load_lora_state_dict(lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=8, targets=("q",))), sd)
    with pytest.raises(ValueError, match="the model holds"):
        lora.load_lora_state_dict(lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=16, targets=("q", "k", "v"))), sd)
    # the merge: W + s.B@A in fp32, exactly; no adapter left; the reference's keys
    before = {k: v.clone() for k, v in model.state_dict().items()}
    merged_sd = lora.merged_state_dict(model)
    assert set(model.state_dict()) == set(before)                          # (merged_state_dict leaves the model alone)
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    lora.merge_lora(model)
    after = model.state_dict()
    assert set(after) == reference_keys == set(merged_sd) and not lora.has_lora(model) and not hasattr(model, "lora_config")
    assert all(p.requires_grad == flags[n] for n, p in model.named_parameters())
    changed = 0
    for k, v in after.items():
        pre = k.rsplit(".", 2)[0]
        pair = [(a, b) for a, b, lin in (("lora_A", "lora_B", "in_proj"), ("lora_A_q", "lora_B_q", "query"), ("lora_A_k", "lora_B_k", "key"),
                                          ("lora_A_v", "lora_B_v", "value")) if k == f"{pre}.{lin}.weight" and f"{pre}.{a}" in before]
        want = before[k] if not pair else before[k] + 2.0 * (before[f"{pre}.{pair[0][1]}"] @ before[f"{pre}.{pair[0][0]}"])
        assert torch.equal(v, want) and torch.equal(merged_sd[k], want), k
        changed += bool(pair)
    assert changed == 2 + 3 * 4


# ------------------------------------------------------------------------------------------------ paths
def test_adapters_send_every_layer_to_the_op_by_op_path():
    from mmdti_hip import paths
    sw = paths.Switches(layer_seq=True, stack_seq=True, stack_max_rows=8192, grouped_dw=True, grouped_dw_min_rows=0, fwd_f16=True, timer=False)
    assert paths.unimol_layer_fwd(sw, True, True, 512, 64) == paths.LAYER
    assert paths.unimol_layer_fwd(sw, True, True, 512, 64, adapters=True) == paths.OPS
    assert paths.unimol_tower_fwd(sw, paths.LAYER, True, 15, 4096, False, True) == paths.STACK
    assert paths.unimol_tower_fwd(sw, paths.LAYER, True, 15, 4096, False, True, adapters=True) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, False, True) == paths.LAYER
    assert paths.unimol_layer_bwd(paths.LAYER, True, False, True, adapters=True) == paths.OPS
    assert paths.bert_tower_fwd(sw, True, True, 6, 4096) == paths.STACK
    assert paths.bert_tower_fwd(sw, True, True, 6, 4096, adapters=True) == paths.LAYER
    for self_attn in (True, False):
        assert paths.bert_layer_fwd(sw, self_attn, True, True, 512, 2048, 4096) == paths.LAYER
        assert paths.bert_layer_fwd(sw, self_attn, True, True, 512, 2048, 4096, adapters=True) == paths.OPS


# ------------------------------------------------------------------------------------------------ the Trainer's parameters
def test_trainer_parameters():
    from mmdti_hip.lora import TOWERS
    from mmdti_hip.tasks.trainer import Trainer
    off = Trainer(task="regression", metrics="mse")
    assert off.lora_rank == 0 and off.lora_config is None
    on = Trainer(task="regression", metrics="mse", lora_rank=16, lora_alpha=32.0, lora_targets=("q", "k"), lora_towers=("bert",), seed=7)
    cfg = on.lora_config
    assert (cfg.rank, cfg.alpha, cfg.targets, cfg.towers, cfg.seed) == (16, 32.0, ("q", "k"), ("bert",), 7)
    assert Trainer(task="regression", metrics="mse", lora_rank=8).lora_config.towers == TOWERS
    with pytest.raises(ValueError, match="rank must be one of"):
        Trainer(task="regression", metrics="mse", lora_rank=12)
    with pytest.raises(ValueError, match="targets"):
        Trainer(task="regression", metrics="mse", lora_rank=8, lora_targets=("out",))


def test_trainer_saves_merged_weights_on_a_stub(tmp_path):
    from mmdti_hip import lora
    from mmdti_hip.tasks.trainer import Trainer
    model = lora.apply_lora(_cpu_model(), lora.LoRAConfig(rank=8))
    with torch.no_grad():
        for n, p in model.named_parameters():
            if ".lora_B" in n:
                p.fill_(0.25)
    trainer = Trainer(task="regression", metrics="mse", lora_rank=8)
    trainer._save(model, str(tmp_path), 0)
    sd = torch.load(os.path.join(str(tmp_path), "model_0.pth"), weights_only=True)["model_state_dict"]
    want = lora.merged_state_dict(model)
    assert set(sd) == set(_cpu_model().state_dict()) and all(torch.equal(sd[k], want[k]) for k in sd)
    assert lora.has_lora(model)                                            # (the model trains on: only the file is merged)


def test_resume_settings_carry_the_adapter_settings():
    from mmdti_hip.tasks.trainer import Trainer
    off = Trainer(task="regression", metrics="mse")._train_settings()
    assert "lora" not in off                                               # (files written without adapters compare as ever)
    a = Trainer(task="regression", metrics="mse", lora_rank=8)._train_settings()
    b = Trainer(task="regression", metrics="mse", lora_rank=8, lora_alpha=32.0)._train_settings()
    c = Trainer(task="regression", metrics="mse", lora_rank=8, lora_targets=("q",))._train_settings()
    assert a["lora"] != b["lora"] and a["lora"] != c["lora"] and {k: v for k, v in a.items() if k != "lora"} == off
