"""Parameter groups on the host (mmdti_hip/param_groups.py, freeze.arena_group_ids): resolve's rules -- first match wins, unmatched
parameters fall into the default group 0, every error --, the three helpers on a model built with MM_Model.from_configs on the CPU (with
the `layers.1` / `layers.10` case), the ids of padding slots and of the last ragged block, and the additive entry point in the header
and the documents."""
import os
from types import SimpleNamespace

import pytest
import torch

from mmdti_hip import _abi
from mmdti_hip import param_groups as PG
from mmdti_hip.freeze import arena_group_ids
from mmdti_hip.param_groups import ParamGroup, by_prefix, layerwise_decay, no_decay, resolve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def model():
    """both towers at the width of the trainer tests, the pair tower 12 layers deep (so that layers 1, 10 and 11 exist)"""
    from mmdti_hip.models import mm_model as mm
    mol = mm.molecule_architecture()
    mol.encoder_layers, mol.encoder_embed_dim, mol.encoder_ffn_embed_dim, mol.encoder_attention_heads = 12, 64, 128, 8
    cross = mm.crossmodal_config()
    cross.hidden_size, cross.num_attention_heads, cross.intermediate_size = 64, 4, 128
    rcfg = SimpleNamespace(layers=2, dim=64, heads=4, ffn=128, vocab=40, max_pos=40, type_vocab=1, pad_idx=1, ln_eps=1e-12, hidden_dropout=0.1, attn_dropout=0.1)
    torch.manual_seed(0)
    return mm.MM_Model.from_configs(2, "classification", mol_args=mol, roberta_cfg=rcfg, cross_cfg=cross, gbf_K=16)


def _by_name(model, groups, wd=0.0):
    index, table = resolve(model, groups, wd)
    names = [n for n, _ in model.named_parameters()]
    assert len(index) == len(names)
    return dict(zip(names, index)), table


def test_first_match_wins_and_the_rest_falls_into_the_default_group(model):
    groups = [ParamGroup("encoder.layers.1.", lr_scale=0.5, weight_decay=0.1, name="one"),
              ParamGroup("encoder, bert", lr_scale=0.25, name="towers"),
              ParamGroup(lambda n, p: n.endswith(".bias"), lr_scale=2.0, weight_decay=0.0, name="biases"),
              ParamGroup([model.classification_head.out_proj.weight], lr_scale=3.0)]
    of, table = _by_name(model, groups, 0.01)
    assert table[0] == [1.0, 0.01] and table[1] == [0.5, 0.1] and table[2] == [0.25, 0.01] and table[3] == [2.0, 0.0] and table[4] == [3.0, 0.01]
    assert of["encoder.layers.1.fc1.weight"] == 1 and of["encoder.layers.1.fc1.bias"] == 1          # the first match, not `biases`
    assert of["encoder.layers.10.fc1.weight"] == 2 and of["encoder.layers.0.fc1.bias"] == 2 and of["bert.pooler.dense.bias"] == 2
    assert of["classification_head.dense.bias"] == 3 and of["classification_head.out_proj.weight"] == 4
    assert of["classification_head.dense.weight"] == 0 and of["embed_tokens.weight"] == 0 and of["gbf.mul.weight"] == 0
    assert PG.group_names(groups) == ["default", "one", "towers", "biases", "group4"]
    of, table = _by_name(model, [], 0.02)
    assert set(of.values()) == {0} and table == [[1.0, 0.02]]
    # the prefix rule is freeze_layers': without the trailing dot layer 1 captures layers 10 and 11
    of, _ = _by_name(model, [ParamGroup("encoder.layers.1", lr_scale=0.5)])
    assert {n.split(".")[2] for n, g in of.items() if g == 1} == {"1", "10", "11"}
    # a generator of Parameters is read once and kept
    g = ParamGroup(p for n, p in model.named_parameters() if n.startswith("infonce."))
    assert sum(resolve(model, [g])[0]) == sum(resolve(model, [g])[0]) == sum(1 for n, _ in model.named_parameters() if n.startswith("infonce."))


def test_resolve_refuses(model):
    with pytest.raises(ValueError, match="matches no parameter"):
        resolve(model, [ParamGroup("encoder"), ParamGroup("no_such_prefix")])
    with pytest.raises(ValueError, match="more than 256"):
        resolve(model, [ParamGroup("encoder")] * 256)
    resolve(model, [ParamGroup("encoder")] * 255)                       # 255 and the default one: the byte's range
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lr_scale"):
            resolve(model, [ParamGroup("encoder", lr_scale=bad)])
        with pytest.raises(ValueError, match="weight_decay"):
            resolve(model, [ParamGroup("encoder", weight_decay=bad)])
        with pytest.raises(ValueError, match="weight_decay"):
            resolve(model, [], bad)
    resolve(model, [ParamGroup("encoder", lr_scale=0.0, weight_decay=0.0)])      # zero is legal: the building block of gradual unfreezing


def test_no_decay_takes_biases_layernorms_and_the_pair_bias_tables(model):
    of, table = _by_name(model, no_decay(model), 0.01)
    assert table == [[1.0, 0.01], [1.0, 0.0]]
    for n, p in model.named_parameters():
        want = 1 if sum(d > 1 for d in p.shape) <= 1 else 0
        assert of[n] == want, n
    for n in ("encoder.layers.0.fc1.bias", "encoder.emb_layer_norm.weight", "bert.embeddings.LayerNorm.bias", "gbf.mul.weight", "gbf.bias.weight", "gbf.means.weight",
              "gbf.stds.weight", "classification_head.out_proj.bias"):
        assert of[n] == 1, n
    for n in ("encoder.layers.0.fc1.weight", "embed_tokens.weight", "bert.embeddings.word_embeddings.weight", "gbf_proj.linear1.weight"):
        assert of[n] == 0, n


def test_by_prefix(model):
    of, table = _by_name(model, by_prefix({"encoder": 0.1, "bert": 0.2}))
    assert table == [[1.0, 0.0], [0.1, 0.0], [0.2, 0.0]]
    assert all(g == (1 if n.startswith("encoder") else 2 if n.startswith("bert") else 0) for n, g in of.items())


def test_layerwise_decay_per_tower_with_the_trailing_dot(model):
    d = 0.5
    groups = layerwise_decay(model, d)
    of, table = _by_name(model, groups)
    scale = lambda n: table[of[n]][0]
    L1, L2 = 12, 2
    for n in ("embed_tokens.weight", "gbf.mul.weight", "gbf_proj.linear2.bias", "encoder.emb_layer_norm.weight"):
        assert scale(n) == d ** (L1 + 1), n                                     # depth 0
    for i in range(L1):
        assert scale(f"encoder.layers.{i}.fc1.weight") == d ** (L1 - i) and scale(f"encoder.layers.{i}.final_layer_norm.bias") == d ** (L1 - i), i
    assert scale("encoder.layers.1.fc2.bias") == d ** 11 and scale("encoder.layers.10.fc2.bias") == d ** 2 and scale("encoder.layers.11.fc2.bias") == d
    assert scale("bert.embeddings.word_embeddings.weight") == scale("bert.embeddings.LayerNorm.bias") == d ** (L2 + 1)
    assert scale("bert.encoder.layer.0.output.dense.weight") == d ** 2 and scale("bert.encoder.layer.1.output.dense.weight") == d
    for n, _ in model.named_parameters():                                       # everything outside the towers, and above their last layer: 1
        if n.startswith(("classification_head.", "cross_modal_module.", "infonce.", "bert.pooler.", "encoder.final_layer_norm.")):
            assert of[n] == 0 and scale(n) == 1.0, n
    assert len(groups) == 1 + L1 + 1 + L2 and [g.name for g in groups][:3] == ["unimol.depth0", "unimol.depth1", "unimol.depth2"]
    # lists concatenate and the first match wins: no_decay claims the biases before their layer's group
    of, table = _by_name(model, no_decay(model) + groups, 0.01)
    assert table[of["encoder.layers.3.fc1.bias"]] == [1.0, 0.0] and table[of["encoder.layers.3.fc1.weight"]] == [d ** 9, 0.01]


def test_arena_group_ids_padding_and_the_last_ragged_block():
    sizes, offsets = [5, 16, 9, 3], [0, 8, 24, 40]                   # padded to 8, 16, 16, 8 -- 43 elements used of 48, numel 43: the last block is ragged
    ids = arena_group_ids([3, 0, 7, 255], offsets, sizes, 43)
    assert ids.dtype == torch.uint8 and ids.tolist() == [3, 0, 0, 7, 7, 255]
    ids = arena_group_ids([3, 0, 7, 255], offsets, sizes, 48)
    assert ids.tolist() == [3, 0, 0, 7, 7, 255]
    assert arena_group_ids([1], [0], [1], 1).tolist() == [1]
    with pytest.raises(AssertionError):
        arena_group_ids([1, 2], [0, 4], [4, 4], 8)                      # an offset that is no multiple of 8
    with pytest.raises(AssertionError):
        arena_group_ids([256], [0], [8], 8)


def test_the_entry_point_is_in_the_header_and_the_documents():
    protos = _abi.parse_header()
    assert "mmdti_adam_step_grouped" in protos
    names = protos["mmdti_adam_step_grouped"][2]
    assert {"guard", "skip", "group", "table_dev"} <= set(names) and "weight_decay" not in names
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2
    header = open(_abi.HEADER).read()
    assert "Purely additive: MMDTI_ABI_VERSION does not move" in header and "tasks/trainer.py:160,270-282" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "mmdti_adam_step_grouped" in doc and f"exporting exactly the {len(protos)} symbols" in doc
    assert "Parameter groups" in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "param_groups" in open(os.path.join(ROOT, "README.md")).read()


def test_the_engine_and_the_trainer_take_the_new_arguments():
    import inspect
    from mmdti_hip.trainer import FineTuner
    sig = inspect.signature(FineTuner.__init__).parameters
    assert sig["weight_decay"].default == 0.0 and sig["decoupled_weight_decay"].default is False and sig["param_groups"].default is None
    assert callable(FineTuner.set_group) and callable(FineTuner.param_group_summary)
    from mmdti_hip.tasks.trainer import Trainer
    src = inspect.getsource(Trainer)
    for key in ("weight_decay", "decoupled_weight_decay", "param_groups", "layer_decay"):
        assert f"params.get('{key}'" in src, key
