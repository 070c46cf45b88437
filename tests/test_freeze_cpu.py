"""CPU tests of partial fine-tuning (the reference's freeze_layers, models/nnmodel.py:112-127): the backward plan of
mmdti_hip.freeze, the masked Adam pass's skip mask, and the prefix matching."""
import torch

from mmdti_hip.freeze import arena_skip_mask, first_trainable, freeze_layers, layer_trainable, plan_tower


def test_plan_stops_at_lowest_trainable_layer():
    # R6: embedding, pair-bias front end, embedding LayerNorm and layers 0-7 frozen
    p = plan_tower([False] * 8 + [True] * 7, below_needs=False, bias_needs=False)
    assert p.lowest == 8 and not p.dx_out and not p.below
    assert not p.needs_dx(8) and p.needs_dx(9)            # layer 8 hands nothing down; layer 9 feeds layer 8


def test_plan_runs_to_layer_zero_when_below_trains():
    # R1: embedding and pair-bias front end frozen, embedding LayerNorm trainable -> every layer runs and dx reaches layer 0's input
    p = plan_tower([True] * 15, below_needs=True, bias_needs=False)
    assert p.lowest == 0 and p.dx_out and p.below and p.needs_dx(0)
    # R4: the whole encoder frozen but the embedding table trains: the backward still walks every (frozen) layer for dx
    p = plan_tower([False] * 15, below_needs=True)
    assert p.lowest == 0 and p.dx_out


def test_plan_pair_bias_keeps_whole_chain():
    # the pair-gradient chain must reach layer 0 through every (even frozen) layer; no stream gradient leaves layer 0
    p = plan_tower([False] * 15, below_needs=False, bias_needs=True)
    assert p.lowest == 0 and not p.dx_out and not p.below and not p.needs_dx(0) and p.needs_dx(1)


def test_plan_frozen_tower_runs_no_layer():
    p = plan_tower([False] * 6, below_needs=False)
    assert p.lowest == 6 and not p.below
    p = plan_tower([], below_needs=False)
    assert p.lowest == 0 and not p.dx_out


def _toy():
    return torch.nn.ModuleDict({"embed_tokens": torch.nn.Embedding(5, 4),
                                "encoder": torch.nn.ModuleDict({"layers": torch.nn.ModuleList([torch.nn.Linear(4, 4) for _ in range(12)])}),
                                "head": torch.nn.Linear(4, 2)})


def test_freeze_layers_matches_reference_prefix_rules():
    m = _toy()
    freeze_layers(m, "embed_tokens, encoder.layers.1")
    frozen = {n for n, p in m.named_parameters() if not p.requires_grad}
    # prefix matching: encoder.layers.1 also hits layers 10 and 11 (a reference quirk, kept)
    assert frozen == {"embed_tokens.weight"} | {f"encoder.layers.{i}.{w}" for i in (1, 10, 11) for w in ("weight", "bias")}
    assert layer_trainable(m["encoder"]["layers"]) == tuple(i not in (1, 10, 11) for i in range(12))
    freeze_layers(m, ["head"], freeze_layers_reversed=True)
    assert {n for n, p in m.named_parameters() if p.requires_grad} == {"head.weight", "head.bias"}
    assert first_trainable(m.parameters()) is m["head"].weight
    assert first_trainable(m["encoder"].parameters()) is None


def test_skip_mask_covers_frozen_ranges_only():
    assert arena_skip_mask([True, True], [0, 8], [5, 3], 16) is None
    m = arena_skip_mask([True, False, True], [0, 8, 24], [5, 13, 8], 32)
    assert m.dtype == torch.uint8 and m.tolist() == [0, 1, 1, 0]


def test_grad_anchor_is_left_out_under_no_grad():
    from mmdti_hip.freeze import grad_anchor
    m = _toy()
    assert grad_anchor(m.parameters()) is m["embed_tokens"].weight
    with torch.no_grad():                     # (needs_input_grad would still report the parameter: inference must keep nothing)
        assert grad_anchor(m.parameters()) is None


def test_reducer_stops_waiting_for_frozen_parameters():
    """ArenaReducer.set_trainable: a parameter frozen after construction never reports, so no bucket waits for it."""
    from types import SimpleNamespace
    from mmdti_hip.parallel import ArenaReducer
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in (16, 8, 24)]
    offs = {id(p): o for p, o in zip(ps, (0, 16, 24))}
    arena = SimpleNamespace(numel=48, params=ps, offsets=offs, grad=torch.zeros(48))
    red = ArenaReducer(arena, bucket_bytes=4 * 16)                 # buckets [0,16) [16,32) [32,48)
    red.begin_step()
    assert [len(u) for u in red.unreported()] == [1, 2, 1]
    red.set_trainable((True, False, True))
    red.begin_step()
    assert [u for u in red.unreported()] == [{id(ps[0])}, {id(ps[2])}, {id(ps[2])}]
    red.set_trainable((True, True, True))
    assert [len(u) for u in red.unreported()] == [1, 2, 1]
