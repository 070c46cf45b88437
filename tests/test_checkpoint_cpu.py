"""mmdti_hip.checkpoint: the plain logic of the training-state file (DESIGN.md "Resuming a run") -- version, RNG streams, the arena's
layout check, the per-rank dropout base, the atomic write and the restricted load.  No device."""
import os
import random

import numpy as np
import pytest
import torch

from mmdti_hip import checkpoint as C


def test_rng_streams_survive_the_file(tmp_path):
    torch.manual_seed(11); np.random.seed(12); random.seed(13)
    np.random.randn(3); random.gauss(0.0, 1.0)                   # (both generators now hold a cached Gaussian)
    path = tmp_path / "rng.pth"
    torch.save(C.pack_rng(), path)
    want = (torch.randperm(17), np.random.rand(5), np.random.randn(2), [random.random() for _ in range(4)], random.gauss(0.0, 1.0))
    torch.manual_seed(99); np.random.seed(98); random.seed(97)   # somewhere else entirely
    C.unpack_rng(C.load(path))
    got = (torch.randperm(17), np.random.rand(5), np.random.randn(2), [random.random() for _ in range(4)], random.gauss(0.0, 1.0))
    assert torch.equal(want[0], got[0])
    assert np.array_equal(want[1], got[1]) and np.array_equal(want[2], got[2])
    assert want[3] == got[3] and want[4] == got[4]


def test_packed_rng_is_tensors_and_plain_values_only():
    def walk(x):
        if isinstance(x, dict):
            assert all(isinstance(k, str) for k in x)
            for v in x.values():
                walk(v)
        elif isinstance(x, (list, tuple)):
            for v in x:
                walk(v)
        else:
            assert x is None or isinstance(x, (torch.Tensor, int, float, str)) and not isinstance(x, np.generic), type(x)
    d = C.pack_rng()
    walk(d)
    assert isinstance(d["numpy"]["key"], torch.Tensor) and d["numpy"]["key"].numel() == 624


LAYOUT = [("enc.q.weight", 64), ("enc.k.weight", 64), ("enc.v.weight", 64), ("head.bias", 3)]


def test_check_layout_names_the_offending_parameters():
    C.check_layout(LAYOUT, list(LAYOUT))
    C.check_layout([list(x) for x in LAYOUT], LAYOUT)                       # (lists, as a file hands them back)
    with pytest.raises(ValueError, match=r"head\.bias \(missing from the file\)"):
        C.check_layout(LAYOUT[:3], LAYOUT)
    with pytest.raises(ValueError, match=r"extra\.weight \(in the file, not in this model\)"):
        C.check_layout(LAYOUT + [("extra.weight", 5)], LAYOUT)
    with pytest.raises(ValueError, match=r"enc\.k\.weight \(64 elements in the file, 128 here\)"):
        C.check_layout(LAYOUT, [LAYOUT[0], ("enc.k.weight", 128)] + LAYOUT[2:])
    with pytest.raises(ValueError, match=r"enc\.k\.weight \(position 0 here, enc\.q\.weight in the file\)") as e:
        C.check_layout(LAYOUT, [LAYOUT[1], LAYOUT[0]] + LAYOUT[2:])
    assert "enc.q.weight (position 1 here" in str(e.value) and "enc.v.weight" not in str(e.value)
    # at most five are listed, the rest counted
    many = [(f"p{i}", 8) for i in range(9)]
    with pytest.raises(ValueError) as e:
        C.check_layout([], many)
    assert str(e.value).count("missing from the file") == 5 and "and 4 more" in str(e.value)


def test_check_version():
    assert C.STATE_VERSION == 1
    C.check_version({"version": 1})
    with pytest.raises(ValueError, match=r"version 2.*version 1"):
        C.check_version({"version": 2})
    with pytest.raises(ValueError, match="None"):
        C.check_version({})


def test_dropout_base_for_rank():
    base = 0x5EED
    for r in range(8):
        own = base + 0x9E37 * (r + 1)                                         # the rule of FineTuner.__init__
        assert C.dropout_base_for_rank(base, None, r) == own
        assert C.dropout_base_for_rank(base + 0x9E37, 0, r) == own            # a state saved by rank 0
        assert C.dropout_base_for_rank(own, r, None) == base                  # and back to the engine on its own
        for s in range(8):
            assert C.dropout_base_for_rank(C.dropout_base_for_rank(base, s, r), r, s) == base
    assert C.dropout_base_for_rank(base, None, None) == base
    assert len({C.dropout_base_for_rank(base, 0, r) for r in range(8)}) == 8


def test_the_constructor_takes_its_rule_from_checkpoint_py():
    """the 0x9E37 rule lives in one place"""
    src = os.path.join(os.path.dirname(C.__file__), "trainer.py")
    text = open(src).read()
    assert "0x9E37" not in text and "dropout_base_for_rank(dropout_state.base, None," in text


def test_atomic_save_leaves_the_old_file_when_the_write_fails(tmp_path, monkeypatch):
    path = tmp_path / "sub" / "state.pth"
    C.atomic_save({"x": torch.arange(4)}, path)
    assert os.listdir(path.parent) == ["state.pth"]
    real = torch.save

    def half_then_raise(obj, f, *a, **k):
        real(obj, f, *a, **k)
        with open(f, "r+b") as fh:
            fh.truncate(10)                                                   # what a kill in mid-write leaves
        raise OSError("disk full")

    monkeypatch.setattr(torch, "save", half_then_raise)
    with pytest.raises(OSError, match="disk full"):
        C.atomic_save({"x": torch.zeros(4, dtype=torch.int64)}, path)
    monkeypatch.setattr(torch, "save", real)
    assert os.listdir(path.parent) == ["state.pth"]
    assert torch.equal(C.load(path)["x"], torch.arange(4))
    C.atomic_save({"x": torch.ones(4)}, path)
    assert os.listdir(path.parent) == ["state.pth"] and torch.equal(C.load(path)["x"], torch.ones(4))


def test_dropout_state_round_trip():
    from mmdti_hip.runtime import DropoutState
    a = DropoutState(123)
    for _ in range(5):
        a.next_seed()
    st = a.state()
    assert st == {"base": 123, "calls": 5}
    want = [a.next_seed() for _ in range(3)]
    b = DropoutState(7)
    b.next_seed()
    b.load_state(**st)
    assert [b.next_seed() for _ in range(3)] == want
    with pytest.raises(ValueError):
        b.load_state(1, -1)


def test_a_full_state_loads_with_weights_only(tmp_path):
    """every optional field set, in the types FineTuner.state_dict and tasks.Trainer write"""
    p = {"exp_avg": torch.randn(2, 3), "exp_avg_sq": torch.rand(2, 3), "ema": torch.randn(2, 3)}
    engine = {
        "version": C.STATE_VERSION,
        "model": {"w": torch.randn(2, 3), "FDS.running_mean": torch.zeros(4, 3), "FDS.epoch": torch.zeros(1)},
        "layout": [("w", 6)],
        "optimizer": {"step_count": 3, "flags": (True,), "params": {"w": p}},
        "trainable": {"w": True},
        "schedule": {"sched_step": 3, "total_steps": 20, "warmup": 2, "lr": 1e-3},
        "guard": torch.zeros(8),
        "graph": {"state": torch.zeros(4), "salt": torch.tensor([1 << 62, -5], dtype=torch.int64), "salted": True},
        "groups": {"names": ["default", "no_decay"], "table": [[1.0, 0.01], [0.5, 0.0]]},
        "ema": {"decay": 0.9, "warmup": True},
        "dropout": {"base": 0x5EED, "calls": 12, "rank": None},
        "task_loss": {"bins": 10, "alpha": 0.5, "last_bin_count": torch.arange(10.0)},
        "fds_stream": {"acc": torch.zeros(6, 7, dtype=torch.int32), "active": False},
        "deterministic": True,
    }
    state = {"engine": engine, "epoch": 1, "min_val_loss": float("inf"), "max_score": float("-inf"), "wait": 0,
             "history": [dict(epoch=0, steps=torch.zeros(4, 4), val_loss=0.5, metric="mse", score=0.5, skipped=0)],
             "rng": C.pack_rng(), "finished": False, "task_loss": None,
             "settings": dict(batch_size=8, accum_steps=1, epochs=4, seed=1)}
    path = tmp_path / "train_state_0.pth"
    C.atomic_save(state, path)
    back = C.load(path)
    C.check_version(back["engine"])
    C.check_layout(back["engine"]["layout"], [("w", 6)])
    assert back["engine"]["optimizer"]["flags"] == (True,) and back["engine"]["dropout"]["rank"] is None
    assert torch.equal(back["engine"]["graph"]["salt"], engine["graph"]["salt"]) and back["min_val_loss"] == float("inf")
    assert torch.equal(back["engine"]["optimizer"]["params"]["w"]["ema"], p["ema"])
    assert back["settings"] == state["settings"] and back["history"][0]["metric"] == "mse"
    # ... and an object that is not plain data does not
    from mmdti_hip.param_groups import ParamGroup
    C.atomic_save({"groups": [ParamGroup("encoder", 0.5)]}, tmp_path / "bad.pth")
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|global"):
        C.load(tmp_path / "bad.pth")
