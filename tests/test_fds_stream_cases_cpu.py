"""The streaming FDS statistics without a GPU: the cases of fds_stream_cases.py hold the situations they claim (so the GPU test cannot
be vacuous), the slot / Chan-merge / finish semantics restated in float64 equal the float64 second pass (models/fds.py:116-155 on the
concatenated epoch), the C ABI declares and binds the three entry points, and the host switches reject what they do not know."""
import os
import sys

import pytest
import torch

import fds_stream_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ENTRY_POINTS = ("mmdti_fds_stream_accumulate", "mmdti_fds_stream_merge", "mmdti_fds_stream_finish")


def test_case_table_covers_the_issue():
    assert {(c[0]) for c in C.CASE_KEYS} == {512, 48} and {(c[1], c[2]) for c in C.CASE_KEYS} == {(0, 30), (3, 9), (2, 3)}
    assert (300,) in C.CHUNKINGS and (256, 44) in C.CHUNKINGS and (1,) * 7 + (293,) in C.CHUNKINGS
    assert any(0 in s for s in C.CHUNKINGS) and all(sum(s) == C.ROWS for s in C.CHUNKINGS)
    claimed = set().union(*(C.case(*k).claims for k in C.CASE_KEYS))
    assert claimed == set(C.SITUATIONS)


@pytest.mark.parametrize("key", C.CASE_KEYS, ids=lambda k: "D%d_bs%d_bn%d" % k)
def test_case_holds_what_it_claims(key):
    c = C.case(*key)
    found = C.situations(c)
    assert c.claims <= found, sorted(c.claims - found)
    assert len(c.epochs) >= 2 and all(f.shape == (C.ROWS, c.D) and y.shape == (C.ROWS, 1) for f, y, _ in c.epochs)
    # the second pass itself shows them: a never-seen bucket keeps its initial statistics, the no-op call changes nothing
    states = C.second_pass(*key)
    if "never_seen_bucket" in c.claims:
        j = 2
        assert float(states[-1]["num_samples_tracked"][j]) == 0.0 and bool((states[-1]["running_var"][j] == 1).all())
    for k in states[-1]:
        assert torch.equal(states[-1][k], states[-2][k]), k
    assert float(states[0]["num_samples_tracked"].sum()) < C.ROWS          # rows were dropped (an overflow slot that did not merge)


@pytest.mark.parametrize("key", C.CASE_KEYS, ids=lambda k: "D%d_bs%d_bn%d" % k)
def test_float64_restatement_equals_second_pass(key):
    """slot accumulation + Chan merge + finish == update_running_stats on the concatenated epoch, to 1e-12, for every chunking and for
    the batches dealt to one, two and three accumulators -- the single-bucket rule included."""
    c = C.case(*key)
    ref = C.second_pass(*key)
    for sizes in C.CHUNKINGS:
        for shards in (1, 2, 3):
            got = C.streamed64(c, sizes, shards)
            for e, (g, r) in enumerate(zip(got, ref)):
                assert torch.equal(g["num_samples_tracked"], r["num_samples_tracked"]), (sizes, shards, e)
                for k in ("running_mean", "running_var"):
                    err = float((g[k] - r[k]).abs().max())
                    assert err <= 1e-12, (sizes, shards, e, k, err)
                assert bool((g["running_var"][:, C.CONST_COL][r["num_samples_tracked"] > 0] >= 0).all())


def test_header_declares_and_abi_binds_the_entry_points():
    from mmdti_hip import _abi
    protos = _abi.parse_header()
    for name in ENTRY_POINTS:
        assert name in protos, f"{name} is not declared in include/mmdti_hip.h"
    names = {n: protos[n][2] for n in ENTRY_POINTS}
    assert names["mmdti_fds_stream_accumulate"] == ["stream", "feats", "bins", "n", "D", "bucket_start", "bucket_num", "acc"]
    assert names["mmdti_fds_stream_merge"] == ["stream", "acc_dst", "acc_src", "nb", "D"]
    assert names["mmdti_fds_stream_finish"] == ["stream", "acc", "D", "bucket_start", "bucket_num", "factor", "running_mean", "running_var",
                                                "num_samples_tracked"]
    src = open(_abi.HEADER).read()
    for name in ENTRY_POINTS:                       # each cites what it restates
        head = src[:src.index("int " + name + "(")]
        comment = head[head.rindex("/*"):]
        assert "models/fds.py:116-155" in comment and "tasks/trainer.py:288-306" in comment, name
    assert _abi.header_constants()["MMDTI_ABI_VERSION"] == 2          # additive: no version bump
    if os.path.exists(_abi.LIB_PATH):
        lib = _abi.lib()                            # binds every declared symbol or raises
        for name in ENTRY_POINTS:
            assert callable(getattr(lib, name))
    from mmdti_hip import ops
    for fn in ("fds_stream_new", "fds_stream_accumulate", "fds_stream_merge", "fds_stream_finish"):
        assert callable(getattr(ops, fn))


def test_unknown_fds_stats_is_rejected_and_the_default_is_the_epoch_pass(tmp_path):
    import inspect
    from mmdti_hip.trainer import FineTuner
    from mmdti_hip.tasks import Trainer
    assert inspect.signature(FineTuner.__init__).parameters["fds_stats"].default == "epoch_pass"
    with pytest.raises(ValueError, match="fds_stats"):
        FineTuner(torch.nn.Linear(2, 2), "regression", fds_stats="both")
    assert Trainer(save_path=str(tmp_path), task="regression", metrics="mse").fds_stats == "epoch_pass"
    assert Trainer(save_path=str(tmp_path), task="regression", metrics="mse", fds_stats="streaming").fds_stats == "streaming"
    with pytest.raises(ValueError, match="fds_stats"):
        Trainer(save_path=str(tmp_path), task="regression", metrics="mse", fds_stats="stream")


def test_state_dict_keys_stay_the_references_with_an_accumulator_present():
    from mmdti_hip.models.fds import FDS
    c = C.case(48, 3, 9)
    keys = {"epoch", "running_mean", "running_var", "running_mean_last_epoch", "running_var_last_epoch", "smoothed_mean_last_epoch",
            "smoothed_var_last_epoch", "num_samples_tracked"}
    fds = FDS(c.D, c.raw, "", False, bucket_num=c.bn, bucket_start=c.bs, ks=c.ks)
    assert fds._stream_acc is None and set(fds.state_dict()) == keys
    fds._stream_acc = torch.zeros(c.nb + 2, 1 + 2 * c.D, dtype=torch.int32)      # what stream_reset() allocates on the device
    sd = fds.state_dict()
    assert set(sd) == keys
    other = FDS(c.D, c.raw, "", False, bucket_num=c.bn, bucket_start=c.bs, ks=c.ks)
    other.load_state_dict(sd, strict=True)                                      # the strict round trip
    assert other._stream_acc is None
