"""The host side of the attention-map read-out that needs no GPU: argument errors of the recorder and of MM_Model.attention_maps (raised
before any forward), the arithmetic of AttentionMaps' two helpers on CPU tensors, and the trimming of tasks.trainer.trim_attention_maps
/ Trainer.attention_maps on a stub model."""
import numpy as np
import pytest
import torch

from mmdti_hip import functional as Fn
from mmdti_hip._abi import MMDTIError
from mmdti_hip.models.mm_model import AttentionMaps
from mmdti_hip.tasks.trainer import trim_attention_maps


def test_recorder_arguments():
    for bad in (dict(which=()), dict(which=("cross", "pair")), dict(which="towers"), dict(layers="first"), dict(layers=[0, -1]), dict(layers=[0.5]),
                dict(head="max"), dict(head=-1), dict(head=True), dict(head=1.0)):
        with pytest.raises(ValueError, match="record_attention"):
            Fn.AttentionRecorder(**bad)
    r = Fn.AttentionRecorder("unimol", [0, 3], 2)
    assert r.which == ("unimol",) and r.layers == (0, 3) and r.head == 2
    assert r.wants("unimol", 3, 15) and not r.wants("unimol", 14, 15) and not r.wants("cross", 0, 1)
    last = Fn.AttentionRecorder(("cross", "bert"))
    assert last.head == -1 and last.wants("bert", 5, 6) and not last.wants("bert", 4, 6) and last.wants("cross", 0, 1) and not last.wants("unimol", 14, 15)
    every = Fn.AttentionRecorder(("bert",), "all")
    assert all(every.wants("bert", i, 6) for i in range(6))


def test_recorder_is_a_module_level_context():
    assert Fn.attention_recorder() is None
    with Fn.record_attention(which=("cross",)) as rec:
        assert Fn.attention_recorder() is rec and isinstance(rec, Fn.AttentionRecorder)
        with pytest.raises(MMDTIError, match="already live"):
            with Fn.record_attention(which=("bert",)):
                pass
        assert Fn.attention_recorder() is rec
    assert Fn.attention_recorder() is None
    with pytest.raises(RuntimeError, match="boom"):
        with Fn.record_attention(dict(which=("cross",))):
            raise RuntimeError("boom")
    assert Fn.attention_recorder() is None


def test_recorder_refusals_name_the_reason():
    r = Fn.AttentionRecorder()
    r.check("X", False, 0.0, 0.0)
    with pytest.raises(MMDTIError, match="X: .*keeps activations for a backward"):
        r.check("X", True, 0.0)
    with pytest.raises(MMDTIError, match="X: .*live dropout"):
        r.check("X", False, 0.0, 0.1)
    with pytest.raises(MMDTIError, match="head 5 asked of an attention with 4 heads"):
        Fn.AttentionRecorder(head=5)._head(4, "X")


def test_model_argument_errors_come_before_any_forward():
    from oracle import mmdti_oracle as O  # noqa: F401
    from g9util import tiny_cfg, product_model
    model = product_model(tiny_cfg("classification", 40))
    model.forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the forward ran"))
    toks = torch.ones(2, 5, dtype=torch.long)
    with pytest.raises(ValueError, match="which must be a non-empty subset"):
        model.attention_maps(src_tokens=toks, input_ids=toks, attention_mask=toks, which=("graph",))
    with pytest.raises(ValueError, match="layers must be"):
        model.attention_maps(src_tokens=toks, input_ids=toks, attention_mask=toks, layers="none")
    with pytest.raises(ValueError, match="head must be"):
        model.attention_maps(src_tokens=toks, input_ids=toks, attention_mask=toks, head="all")
    assert model.training


def _maps():
    g = torch.Generator().manual_seed(3)
    B, L, N = 3, 6, 5
    tok = torch.tensor([[1, 1, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]], dtype=torch.bool)
    atm = torch.tensor([[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0]], dtype=torch.bool)

    def probs(qm, km):
        x = torch.rand(B, qm.shape[1], km.shape[1], generator=g) + 0.1
        x = x * km.unsqueeze(1) * qm.unsqueeze(2)
        return x / x.sum(-1, keepdim=True).clamp_min(1e-30)

    maps = {"text_to_graph": {0: probs(tok, atm), 1: probs(tok, atm)}, "graph_to_text": {1: probs(atm, tok)}, "unimol": {14: probs(atm, atm)},
            "bert": {}}
    return AttentionMaps(torch.arange(6.0).view(3, 2), maps, atm, tok), maps, atm, tok


def test_relevance_helpers():
    am, maps, atm, tok = _maps()
    ar, tr = am.atom_relevance(), am.token_relevance()
    assert ar.shape == (3, 5) and tr.shape == (3, 6)
    for b in range(3):
        nt, na = int(tok[b].sum()), int(atm[b].sum())
        want_a = maps["text_to_graph"][1][b, :nt].mean(0)               # the LAST text_to_graph layer, real token queries only
        want_t = maps["graph_to_text"][1][b, :na].mean(0)
        assert torch.allclose(ar[b], want_a, atol=1e-7) and torch.allclose(tr[b], want_t, atol=1e-7)
        assert abs(float(ar[b].sum()) - 1) < 1e-6 and abs(float(tr[b].sum()) - 1) < 1e-6
        assert float(ar[b, na:].abs().sum()) == 0 and float(tr[b, nt:].abs().sum()) == 0
    empty = AttentionMaps(None, {"unimol": maps["unimol"]}, atm, tok)
    with pytest.raises(ValueError, match="no text_to_graph map was recorded"):
        empty.atom_relevance()
    with pytest.raises(ValueError, match="no graph_to_text map was recorded"):
        empty.token_relevance()


def test_trimming_per_molecule():
    am, maps, atm, tok = _maps()
    recs = list(trim_attention_maps(am))
    assert len(recs) == 3
    for b, r in enumerate(recs):
        na, nt = int(atm[b].sum()), int(tok[b].sum())
        assert (r["atoms"], r["tokens"]) == (na, nt) and np.array_equal(r["prediction"], np.array([2.0 * b, 2.0 * b + 1], dtype=np.float32))
        assert sorted(r["text_to_graph"]) == [0, 1] and r["text_to_graph"][1].shape == (nt, na) and r["graph_to_text"][1].shape == (na, nt)
        assert r["unimol"][14].shape == (na, na) and "bert" not in r
        assert np.array_equal(r["text_to_graph"][0], maps["text_to_graph"][0][b, :nt, :na].numpy())
        assert r["atom_relevance"].shape == (na,) and r["token_relevance"].shape == (nt,)
        assert abs(float(r["atom_relevance"].sum()) - 1) < 1e-6
        assert all(isinstance(v, np.ndarray) for d in (r["text_to_graph"], r["graph_to_text"], r["unimol"]) for v in d.values())


def test_trainer_generator_on_a_stub(monkeypatch):
    """Trainer.attention_maps walks the loader as predict does and yields one trimmed record per molecule, batch after batch"""
    from mmdti_hip.tasks import trainer as T
    am, maps, atm, tok = _maps()
    calls = []

    class Stub:
        def to(self, device):
            return self

        def attention_maps(self, **kw):
            calls.append(kw)
            return am

    tr = T.Trainer.__new__(T.Trainer)
    tr.batch_size, tr.device = 3, "cpu"
    monkeypatch.setattr(T.Trainer, "_require_device", lambda self: None)
    monkeypatch.setattr(T.Trainer, "_collate_for", lambda self, model: None)
    monkeypatch.setattr(T.Trainer, "_loader_kwargs", lambda self: {})
    monkeypatch.setattr(T, "NNDataLoader", lambda **kw: ["batch0", "batch1"])
    monkeypatch.setattr(T.Trainer, "device_batches", lambda self, dl, fn: (({"src_tokens": i}, None) for i, _ in enumerate(dl)))
    gen = tr.attention_maps(Stub(), dataset=None, dump_dir=None, fold=0, load_model=False, which=("cross", "unimol"), head=3)
    assert not calls                                   # a generator: nothing runs before the first record is asked for
    recs = list(gen)
    assert len(recs) == 6 and [c["src_tokens"] for c in calls] == [0, 1]
    assert all(c["which"] == ("cross", "unimol") and c["head"] == 3 for c in calls)
    assert [r["atoms"] for r in recs] == [3, 5, 1, 3, 5, 1]
