"""Drop-in for the reference's ``models/infonce.py`` (InfoNCE module + info_nce function), MI355X-native.

Same class/function names, ctor arguments, child names (``info_proj_query.{0,2}``, ``info_proj_positive.{0,2}``) and
``ValueError`` behaviour as /root/reference/models/infonce.py:6-105.  Reference quirks kept: the per-token projections
are averaged over ALL sequence positions including padding (:32-33); dropout (p=0.1) is applied to the query side only
(:24); the explicit ``negative_keys`` branches can never return (the symmetric cross-entropy at :98 raises for
non-square logits) -- here they raise ``ValueError`` up front.

Extension for data parallelism (absent from the reference): ``set_global_negatives(gather, reduce_scatter, rank_row0)``
makes the B x B logits use every rank's keys.

Second extension, opt-in: ``InfoNCE(..., pool="real")`` averages the per-token projections over the REAL positions only (the
reference's :32-33 averages over padding too; ``pool="all"``, the default, keeps that).  The head is random-initialised at
fine-tune time, so no checkpoint carries the difference; with it no padded row is read by anything in the model, the embedding
of a molecule no longer depends on how far its batch is padded, and packed token rows need no pad row (packing.py).

Third extension, opt-in: ``InfoNCE(..., memory_bank=Q)`` keeps, per side, a ring of the last Q L2-normalised embeddings on the device
and uses them as extra negatives that receive no gradient (XBM, Wang et al. 2020; the MoCo queue): at the reference's batch of 32 an
anchor meets 31 + Q negatives instead of 31, for no extra forward.  Stored keys are stale by up to Q / batch steps.  Only training
forwards with gradients enabled read or write the ring; ``memory_bank=0`` (default) allocates and launches nothing.
"""
import torch
from torch import nn

from ..functional import InfoNCEFn, InfoNCELossFn
from ..freeze import grad_anchor


POOLS = ("all", "real")


def pool_from_env(value=None):
    """The pooling MM_Model(infonce_pool=None) takes: MMDTI_INFONCE_POOL = all | real, unset = "all" (the reference)."""
    import os
    v = os.environ.get("MMDTI_INFONCE_POOL") if value is None else value
    if v is None or v == "":
        return "all"
    if v not in POOLS:
        raise ValueError(f"MMDTI_INFONCE_POOL / infonce_pool must be one of {POOLS} (got {v!r})")
    return v


def check_memory_bank(Q, who="InfoNCE"):
    """-> Q as a non-negative int (0: no bank), or ValueError"""
    if isinstance(Q, bool) or not isinstance(Q, int) or Q < 0 or Q > (1 << 24):
        raise ValueError(f"{who}: memory_bank must be an int in [0, 2**24] (slots per side; 0 = off), got {Q!r}")
    return Q


class MemoryRing:
    """One side's ring: rows [Q, d] fp32, valid [Q] uint8, ids [Q] int64 (-1: none), head [1] int32 -- plain device tensors."""
    FIELDS = ("rows", "valid", "ids", "head")

    def __init__(self, Q, d, device):
        self.rows = torch.zeros(Q, d, device=device, dtype=torch.float32)
        self.valid = torch.zeros(Q, device=device, dtype=torch.uint8)
        self.ids = torch.full((Q,), -1, device=device, dtype=torch.int64)
        self.head = torch.zeros(1, device=device, dtype=torch.int32)

    def reset(self):
        self.valid.zero_()
        self.head.zero_()

    def tensors(self):
        return [getattr(self, f) for f in self.FIELDS]

    def to(self, device):
        for f in self.FIELDS:
            setattr(self, f, getattr(self, f).to(device))


class InfoNCE(nn.Module):
    def __init__(self, bert_output_size, graph_ouput_size, temperature=0.1, reduction='mean', negative_mode='unpaired', pool="all",
                 memory_bank=0):
        super().__init__()
        self.memory_bank, self.bank_q, self.bank_k = 0, None, None
        if pool not in POOLS:
            raise ValueError(f"InfoNCE: pool must be one of {POOLS} (got {pool!r})")
        self.pool = pool
        self.temperature = temperature
        self.reduction = reduction
        self.negative_mode = negative_mode
        self.orig_d_l = bert_output_size
        self.orig_d_av = graph_ouput_size
        self.d_l, self.d_av = 50, 50
        self.embed_dropout = 0.1
        self.training = True
        self.info_proj_query = nn.Sequential(nn.Linear(self.orig_d_l, self.orig_d_l), nn.GELU(), nn.Linear(self.orig_d_l, self.d_l))
        self.info_proj_positive = nn.Sequential(nn.Linear(self.orig_d_av, self.orig_d_av), nn.GELU(), nn.Linear(self.orig_d_av, self.d_av))
        self._gather = None
        self._reduce_scatter = None
        self._row0 = 0
        self.set_memory_bank(memory_bank)

    def set_global_negatives(self, gather, reduce_scatter, row0):
        self._gather, self._reduce_scatter, self._row0 = gather, reduce_scatter, int(row0)

    # ------------------------------------------------------------------ memory bank of negatives
    def set_memory_bank(self, Q):
        """Q slots per side (0: none).  bank_q holds past query-side embeddings (keys of direction b), bank_k past positive-side ones
        (keys of direction a); both start empty.  Plain tensors on the parameters' device, not buffers: state_dict() keeps the
        reference's keys (FineTuner.state_dict carries the rings)."""
        Q = check_memory_bank(Q)
        self.memory_bank = Q
        if Q == 0:
            self.bank_q = self.bank_k = None
            return
        dev = self.info_proj_query[0].weight.device
        self.bank_q, self.bank_k = MemoryRing(Q, self.d_l, dev), MemoryRing(Q, self.d_av, dev)

    def reset_memory_bank(self):
        for ring in (self.bank_q, self.bank_k):
            if ring is not None:
                ring.reset()

    def memory_bank_state(self):
        """-> [(name, tensor)] of both rings in a fixed order (FineTuner.state_dict / load_state_dict / graph capture); [] without a bank"""
        if self.bank_q is None:
            return []
        return [(f"{side}.{f}", getattr(ring, f)) for side, ring in (("q", self.bank_q), ("k", self.bank_k)) for f in MemoryRing.FIELDS]

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        if self.bank_q is not None:       # (the rings follow the parameters' device; their dtypes are fixed)
            dev = self.info_proj_query[0].weight.device
            self.bank_q.to(dev)
            self.bank_k.to(dev)
        return out

    def _bank(self, sample_ids, batch):
        """What a forward hands to InfoNCEFn: None unless this is a training forward with gradients enabled -- eval, the FDS epoch pass
        and any no_grad forward neither read nor write the rings."""
        if self.bank_q is None or not (self.training and torch.is_grad_enabled()):
            return None
        if sample_ids is not None and (sample_ids.dtype != torch.int64 or sample_ids.dim() != 1 or sample_ids.shape[0] != batch):
            raise ValueError(f"InfoNCE: sample_ids must be [{batch}] int64, got {tuple(sample_ids.shape)} {sample_ids.dtype}")
        return (self.bank_q, self.bank_k, sample_ids)

    def forward(self, query, positive_key, negative_keys=None, packs=None, query_mask=None, key_mask=None, sample_ids=None):
        """packs = (PackedRows of query, PackedRows of positive_key): the inputs are packed rows [M, D] (packing.py); the
        unmasked mean of infonce.py:32-33 weights each representative pad row by the padded positions it stands for.
        pool="real": padded inputs need query_mask / key_mask ([B,S] bool / uint8, non-zero = real); packed rows need pad-free packs
        (PackedRows(pad_row=False)).  pool="all" reads no mask and refuses a pad-free pack: it has no pad row to weight."""
        masks = None
        if self.pool == "real":
            if packs is not None:
                if any(getattr(pk, "pad_row", True) and pk.n_pad_rows for pk in packs):
                    raise ValueError("InfoNCE(pool='real'): packed rows must be pad-free (PackedRows(pad_row=False))")
            else:
                if query_mask is None or key_mask is None:
                    raise ValueError("InfoNCE(pool='real'): padded inputs need query_mask and key_mask ([B,S], non-zero = real)")
                for m, x in ((query_mask, query), (key_mask, positive_key)):
                    if m.dtype not in (torch.bool, torch.uint8) or tuple(m.shape) != tuple(x.shape[:2]):
                        raise ValueError("InfoNCE(pool='real'): a mask must be [batch, seq] bool / uint8 over its input")
                masks = (query_mask, key_mask)
        elif packs is not None and any(not getattr(pk, "pad_row", True) and int(pk.counts_host.min()) < pk.S for pk in packs):
            raise ValueError("InfoNCE(pool='all'): a pad-free pack has no pad row for the mean over all positions (infonce.py:32-33)")
        if packs is not None:
            if negative_keys is not None or self.reduction != 'mean' or query.dim() != 2 or positive_key.dim() != 2 or packs[0].B != packs[1].B:
                raise ValueError('packed rows: <query> / <positive_key> must be [rows, dim] with one packing each, implicit negatives.')
            return InfoNCEFn.apply(query.float(), positive_key.float(), self, self.training, self._gather, self._reduce_scatter, self._row0, packs,
                                   grad_anchor(self.parameters()), masks, self._bank(sample_ids, packs[0].B))
        if negative_keys is not None:
            raise ValueError("explicit negative_keys are unreachable in the reference (infonce.py:98 raises); not supported")
        if self.reduction != 'mean':
            raise ValueError("only reduction='mean' is on the MM-DTI path")
        if self.orig_d_l == self.d_l or self.orig_d_av == self.d_av:
            raise ValueError("identity projection (input width == 50) is not on the MM-DTI path")
        if query.dim() != 3 or positive_key.dim() != 3:
            raise ValueError('<query> and <positive_key> must be [batch, seq, dim] token representations.')
        if len(query) != len(positive_key):
            raise ValueError('<query> and <positive_key> must must have the same number of samples.')
        return InfoNCEFn.apply(query.float(), positive_key.float(), self, self.training, self._gather, self._reduce_scatter, self._row0, None,
                               grad_anchor(self.parameters()), masks, self._bank(sample_ids, len(query)))


def info_nce(query, positive_key, negative_keys=None, temperature=0.1, reduction='mean', negative_mode='unpaired'):
    # Check input dimensionality (models/infonce.py:45-67).
    if query.dim() != 2:
        raise ValueError('<query> must have 2 dimensions.')
    if positive_key.dim() != 2:
        raise ValueError('<positive_key> must have 2 dimensions.')
    if negative_keys is not None:
        if negative_mode == 'unpaired' and negative_keys.dim() != 2:
            raise ValueError("<negative_keys> must have 2 dimensions if <negative_mode> == 'unpaired'.")
        if negative_mode == 'paired' and negative_keys.dim() != 3:
            raise ValueError("<negative_keys> must have 3 dimensions if <negative_mode> == 'paired'.")
    if len(query) != len(positive_key):
        raise ValueError('<query> and <positive_key> must must have the same number of samples.')
    if negative_keys is not None:
        if negative_mode == 'paired' and len(query) != len(negative_keys):
            raise ValueError("If negative_mode == 'paired', then <negative_keys> must have the same number of samples as <query>.")
    if query.shape[-1] != positive_key.shape[-1]:
        raise ValueError('Vectors of <query> and <positive_key> should have the same number of components.')
    if negative_keys is not None:
        if query.shape[-1] != negative_keys.shape[-1]:
            raise ValueError('Vectors of <query> and <negative_keys> should have the same number of components.')
        raise ValueError("explicit negative_keys: the reference's symmetric cross-entropy (infonce.py:98) raises for "
                         "non-square logits; this path is unreachable there and unsupported here")
    if reduction != 'mean':
        raise ValueError("only reduction='mean' is on the MM-DTI path")
    return InfoNCELossFn.apply(query.float(), positive_key.float(), float(temperature))
