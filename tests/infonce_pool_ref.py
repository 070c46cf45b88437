"""Restatement of InfoNCE(pool="real") from the oracle's public pieces (oracle/ itself stays as it is): the per-token
Linear - GELU - Linear of infonce.py:28-31 (O.linear, O.gelu), then the mean over the REAL positions where infonce.py:32-33 -- and
O.infonce_embed -- average over every position, then O.info_nce.  Everything else of a step is O.mm_forward's.

Any dtype: hand it float64 tensors for a float64 reference, bf16=True for the oracle's 16-bit contract."""
import torch

from oracle import mmdti_oracle as O


def masked_mean(x, mask):
    """x [B, S, d], mask [B, S] (non-zero = real) -> [B, d]: sum over real positions / their number (an empty sequence: zeros).  Masked
    rows are selected away, never multiplied: they may hold anything."""
    m = mask.bool()
    kept = torch.where(m.unsqueeze(-1), x, torch.zeros((), dtype=x.dtype))
    return kept.sum(dim=1) / m.sum(dim=1).clamp(min=1).view(-1, 1).to(x.dtype)


def infonce_embed_real(query, positive, query_mask, key_mask, P, pre="infonce.", p=0.0, training=False, bf16=False):
    xq = O.dropout(query, p, training)

    def proj(x, name):
        h = O.gelu(O.linear(x, P[pre + name + ".0.weight"], P[pre + name + ".0.bias"], bf16))
        return O._r(O.linear(h, P[pre + name + ".2.weight"], P[pre + name + ".2.bias"], bf16), bf16, "proj")

    return masked_mean(proj(xq, "info_proj_query"), query_mask), masked_mean(proj(positive, "info_proj_positive"), key_mask)


def infonce_forward_real(query, positive, query_mask, key_mask, P, pre="infonce.", temperature=0.1, p=0.0, training=False, bf16=False):
    a, b = infonce_embed_real(query, positive, query_mask, key_mask, P, pre, p, training, bf16)
    return O.info_nce(a, b, temperature=temperature)


def mm_forward_real(batch, P, cfg, **kw):
    """O.mm_forward with the InfoNCE term pooled over the real tokens (dropout off: the callers compare at p = 0)."""
    out = O.mm_forward(batch, P, cfg, **kw)
    img_mask = ~batch["src_tokens"].eq(cfg.unimol.pad_idx)
    out["infonce"] = infonce_forward_real(out["enc"], out["bert"], img_mask, batch["attention_mask"].bool(), P, "infonce.", cfg.infonce_temp,
                                          0.0, False, kw.get("bf16", False))
    return out
