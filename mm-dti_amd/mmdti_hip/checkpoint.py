"""Resuming a run: the plain logic of the training-state file (DESIGN.md "Resuming a run").  No device needed to import or to test.

The state ``FineTuner.state_dict()`` and ``tasks.Trainer`` write is tensors, numbers, strings, None, lists, tuples and dicts only, so the
whole file loads with ``torch.load(..., weights_only=True)``: no numpy arrays, no pickled objects.  What lives here is what the CPU
suite can hold to account: the version check, the host RNG streams as tensors and ints, the layout check of the parameter arena, the
per-rank dropout base and the atomic write.
"""
from __future__ import annotations

import os
import random
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

STATE_VERSION = 1

_RANK_STRIDE = 0x9E37       # distance between the dropout bases of two neighbouring ranks


def check_version(sd) -> int:
    """The state's ``version`` must be this module's STATE_VERSION; anything else is a ValueError naming both."""
    v = sd.get("version") if isinstance(sd, dict) else None
    if v != STATE_VERSION:
        raise ValueError(f"training state: the file has version {v!r}, this code reads version {STATE_VERSION}")
    return v


# ------------------------------------------------------------------------------------------------ host (and device) RNG streams
def pack_rng() -> dict:
    """The four generators that order batches and draw host-side randomness: torch's CPU generator, torch's device generators (once a
    device is initialised; None before), numpy's global MT19937 and Python's ``random`` -- as tensors, ints, strings and lists."""
    kind, key, pos, has_gauss, cached = np.random.get_state()
    version, words, gauss_next = random.getstate()
    device = None
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        device = [s.clone() for s in torch.cuda.get_rng_state_all()]
    return {
        "torch_cpu": torch.get_rng_state().clone(),
        "torch_device": device,
        "numpy": {"kind": str(kind), "key": torch.from_numpy(np.asarray(key, dtype=np.int64).copy()), "pos": int(pos),
                  "has_gauss": int(has_gauss), "cached_gaussian": float(cached)},
        "python": {"version": int(version), "words": [int(w) for w in words], "gauss_next": None if gauss_next is None else float(gauss_next)},
    }


def unpack_rng(d: dict):
    """Put the generators back where pack_rng found them.  The device generators are restored when the state has them, a device is
    there and the device count agrees (a state taken before the device was initialised carries none)."""
    torch.set_rng_state(d["torch_cpu"].cpu().to(torch.uint8))
    dev = d.get("torch_device")
    if dev is not None and torch.cuda.is_available() and len(dev) == torch.cuda.device_count():
        torch.cuda.set_rng_state_all([s.cpu().to(torch.uint8) for s in dev])
    n = d["numpy"]
    np.random.set_state((n["kind"], n["key"].cpu().numpy().astype(np.uint32), int(n["pos"]), int(n["has_gauss"]), float(n["cached_gaussian"])))
    p = d["python"]
    random.setstate((int(p["version"]), tuple(int(w) for w in p["words"]), p["gauss_next"]))


# ------------------------------------------------------------------------------------------------ the arena's layout
def check_layout(saved_names_numels: Sequence[Tuple[str, int]], own_names_numels: Sequence[Tuple[str, int]]):
    """The arena's parameters of the file against this engine's, (name, numel) pairs in arena order: passes only on an exact match,
    same order included.  ValueError lists up to five parameters that are missing from the file, unexpected in it, of another size, or
    in another place."""
    saved = [(str(n), int(k)) for n, k in saved_names_numels]
    own = [(str(n), int(k)) for n, k in own_names_numels]
    if saved == own:
        return
    s, o = dict(saved), dict(own)
    problems = [f"{n} (missing from the file)" for n, _ in own if n not in s]
    problems += [f"{n} (in the file, not in this model)" for n, _ in saved if n not in o]
    problems += [f"{n} ({s[n]} elements in the file, {k} here)" for n, k in own if n in s and s[n] != k]
    if not problems:
        problems = [f"{b} (position {i} here, {a} in the file)" for i, ((a, _), (b, _)) in enumerate(zip(saved, own)) if a != b]
    if not problems:            # (the same name twice on one side: no name is missing, the counts differ)
        problems = [f"{len(saved)} parameters in the file, {len(own)} here"]
    more = f" and {len(problems) - 5} more" if len(problems) > 5 else ""
    raise ValueError("training state: the optimizer's parameters differ from this engine's: " + "; ".join(problems[:5]) + more)


# ------------------------------------------------------------------------------------------------ the dropout stream of a rank
def dropout_base_for_rank(saved_base: int, saved_rank: Optional[int], rank: Optional[int]) -> int:
    """Under data parallelism rank r draws its dropout masks from ``base + 0x9E37 * (r + 1)`` (each rank holds other molecules), an
    engine on its own from ``base`` itself.  -> the base of ``rank`` given the base ``saved_base`` of ``saved_rank``; None on either side
    is the engine on its own, so ``dropout_base_for_rank(base, None, r)`` is the rule FineTuner applies when it is built and a state
    written by rank 0 gives every rank its own stream again."""
    off = lambda r: 0 if r is None else _RANK_STRIDE * (int(r) + 1)
    return int(saved_base) - off(saved_rank) + off(rank)


# ------------------------------------------------------------------------------------------------ the file
def atomic_save(obj, path):
    """torch.save to a temporary name carrying the pid, then os.replace: a reader (or a resumed run after a kill in mid-write) sees the
    previous file or the new one, never a part of one.  A failed write leaves the previous file as it was and no temporary file."""
    path = os.fspath(path)
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = path + f".tmp{os.getpid()}"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        _remove_quietly(tmp)
        raise


def _remove_quietly(path):
    try:
        os.remove(path)
    except OSError:
        pass


def load(path, map_location="cpu"):
    """The file as written by atomic_save, through the restricted unpickler (tensors and plain containers only)."""
    return torch.load(os.fspath(path), map_location=map_location, weights_only=True)
