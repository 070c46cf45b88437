"""Two gloo ranks (CPU): parallel.gather_fds_accumulators -- the one collective of the streaming FDS statistics under data parallelism
-- returns both ranks' accumulators in rank order on both ranks, bit for bit (the merge and the finish that follow are device kernels:
tests/test_fds_stream_gpu.py)."""
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _acc_of(rank, nb, D):
    """a filled accumulator as ops.fds_stream_new lays it out: int32 [nb + 2, 1 + 2 D] = { rows | fp32 mean | fp32 M2 } per slot"""
    g = torch.Generator().manual_seed(17 + rank)
    acc = torch.zeros(nb + 2, 1 + 2 * D, dtype=torch.int32)
    acc[:, 0] = torch.randint(0, 50, (nb + 2,), generator=g, dtype=torch.int32)
    acc.view(torch.float32)[:, 1:] = torch.randn(nb + 2, 2 * D, generator=g)
    return acc


def _worker_gather(rank, world, initfile, out):
    for p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world, init_method=f"file://{initfile}")
    from mmdti_hip.parallel import gather_fds_accumulators
    nb, D = 6, 48
    mine = _acc_of(rank, nb, D)
    before = mine.clone()
    parts = gather_fds_accumulators(mine)
    assert isinstance(parts, list) and len(parts) == world
    for r, part in enumerate(parts):
        assert part.dtype == torch.int32 and part.shape == (nb + 2, 1 + 2 * D)
        assert torch.equal(part, _acc_of(r, nb, D)), r                  # rank order, every word as sent
    assert torch.equal(mine, before)                                    # the input is not written
    if rank == 0:
        torch.save({"ok": True}, out)
    dist.destroy_process_group()


def test_two_ranks_gather_accumulators_in_rank_order():
    with tempfile.TemporaryDirectory() as td:
        initfile, out = os.path.join(td, "init"), os.path.join(td, "out.pt")
        mp.spawn(_worker_gather, args=(2, initfile, out), nprocs=2, join=True)
        assert torch.load(out)["ok"]


def test_one_process_returns_the_accumulator_itself():
    for p in (ROOT, os.path.join(ROOT, "mm-dti_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from mmdti_hip.parallel import gather_fds_accumulators
    acc = _acc_of(0, 3, 8)
    parts = gather_fds_accumulators(acc)
    assert len(parts) == 1 and parts[0] is acc
