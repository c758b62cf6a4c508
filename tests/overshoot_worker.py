"""The case and the gloo worker of ``tests/test_overshoot_gloo.py``: a rank takes the overshoot KL of its own rows of a batch (the
non-GPU route of ``LatentOvershoot.kl``), all-reduces its loss term (mean) and its ``OvershootTable`` over the group
``FlatDataParallel.overshoot`` bound."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
B, T, K, C = 8, 9, 3, 4
DEPTH, STRIDE, OFFSET = 4, 2, 1


def case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 closed-loop posterior logits ``[B, T, K * C]``, the overshoot rows' prior logits ``[B * N, D, K * C]`` and the rows' lengths
    (a dead row, a whole row, the rest random)."""
    from multimodal_mtrssm_amd import LatentOvershoot  # noqa: PLC0415

    n = LatentOvershoot(DEPTH, stride=STRIDE, offset=OFFSET).rows(T)
    g = torch.Generator().manual_seed(41)
    post = torch.randn(B, T, K * C, generator=g) * 2.0
    os_logits = torch.randn(B * n, DEPTH, K * C, generator=g) * 2.0
    valid = torch.randint(0, T + 2, (B,), generator=g).to(torch.int32)
    valid[2], valid[5] = 0, T
    return post, os_logits, valid


def terms_of(lo, rows: slice):  # noqa: ANN001, ANN201
    """``lo.kl`` on the rows ``rows`` of the case, with the lengths of ALL rows."""
    post, os_logits, valid = case()
    n = lo.rows(T)
    return lo.kl(post[rows].contiguous(), os_logits[rows.start * n : rows.stop * n].contiguous(), K, valid, rows.start, (1.0, 1.0))


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import LatentOvershoot, OvershootTable  # noqa: PLC0415
    from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415
    from multimodal_mtrssm_amd.parallel import FlatDataParallel  # noqa: PLC0415

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = LatentOvershoot(DEPTH, stride=STRIDE, offset=OFFSET)
        lo = dp.overshoot(free)
        assert lo is not free and lo.group is group and free.group is None and (lo.world, lo.rank, free.world) == (world, rank, 1)
        per = B // world
        terms = terms_of(lo, slice(rank * per, (rank + 1) * per))
        table = OvershootTable(1, DEPTH).fold([terms.table])
        own = table.buffer.clone()
        assert table.all_reduce(lo.group) is table
        loss = terms.term.detach().to(torch.float64).clone()
        dist.all_reduce(loss, op=dist.ReduceOp.SUM, group=group)
        torch.save({"own": own, "reduced": table.buffer.clone(), "term": terms.term.detach(), "mean": loss / world, "count": terms.count},
                   f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
