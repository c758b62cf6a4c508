"""The case and the gloo worker of ``tests/test_census_gloo.py``: a rank folds the census of its own rows of a batch (the non-GPU route of
``LatentCensus.fold``, two latent levels) into a ``CensusTable`` and all-reduces it over the group ``FlatDataParallel.census`` bound."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
B, G, T = 8, 3, 7
LEVELS = (("l", 3, 4), ("h", 2, 5))
OBSERVE = ("both", "audio", "vision")


def case() -> tuple[list[tuple[torch.Tensor, torch.Tensor, torch.Tensor]], torch.Tensor]:
    """Per level fp32 ``(post_logits, prior_logits, stoch)`` ``[B * G, T, K * C]`` and the rows' lengths (a dead row, a whole row, a
    one-frame row, the rest random)."""
    g = torch.Generator().manual_seed(43)
    levels = []
    for _, k, c in LEVELS:
        post, prior = torch.randn(B * G, T, k * c, generator=g) * 2.0, torch.randn(B * G, T, k * c, generator=g) * 2.0
        idx = torch.randint(0, c, (B * G, T, k), generator=g)
        levels.append((post, prior, torch.nn.functional.one_hot(idx, c).to(torch.float32).reshape(B * G, T, k * c)))
    valid = torch.randint(0, T + 2, (B,), generator=g).to(torch.int32)
    valid[2], valid[5], valid[6] = 0, T, 1
    return levels, valid


def table_of(rows: slice):  # noqa: ANN201
    """The ``CensusTable`` of the batch rows ``rows`` of the case."""
    from multimodal_mtrssm_amd import CensusTable, LatentCensus  # noqa: PLC0415

    levels, valid = case()
    table = CensusTable(LEVELS, G, T, observe=OBSERVE)
    for level, ((_, k, c), tensors) in enumerate(zip(LEVELS, levels, strict=True)):
        mine = [x[rows.start * G : rows.stop * G].contiguous() for x in tensors]
        LatentCensus.fold(*mine, G, k, c, valid[rows].contiguous(), table=table.level_view(level), planes=False)
    return table


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import LatentCensus  # noqa: PLC0415
    from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415
    from multimodal_mtrssm_amd.parallel import FlatDataParallel  # noqa: PLC0415

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = LatentCensus(OBSERVE)
        census = dp.census(free)
        assert census is not free and census.group is group and free.group is None and census.observe == OBSERVE
        per = B // world
        table = table_of(slice(rank * per, (rank + 1) * per))
        own = table.buffer.clone()
        assert table.all_reduce(census.group) is table
        torch.save({"own": own, "reduced": table.buffer.clone()}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
