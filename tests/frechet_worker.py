"""The case and the gloo worker of ``tests/test_frechet_gloo.py``: a rank folds the moments of its own feature rows (the non-GPU route of
``FrechetDistance.fold``, two streams, both sides) into a ``FrechetTable`` and all-reduces it over the group ``FlatDataParallel.frechet``
bound."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
ROWS, D = 48, 12
STREAMS = ("audio", "vision")
EDGES = (1, 2, 4)
NAMES = ("obs", "h1", "h2", "h4")


def case() -> dict[tuple[int, int], tuple[torch.Tensor, torch.Tensor]]:
    """Per (stream, side) fp32 features ``[ROWS, D]`` and int32 bins ``[ROWS]`` (some rows -1)."""
    g = torch.Generator().manual_seed(47)
    return {(s, side): (torch.randn(ROWS, D, generator=g) * (1.0 + s + side), torch.randint(-1, len(NAMES), (ROWS,), generator=g).to(torch.int32))
            for s in range(len(STREAMS)) for side in range(2)}


def table_of(rows: slice):  # noqa: ANN201
    """The ``FrechetTable`` of the rows ``rows`` of the case."""
    from multimodal_mtrssm_amd import FrechetDistance, FrechetTable  # noqa: PLC0415

    table = FrechetTable(STREAMS, D, NAMES)
    for (s, side), (x, bins) in case().items():
        FrechetDistance.fold(x[rows].contiguous(), bins[rows].contiguous(), len(NAMES), table.block(s, side))
    return table


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import FrechetDistance  # noqa: PLC0415
    from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415
    from multimodal_mtrssm_amd.parallel import FlatDataParallel  # noqa: PLC0415

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = FrechetDistance(3, samples=2, edges=EDGES)
        fd = dp.frechet(free)
        assert fd is not free and fd.group is group and free.group is None and fd.edges == EDGES and fd.bin_names == NAMES
        per = ROWS // world
        table = table_of(slice(rank * per, (rank + 1) * per))
        own = table.buffer.clone()
        assert table.all_reduce(fd.group) is table
        torch.save({"own": own, "reduced": table.buffer.clone()}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
