"""The case and the gloo worker of ``tests/test_particle_gloo.py``: a rank folds its own rows of a batch segment by segment (the non-GPU
route of ``ParticleFilter.fold``) into a ``ParticleTable`` and all-reduces it over the group ``FlatDataParallel.particle`` bound."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
B, T, S, C = 12, 9, 4, 2
EVENTS = (96, 40)
THRESHOLD = 0.75


def case() -> tuple[tuple[torch.Tensor, torch.Tensor, torch.Tensor], torch.Tensor, torch.Tensor]:
    """fp32 errors and log-ratios ``[B, S, T]``, the rows' lengths (a dead row, a whole row, the rest random) and ``u_resample``."""
    g = torch.Generator().manual_seed(31)
    se_a = torch.rand(B, S, T, generator=g) * 3.0 + 40.0
    se_v = torch.rand(B, S, T, generator=g) * 3.0 + 10.0
    ratio = -torch.rand(B, S, T, generator=g)
    valid = torch.randint(0, T + 2, (B,), generator=g).to(torch.int32)
    valid[2], valid[7] = 0, T
    return (se_a, se_v, ratio), valid, torch.rand(B, T, generator=g)


def table_of(rows: slice):  # noqa: ANN201
    """The ``ParticleTable`` of the rows ``rows``: one ``fold`` per segment, the carry chained, the planes folded by frame position."""
    from multimodal_mtrssm_amd import ParticleFilter, ParticleTable  # noqa: PLC0415

    inputs, valid, u = case()
    inputs, valid, u = [x[rows].contiguous() for x in inputs], valid[rows].contiguous(), u[rows].contiguous()
    pf = ParticleFilter(S, C, THRESHOLD)
    carry = ParticleFilter.new_carry(valid.numel(), S)
    planes = torch.empty(8, valid.numel(), T)
    for t0, t1 in pf.segments(T):
        last = t1 == T
        part, _ = ParticleFilter.fold(*(x[:, :, t0:t1] for x in inputs), valid, None if last else u[:, t1 - 1], t0, pf.threshold, last, carry, *EVENTS)
        planes[:, :, t0:t1] = part
    return ParticleTable(T).fold(planes, valid)


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import ParticleFilter  # noqa: PLC0415
    from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415
    from multimodal_mtrssm_amd.parallel import FlatDataParallel  # noqa: PLC0415

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = ParticleFilter(S, C, THRESHOLD)
        pf = dp.particle(free)
        assert pf is not free and pf.group is group and free.group is None and (pf.samples, pf.resample_every, pf.threshold) == (S, C, THRESHOLD)
        per = B // world
        table = table_of(slice(rank * per, (rank + 1) * per))
        own = table.buffer.clone()
        assert table.all_reduce(pf.group) is table
        torch.save({"own": own, "reduced": table.buffer.clone()}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
