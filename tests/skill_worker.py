"""CPU worker for tests/test_forecast_skill_host.py: each gloo rank tables its half of the rows of fixed score planes with the torch
rule, then ``SkillTable.all_reduce`` sums the halves.  ``planes_case`` is shared with the single-process side of the test."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

B, T = 12, 9


def planes_case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Non-negative fp32 planes ``[8, B, T]``, per-row contexts and lengths (a dead row, a context past T, a row shorter than its context)."""
    g = torch.Generator().manual_seed(17)
    planes = torch.rand(8, B, T, generator=g) * 40.0
    context = torch.randint(1, T + 3, (B,), generator=g).to(torch.int32)
    valid = torch.randint(0, T + 2, (B,), generator=g).to(torch.int32)
    context[0], valid[0] = 2, T
    context[1], valid[1] = T + 2, T
    valid[2] = 0
    context[3], valid[3] = 5, 3
    return planes, context, valid


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    from multimodal_mtrssm_amd import ForecastSkill, SkillTable

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        planes, context, valid = planes_case()
        per = B // world
        rows = slice(rank * per, (rank + 1) * per)
        table = SkillTable(T)
        ForecastSkill.table_add(planes[:, rows].contiguous(), context[rows], valid[rows], table.sums, table.counts)
        table.all_reduce()
        torch.save(table.buffer.clone(), f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
