"""The case and the gloo worker of ``tests/test_coherence_gloo.py``: a rank folds the coherence of its own rows of a batch (the non-GPU
route of ``GenerationCoherence.fold``) into a ``CoherenceTable`` and all-reduces it over the group ``FlatDataParallel.coherence`` bound."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
B, G, S, T, CONTEXT = 8, 3, 2, 9, 4
OBSERVE = ("both", "audio", "vision")


def case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 logits of both readers ``[B * G * S, T, 10]``, int32 labels ``[B, T]`` and the rows' lengths (a dead row, a whole row, a
    one-frame row, the rest random)."""
    from tests.test_coherence_host import coherence_inputs  # noqa: PLC0415

    lv, la, labels = coherence_inputs(B, G, S, T, seed=43)
    valid = torch.randint(0, T + 2, (B,), generator=torch.Generator().manual_seed(43)).to(torch.int32)
    valid[2], valid[5], valid[6] = 0, T, 1
    return lv, la, labels, valid


def table_of(rows: slice):  # noqa: ANN201
    """The ``CoherenceTable`` of the batch rows ``rows`` of the case."""
    from multimodal_mtrssm_amd import CoherenceTable, GenerationCoherence  # noqa: PLC0415

    lv, la, labels, valid = case()
    table = CoherenceTable(G, T, observe=OBSERVE)
    pick = slice(rows.start * G * S, rows.stop * G * S)
    GenerationCoherence.fold(lv[pick].contiguous(), la[pick].contiguous(), labels[rows].contiguous(), G, S, CONTEXT, valid[rows].contiguous(),
                             table=table.buffer, planes=False)
    return table


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import GenerationCoherence  # noqa: PLC0415
    from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415
    from multimodal_mtrssm_amd.parallel import FlatDataParallel  # noqa: PLC0415

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = GenerationCoherence(CONTEXT, samples=S, observe=OBSERVE)
        gc = dp.coherence(free)
        assert gc is not free and gc.group is group and free.group is None and gc.observe == OBSERVE and gc.samples == S
        per = B // world
        table = table_of(slice(rank * per, (rank + 1) * per))
        own = table.buffer.clone()
        assert table.all_reduce(gc.group) is table
        torch.save({"own": own, "reduced": table.buffer.clone()}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
