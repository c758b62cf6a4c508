"""CPU worker for tests/test_latent_probe_gloo.py: each gloo rank holds half the rows of a fixed probe problem, folds its own
``ProbeTable`` and runs ``LinearProbe.fit`` over the group ``FlatDataParallel.probe`` bound.  ``probe_case`` is shared with the
single-process side of the test."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

G, B, T, F, C = 3, 12, 9, 20, 10
FIT_STEPS, FIT_LR = 5, 1e-2


def probe_case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Features ``[G, B, T, F]``, labels ``[B, T]`` (a silent row, about a fifth -1) and seeded classifier weights."""
    g = torch.Generator().manual_seed(41)
    x = torch.tanh(torch.randn(G, B, T, F, generator=g))
    labels = torch.randint(0, C, (B, T), generator=g).to(torch.int32)
    labels[torch.rand(B, T, generator=g) < 0.2] = -1  # noqa: PLR2004
    labels[2] = -1
    return x, labels, torch.randn(G, C, F, generator=g) / F ** 0.5, 0.5 * torch.randn(G, C, generator=g)


def evaluate(rows: slice):  # noqa: ANN201
    """The ``ProbeTable`` of ``rows`` under the seeded weights (the non-GPU route of ``LinearProbe.step``)."""
    from multimodal_mtrssm_amd import LinearProbe, ProbeTable

    x, labels, weight, bias = probe_case()
    x, labels = x[:, rows].contiguous(), labels[rows].contiguous()
    b = x.shape[1]
    linear = LinearProbe(G, F, C)
    with torch.no_grad():
        linear.weight.copy_(weight)
        linear.bias.copy_(bias)
    stats = linear.step(x.reshape(G, b * T, F), labels.reshape(-1), grad=False, planes=True)
    return ProbeTable(G, T).fold(stats.hit.reshape(G, b, T), stats.nll.reshape(G, b, T), labels >= 0)


def fit(rows: slice, group=None):  # noqa: ANN001, ANN201
    """``FIT_STEPS`` iterations from zero weights on ``rows`` (sharded over ``group``)."""
    from multimodal_mtrssm_amd import LinearProbe

    x, labels, _, _ = probe_case()
    x, labels = x[:, rows].contiguous(), labels[rows].contiguous()
    linear = LinearProbe(G, F, C)
    stats = linear.fit(x.reshape(G, -1, F), labels.reshape(-1), FIT_STEPS, lr=FIT_LR, group=group)
    return linear, stats


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    from multimodal_mtrssm_amd import LatentProbe
    from multimodal_mtrssm_amd.optim import FlatParameters
    from multimodal_mtrssm_amd.parallel import FlatDataParallel

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = LatentProbe()
        probe = dp.probe(free)
        assert probe is not free and probe.group is group and free.group is None
        per = B // world
        rows = slice(rank * per, (rank + 1) * per)
        table = evaluate(rows)
        own = table.buffer.clone()
        assert table.all_reduce(probe.group) is table
        linear, stats = fit(rows, probe.group)
        torch.save({"own": own, "reduced": table.buffer.clone(), "weight": linear.weight.detach().clone(), "bias": linear.bias.detach().clone(),
                    "stats": torch.stack([stats.nll_sum, stats.hits, stats.count])}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
