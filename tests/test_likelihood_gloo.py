"""CPU, world size 2 over gloo: two ranks fill ``LikelihoodTable``s from the planes of their shard of a batch (the non-GPU route of
``LikelihoodBound.bound``), ``FlatDataParallel.likelihood`` binds the process group, and ``LikelihoodTable.all_reduce`` over that group
gives the single-process table of the whole batch -- counts exactly, sums within fp32 addition order."""

from __future__ import annotations

import os
import socket
import sys
from pathlib import Path

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
B, T, S = 12, 9, 4
EVENTS = (96, 40)


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _case() -> tuple[tuple[torch.Tensor, torch.Tensor, torch.Tensor], torch.Tensor]:
    """fp32 errors and log-ratios ``[B, S, T]`` and the rows' lengths (a dead row, a whole row, the rest random)."""
    g = torch.Generator().manual_seed(23)
    se_a = torch.rand(B, S, T, generator=g) * 3.0 + 40.0
    se_v = torch.rand(B, S, T, generator=g) * 3.0 + 10.0
    ratio = -torch.rand(B, S, T, generator=g)
    valid = torch.randint(0, T + 2, (B,), generator=g).to(torch.int32)
    valid[2], valid[7] = 0, T
    return (se_a, se_v, ratio), valid


def _table(rows: slice):  # noqa: ANN202
    from multimodal_mtrssm_amd import LikelihoodBound, LikelihoodTable

    inputs, valid = _case()
    planes = LikelihoodBound.bound(*(x[rows].contiguous() for x in inputs), valid[rows].contiguous(), *EVENTS)
    return LikelihoodTable(T).fold(planes, valid[rows].contiguous())


def _worker(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    from multimodal_mtrssm_amd import LikelihoodBound
    from multimodal_mtrssm_amd.optim import FlatParameters
    from multimodal_mtrssm_amd.parallel import FlatDataParallel

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        dp = FlatDataParallel(FlatParameters(torch.nn.Linear(2, 2)), group)
        free = LikelihoodBound(samples=S)
        bound = dp.likelihood(free)
        assert bound is not free and bound.group is group and free.group is None and bound.samples == S
        per = B // world
        table = _table(slice(rank * per, (rank + 1) * per))
        own = table.buffer.clone()
        assert table.all_reduce(bound.group) is table
        torch.save({"own": own, "reduced": table.buffer.clone()}, f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()


def test_two_rank_likelihood_table_matches_single_process(tmp_path: Path) -> None:
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    one = _table(slice(0, B))
    _, valid = _case()
    assert torch.equal(r0["reduced"][6], one.counts) and float(one.counts.sum()) == float(valid.clamp(0, T).sum())  # counts: exact
    assert torch.equal(r0["own"][6] + r1["own"][6], one.counts) and int((one.counts > 2).sum()) >= 3  # noqa: PLR2004  (bins split over the ranks)
    # the addends of a row share their sign (log-likelihoods < 0, ESS > 0): any summation order stays within (n - 1) 2^-24 relative
    for t in range(T):
        n = float(one.counts[t])
        torch.testing.assert_close(r0["reduced"][:6, t], one.sums[:, t], rtol=2.0 * n * 2.0 ** -24, atol=0.0)
    per = one.per_frame()
    assert float(per["iw"]) >= float(per["elbo"]) and float(per["elbo"]) < -100.0  # noqa: PLR2004
