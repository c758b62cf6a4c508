"""CPU, world size 2 over gloo: two ranks fold their own rows of a batch through the particle filter's host rule
(``tests/particle_worker.py``), ``FlatDataParallel.particle`` binds the process group, and ONE ``ParticleTable.all_reduce`` over that
group gives the single-process table of all rows -- counts exactly, sums within fp32 addition order."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from tests.particle_worker import B, T, case, table_of, worker


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_particle_table_matches_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    one = table_of(slice(0, B))  # (a row's fold depends on that row only: the shards' planes are the whole batch's)
    _, valid, _ = case()
    assert torch.equal(r0["reduced"][7], one.counts) and float(one.counts.sum()) == float(valid.clamp(0, T).sum())  # counts: exact
    assert torch.equal(r0["own"][7] + r1["own"][7], one.counts) and int((one.counts > 2).sum()) >= 3  # noqa: PLR2004  (bins split over the ranks)
    # the addends of a row share their sign (log-likelihoods < 0; ESS, flags >= 0): any summation order stays within (n - 1) 2^-24 relative
    for t in range(T):
        n = float(one.counts[t])
        torch.testing.assert_close(r0["reduced"][:7, t], one.sums[:, t], rtol=2.0 * n * 2.0 ** -24, atol=0.0)
    assert torch.equal(r0["reduced"][6], one.sums[6]) and float(one.sums[6].sum()) > 0  # the resampling counts: whole numbers, exact
    per = one.per_frame()
    assert float(per["smc"]) >= float(per["mean"]) and float(per["mean"]) < -100.0 and 0.0 < float(per["resampled"]) < 0.5  # noqa: PLR2004
