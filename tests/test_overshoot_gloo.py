"""CPU, world size 2 over gloo: two ranks hold half the rows each (``tests/overshoot_worker.py``); the mean of their overshoot losses and
their all-reduced ``OvershootTable`` equal those of one rank with all rows -- the counts exactly, the sums within addition order."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from multimodal_mtrssm_amd import LatentOvershoot
from tests.overshoot_worker import B, DEPTH, OFFSET, STRIDE, terms_of, worker


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_overshoot_loss_and_table_match_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    one = terms_of(LatentOvershoot(DEPTH, stride=STRIDE, offset=OFFSET), slice(0, B))
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    assert float(r0["count"]) == float(r1["count"]) == float(one.count) > 0  # every rank divides by the GLOBAL count
    assert float(r0["term"]) != float(r1["term"])
    # the mean over the ranks is the one-rank loss: each rank's term is fp32 (2^-24 relative), the mean is taken in double
    torch.testing.assert_close(r0["mean"], one.term.to(torch.float64), rtol=4.0 * 2.0 ** -24, atol=0.0)
    assert torch.equal(r0["mean"], r1["mean"])
    # the table is a double: the counts exactly, the sums of positive addends within a few ulps of any order
    assert torch.equal(r0["reduced"][0, 1], one.table[1]) and torch.equal(r0["own"][0, 1] + r1["own"][0, 1], one.table[1])
    assert int((one.table[1] > 2).sum()) == DEPTH  # noqa: PLR2004  (every distance has terms on both ranks)
    assert bool((r0["own"][0, 1] > 0).all()) and bool((r1["own"][0, 1] > 0).all())
    torch.testing.assert_close(r0["reduced"][0, 0], one.table[0], rtol=1e-12, atol=0.0)
