"""CPU, world size 2 over gloo: two ranks hold half the feature rows each (``tests/frechet_worker.py``); their all-reduced
``FrechetTable`` equals that of one rank with all rows -- the counts exactly, the moments within the bound of
``tests/test_frechet_host.py`` (both sides add each bin's rows in double, in a different order)."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from tests.frechet_worker import D, NAMES, ROWS, STREAMS, case, table_of, worker
from tests.test_frechet_host import moment_bound


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_frechet_table_matches_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    one = table_of(slice(0, ROWS))
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    assert r0["reduced"].dtype == torch.float64 and tuple(r0["reduced"].shape) == tuple(one.buffer.shape) == (len(STREAMS), 2, len(NAMES), 1 + D + D * D)
    for (s, side), (x, bins) in case().items():
        got, want = r0["reduced"][s, side], one.buffer[s, side]
        assert torch.equal(got[:, 0], want[:, 0]) and float(want[:, 0].min()) >= 2, (s, side)  # noqa: PLR2004
        err, bound = (got - want).abs(), moment_bound(x, bins, len(NAMES))
        assert bool((err <= bound).all()), (s, side, float((err - bound).max()))
