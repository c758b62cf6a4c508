"""CPU, world size 2 over gloo: two ranks hold half the rows each (``tests/census_worker.py``); their all-reduced ``CensusTable`` equals
that of one rank with all rows -- the counts and ``n`` exactly, the double sums within addition order (rtol 1e-12)."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from multimodal_mtrssm_amd import CensusTable
from multimodal_mtrssm_amd.census import PLANES
from tests.census_worker import B, G, LEVELS, OBSERVE, T, table_of, worker


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_census_table_matches_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    one = table_of(slice(0, B))
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    assert r0["reduced"].dtype == torch.float64 and tuple(r0["reduced"].shape) == tuple(one.buffer.shape)
    both = CensusTable(LEVELS, G, T, observe=OBSERVE)
    both.buffer.copy_(r0["reduced"])
    for level in range(len(LEVELS)):
        got, want = both.views(level), one.views(level)
        for name in ("n", "frames", "pairs", "counts"):
            assert torch.equal(got[name], want[name]), (level, name)
        assert float(want["frames"][0]) > 0 and bool((want["counts"][:, 0] >= 2).all())  # noqa: PLR2004  (both ranks have live rows)
        for name in ("qsum", "psum", "positions", *PLANES):
            torch.testing.assert_close(got[name], want[name], rtol=1e-12, atol=0.0, msg=f"level {level} {name}")
    for key, x in one.scalars("val/latent").items():
        torch.testing.assert_close(both.scalars("val/latent")[key], x, rtol=1e-6, atol=0.0, msg=key)
