"""CPU, world size 2 over gloo: two ranks hold half the rows each (``tests/coherence_worker.py``); their all-reduced ``CoherenceTable``
equals that of one rank with all rows -- the whole-number cells exactly, the ``soft`` sums within addition order (rtol 1e-12)."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from multimodal_mtrssm_amd import CoherenceTable
from tests.coherence_worker import B, G, OBSERVE, T, table_of, worker


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_coherence_table_matches_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    one = table_of(slice(0, B))
    assert torch.equal(r0["reduced"], r1["reduced"]) and not torch.equal(r0["own"], r1["own"])
    assert r0["reduced"].dtype == torch.float64 and tuple(r0["reduced"].shape) == tuple(one.buffer.shape)
    both = CoherenceTable(G, T, observe=OBSERVE)
    both.buffer.copy_(r0["reduced"])
    got, want = both.views(), one.views()
    assert torch.equal(got["counts"], want["counts"]) and torch.equal(got["pairs"], want["pairs"])
    assert torch.equal(got["sums"][:, :4], want["sums"][:, :4])  # vision, audio, agree, joint: whole numbers
    for rank in (r0, r1):  # both ranks have live rows in both phases
        own = CoherenceTable(G, T, observe=OBSERVE)
        own.buffer.copy_(rank["own"])
        assert bool((own.views()["pairs"].sum((2, 3)) > 0).all())
    assert bool((want["sums"][:, 4, :4] > 0).all())
    torch.testing.assert_close(got["sums"][:, 4], want["sums"][:, 4], rtol=1e-12, atol=0.0, msg="soft")
    scalars = both.scalars("val/coherence")
    for key, x in one.scalars("val/coherence").items():
        torch.testing.assert_close(scalars[key], x, rtol=1e-6, atol=0.0, equal_nan=True, msg=key)
