"""CPU, world size 2 over gloo: the ``Trainer`` on two ranks (``tests/fit_worker.py``: a stub step around the real one-all-reduce
exchange).  Both ranks compute identical epoch metrics -- the train scalars come out of the all-reduced tail, the validation sums are
all-reduced once per epoch -- so both take the same plateau and early-stopping decisions and stop at the same epoch; only rank 0
writes files; and the metrics are those of one process over the whole batches."""

from __future__ import annotations

import json
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from tests import fit_worker  # noqa: E402


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_compute_identical_metrics_and_stop_at_the_same_epoch(tmp_path: Path) -> None:
    two, one = tmp_path / "two", tmp_path / "one"
    two.mkdir()
    one.mkdir()
    mp.spawn(fit_worker.run, args=(2, _free_port(), str(two)), nprocs=2, join=True)
    r0 = torch.load(two / "rank0of2.pt", weights_only=True)
    r1 = torch.load(two / "rank1of2.pt", weights_only=True)
    assert r0["lines"] == r1["lines"] and torch.equal(r0["param"], r1["param"])  # identical metrics, bit for bit, and weights
    assert r0["stopped"] == r1["stopped"] == 4 and [ln["epoch"] for ln in r0["lines"]] == [0, 1, 2, 3, 4]
    assert r0["best"] == r1["best"] and r0["best"]["epoch"] == 1
    assert [ln["lr"] for ln in r0["lines"]] == [0.1, 0.1, 0.1, 0.1, 0.05]
    # only rank 0 writes: one line per epoch (not two), one set of checkpoints
    assert r0["saved"] is True and r1["saved"] is False
    on_disk = [json.loads(x) for x in (two / "run" / "metrics.jsonl").read_text().splitlines()]
    assert [{k: v for k, v in ln.items() if not k.endswith("_time")} for ln in on_disk] == r0["lines"]
    assert sorted(p.name for p in (two / "run").iterdir()) == ["best.ckpt", "extra.ckpt", "last.ckpt", "metrics.jsonl"]
    assert torch.load(two / "run" / "last.ckpt", weights_only=True)["world"] == 2
    # one process over the whole batches: the same metrics up to the order of fp32 additions in the exchange
    fit_worker.run(0, 1, 0, str(one))
    single = torch.load(one / "rank0of1.pt", weights_only=True)
    assert [ln["epoch"] for ln in single["lines"]] == [0, 1, 2, 3, 4] and single["stopped"] == 4
    x, _ = fit_worker.data()
    for a, b in zip(r0["lines"], single["lines"], strict=True):
        assert set(a) == set(b)
        for key in a:
            assert a[key] == pytest.approx(b[key], rel=1e-5, abs=1e-7), key
        assert a["val/mean_x"] == pytest.approx(float(x.mean()), rel=1e-5, abs=1e-7)  # rows of BOTH ranks
        assert a["train/twice"] == pytest.approx(2.0 * a["train/loss"], rel=1e-6)
