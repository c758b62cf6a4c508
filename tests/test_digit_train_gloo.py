"""CPU, world size 2 over gloo: ``DigitTrainer.step`` and ``DigitTrainer.fit`` with ``group`` over rows split in two
leave the parameters of one process over all rows, and return the global stats.

Bound.  Each rank rounds its float64 partial gradient to fp32 and the all-reduce adds the two in fp32: a relative error of at most
``3 x 2^-24`` of the partial sums, that is ``r <= 3 x 2^-24 x c`` of the gradient entry when the partial sums cancel by a factor ``c``.  Adam's
update ``lr m / (sqrt(v) + eps)`` is homogeneous of degree 0 in the gradient history, so to first order an entry moves by at most
``2 lr r`` per update.  The test allows ``c`` up to ``2^10``: ``|sharded - single| <= updates x 2 lr x 3 x 2^-14``."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from tests.digit_train_worker import LR, ROWS, STEPS, UPDATES, train, worker
from tests.test_digits_host import seeded_classifier


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_step_and_fit_match_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    for key in r0:
        assert torch.equal(r0[key], r1[key]), key  # both ranks hold the same parameters and the same (global) stats
    one = train(slice(0, ROWS))
    bound = UPDATES * 2.0 * LR * 3.0 * 2.0 ** -14
    for key, want in one.items():
        if key.startswith("step") or key == "fit":
            assert r0[key][2] == want[2] and float(want[2]) > ROWS // 2, key  # the live count of ALL rows: exact
            torch.testing.assert_close(r0[key][0], want[0], rtol=1e-5, atol=0.0)
            assert r0[key][1] == want[1], key  # hits are whole numbers
            continue
        err = float((r0[key] - want).abs().max())
        print(f"{key}: worst |sharded - single| {err:.3e}, bound {bound:.3e}")
        assert err <= bound, key
    assert float(one["step0"][2]) == float(one[f"step{STEPS - 1}"][2])
    start = seeded_classifier(5).state_dict()
    assert float((one["fc1.weight"] - start["fc1.weight"]).abs().max()) > 0.5 * UPDATES * LR  # (the fit moved)
