"""CPU worker for tests/test_digit_train_gloo.py: each gloo rank holds half the rows of the memorisation set and runs
``DigitTrainer.step`` and ``DigitTrainer.fit`` over the group.  ``train`` is shared with the single-process side of the test."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

ROWS, STEPS, EPOCHS, BATCH, LR, SEED = 40, 2, 2, 16, 1e-3, 17
UPDATES = STEPS + EPOCHS * -(-ROWS // BATCH)


def train(rows: slice, group=None) -> dict[str, torch.Tensor]:  # noqa: ANN001
    """``STEPS`` steps on all of ``rows``, then ``EPOCHS`` epochs in minibatches of ``BATCH``, with dropout 0.5 (sharded over ``group``)."""
    from multimodal_mtrssm_amd import DigitClassifier, DigitTrainer
    from tests.test_digit_train_host import memorise_set
    from tests.test_digits_host import seeded_classifier

    raw, labels = memorise_set()
    labels = labels.clone()
    labels[5::9] = -1
    raw, labels = raw[rows].contiguous(), labels[rows].contiguous()
    clf = DigitClassifier()
    clf.load_state_dict(seeded_classifier(5).state_dict())
    out = {}
    with DigitTrainer(clf, lr=LR, dropout=0.5, seed=SEED) as trainer:
        for i in range(STEPS):
            stats = trainer.step(raw, labels, act=3, group=group, row0=rows.start)
            out[f"step{i}"] = torch.stack(list(stats))
        out["fit"] = torch.stack(list(trainer.fit(raw, labels, epochs=EPOCHS, batch_size=BATCH, act=3, group=group)))
        assert trainer.steps == UPDATES
    out.update({k: v.clone() for k, v in clf.state_dict().items()})
    return out


def worker(rank: int, world: int, port: int, out_dir: str) -> None:
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.new_group(list(range(world)))
        per = ROWS // world
        torch.save(train(slice(rank * per, (rank + 1) * per), group), f"{out_dir}/rank{rank}.pt")
    finally:
        dist.destroy_process_group()
