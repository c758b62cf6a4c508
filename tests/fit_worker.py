"""One rank of ``tests/test_fit_gloo.py``: a ``Trainer`` over a CPU module, a stub step that runs the real exchange
(``FlatDataParallel.sync``: gradients and scalars in one all-reduce) and plain SGD, loaders that hand each rank its rows."""

from __future__ import annotations

import os
import sys
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parents[1]
N, B = 16, 8  # episodes, global batch
VAL_LOSSES = (1.0, 0.8, 0.9, 0.85, 0.95, 0.7)  # (the last is never reached: patience 3 stops after epoch 4)


class Net(torch.nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.body = torch.nn.Linear(6, 4)
        self.head = torch.nn.Linear(4, 1)
        self.val_epochs = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.head(torch.tanh(self.body(x))).squeeze(-1)

    def validation_step(self, batch: tuple[torch.Tensor, ...], _k: int = 0) -> dict[str, torch.Tensor]:
        # the rows' own term differs from rank to rank: only the all-reduced sums make the ranks agree
        return {"val/loss": torch.tensor(VAL_LOSSES[self.val_epochs]) + 0.0 * batch[0].sum(), "val/mean_x": batch[0].mean()}

    def on_validation_epoch_end(self) -> dict[str, torch.Tensor]:
        self.val_epochs += 1
        return {}


def data() -> tuple[torch.Tensor, torch.Tensor]:
    g = torch.Generator().manual_seed(5)
    return torch.randn(N, 6, generator=g), torch.randn(N, generator=g)


def batches(rank: int, world: int) -> list[tuple[torch.Tensor, torch.Tensor]]:
    """The global batches' contiguous block of this rank (what ``FlatDataParallel.shard`` cuts)."""
    x, y = data()
    per = B // world
    return [(x[lo + rank * per: lo + (rank + 1) * per], y[lo + rank * per: lo + (rank + 1) * per]) for lo in range(0, N, B)]


def run(rank: int, world: int, port: int, out_dir: str) -> None:
    sys.path.insert(0, str(ROOT))
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.optim import FlatParameters

    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(100 + rank)  # ranks start different on purpose: the broadcast fixes it
        net = Net()
        flat = FlatParameters(net)
        dp = mt.FlatDataParallel(flat)
        dp.broadcast_parameters(0)
        opt = mt.FlatAdamW(flat, lr=0.1)

        def step(batch: tuple[torch.Tensor, ...]) -> dict[str, torch.Tensor]:
            flat.zero_grad()
            loss = (net(batch[0]) - batch[1]).square().mean()
            loss.backward()
            logs = dp.sync({"loss": loss, "twice": 2.0 * loss})
            with torch.no_grad():
                flat.param.sub_(flat.grad * dp.grad_scale * float(opt.param_groups[0]["lr"]))
            return logs

        trainer = mt.Trainer(net, flat, opt, dp, seed=7, max_epochs=6, scheduler=mt.ReduceLROnPlateau(opt, factor=0.5, patience=1),
                             early_stopping=mt.EarlyStopping("val/loss", patience=3), directory=Path(out_dir) / "run", train_step=step)
        lines = trainer.fit(batches(rank, world), batches(rank, world))
        torch.save({"lines": [{k: v for k, v in ln.items() if not k.endswith("_time")} for ln in lines], "param": flat.param.clone(),
                    "stopped": trainer.early_stopping.stopped_epoch, "best": trainer.best, "saved": trainer.save("extra.ckpt") is not None},
                   f"{out_dir}/rank{rank}of{world}.pt")
    finally:
        if world > 1:
            dist.destroy_process_group()
