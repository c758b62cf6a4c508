#!/usr/bin/env python
"""Time one training step of the digit reader on the GPU, next to the literal torch network on the same GPU.

    python tools/digit_train_bench.py [--sizes 64 4096] [--warmup 2] [--repeats 5]

Per batch size: the whole ``DigitTrainer.step`` (dropout 0.5), the trunk backward alone and the training forward alone, each as the median
of ``--repeats`` runs between HIP events after ``--warmup`` runs (min - max alongside), one process; and the yardstick, the same network
written with torch's own layers: ``cross_entropy``, ``backward``, ``torch.optim.Adam``.  One JSON line per size."""

from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

ROOT = Path(__file__).resolve().parents[1]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from multimodal_mtrssm_amd import DigitClassifier, DigitTrainer  # noqa: E402
from multimodal_mtrssm_amd.digit_train import features_train, trunk_backward  # noqa: E402


class Literal(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3, padding=1)
        self.fc1 = nn.Linear(64 * 8 * 8, 128)
        self.fc2 = nn.Linear(128, 10)
        self.dropout = nn.Dropout(0.5)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = F.max_pool2d(F.relu(self.conv1(x)), 2, 2)
        x = F.max_pool2d(F.relu(self.conv2(x)), 2, 2)
        return self.fc2(self.dropout(F.relu(self.fc1(x.view(-1, 64 * 8 * 8)))))


def timed(fn, warmup: int, repeats: int) -> dict[str, float]:  # noqa: ANN001
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e3)
    return {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    dev = "cuda:0"
    for n in args.sizes:
        g = torch.Generator().manual_seed(n)
        raw = torch.randn(n, 1024, generator=g).to(dev)
        labels = torch.randint(0, 10, (n,), generator=g).to(torch.int32).to(dev)
        torch.manual_seed(0)
        literal = Literal().to(dev)
        clf = DigitClassifier()
        clf.load_state_dict(literal.state_dict())
        clf.to(dev)
        images = DigitClassifier.images(raw, 3)
        opt = torch.optim.Adam(literal.parameters(), lr=1e-3)

        def torch_step() -> None:
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(literal(images), labels.long()).backward()  # noqa: B023
            opt.step()  # noqa: B023

        row = {"frames": n, "torch": timed(torch_step, args.warmup, args.repeats)}
        with DigitTrainer(clf, dropout=0.5) as trainer:
            row["step"] = timed(lambda: trainer.step(raw, labels, act=3), args.warmup, args.repeats)  # noqa: B023
            feats, tape = features_train(clf, raw, 3)
            g_feat = torch.randn(n, 4096, generator=g).to(dev)
            row["features_train"] = timed(lambda: features_train(clf, raw, 3, out=feats, tape=tape), args.warmup, args.repeats)  # noqa: B023
            row["features"] = timed(lambda: clf.features(raw, 3, out=feats), args.warmup, args.repeats)  # noqa: B023
            row["trunk_bwd"] = timed(lambda: trunk_backward(clf, raw, tape, g_feat, labels, 3), args.warmup, args.repeats)  # noqa: B023
        row["trunk_bwd_share_of_step"] = row["trunk_bwd"]["median_us"] / row["step"]["median_us"]
        row["trunk_bwd_ns_per_frame"] = 1e3 * row["trunk_bwd"]["median_us"] / n
        row["features_ns_per_frame"] = 1e3 * row["features"]["median_us"] / n
        row["torch_over_step"] = row["torch"]["median_us"] / row["step"]["median_us"]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
