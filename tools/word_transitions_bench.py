"""Time of the digit reader on the frames of one validation pass: S = 16 futures of a B = 64, T = 50 batch,
51 200 vision frames of 32 x 32, one JSON line.

    python tools/word_transitions_bench.py [--frames 51200] [--steps 5] [--warmup 2] [--chunk 6400]

On random raw frames (Tanh applied by the reader) and seeded weights, `warmup` untimed runs, then `steps` runs between HIP events
(the median is reported, with the minimum and maximum):

  fused_trunk    ONE mtrssm_digit_features launch: activation, denormalisation, conv1, ReLU, pool, conv2, ReLU, pool -> features
  reader         the whole read: the trunk, fc1 on mtrssm_gemm (bias + ReLU epilogue), mtrssm_digit_head
  general_trunk  the yardstick at the same commit: the same trunk as separate launches -- torch's tanh / denormalise / clamp,
                 conv.conv2d (the project's general gather-GEMM path) for conv1, torch ReLU + max_pool2d, conv.conv2d for conv2,
                 torch ReLU + max_pool2d -- over chunks of `chunk` frames (its conv1 output alone is 128 KB per frame)

`general_trunk` is reported as an error string when the general path has no instance for a layer's shape.  The two trunks' features
are compared once (`trunk_max_diff`, relative to the largest feature).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F  # noqa: N812

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def timed(fn, steps: int, warmup: int) -> dict[str, float]:  # noqa: ANN001
    for _ in range(warmup):
        fn()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    for i in range(steps):
        marks[i].record()
        fn()
    marks[steps].record()
    torch.cuda.synchronize()
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return {"median_ms": per[len(per) // 2], "min_ms": per[0], "max_ms": per[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=51200)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=6400)
    args = ap.parse_args()
    if min(args.frames, args.steps, args.chunk) < 1 or args.warmup < 0:
        ap.error("frames, steps, chunk >= 1 and warmup >= 0")
    assert torch.cuda.is_available(), "word_transitions_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import DigitClassifier, conv

    dev = "cuda:0"
    torch.manual_seed(0)
    clf = DigitClassifier().to(dev)
    n = args.frames
    raw = torch.randn(n, 1024, device=dev) * 1.5
    feat = torch.empty(n, 4096, device=dev)
    res: dict[str, object] = {"metric": "ms per pass of the digit reader", "frames": n, "timed_steps": args.steps, "warmup": args.warmup}
    res["fused_trunk"] = timed(lambda: clf.features(raw, 3, out=feat), args.steps, args.warmup)
    res["reader"] = timed(lambda: clf.read(raw, 3, want_logits=False), args.steps, args.warmup)

    def general(out: torch.Tensor | None = None) -> None:
        for c0 in range(0, n, args.chunk):
            x = ((torch.tanh(raw[c0 : c0 + args.chunk]) + 1.0) / 2.0).clamp(0.0, 1.0).reshape(-1, 1, 32, 32)
            x = conv.conv2d(x, clf.conv1.weight, clf.conv1.bias, stride=1, padding=1, pre_act=False, act=0)
            x = F.max_pool2d(F.relu(x), 2, 2)
            x = conv.conv2d(x, clf.conv2.weight, clf.conv2.bias, stride=1, padding=1, pre_act=False, act=0)
            x = F.max_pool2d(F.relu(x), 2, 2)
            if out is not None:
                out[c0 : c0 + args.chunk] = x.reshape(-1, 4096)

    try:
        with torch.no_grad():
            other = torch.empty_like(feat)
            conv.begin_step(torch.device(dev))
            general(other)
            clf.features(raw, 3, out=feat)
            res["trunk_max_diff"] = float((other - feat).abs().max() / feat.abs().max())
            del other
            res["general_trunk"] = timed(general, args.steps, args.warmup)
            res["general_chunk"] = args.chunk
    except Exception as e:  # noqa: BLE001  (reported, not hidden: the yardstick is then "not measured")
        res["general_trunk"] = f"not measured: {type(e).__name__}: {e}"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
