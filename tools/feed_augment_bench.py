"""The augmented gather against the seeded gather it extends, at the bench frame shapes, one JSON line.

    timeout -k 10 300 python tools/feed_augment_bench.py [--blocks 7] [--iters 50] [--warmup 10] [--episodes 128]

One process, one GPU.  Per stream (B = 64, T = 50, bench.py's audio and vision frames, T_full = 180 stored steps, random windows, noise
std 0.1): alternating timed blocks of
  seeded      mtrssm_episode_gather_seeded                                      (3 passes over B x T x E floats: the store read, input and
              target written)
  augmented   mtrssm_episode_gather_augmented, shift (4, 5), 2 bands of up to 8 rows and 8 columns per frame   (the same 3 passes; the
              shifted read of a row is unaligned whenever dx % 4 != 0, and vacated pixels are not read)
  unshifted   the augmented entry with FeedAugment(): what the new kernel's work mapping alone costs, with the aligned reads of the seeded one
each block `iters` calls between two device events.  Prints per stream and path the median microseconds per call over the blocks, the
minimum and maximum (the run-to-run spread within this process), the bytes moved and the rate they imply, and the ratio of the augmented
median to the seeded one.  The command above puts the one GPU step under its own time limit.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the flagship benchmark's shapes)

T_FULL = 180
PATHS = ("seeded", "augmented", "unshifted")
SEED = 7


def time_block(fn, iters: int) -> float:  # noqa: ANN001
    """Microseconds per call of `iters` calls of `fn` between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def run_stream(event: tuple, blocks: int, iters: int, warmup: int, episodes: int, device: str) -> dict[str, object]:
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import transform as tr

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    g = torch.Generator(device=device).manual_seed(5)
    chain = lambda std: tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std else []))  # noqa: E731
    stream = ds._Stream(torch.randn(episodes, T_FULL, *event, generator=g, device=device), chain(0.1), chain(None))  # noqa: SLF001
    idx = torch.randperm(episodes, generator=g, device=device)[:b].contiguous()
    start = torch.randint(0, T_FULL - t + 1, (b,), generator=g, device=device).to(torch.int32)
    words = (*ds.stream_key(SEED, 1), *ds.augment_key(SEED, 1), 0)
    aug = ds.FeedAugment(shift=(4, 5), bands=2, max_rows=8, max_cols=8, per_frame=True)
    calls = {"seeded": lambda: stream.batch(idx, None, start, seeded=(*words[:2], 0)),
             "augmented": lambda: stream.batch(idx, None, start, augment=(aug, *words)),
             "unshifted": lambda: stream.batch(idx, None, start, augment=(ds.FeedAugment(), *words))}
    moved = 3 * 4 * b * t * stream.event
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {p: [] for p in PATHS}
    for _ in range(blocks):
        for p in PATHS:  # alternating: every path sees the same machine
            times[p].append(time_block(calls[p], iters))
    out: dict[str, object] = {}
    for p in PATHS:
        s = sorted(times[p])
        med = s[len(s) // 2]
        out[p] = {"median_us": med, "min_us": s[0], "max_us": s[-1], "bytes": float(moved), "gb_per_s": moved / med * 1e-3}
    out["augmented_over_seeded"] = out["augmented"]["median_us"] / out["seeded"]["median_us"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=128)
    args = ap.parse_args()
    w = bench.WORKLOAD
    if args.blocks < 1 or args.iters < 1 or args.episodes < w["batch_per_gpu"]:
        ap.error("need blocks, iters >= 1 and at least one batch of episodes")
    assert torch.cuda.is_available(), "feed_augment_bench.py needs the MI355X"
    res: dict[str, object] = {"metric": "episode feed: seeded gather vs augmented gather (shift + band masks + seeded noise), us per call",
                              "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"], "t_full": T_FULL, "episodes": args.episodes,
                              "blocks": args.blocks, "iters_per_block": args.iters, "warmup": args.warmup}
    for name in ("audio", "vision"):
        event = tuple(w[name])
        res[name] = {"event": list(event), **run_stream(event, args.blocks, args.iters, args.warmup, args.episodes, "cuda:0")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
