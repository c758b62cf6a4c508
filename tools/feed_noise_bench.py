"""Seeded input noise inside the gather against the parent's two launches, at the bench frame shapes, one JSON line (DESIGN.md
section 6e).

    timeout -k 10 300 python tools/feed_noise_bench.py [--blocks 7] [--iters 50] [--warmup 10] [--episodes 128]

One process, one GPU.  Per stream (B = 64, T = 50, bench.py's audio and vision frames, T_full = 180 stored steps, random windows):
alternating timed blocks of
  randn   torch.randn([B, T, *event]) + mtrssm_episode_gather_window reading it   (4 passes over B x T x E floats: the normals
          written and read back, the store read, input and target written -- target counted once)
  seeded  mtrssm_episode_gather_seeded                                            (3 passes: no normals in memory)
each block `iters` calls between two device events.  Prints per stream and path the median microseconds per call over the blocks, the
minimum and maximum (the run-to-run spread within this process), the bytes moved and the rate they imply.  The command above puts
the one GPU step under its own time limit.
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
PATHS = ("randn", "seeded")


def time_block(fn, iters: int) -> float:  # noqa: ANN001
    """Microseconds per call of `iters` calls of `fn` between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def run_stream(event: tuple, blocks: int, iters: int, warmup: int, episodes: int, device: str) -> dict[str, dict[str, float]]:
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import transform as tr

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    g = torch.Generator(device=device).manual_seed(5)
    chain = lambda std: tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std else []))  # noqa: E731
    stream = ds._Stream(torch.randn(episodes, T_FULL, *event, generator=g, device=device), chain(0.1), chain(None))  # noqa: SLF001
    idx = torch.randperm(episodes, generator=g, device=device)[:b].contiguous()
    start = torch.randint(0, T_FULL - t + 1, (b,), generator=g, device=device).to(torch.int32)
    key = ds.stream_key(7, 1)
    calls = {"randn": lambda: stream.batch(idx, None, start), "seeded": lambda: stream.batch(idx, None, start, seeded=(*key, 0))}
    floats = b * t * stream.event
    moved = {"randn": 4 * 4 * floats, "seeded": 3 * 4 * floats}
    for fn in calls.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {p: [] for p in PATHS}
    for _ in range(blocks):
        for p in PATHS:  # alternating: both paths see the same machine
            times[p].append(time_block(calls[p], iters))
    out = {}
    for p in PATHS:
        s = sorted(times[p])
        med = s[len(s) // 2]
        out[p] = {"median_us": med, "min_us": s[0], "max_us": s[-1], "bytes": float(moved[p]), "gb_per_s": moved[p] / med * 1e-3}
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
    assert torch.cuda.is_available(), "feed_noise_bench.py needs the MI355X"
    res: dict[str, object] = {"metric": "input noise of the episode feed: torch.randn + window gather vs seeded gather (us per call)",
                              "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"], "t_full": T_FULL, "episodes": args.episodes,
                              "blocks": args.blocks, "iters_per_block": args.iters, "warmup": args.warmup}
    for name in ("audio", "vision"):
        event = tuple(w[name])
        res[name] = {"event": list(event), **run_stream(event, args.blocks, args.iters, args.warmup, args.episodes, "cuda:0")}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
