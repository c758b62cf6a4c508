"""Time of the episode panel kernel at the bench's frame sizes: N = 8 episodes of T = 50 frames, 64 x 64 vision
over 128 x 32 audio, `prior | observation | posterior` at scale 2 (a 387 x 386 canvas per frame, 179 MB of video), one JSON line.

    python tools/episode_panel_bench.py [--episodes 8] [--frames 50] [--scale 2] [--steps 10] [--warmup 3]

On seeded random frames in [-1.05, 1.05], `warmup` untimed runs, then `steps` runs between HIP events (the median is reported, with the
minimum and maximum):

  kernel      ONE mtrssm_episode_panel launch into a given buffer
  torch_rule  the yardstick at the same commit: EpisodePanel.reference -- the same rule as torch ops on the same GPU (denormalise,
              clamp, table lookup, repeat_interleave, slice assignments, one small copy per frame number)

`hbm_fraction` is the kernel's bytes (the video written plus the six inputs read once) per second of its median, as a fraction of
8 TB/s.  The two results are compared once (`differing_bytes`).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8.0e12


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
    ap.add_argument("--episodes", type=int, default=8)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if min(args.episodes, args.frames, args.scale, args.steps) < 1 or args.warmup < 0:
        ap.error("episodes, frames, scale, steps >= 1 and warmup >= 0")
    assert torch.cuda.is_available(), "episode_panel_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import EpisodePanel

    dev = "cuda:0"
    n, t = args.episodes, args.frames
    audio, vision = (1, 128, 32), (1, 64, 64)
    g = torch.Generator().manual_seed(0)
    frames = [(torch.rand(n, t, *chw, generator=g) * 2.1 - 1.05).to(dev) for chw in (audio,) * 3 + (vision,) * 3]
    panel = EpisodePanel(max(1, t // 3), scale=args.scale)
    hc, wc = panel.shape(audio, vision)
    out = torch.empty(n, t, hc, wc, 3, dtype=torch.uint8, device=dev)
    moved = out.numel() + 4 * sum(f.numel() for f in frames)
    res: dict[str, object] = {"metric": "ms per episode panel video", "episodes": n, "frames": t, "scale": args.scale, "canvas": [hc, wc],
                              "video_bytes": out.numel(), "bytes_moved": moved, "timed_steps": args.steps, "warmup": args.warmup}
    res["kernel"] = timed(lambda: panel.render(*frames, frame0=0, out=out), args.steps, args.warmup)
    res["hbm_fraction"] = moved / (res["kernel"]["median_ms"] * 1e-3) / HBM_BYTES_PER_S
    with torch.no_grad():
        res["differing_bytes"] = int((panel.reference(*frames) != out).sum())
        res["torch_rule"] = timed(lambda: panel.reference(*frames), args.steps, args.warmup)
    res["speedup"] = res["torch_rule"]["median_ms"] / res["kernel"]["median_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
