"""The windowed episode feed and the carried train step at the bench shape, one JSON line.

    python tools/window_feed_bench.py [--steps 20] [--warmup 5] [--rounds 2] [--episodes 128] [--skip-step]

feed   the 6-tuple feed (B = 64, T = 50, bench.py's frame sizes, T_full = 180 stored steps) in the modes first / random /
       sequential, all three in ONE process on the same stores, alternating `rounds` times: seq-steps/s per mode and round.
       `first` launches episode_gather_kernel<first>, the other two episode_gather_kernel<window>, on the same shape, so a
       `rocprofv3 --kernel-trace --stats -- python tools/window_feed_bench.py --skip-step` run compares the two per launch.
step   one unmasked MoPoE-MRSSM train step, eager and captured, without and with a StateCarry (reset on every third step, as
       a three-chunk episode): ms per step, bench.py's warm-up / step discipline.
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the workload, model and batch of the flagship benchmark)

T_FULL = 180
FEED_MODES = ("first", "random", "sequential")
STEP_MODES = ("eager", "eager_carry", "graph", "graph_carry")


def feed_streams(episodes: int, device: str) -> tuple:
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import transform as tr

    w = bench.WORKLOAD
    t = w["steps"]
    g = torch.Generator(device=device).manual_seed(5)
    chain = lambda std: tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std else []))  # noqa: E731
    shapes = ((w["action"],), tuple(w["audio"]), tuple(w["vision"]))
    return tuple(ds._Stream(torch.randn(episodes, T_FULL, *s, generator=g, device=device), chain(0.1), chain(None)) for s in shapes)  # noqa: SLF001


def time_feed(loader, batches: int, warmup: int) -> float:  # noqa: ANN001
    """seq-steps/s of `batches` full batches (epochs are strung together; a short last batch is skipped)."""
    def stream():  # noqa: ANN202
        while True:
            for b in loader:
                if b[0].shape[0] == loader.batch_size:
                    yield b

    it = stream()
    for _ in range(warmup):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        next(it)
    torch.cuda.synchronize()
    return batches * loader.batch_size * loader.steps / (time.perf_counter() - t0)


def run_feed(steps: int, warmup: int, rounds: int, episodes: int, device: str) -> dict[str, list[float]]:
    from multimodal_mtrssm_amd import dataset as ds

    streams = feed_streams(episodes, device)
    b = bench.WORKLOAD["batch_per_gpu"]
    loaders = {m: ds.DeviceEpisodeLoader(streams, b, shuffle=True, seed=1, window=m) for m in FEED_MODES}
    out: dict[str, list[float]] = {m: [] for m in FEED_MODES}
    for _ in range(rounds):
        for m in FEED_MODES:
            out[m].append(time_feed(loaders[m], steps, warmup))
    return out


def run_step(mode: str, steps: int, warmup: int, device: str) -> dict[str, float]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd.dataset import EpisodeBatch
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, "mrssm")
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = bench.synthetic_batch(b, device, seed=1000)
    source = dp.noise_source(seed=7)
    shapes = model.noise_shapes(b, t)
    sc = mt.StateCarry.for_model(model, b) if mode.endswith("carry") else None
    zeros = torch.zeros(b, dtype=torch.int32)
    chunks = []
    for c in range(3):  # the batches of a three-chunk episode: reset on chunk 0 (made once; the feed is timed separately)
        reset = torch.full((b,), c == 0, dtype=torch.bool)
        chunks.append(EpisodeBatch(batch, zeros.to(device), reset.to(device), zeros, reset))
    count = [0]

    def next_batch():  # noqa: ANN202
        count[0] += 1
        return chunks[(count[0] - 1) % 3] if sc is not None else batch

    def eager_step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        out = model.shared_step(next_batch(), noise, state_carry=sc) if sc is not None else model.shared_step(next_batch(), noise)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

    step = eager_step
    captured = None
    if mode.startswith("graph"):
        from multimodal_mtrssm_amd.graph import CapturedTrainStep

        kw = {"state_carry": sc} if sc is not None else {}
        captured = CapturedTrainStep(model, flat, opt, dp, batch, source, **kw)
        step = lambda: captured.step(next_batch())  # noqa: E731
    for _ in range(3 * ((warmup + 2) // 3)):  # whole episodes: the timed steps start on a reset
        step()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        step()
    marks[steps].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    scan.check_cluster_status()
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    if captured is not None:
        captured.close()
    return {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0], "max_ms": per_step[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--episodes", type=int, default=128)
    ap.add_argument("--skip-step", action="store_true", help="time the feed only")
    ap.add_argument("--skip-feed", action="store_true", help="time the train step only")
    args = ap.parse_args()
    if args.steps < 1 or args.rounds < 1 or args.episodes < bench.WORKLOAD["batch_per_gpu"]:
        ap.error("need steps, rounds >= 1 and at least one batch of episodes")
    assert torch.cuda.is_available(), "window_feed_bench.py needs the MI355X"
    w = bench.WORKLOAD
    res: dict[str, object] = {"metric": "windowed feed (seq-steps/s) and carried train step (ms)", "batch": w["batch_per_gpu"],
                              "steps_per_sequence": w["steps"], "t_full": T_FULL, "episodes": args.episodes, "timed_steps": args.steps,
                              "warmup": args.warmup}
    if not args.skip_feed:
        res["feed_seq_steps_per_s"] = run_feed(args.steps, args.warmup, args.rounds, args.episodes, "cuda:0")
    if not args.skip_step:
        res["step"] = {m: [run_step(m, args.steps, args.warmup, "cuda:0") for _ in range(args.rounds)] for m in STEP_MODES}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
