"""Step time of the RAGGED train step at the bench shape (bench.py's MoPoE-MRSSM, B = 64, T = 50, lengths uniform on 10..50), one
JSON line.

    python tools/ragged_step_bench.py [--steps 20] [--warmup 5] [--modes unmasked_eager,unmasked_graph,ragged_eager,ragged_graph]
                                      [--skip-step] [--skip-feed] [--rounds 3] [--episodes 256]

Feed (as tools/window_feed_bench.py: a store of `episodes` episodes of T_FULL = 180 frames at the bench's frame sizes, window="random",
seq-steps/s, the two loaders alternating `rounds` times in one process): `window` = a loader without lengths
(mtrssm_episode_gather_window), `ragged` = the same store with lengths uniform on 10..180 (mtrssm_episode_gather_ragged).  Under
rocprofv3 --kernel-trace --stats this is the program that gives the two kernels' time per launch side by side.

Modes (each on a freshly built model, bench.py's warm-up / step discipline as tools/masked_step_bench.py: `warmup` untimed steps,
then `steps` steps between two synchronisations, wall clock over all of them and the median of per-step HIP-event intervals):

  unmasked_eager / unmasked_graph   bench.py --graph off / on, for scale
  ragged_eager                      shared_step on a batch that carries its lengths: the mask launch with its clear, the masked scans
                                    and NLLs, the counted ELBO epilogue, the save at each row's last live step
  ragged_graph                      CapturedTrainStep(..., ragged=True, state_carry=...): the same inside one hipGraph replay, a new
                                    set of lengths copied into the graph's buffer every step
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

MODES = ("unmasked_eager", "unmasked_graph", "ragged_eager", "ragged_graph")
FEED_MODES = ("window", "ragged")
LOW = 10  # lengths are uniform on LOW .. T
T_FULL = 180


def run_feed(steps: int, warmup: int, rounds: int, episodes: int, device: str) -> dict[str, list[float]]:
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import transform as tr

    w = bench.WORKLOAD
    t, b = w["steps"], w["batch_per_gpu"]
    g = torch.Generator(device=device).manual_seed(5)
    chain = lambda std: tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std else []))  # noqa: E731
    shapes = ((w["action"],), tuple(w["audio"]), tuple(w["vision"]))
    streams = tuple(ds._Stream(torch.randn(episodes, T_FULL, *s, generator=g, device=device), chain(0.1), chain(None)) for s in shapes)  # noqa: SLF001
    lengths = torch.randint(LOW, T_FULL + 1, (episodes,), generator=torch.Generator().manual_seed(6))
    loaders = {"window": ds.DeviceEpisodeLoader(streams, b, shuffle=True, seed=1, window="random"),
               "ragged": ds.DeviceEpisodeLoader(streams, b, shuffle=True, seed=1, window="random", lengths=lengths)}

    def time_feed(loader) -> float:  # noqa: ANN001
        def stream():  # noqa: ANN202
            while True:
                for batch in loader:
                    if batch[0].shape[0] == loader.batch_size:
                        yield batch

        it = stream()
        for _ in range(warmup):
            next(it)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            next(it)
        torch.cuda.synchronize()
        return steps * loader.batch_size * loader.steps / (time.perf_counter() - t0)

    out: dict[str, list[float]] = {m: [] for m in FEED_MODES}
    for _ in range(rounds):
        for m in FEED_MODES:
            out[m].append(time_feed(loaders[m]))
    return out


def ragged_batches(batch: tuple, count: int, device: str) -> list:
    """`count` EpisodeBatches over the bench batch's frames, each with its own lengths (frames past them zeroed, as the gather does)."""
    from multimodal_mtrssm_amd.dataset import EpisodeBatch

    b, t = batch[0].shape[:2]
    gen = torch.Generator().manual_seed(5)
    out = []
    for i in range(count):
        valid = torch.randint(LOW, t + 1, (b,), generator=gen).to(torch.int32)
        live = (torch.arange(t) < valid.unsqueeze(1)).to(device)
        items = tuple(x * live.reshape(b, t, *([1] * (x.dim() - 2))) for x in batch)
        reset = torch.full((b,), i == 0, dtype=torch.bool)
        out.append(EpisodeBatch(items, torch.zeros(b, dtype=torch.int32, device=device), reset.to(device), torch.zeros(b, dtype=torch.int32), reset,
                                valid=valid.to(device), valid_host=valid))
    return out


def run_mode(mode: str, steps: int, warmup: int, device: str) -> dict[str, float]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
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
    ragged = mode.startswith("ragged")
    batches = ragged_batches(batch, 4, device) if ragged else []
    carry = mt.StateCarry.for_model(model, b) if ragged else None
    calls = [0]

    def eager_step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        if ragged:
            out = model.shared_step(batches[calls[0] % len(batches)], noise, state_carry=carry)
            calls[0] += 1
        else:
            out = model.shared_step(batch, noise)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

    step = eager_step
    captured = None
    if mode.endswith("graph"):
        from multimodal_mtrssm_amd.graph import CapturedTrainStep

        if ragged:
            captured = CapturedTrainStep(model, flat, opt, dp, batches[0], source, ragged=True, state_carry=carry)

            def step() -> None:
                captured.step(batches[calls[0] % len(batches)])
                calls[0] += 1
        else:
            captured = CapturedTrainStep(model, flat, opt, dp, batch, source)
            step = captured.step
    for _ in range(warmup):
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
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-feed", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=256)
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    unknown = set(modes) - set(MODES)
    if unknown or args.steps < 1:
        ap.error(f"unknown modes {sorted(unknown)} (of {MODES}) or steps < 1")
    assert torch.cuda.is_available(), "ragged_step_bench.py needs the MI355X"
    feed = None if args.skip_feed else run_feed(args.steps, args.warmup, args.rounds, args.episodes, "cuda:0")
    results = {} if args.skip_step else {m: run_mode(m, args.steps, args.warmup, "cuda:0") for m in modes}
    w = bench.WORKLOAD
    print(json.dumps({"metric": "ms per MoPoE-MRSSM train step, ragged; feed in seq-steps/s", "batch": w["batch_per_gpu"],
                      "steps_per_sequence": w["steps"], "lengths": [LOW, w["steps"]], "timed_steps": args.steps, "warmup": args.warmup,
                      "modes": results, "feed": feed}))


if __name__ == "__main__":
    main()
