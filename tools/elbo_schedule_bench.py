"""Step time of the train step under an ELBO SCHEDULE at the bench shape (bench.py's models, B = 64, T = 50), one
JSON line.

    python tools/elbo_schedule_bench.py [--steps 20] [--warmup 5] [--models mrssm,mmtrssm]
                                        [--modes plain_eager,plain_graph,scheduled_eager,scheduled_graph]

Modes (each on a freshly built model, bench.py's warm-up / step discipline as tools/forecast_step_bench.py: `warmup` untimed steps, then
`steps` steps between two synchronisations, wall clock over all of them and the median of per-step HIP-event intervals):

  plain_eager / plain_graph   bench.py --graph off / on: the existing epilogue kernels
  scheduled_eager             shared_step(..., elbo_schedule=ElboSchedule(free nats, a beta warm-up, modality weights)) bound to the
                              optimizer: mtrssm_elbo_schedule_fwd / _bwd in place of mtrssm_elbo_combine_fwd / _bwd, nothing else changes
  scheduled_graph             CapturedTrainStep(..., elbo_schedule=...): the same inside one hipGraph replay, a new beta every replay

Under rocprofv3 --kernel-trace --stats this is the program that gives the two schedule kernels' time per launch.
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

MODES = ("plain_eager", "plain_graph", "scheduled_eager", "scheduled_graph")
MODELS = ("mrssm", "mmtrssm")
SCHEDULE = {"free_nats": 1.0, "free_nats_h": 0.5, "beta_start": 0.1, "warmup_steps": 1000, "recon_weights": (1.0, 0.5)}


def run_mode(kind: str, mode: str, steps: int, warmup: int, device: str) -> dict[str, float]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, kind)
    schedule = mt.ElboSchedule(**SCHEDULE) if mode.startswith("scheduled") else None  # (no draw is added: both kinds draw what bench.py draws)
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = bench.synthetic_batch(b, device, seed=1000)
    source = dp.noise_source(seed=7)
    shapes = model.noise_shapes(b, t)
    if schedule is not None:
        schedule.bind(opt)

    def eager_step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        out = model.shared_step(batch, noise) if schedule is None else model.shared_step(batch, noise, elbo_schedule=schedule)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

    step = eager_step
    captured = None
    if mode.endswith("graph"):
        from multimodal_mtrssm_amd.graph import CapturedTrainStep

        captured = CapturedTrainStep(model, flat, opt, dp, batch, source, elbo_schedule=schedule)
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
    ap.add_argument("--models", default=",".join(MODELS))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    kinds = [k for k in args.models.split(",") if k]
    unknown = (set(modes) - set(MODES)) | (set(kinds) - set(MODELS))
    if unknown or args.steps < 1:
        ap.error(f"unknown modes or models {sorted(unknown)} (of {MODES}, {MODELS}) or steps < 1")
    assert torch.cuda.is_available(), "elbo_schedule_bench.py needs the MI355X"
    results = {k: {m: run_mode(k, m, args.steps, args.warmup, "cuda:0") for m in modes} for k in kinds}
    w = bench.WORKLOAD
    print(json.dumps({"metric": "ms per train step, ELBO schedule", "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"],
                      "schedule": {k: list(v) if isinstance(v, tuple) else v for k, v in SCHEDULE.items()}, "timed_steps": args.steps, "warmup": args.warmup, "models": results}))


if __name__ == "__main__":
    main()
