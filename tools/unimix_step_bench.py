"""Step time of the train step with UNIFORM MIXING of the categorical latents at the bench shape (bench.py's
models and batch), one JSON line.

    python tools/unimix_step_bench.py [--model mrssm|mmtrssm|large] [--steps 20] [--warmup 5] [--eps 0.01] [--modes eager,graph]

Per mode (bench.py --graph off / on) two freshly built models, ``unimix`` 0 and ``--eps`` (bench.py's warm-up / step discipline as
tools/elbo_schedule_bench.py: `warmup` untimed steps, then `steps` steps between two synchronisations, wall clock over all of them
and the median of per-step HIP-event intervals).  After the timed steps three more eager steps run under the library's kernel
timers: ``scan`` holds, per scan kernel of the model's family, the mean launch time and that time per timestep -- the mixing is a
constant kernel argument, so the same kernels run either way and the difference of the two is its cost on the timestep's chain.
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

MODES = ("eager", "graph")
MODELS = ("mrssm", "mmtrssm", "large")


def run_mode(kind: str, mode: str, eps: float, steps: int, warmup: int, device: str) -> dict[str, object]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import _lib, scan
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, kind)
    model.unimix = eps  # (config, not state: the same parameters either way)
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = bench.synthetic_batch(b, device, seed=1000)
    source = dp.noise_source(seed=7)
    shapes = model.noise_shapes(b, t)

    def eager_step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        out = model.shared_step(batch, noise)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

    step = eager_step
    captured = None
    if mode == "graph":
        from multimodal_mtrssm_amd.graph import CapturedTrainStep

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
    result: dict[str, object] = {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0],
                                 "max_ms": per_step[-1]}
    if mode == "eager":  # the scan kernels on their own: HIP events around each launch
        _lib.TIMERS.enable()
        try:
            for _ in range(3):
                eager_step()
            rows = _lib.TIMERS.summary()
        finally:
            _lib.TIMERS.disable()
        result["scan"] = {k.split("<")[0].removeprefix("mtrssm::"): {"ms_per_launch": v["avg_ms"], "us_per_timestep": v["avg_ms"] * 1e3 / t}
                          for k, v in rows.items() if k.startswith(("mtrssm::mrssm_", "mtrssm::mmtrssm_"))}
    return result


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=MODELS, default="mrssm")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.01)
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    if set(modes) - set(MODES) or args.steps < 1 or not 0.0 < args.eps < 1.0:
        ap.error(f"unknown modes {sorted(set(modes) - set(MODES))} (of {MODES}), steps < 1 or eps outside (0, 1)")
    assert torch.cuda.is_available(), "unimix_step_bench.py needs the MI355X"
    bench.WORKLOAD = bench.WORKLOADS["large" if args.model == "large" else "base"]
    w = bench.WORKLOAD
    results = {m: {f"unimix_{eps:g}": run_mode(args.model, m, eps, args.steps, args.warmup, "cuda:0") for eps in (0.0, args.eps)} for m in modes}
    print(json.dumps({"metric": "ms per train step, unimix off and on", "model": args.model, "batch": w["batch_per_gpu"],
                      "steps_per_sequence": w["steps"], "eps": args.eps, "timed_steps": args.steps, "warmup": args.warmup, "modes": results}))


if __name__ == "__main__":
    main()
