"""Step time of the WEIGHTED masked train step next to the plain masked one at the bench shape (bench.py's models, B = 64, T = 50),
and the mean time per launch of the masked scans in each, one JSON line.

    python tools/weighted_mopoe_bench.py [--model mrssm|mmtrssm] [--steps 20] [--warmup 5] [--modes masked,explicit,static,gated]

Modes (each on a freshly built model, eager steps with bench.py's warm-up / step discipline: `warmup` untimed steps, then `steps`
steps between two synchronisations, wall clock over all of them and the median of per-step HIP-event intervals; the same fixed
device-side modality mask in every mode, so all of them run the MASKED scan instances):

  masked     the plain masked step: no weights, the kernels' constant 1/3 (runs on commits before the weights too)
  explicit   the same step handed a constant [B, T, 3] tensor of log-weights: the scans' cost of the weights alone
  static     model.expert_weights = ExpertWeights("static"): one learned triple
  gated      model.expert_weights = ExpertWeights("gated", embed): the per-frame gate, its GEMMs and its softmax included

After the timed steps a few more run with the library's HIP-event timers on: `scans` is the mean milliseconds per launch of every
scan kernel of the mode, keyed as rocprofv3 names it.  The weighted and the plain masked step launch the SAME kernel instances, so a
kernel trace tells them apart only by process: profile one mode per run
(`rocprofv3 --kernel-trace --stats -- python tools/weighted_mopoe_bench.py --modes gated`).
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

import bench  # noqa: E402  (the workload, models and batch of the flagship benchmark)

MODES = ("masked", "explicit", "static", "gated")
P_PRESENT = 0.7  # each modality of a frame is observed with this probability; frame 0 observes both


def fixed_mask(b: int, t: int, device: str) -> torch.Tensor:
    mask = torch.rand(b, t, 2, generator=torch.Generator().manual_seed(3)) < P_PRESENT
    mask[:, 0] = True
    return mask.to(device)


def run_mode(mode: str, kind: str, steps: int, warmup: int, device: str) -> dict[str, object]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, kind)
    kw = {}
    if mode in ("static", "gated"):
        from multimodal_mtrssm_amd.experts import ExpertWeights

        model.expert_weights = ExpertWeights(mode, w["embed"] if mode == "gated" else None).to(device)  # (before FlatParameters)
    elif mode == "explicit":
        from multimodal_mtrssm_amd.experts import LOG_THIRD

        kw["expert_log_weights"] = torch.full((b, t, 3), LOG_THIRD, dtype=torch.float32, device=device)
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = (*bench.synthetic_batch(b, device, seed=1000), fixed_mask(b, t, device))
    source = dp.noise_source(seed=7)
    shapes = model.noise_shapes(b, t)

    def step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        out = model.shared_step(batch, noise, **kw)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

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
    scan.KERNEL_TIMERS.enable()
    for _ in range(min(steps, 5)):
        step()
    rows = scan.KERNEL_TIMERS.summary()
    scan.KERNEL_TIMERS.disable()
    scans = {k: round(v["avg_ms"], 4) for k, v in rows.items() if "rssm_" in k and ("fwd" in k or "bwd" in k)}
    result: dict[str, object] = {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0],
                                 "max_ms": per_step[-1], "scans": scans}
    if model.__dict__.get("weights_timeseries") is not None:
        both = model._weights_both.unsqueeze(-1).float()  # noqa: SLF001
        mean = (model.weights_timeseries * both).sum(dim=(0, 1)) / both.sum().clamp(min=1.0)
        result["mean_weights"] = [round(float(x), 4) for x in mean]
    return result


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    unknown = set(modes) - set(MODES)
    if unknown or args.steps < 1:
        ap.error(f"unknown modes {sorted(unknown)} (of {MODES}) or steps < 1")
    assert torch.cuda.is_available(), "weighted_mopoe_bench.py needs the MI355X"
    results = {m: run_mode(m, args.model, args.steps, args.warmup, "cuda:0") for m in modes}
    w = bench.WORKLOAD
    print(json.dumps({"metric": f"ms per MoPoE-{args.model.upper()} train step, masked, with and without expert weights",
                      "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"], "p_present": P_PRESENT, "timed_steps": args.steps,
                      "warmup": args.warmup, "modes": results}))


if __name__ == "__main__":
    main()
