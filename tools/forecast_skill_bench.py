"""Time of a forecast SKILL step at the bench shape (bench.py's models, B = 64, T = 50, context q = 10) for
S = 1, 4, 16 samples per row, next to this build's plain validation step in the same process, one JSON line.

    python tools/forecast_skill_bench.py [--steps 10] [--warmup 3] [--models mrssm,mmtrssm] [--samples 1,4,16]
    python tools/forecast_skill_bench.py --kernels S

Per model, on one freshly built model (`warmup` untimed steps, then `steps` steps between two synchronisations; wall clock over all of
them and the median of per-step HIP-event intervals):

  validation     model.validation_step(batch) with val_skill None: the closed-loop ELBO terms under no_grad
  skill_S        model.forecast_skill(batch, ForecastSkill(10, samples=S)): both encoders once, ONE masked rollout over B * S rows, the
                 decoders and the scorer over chunks of at most 4096 frames, the horizon fold

`--kernels S` builds no model: on random tensors of one decode chunk's shape (the rows of a 4096-frame chunk, S samples, T = 50, the
4096 elements of a bench frame) it launches the scorer (Tanh) twice and the sibling NLL kernel (`nll_fwd_kernel<true>`: the same access
pattern over two streams) twice on the same frames, and nothing else from the library but the NLL's 4-byte clear.  Under
`rocprofv3 --kernel-trace --stats` the rows `ensemble_score_kernel<S, true>` and `nll_fwd_kernel<true>` of such a process therefore
hold exactly these launches (two calls each, the first cold); `scorer_bytes` / `nll_bytes` are the bytes one launch moves.  In the
default mode the same pair is timed with HIP events after each S, but there the per-name rows of `--stats` also hold the launches of
the timed steps.
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

MODELS = ("mrssm", "mmtrssm")
CONTEXT = 10


def timed(step, steps: int, warmup: int) -> dict[str, float]:  # noqa: ANN001
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
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0], "max_ms": per_step[-1]}


def kernel_pair(samples: int, rows: int, t: int, event: int, device: str) -> dict[str, float]:
    """The scorer on random tensors of `rows` rows of S samples and the NLL kernel on the same frames: each launched once to warm, once
    between two HIP events (rocprofv3 times them better)."""
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import ForecastSkill

    g = torch.Generator(device=device).manual_seed(3)
    pred = torch.randn(rows, samples, t, event, device=device, generator=g)
    target = torch.rand(rows, t, event, device=device, generator=g) * 2.0 - 1.0
    wide = target[:, None].expand(rows, samples, t, event).contiguous()
    out: dict[str, float] = {"rows": rows, "scorer_bytes": 4.0 * (samples + 1) * rows * t * event, "nll_bytes": 8.0 * rows * samples * t * event}
    for name, fn in (("scorer_ms", lambda: ForecastSkill.score(pred, target, None, 3)),
                     ("nll_ms", lambda: mt.likelihood(pred, wide, event_ndims=1, out_act=3))):
        fn()  # (warm: code object, allocator)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out[name] = a.elapsed_time(b)
    return out


def run_model(kind: str, samples: list[int], steps: int, warmup: int, device: str) -> dict[str, object]:
    from multimodal_mtrssm_amd import ForecastSkill, scan

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, kind)
    batch = bench.synthetic_batch(b, device, seed=1000)
    event = batch[5][0, 0].numel()
    res: dict[str, object] = {}
    with torch.no_grad():
        res["validation"] = timed(lambda: model.validation_step(batch), steps, warmup)
    for s in samples:
        skill = ForecastSkill(CONTEXT, samples=s)
        res[f"skill_{s}"] = timed(lambda skill=skill: model.forecast_skill(batch, skill), steps, warmup)
        rows = min(b, max(1, skill.max_frames // (s * t)))
        res[f"kernels_{s}"] = kernel_pair(s, rows, t, event, device)
    scan.check_cluster_status()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--samples", default="1,4,16")
    ap.add_argument("--kernels", type=int, default=0, metavar="S", help="only the scorer / NLL kernel pair at S samples, no model")
    args = ap.parse_args()
    w = bench.WORKLOAD
    if args.kernels:
        if not 1 <= args.kernels <= 16:  # noqa: PLR2004
            ap.error("--kernels takes S in 1 .. 16")
        assert torch.cuda.is_available(), "forecast_skill_bench.py needs the MI355X"
        b, t, s = w["batch_per_gpu"], w["steps"], args.kernels
        event = 1
        for n in w["vision"]:
            event *= n
        print(json.dumps({"metric": "scorer and NLL kernel on one decode chunk", "samples": s, "steps_per_sequence": t, "event": event,
                          **kernel_pair(s, min(b, max(1, 4096 // (s * t))), t, event, "cuda:0")}))
        return
    kinds = [k for k in args.models.split(",") if k]
    samples = [int(s) for s in args.samples.split(",") if s]
    if set(kinds) - set(MODELS) or args.steps < 1 or not samples or not all(1 <= s <= 16 for s in samples):  # noqa: PLR2004
        ap.error(f"models of {MODELS}, steps >= 1, samples in 1 .. 16")
    assert torch.cuda.is_available(), "forecast_skill_bench.py needs the MI355X"
    results = {k: run_model(k, samples, args.steps, args.warmup, "cuda:0") for k in kinds}
    print(json.dumps({"metric": "ms per forecast skill step", "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"], "context": CONTEXT,
                      "samples": samples, "timed_steps": args.steps, "warmup": args.warmup, "models": results}))


if __name__ == "__main__":
    main()
