"""Time of a LIKELIHOOD step at the bench shape (bench.py's MRSSM, B = 64, T = 50) with S samples per row, the two
new kernels alone, and a same-commit yardstick: the same scoring composed from torch ops in fp64 on the same device tensors.  One JSON
line.

    python tools/likelihood_bench.py [--samples 16] [--steps 5] [--warmup 2] [--model mrssm]

Every figure is the median of `steps` runs between two HIP events after `warmup` untimed runs, with the min and max beside it:

  step         model.likelihood_bound(batch, LikelihoodBound(samples=S)): both encoders once, ONE masked rollout over B * S rows, the
               log-ratio kernel, then per chunk of at most 4096 frames the decoders, the scorer, the bound kernel and the table fold
  validation   model.validation_step(batch) with no val_* set, for scale
  fused_pair   mtrssm_latent_log_ratio + mtrssm_iw_bound on tensors of the step's shapes (random logits, a one-hot sample, random errors)
  log_ratio, iw_bound   each of the two alone
  torch_fp64   the yardstick on the same tensors: log_softmax, gather, sum, cumsum, logsumexp, exp, stack, all in float64 as the rule
               demands (about two dozen launches over the same bytes); `max_abs_diff` is its distance from the fused pair's planes

`kernels_ms` lists the step's library launches by device kernel (one extra step under the library's HIP-event timers), so the shares of
the decoders, the scan and the two new kernels can be read off.
"""

from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the workload, model and batch of the flagship benchmark)


def timed(fn, steps: int, warmup: int) -> dict[str, float]:  # noqa: ANN001
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def torch_fp64(post, prior, stoch, se_a, se_v, cats: int, classes: int, e_a: int, e_v: int) -> torch.Tensor:  # noqa: ANN001, PLR0913, PLR0914
    """The quantity of DESIGN.md 6k from torch ops, in float64 (every frame live): the yardstick."""
    b, s, t = se_a.shape
    q = post.double().reshape(-1, cats, classes)
    p = prior.double().reshape(-1, cats, classes)
    idx = stoch.reshape(-1, cats, classes).argmax(-1, keepdim=True)
    ratio = (torch.log_softmax(p, -1).gather(-1, idx) - torch.log_softmax(q, -1).gather(-1, idx)).sum((-1, -2)).reshape(b, s, t)
    a = -se_a.double() - 0.5 * e_a * math.log(2.0 * math.pi)
    v = -se_v.double() - 0.5 * e_v * math.log(2.0 * math.pi)
    cum = ((a + v) + ratio).cumsum(-1)
    prefix_iw = torch.logsumexp(cum, 1) - math.log(s)
    prefix_elbo = cum.mean(1)
    zero = torch.zeros(b, 1, dtype=torch.float64, device=cum.device)
    w = torch.exp(cum - cum.max(1, keepdim=True).values)
    return torch.stack([torch.diff(prefix_iw, prepend=zero), torch.diff(prefix_elbo, prepend=zero), a.mean(1), v.mean(1), ratio.mean(1),
                        w.sum(1) ** 2 / (w * w).sum(1), prefix_iw, prefix_elbo]).float()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="mrssm", choices=("mrssm", "mmtrssm"))
    args = ap.parse_args()
    if not 1 <= args.samples <= 16 or args.steps < 1:  # noqa: PLR2004
        ap.error("samples in 1 .. 16, steps >= 1")
    assert torch.cuda.is_available(), "likelihood_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import LikelihoodBound, _lib, scan

    dev = "cuda:0"
    w = bench.WORKLOAD
    b, t, s = w["batch_per_gpu"], w["steps"], args.samples
    model = bench.build_model(dev, args.model)
    batch = bench.synthetic_batch(b, dev, seed=1000)
    bound = LikelihoodBound(samples=s)
    res: dict[str, object] = {}
    with torch.no_grad():
        res["validation"] = timed(lambda: model.validation_step(batch), args.steps, args.warmup)
    res["step"] = timed(lambda: model.likelihood_bound(batch, bound), args.steps, args.warmup)
    _lib.TIMERS.enable()
    table = model.likelihood_bound(batch, bound)
    rows = _lib.TIMERS.summary()
    _lib.TIMERS.disable()
    res["kernels_ms"] = {k: round(v["total_ms"], 4) for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"])}
    res["per_frame"] = {k: float(v) for k, v in table.scalars("loglik").items()}

    level = model._latent_levels()[0][1]  # noqa: SLF001  (the lower level's K and C: the kernel pair is timed on one level)
    cats, classes = level.category_size, level.class_size
    e_a, e_v = batch[4][0, 0].numel(), batch[5][0, 0].numel()
    g = torch.Generator(device=dev).manual_seed(3)
    post = torch.randn(b * s, t, cats * classes, device=dev, generator=g) * 2.0
    prior = torch.randn(b * s, t, cats * classes, device=dev, generator=g) * 2.0
    idx = torch.randint(0, classes, (b * s, t, cats), device=dev, generator=g)
    stoch = torch.nn.functional.one_hot(idx, classes).to(torch.float32).reshape(b * s, t, cats * classes)
    se_a = torch.rand(b, s, t, device=dev, generator=g) * 50.0 + 0.25 * e_a
    se_v = torch.rand(b, s, t, device=dev, generator=g) * 50.0 + 0.25 * e_v
    ratio = torch.empty(b * s, t, device=dev)
    planes = torch.empty(8, b, t, device=dev)

    def log_ratio() -> None:
        LikelihoodBound.log_ratio(post, prior, stoch, cats, classes, out=ratio)

    def iw_bound() -> None:
        LikelihoodBound.bound(se_a, se_v, ratio.view(b, s, t), None, e_a, e_v, out=planes)

    def pair() -> None:
        log_ratio()
        iw_bound()

    res["fused_pair"] = timed(pair, args.steps, args.warmup)
    res["log_ratio"] = timed(log_ratio, args.steps, args.warmup)
    res["iw_bound"] = timed(iw_bound, args.steps, args.warmup)
    res["torch_fp64"] = timed(lambda: torch_fp64(post, prior, stoch, se_a, se_v, cats, classes, e_a, e_v), args.steps, args.warmup)
    pair()
    want = torch_fp64(post, prior, stoch, se_a, se_v, cats, classes, e_a, e_v)
    res["max_abs_diff"] = float((planes - want).abs().max())
    res["max_rel_diff"] = float(((planes - want).abs() / want.abs().clamp_min(1.0)).max())
    res["mean_ess_random_inputs"] = float(planes[5].mean())
    scan.check_cluster_status()
    print(json.dumps({"metric": "ms per likelihood step and per kernel", "model": args.model, "batch": b, "steps_per_sequence": t, "samples": s,
                      "cats": cats, "classes": classes, "events": [e_a, e_v], "timed_steps": args.steps, "warmup": args.warmup, **res}))


if __name__ == "__main__":
    main()
