"""Time of ONE linear-probe step -- the fused `mtrssm_linear_probe_step`, its evaluation-only form, and a
same-commit yardstick: the same step composed from torch ops on the same device tensors.  One JSON line.

    python tools/latent_probe_bench.py [--steps 5] [--warmup 2] [--groups 3] [--features 230] [--classes 10] [--rows 3200,65536]

Every figure is the median of `steps` runs between two HIP events after `warmup` untimed runs, in one process, with the min and max
beside it.  Per row count N (3200 = one bench batch of 64 x 50 frames, 65 536 = a cached fit set):

  fused    LinearProbe.step(x, labels): loss, hits and both gradients, ONE library call (the step kernel and its ordered reducer)
  eval     LinearProbe.step(x, labels, grad=False, planes=True): no gradient work, the per-frame planes written
  torch    the yardstick: x @ W^T + b, log_softmax, nll_loss, autograd backward, argmax -- about ten launches that read x three times
           and write [G, N, C] logits and probabilities; `max_*_diff` is its distance from the fused step's results
  gbps     the fused step's G * N * F * 4 feature bytes per second of its median (about a fifth of the labels are -1 and those rows are
           not read: the figure counts them all, as the composition reads them all)
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


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


def torch_step(x: torch.Tensor, labels: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> tuple[torch.Tensor, ...]:
    """The composition: mean loss over the live frames (ignore_index = -1), its gradients by autograd, the hits."""
    weight.grad = bias.grad = None
    z = torch.baddbmm(bias[:, None, :], x, weight.transpose(1, 2))
    logp = torch.log_softmax(z, dim=-1)
    loss = torch.nn.functional.nll_loss(logp.reshape(-1, logp.shape[-1]), labels.repeat(x.shape[0]), ignore_index=-1, reduction="sum")
    loss.backward()
    hits = (z.argmax(-1) == labels[None]).sum(1)
    return loss.detach(), hits, weight.grad, bias.grad


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--groups", type=int, default=3)
    ap.add_argument("--features", type=int, default=230)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--rows", default="3200,65536")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("steps >= 1")
    assert torch.cuda.is_available(), "latent_probe_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import LinearProbe

    dev = "cuda:0"
    g, f, c = args.groups, args.features, args.classes
    res: dict[str, object] = {}
    for n in (int(r) for r in args.rows.split(",")):
        gen = torch.Generator(device=dev).manual_seed(7)
        x = torch.tanh(torch.randn(g, n, f, device=dev, generator=gen))
        labels = torch.randint(0, c, (n,), device=dev, generator=gen).to(torch.int32)
        labels[torch.rand(n, device=dev, generator=gen) < 0.2] = -1  # noqa: PLR2004
        probe = LinearProbe(g, f, c).to(dev)
        with torch.no_grad():
            probe.weight.copy_(torch.randn(g, c, f, device=dev, generator=gen) / f ** 0.5)
            probe.bias.copy_(0.5 * torch.randn(g, c, device=dev, generator=gen))
        w = probe.weight.detach().clone().requires_grad_()
        b = probe.bias.detach().clone().requires_grad_()
        long_labels = labels.long()
        row: dict[str, object] = {}
        row["fused"] = timed(lambda: probe.step(x, labels, normalize=False), args.steps, args.warmup)  # noqa: B023
        row["eval"] = timed(lambda: probe.step(x, labels, grad=False, planes=True), args.steps, args.warmup)  # noqa: B023
        row["torch"] = timed(lambda: torch_step(x, long_labels, w, b), args.steps, args.warmup)  # noqa: B023
        stats = probe.step(x, labels, normalize=False)
        loss, hits, g_w, g_b = torch_step(x, long_labels, w, b)
        row["max_grad_diff"] = float((probe.weight.grad - g_w).abs().max())
        row["max_bias_grad_diff"] = float((probe.bias.grad - g_b).abs().max())
        row["max_grad"] = float(g_w.abs().max())
        row["nll_rel_diff"] = float(((stats.nll_sum.sum() - loss).abs() / loss.abs()))
        row["hits_diff"] = int((stats.hits.long() - hits).abs().max())
        row["gbps"] = 4.0 * g * n * f / (row["fused"]["median_ms"] * 1e-3) / 1e9
        row["speedup"] = row["torch"]["median_ms"] / row["fused"]["median_ms"]
        res[f"N={n}"] = row
    print(json.dumps({"metric": "ms per linear-probe step", "groups": g, "features": f, "classes": c, "timed_steps": args.steps,
                      "warmup": args.warmup, **res}))


if __name__ == "__main__":
    main()
