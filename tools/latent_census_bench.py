"""Time of the LATENT CENSUS: the fold alone -- `mtrssm_latent_census` against the float64 torch rule
(`LatentCensus.reference`) on the same device tensors -- and a whole `model.latent_census` step against the likelihood step that runs
the same rollout with a smaller fold.  One JSON line per configuration.

    python tools/latent_census_bench.py [--steps 7] [--warmup 2] [--skip-large]

Every time is the median of `steps` runs between two HIP events after `warmup` untimed runs, with the min and max beside it, all in
one process:

  fold   kernel / rule at `(B, G, T, K, C)`: the MRSSM bench dims (64, 3, 50, 6, 5), the Large dims (256, 3, 100, 16, 8) and MMTRSSM's two
         levels at the bench dims (two calls each); random logits and one-hot samples, every frame live.  `max_plane_diff` and
         `max_rel_table_diff` say how far the two are apart.
  step   `model.latent_census(batch, LatentCensus(("both", "audio", "vision")))` next to `model.likelihood_bound(batch,
         LikelihoodBound(samples=3, score=(), latent=True))` on the same batch (bench.py's model and batch, B = 64, T = 50), and the
         census step's library launches by device kernel (one extra step under the library's HIP-event timers).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import bench  # noqa: E402  (the workload, model and batch of the flagship benchmark)
from likelihood_bench import timed  # noqa: E402

OBSERVE = ("both", "audio", "vision")


def inputs(b: int, g: int, t: int, k: int, c: int, dev: str, gen: torch.Generator) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    post, prior = (torch.randn(b * g, t, k * c, device=dev, generator=gen) for _ in range(2))
    idx = torch.randint(0, c, (b * g, t, k), device=dev, generator=gen)
    return post, prior, torch.nn.functional.one_hot(idx, c).to(torch.float32).reshape(b * g, t, k * c)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-large", action="store_true")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("steps >= 1")
    assert torch.cuda.is_available(), "latent_census_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import LatentCensus, LikelihoodBound, _lib, scan
    from multimodal_mtrssm_amd.census import table_views

    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(5)
    common = {"device": torch.cuda.get_device_name(0), "timed_steps": args.steps, "warmup": args.warmup}
    folds = [("mrssm_bench", [(64, 3, 50, 6, 5)]), ("mmtrssm_bench_two_levels", [(64, 3, 50, 6, 5)] * 2)]
    if not args.skip_large:
        folds.insert(1, ("mrssm_large", [(256, 3, 100, 16, 8)]))
    for name, levels in folds:
        data = [(inputs(*shape, dev, gen), shape) for shape in levels]
        kernel = timed(lambda d=data: [LatentCensus.fold(*x, s[1], s[3], s[4]) for x, s in d], args.steps, args.warmup)
        rule = timed(lambda d=data: [LatentCensus.reference(*x, s[1], s[3], s[4]) for x, s in d], args.steps, args.warmup)
        (x, s) = data[0]
        got_planes, got = LatentCensus.fold(*x, s[1], s[3], s[4])
        want_planes, want = LatentCensus.reference(*x, s[1], s[3], s[4])
        sums = ("qsum", "psum", "post_entropy", "prior_entropy", "kl", "cross")
        a, b = table_views(got, s[3], s[4], s[2]), table_views(want, s[3], s[4], s[2])
        rel = max(float(((a[key] - b[key]).abs() / b[key].abs().clamp_min(1e-300)).max()) for key in sums)
        print(json.dumps({"metric": "ms per census fold: kernel and float64 torch rule", "config": name, "shapes_BGTKC": levels, "kernel": kernel,
                          "torch_fp64_rule": rule, "rule_over_kernel": rule["median_ms"] / kernel["median_ms"],
                          "max_plane_diff": float((got_planes.double() - want_planes).abs().max()), "max_rel_table_diff": rel,
                          "counts_equal": bool(torch.equal(a["n"], b["n"])), **common}), flush=True)

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    for kind in ("mrssm", "mmtrssm"):
        model = bench.build_model(dev, kind)
        batch = bench.synthetic_batch(b, dev, seed=1000)
        census, bound = LatentCensus(OBSERVE), LikelihoodBound(samples=3, score=(), latent=True)
        step = timed(lambda m=model, x=batch, c=census: m.latent_census(x, c), args.steps, args.warmup)
        likelihood = timed(lambda m=model, x=batch, lb=bound: m.likelihood_bound(x, lb), args.steps, args.warmup)
        _lib.TIMERS.enable()
        table = model.latent_census(batch, census)
        rows = _lib.TIMERS.summary()
        _lib.TIMERS.disable()
        kernels = {k: [int(v["launches"]), round(v["total_ms"], 4)] for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"])}
        fold_ms = sum(v[1] for k, v in kernels.items() if "census" in k)
        scan.check_cluster_status()
        print(json.dumps({"metric": "ms per census step and per likelihood step (samples = 3, latent only)", "config": f"{kind}_bench_step", "batch": b,
                          "steps_per_sequence": t, "observe": OBSERVE, "census_step": step, "likelihood_step": likelihood,
                          "census_over_likelihood": step["median_ms"] / likelihood["median_ms"], "census_fold_ms": fold_ms,
                          "fold_share_of_step": fold_ms / step["median_ms"], "kernels_ms": kernels,
                          "scalars": {k: float(v) for k, v in table.scalars("latent").items()}, **common}), flush=True)


if __name__ == "__main__":
    main()
