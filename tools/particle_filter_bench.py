"""Time of a PARTICLE-FILTER step at the bench shape (bench.py's MRSSM, B = 64, T = 50) with S particles per row
for several segment lengths, next to the likelihood step of section 6k at the same commit; the two new kernels alone against the same
rule composed from torch ops in fp64 on the same device tensors; the step by kernel; and what the two bounds say.  One JSON line.

    python tools/particle_filter_bench.py [--samples 16] [--steps 5] [--warmup 2] [--model mrssm] [--every 1,5,10,50] [--threshold 0.5]

Every time is the median of `steps` runs between two HIP events after `warmup` untimed runs, with the min and max beside it:

  likelihood_step   model.likelihood_bound(batch, LikelihoodBound(samples=S))
  step[c]           model.particle_filter(batch, ParticleFilter(S, c, threshold)): encoders, gate, codes and initial state once, then per
                    segment the rollout, the log-ratio, the decoders and the scorer, mtrssm_particle_fold and mtrssm_particle_gather
  fold, gather      each of the two kernels alone at the shapes of a segment of c = 5 frames (random errors; the state tensors of the model)
  torch_fp64_fold, torch_fp64_gather   the yardsticks on the same tensors: ParticleFilter.segment_reference (float64 torch ops, one
                    host read for its margin) and ParticleFilter.gather_reference (select + index_select per tensor)

`kernels_ms[c]` lists one step's library launches by device kernel (one extra step under the library's HIP-event timers).
`bounds` are nats per live frame under ONE set of uniforms: the particle filter's `smc`, mean `ess` and resampled fraction per c, and the
likelihood step's `iw`, `elbo` and `ess`.  `spread50` are the same figures of the two fold kernels alone on synthetic inputs whose
per-frame log-weights are spread over 50 nats, where the two bounds must differ.
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


def chain(inputs, u, c: int, threshold: float, events: tuple[int, int]) -> torch.Tensor:  # noqa: ANN001
    """The fold kernel chained over the segments of ``[B, S, T]`` inputs: the planes ``[8, B, T]``."""
    from multimodal_mtrssm_amd import ParticleFilter

    b, s, t = inputs[0].shape
    carry = ParticleFilter.new_carry(b, s, inputs[0].device)
    planes = torch.empty(8, b, t, device=inputs[0].device)
    for t0 in range(0, t, c):
        t1 = min(t, t0 + c)
        part, _ = ParticleFilter.fold(*(x[:, :, t0:t1].contiguous() for x in inputs), None, None if t1 == t else u[:, t1 - 1], t0, threshold, t1 == t,
                                      carry, *events)
        planes[:, :, t0:t1] = part
    return planes


def main() -> None:  # noqa: PLR0914, PLR0915
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="mrssm", choices=("mrssm", "mmtrssm"))
    ap.add_argument("--every", default="1,5,10,50")
    ap.add_argument("--threshold", type=float, default=0.5)
    args = ap.parse_args()
    every = [int(x) for x in args.every.split(",")]
    if not 1 <= args.samples <= 16 or args.steps < 1 or min(every) < 1:  # noqa: PLR2004
        ap.error("samples in 1 .. 16, steps >= 1, every >= 1")
    assert torch.cuda.is_available(), "particle_filter_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import LikelihoodBound, ParticleFilter, StateCarry, _lib, scan

    dev = "cuda:0"
    w = bench.WORKLOAD
    b, t, s = w["batch_per_gpu"], w["steps"], args.samples
    model = bench.build_model(dev, args.model)
    batch = bench.synthetic_batch(b, dev, seed=1000)
    bound = LikelihoodBound(samples=s)
    res: dict[str, object] = {"likelihood_step": timed(lambda: model.likelihood_bound(batch, bound), args.steps, args.warmup), "step": {},
                              "kernels_ms": {}, "bounds": {}}
    g = torch.Generator(device=dev).manual_seed(3)
    noise = {k: torch.rand(shape, device=dev, generator=g) for k, shape in ParticleFilter(s).noise_shapes(model, b, t).items()}
    shared = {k: v for k, v in noise.items() if k != "u_resample"}
    res["bounds"]["likelihood"] = {k: float(v) for k, v in model.likelihood_bound(batch, bound, shared).scalars("loglik").items()}
    for c in every:
        pf = ParticleFilter(s, c, args.threshold)
        res["step"][str(c)] = timed(lambda pf=pf: model.particle_filter(batch, pf), args.steps, args.warmup)
        _lib.TIMERS.enable()
        model.particle_filter(batch, pf)
        rows = _lib.TIMERS.summary()
        _lib.TIMERS.disable()
        res["kernels_ms"][str(c)] = {k: [int(v["launches"]), round(v["total_ms"], 4)] for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"])}
        res["bounds"][str(c)] = {k: float(v) for k, v in model.particle_filter(batch, pf, noise).scalars("smc").items()}

    # the two kernels alone, at the shapes of one segment of 5 frames
    c = 5
    e_a, e_v = batch[4][0, 0].numel(), batch[5][0, 0].numel()
    se_a = torch.rand(b, s, c, device=dev, generator=g) * 50.0 + 0.25 * e_a
    se_v = torch.rand(b, s, c, device=dev, generator=g) * 50.0 + 0.25 * e_v
    ratio = -torch.rand(b, s, c, device=dev, generator=g) * 5.0
    u = torch.rand(b, t, device=dev, generator=g)
    carry, planes, anc = ParticleFilter.new_carry(b, s, dev), torch.empty(8, b, c, device=dev), torch.empty(b, s, device=dev, dtype=torch.int32)

    def fold() -> None:
        carry.zero_()
        ParticleFilter.fold(se_a, se_v, ratio, None, u[:, c - 1], 0, 1.0, False, carry, e_a, e_v, planes=planes, ancestor=anc)  # noqa: FBT003

    def fold_fp64():  # noqa: ANN202
        carry.zero_()
        return ParticleFilter.segment_reference(se_a, se_v, ratio, None, u[:, c - 1], 0, 1.0, False, carry, e_a, e_v)  # noqa: FBT003

    widths = list(StateCarry.for_model(model, 1).widths.values())  # the tensors of a state: MRSSM 2, MMTRSSM 6
    last = [torch.randn(b * s, c, wd, device=dev, generator=g) for wd in widths]
    out = [torch.empty(b * s, wd, device=dev) for wd in widths]
    res["fold"] = timed(fold, args.steps, args.warmup)
    res["torch_fp64_fold"] = timed(fold_fp64, args.steps, args.warmup)
    fold()
    want, want_anc, margin = fold_fp64()
    res["fold_max_rel_diff"] = float(((planes.double() - want).abs() / want.abs().clamp_min(1.0)).max())
    res["fold_ancestors_equal"] = bool(torch.equal(anc, want_anc))
    res["fold_margin"] = margin
    res["gather"] = timed(lambda: ParticleFilter.gather(last, anc, out), args.steps, args.warmup)
    res["torch_fp64_gather"] = timed(lambda: ParticleFilter.gather_reference(last, anc), args.steps, args.warmup)
    res["gather_equal"] = all(torch.equal(x, y) for x, y in zip(ParticleFilter.gather(last, anc, out), ParticleFilter.gather_reference(last, anc), strict=True))
    res["gather_widths"] = widths

    # per-frame log-weights spread over 50 nats: the whole-trajectory bound follows its luckiest sample, the filter resamples
    wide = [torch.rand(b, s, t, device=dev, generator=g) * 25.0 + 0.25 * e for e in (e_a, e_v)]
    wide.append(torch.zeros(b, s, t, device=dev))
    iw = LikelihoodBound.bound(*wide, None, e_a, e_v)
    spread: dict[str, object] = {"iw": float(iw[0].mean()), "elbo": float(iw[1].mean()), "iw_ess": float(iw[5].mean())}
    for c in every:
        p = chain(wide, u, c, args.threshold, (e_a, e_v))
        spread[str(c)] = {"smc": float(p[0].mean()), "mean": float(p[1].mean()), "ess": float(p[5].mean()), "resampled": float(p[6].mean())}
    res["spread50"] = spread
    scan.check_cluster_status()
    print(json.dumps({"metric": "ms per particle-filter step and per kernel", "model": args.model, "batch": b, "steps_per_sequence": t, "samples": s,
                      "threshold": args.threshold, "events": [e_a, e_v], "timed_steps": args.steps, "warmup": args.warmup, **res}))


if __name__ == "__main__":
    main()
