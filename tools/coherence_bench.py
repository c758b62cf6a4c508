"""Time of GENERATION COHERENCE at one fixed shape: a whole `model.generation_coherence` step with and without its
fold, and the fold alone -- `mtrssm_coherence_fold` -- against the same scoring composed from torch ops on the same device logits.  One
JSON line each.

    python tools/coherence_bench.py [--steps 7] [--warmup 2] [--model mrssm|mmtrssm]

Every time is the median of `steps` runs between two HIP events after `warmup` untimed runs, with the min and max beside it, all in
one process.  The shape is the evaluation's: the 1 x 32 x 32 model of `tools/generation_coherence.py` at its default dims (untrained),
B = 16 windows of T = 40 frames, 30 observed, S = 10 futures for each of G = 3 subsets (480 scan rows, 19200 copy-frames), seeded
untrained readers, random labels with a tenth of silence.

  step   `model.generation_coherence(batch, labels, gc, readers, noise)`; the same call with `GenerationCoherence.fold` replaced by a
         function that returns at once (rollout, decoders and readers only); the library launches of one step by device kernel.
  fold   `GenerationCoherence.fold` on the step's logits, with and without planes; `torch_scoring` on the same logits: the same
         quantities in float64 from vectorised torch ops (`argmax`, `softmax`, `index_add_`, `bincount`) -- what the step would run
         without the kernel; its sums follow torch's reduction order, not the fold's.  `max_rel_soft_diff` and `whole_cells_equal` say
         how far the two are apart.
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

from likelihood_bench import timed  # noqa: E402
from word_transitions import build_model  # noqa: E402

B, T, CONTEXT, S = 16, 40, 30, 10
OBSERVE = ("both", "audio", "vision")
DIMS = (32, 32, 4, 4, 64)


def torch_scoring(lv: torch.Tensor, la: torch.Tensor, labels: torch.Tensor, groups: int, samples: int, context: int) -> torch.Tensor:  # noqa: PLR0914
    """The table ``[G, 6 T + 242]`` of one step from torch ops, in float64 (every row whole: no ``valid``)."""
    rows, t, _ = lv.shape
    b, g, s, f64 = rows // (groups * samples), groups, samples, torch.float64
    zv, za = lv.to(f64).reshape(b, g, s, t, 10), la.to(f64).reshape(b, g, s, t, 10)
    ok_v, ok_a = torch.isfinite(zv).all(-1), torch.isfinite(za).all(-1)
    dv = torch.where(ok_v, zv.argmax(-1), 10)
    da = torch.where(ok_a, za.argmax(-1), 10)
    word = labels.to(torch.int64)[:, None, None, :]
    live = ((word >= 0) & (word < 10)).expand(b, g, s, t)  # noqa: PLR2004
    soft = torch.where(ok_v & ok_a, (torch.softmax(zv, -1) * torch.softmax(za, -1)).sum(-1), 0.0)
    per_copy = torch.stack([(dv == word).to(f64), (da == word).to(f64), ((dv == da) & (dv < 10)).to(f64), ((dv == da) & (dv == word)).to(f64),  # noqa: PLR2004
                            soft, torch.ones_like(soft)])
    per_copy = torch.where(live, per_copy, 0.0).sum(3)  # [6, B, G, T]
    c = min(context, t)
    horizon = (torch.arange(t, device=lv.device) - c + 1).clamp_min(0)
    sums = torch.zeros(6, g, t, dtype=f64, device=lv.device).index_add_(2, horizon, per_copy.sum(1))
    phase = (torch.arange(t, device=lv.device) >= c).to(torch.int64)
    cell = ((torch.arange(g, device=lv.device)[None, :, None, None] * 2 + phase) * 11 + dv) * 11 + da
    pairs = torch.bincount(cell[live], minlength=g * 242).reshape(g, 242).to(f64)
    return torch.cat([sums.permute(1, 0, 2).reshape(g, 6 * t), pairs], dim=1)


def main() -> None:  # noqa: PLR0914
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("steps >= 1")
    assert torch.cuda.is_available(), "coherence_bench.py needs the MI355X"
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import _lib
    from multimodal_mtrssm_amd.coherence import table_views

    dev = "cuda:0"
    torch.manual_seed(0)
    gen = torch.Generator(device=dev).manual_seed(5)
    common = {"device": torch.cuda.get_device_name(0), "timed_steps": args.steps, "warmup": args.warmup, "model": args.model,
              "shape_BGST": [B, len(OBSERVE), S, T], "context": CONTEXT}
    model = build_model(args.model, DIMS, dev).eval()
    readers = {}
    for i, name in enumerate(("vision", "audio")):
        torch.manual_seed(10 + i)
        readers[name] = mt.DigitClassifier()
        for layer in (readers[name].conv1, readers[name].conv2, readers[name].fc1, readers[name].fc2):
            layer.reset_parameters()
        readers[name].to(dev)
    frames = lambda: torch.rand(B, T, 1, 32, 32, device=dev, generator=gen) * 2.0 - 1.0  # noqa: E731
    action = torch.nn.functional.one_hot(torch.randint(0, 6, (B, 1), device=dev, generator=gen), 6).float().expand(B, T, 6).contiguous()
    audio, vision = frames(), frames()
    batch = (action, audio, vision, action, audio, vision)
    labels = torch.randint(0, 10, (B, T), device=dev, generator=gen).to(torch.int32)
    labels[torch.rand(B, T, device=dev, generator=gen) < 0.1] = -1  # noqa: PLR2004
    gc = mt.GenerationCoherence(CONTEXT, samples=S, observe=OBSERVE)
    noise = {k: torch.rand(shape, device=dev, generator=gen) for k, shape in gc.noise_shapes(model, B, T).items()}
    run = lambda: model.generation_coherence(batch, labels, gc, readers, noise)  # noqa: E731

    step = timed(run, args.steps, args.warmup)
    real_fold = mt.GenerationCoherence.fold
    mt.GenerationCoherence.fold = staticmethod(lambda *a, table=None, **kw: (None, table))  # noqa: ARG005
    try:
        bare = timed(run, args.steps, args.warmup)
    finally:
        mt.GenerationCoherence.fold = staticmethod(real_fold)
    _lib.TIMERS.enable()
    kept = model.generation_coherence(batch, labels, gc, readers, noise, keep_states=True)
    rows = _lib.TIMERS.summary()
    _lib.TIMERS.disable()
    kernels = {k: [int(v["launches"]), round(v["total_ms"], 4)] for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"])}
    print(json.dumps({"metric": "ms per coherence step, with and without the fold", "step": step, "step_without_fold": bare,
                      "fold_share_of_step": 1.0 - bare["median_ms"] / step["median_ms"], "kernels_ms": kernels,
                      "scalars": {k: float(v) for k, v in kept.scalars("coherence").items() if k.endswith(("/obs", "/h8", "reads"))}, **common}),
          flush=True)

    lv, la = kept.logits
    g = len(OBSERVE)
    kernel = timed(lambda: mt.GenerationCoherence.fold(lv, la, labels, g, S, CONTEXT, planes=False), args.steps, args.warmup)
    with_planes = timed(lambda: mt.GenerationCoherence.fold(lv, la, labels, g, S, CONTEXT), args.steps, args.warmup)
    composed = timed(lambda: torch_scoring(lv, la, labels, g, S, CONTEXT), args.steps, args.warmup)
    _, got = mt.GenerationCoherence.fold(lv, la, labels, g, S, CONTEXT, planes=False)
    a, b = table_views(got, T), table_views(torch_scoring(lv, la, labels, g, S, CONTEXT), T)
    whole = all(bool(torch.equal(a[key], b[key])) for key in ("counts", "pairs")) and bool(torch.equal(a["sums"][:, :4], b["sums"][:, :4]))
    rel = float(((a["sums"][:, 4] - b["sums"][:, 4]).abs() / b["sums"][:, 4].abs().clamp_min(1e-300)).max())
    print(json.dumps({"metric": "ms per coherence fold: kernel and the same scoring from torch ops (float64)", "kernel": kernel,
                      "kernel_with_planes": with_planes, "torch_ops": composed, "torch_ops_over_kernel": composed["median_ms"] / kernel["median_ms"],
                      "whole_cells_equal": whole, "max_rel_soft_diff": rel, **common}), flush=True)


if __name__ == "__main__":
    main()
