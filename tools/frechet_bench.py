"""Time of the FRECHET DISTANCE step: the fold alone -- `mtrssm_feature_moments` against the same statistic done
with torch on the device (`x.double()`, one masked `x^T x` per bin: `FrechetDistance.reference_moments`) -- and a whole
`model.frechet_distance` step with its stages.  JSON lines.

    python tools/frechet_bench.py [--steps 7] [--warmup 2]

  fold   N = 25 600 feature rows (B 64 x S 8 x T 50), D = 128, J = 5, the bins of a context of 10: kernel and torch, and their
         largest difference relative to the bound 2 n_j 2^-53 sum |x_i x_j|.  Also D = 256 (the widest).
  step   B 64, T 50, S 8, q 10.  `reader`: an MRSSM at the reference's default dims with 32 x 32 frames (what the digit reader
         reads) and a seeded `DigitClassifier`; `encoder`: the flagship benchmark's model (64 x 64 vision, embedding 256).  The whole
         step, then its stages on the same tensors: the rollout, the decoders, the features (generated and real), the folds.
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

B, T, S, Q = 64, 50, 8, 10


def main() -> None:  # noqa: PLR0914, PLR0915
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("steps >= 1")
    assert torch.cuda.is_available(), "frechet_bench.py needs the MI355X"
    from multimodal_mtrssm_amd import DigitClassifier, FrechetDistance, FrechetTable
    from multimodal_mtrssm_amd.frechet import cells
    from word_transitions import build_model

    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(5)
    common = {"device": torch.cuda.get_device_name(0), "timed_steps": args.steps, "warmup": args.warmup}
    fd = FrechetDistance(Q, samples=S)
    j = len(fd.bin_names)
    bins = fd.bins(B, T, None, torch.device(dev))[:, None].expand(B, S, T).reshape(-1).contiguous()
    for d in (128, 256):
        x = torch.randn(B * S * T, d, device=dev, generator=gen)
        table, other = (torch.zeros(j, cells(d), dtype=torch.float64, device=dev) for _ in range(2))
        kernel = timed(lambda x=x, t=table: FrechetDistance.fold(x, bins, j, t), args.steps, args.warmup)
        rule = timed(lambda x=x, t=other: FrechetDistance.reference_moments(x, bins, j, t), args.steps, args.warmup)
        n_j = table[:, :1] / (args.steps + args.warmup)
        bound = 2.0 * n_j * 2.0**-53 * table[:, 1 + d :]  # (>= the bound on the diagonal; an order-of-magnitude yardstick elsewhere)
        diag = torch.arange(d, device=dev) * (d + 1)
        err = ((table - other).abs()[:, 1 + d :][:, diag] / bound[:, diag].clamp_min(1e-300)).max()
        print(json.dumps({"metric": "ms per fold of feature moments: kernel and torch float64 on the device", "N": B * S * T, "D": d, "J": j,
                          "kernel": kernel, "torch_fp64": rule, "torch_over_kernel": rule["median_ms"] / kernel["median_ms"],
                          "counts_equal": bool(torch.equal(table[:, 0], other[:, 0])), "diag_err_over_bound": float(err), **common}), flush=True)

    torch.manual_seed(0)
    setups = [("reader", build_model("mrssm", (32, 32, 4, 4, 64), dev), (1, 32, 32), (1, 32, 32), DigitClassifier().to(dev)),
              ("encoder", bench.build_model(dev, "mrssm"), None, None, None)]
    for features, model, audio_shape, vision_shape, clf in setups:
        model.eval()
        if audio_shape is None:
            batch = bench.synthetic_batch(B, dev, seed=1000)
            batch = tuple(x[:, :T] for x in batch)
        else:
            action = torch.nn.functional.one_hot(torch.randint(0, 6, (B, T), device=dev, generator=gen), 6).float()
            audio, vision = (torch.rand(B, T, *shape, device=dev, generator=gen) * 2.0 - 1.0 for shape in (audio_shape, vision_shape))
            batch = (action, audio, vision, action, audio, vision)
        cfg = FrechetDistance(Q, samples=S, features=features)
        step = timed(lambda m=model, x=batch, c=cfg, r=clf: m.frechet_distance(x, c, r), args.steps, args.warmup)
        with torch.no_grad():
            rollout = timed(lambda m=model, x=batch, c=cfg: m._evaluation_rollout(x, c.plan(), None, None, None), args.steps, args.warmup)  # noqa: SLF001
            out, _ = model._evaluation_rollout(batch, cfg.plan(), None, None, None)  # noqa: SLF001
            feature = model._feature_of(out)  # noqa: SLF001
            per = max(1, cfg.max_frames // (S * T))
            chunks = [(r0, min(B, r0 + per)) for r0 in range(0, B, per)]
            reader = features == "reader"
            decode = timed(lambda: [model._decode_for_score(feature[r0 * S : r1 * S], audio=not reader) for r0, r1 in chunks],  # noqa: SLF001
                           args.steps, args.warmup)
            targets = model.get_targets_from_batch(batch)
            if reader:
                preds = [model._decode_for_score(feature[r0 * S : r1 * S], audio=False) for r0, r1 in chunks]  # noqa: SLF001
                embed = lambda: ([model._reader_features(clf, p[1], a[1]) for p, a in preds]  # noqa: E731, SLF001
                                 + [model._reader_features(clf, targets["recon/vision"][r0:r1], 0) for r0, r1 in chunks])  # noqa: SLF001
            else:
                preds = [model._decode_for_score(feature[r0 * S : r1 * S]) for r0, r1 in chunks]  # noqa: SLF001
                embed = lambda: ([model._encode_both(torch.tanh(p[0]).float(), torch.tanh(p[1]).float()) for p, _ in preds]  # noqa: E731, SLF001
                                 + [model._encode_both(targets["recon/audio"][r0:r1], targets["recon/vision"][r0:r1]) for r0, r1 in chunks])  # noqa: SLF001
            feats = timed(embed, args.steps, args.warmup)
            table = model.frechet_distance(batch, cfg, clf, keep_states=True)
            scratch = FrechetTable(table.streams, table.dim, table.bin_names, dev)
            fold = timed(lambda t=table, s=scratch: [FrechetDistance.fold(t.features[name][side], t.bins[side], j, s.block(name, side))
                                                     for name in t.streams for side in (0, 1)], args.steps, args.warmup)
        print(json.dumps({"metric": "ms per Frechet step and per stage", "features": features, "model": type(model).__name__, "batch": B, "steps_per_sequence": T,
                          "samples": S, "context": Q, "D": table.dim, "streams": table.streams, "step": step, "rollout": rollout, "decode": decode,
                          "features_ms": feats, "fold": fold, "fold_share_of_step": fold["median_ms"] / step["median_ms"],
                          "fd": {k: float(v) for k, v in table.scalars("frechet").items() if "/fd/" in k}, **common}), flush=True)


if __name__ == "__main__":
    main()
