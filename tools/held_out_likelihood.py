#!/usr/bin/env python3
"""Held-out likelihood of a trained model (DESIGN.md sections 6k and 6q): the importance-weighted bound of whole sampled trajectories
and the particle filter's bound, which weights per frame and resamples in time, side by side in nats per frame, printed and written as
`<output>.md` and `<output>.json`.

    python tools/held_out_likelihood.py --checkpoint model.ckpt --data-dir data/test [--samples 16] [--resample-every 5] \\
        [--threshold 0.5] [--model mrssm|mmtrssm] [--dims 32,32,4,4,64] [--window 50] [--batch 64] [--observe both] [--seed 0]

The data are the `.npz` episodes of `tools/word_transitions.py` (`audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `speaker (T, 6)` one-hot);
the model is built at `--dims deter,hidden,classes,cats,embed` and the checkpoint loaded by parameter name, as there.  Every episode is
cut into windows of `--window` frames (a shorter tail is kept and runs with its length).  Each batch of windows runs
`model.likelihood_bound` and `model.particle_filter` under the SAME initial and posterior uniforms, so at `--threshold 0` the two `smc`
and `iw` columns agree; both tables are folded by frame position over all windows.  The `.json` also holds the curves by position.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def main() -> None:  # noqa: PLR0914
    ap = argparse.ArgumentParser(description="Importance-weighted and particle-filter bounds on held-out episodes")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--output", default="results/held_out_likelihood")
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--resample-every", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--observe", choices=("both", "audio", "vision"), default="both")
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if min(args.window, args.batch) < 1:
        ap.error("--window and --batch are >= 1")
    assert torch.cuda.is_available(), "held_out_likelihood.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from latent_probe import windows_of
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage
    from word_transitions import build_model, load_episodes

    try:
        bound = mt.LikelihoodBound(args.samples, args.observe)
        pf = mt.ParticleFilter(args.samples, args.resample_every, args.threshold, args.observe)
    except ValueError as e:
        ap.error(str(e))
    dev = "cuda:0"
    episodes = load_episodes(Path(args.data_dir))
    if not episodes:
        ap.error("no .npz episodes in --data-dir")
    model = build_model(args.model, tuple(int(x) for x in args.dims.split(",")), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    audio_t, vision_t = NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), NormalizeVisionImage()
    steps = args.window
    wins = windows_of(episodes, steps)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    iw_table, smc_table = mt.LikelihoodTable(steps, dev), mt.ParticleTable(steps, dev)

    def cut(key: str, e: int, s: int, n: int, *shape: int) -> torch.Tensor:
        out = torch.zeros(steps, *shape)
        out[:n] = torch.from_numpy(np.asarray(episodes[e][key][s : s + n])).float().reshape(n, *shape)
        return out

    for i in range(0, len(wins), args.batch):
        part = wins[i : i + args.batch]
        audio = torch.stack([audio_t(cut("audio", e, s, n, 1, 32, 32)) for e, s, n in part]).to(dev)
        vision = torch.stack([vision_t(cut("image", e, s, n, 1, 32, 32)) for e, s, n in part]).to(dev)
        action = torch.stack([cut("speaker", e, s, n, 6) for e, s, n in part]).to(dev)
        lengths = torch.tensor([n for _, _, n in part], dtype=torch.int32, device=dev)
        batch = (action, audio, vision, action, audio, vision)
        noise = {k: torch.rand(shape, device=dev, generator=gen) for k, shape in pf.noise_shapes(model, len(part), steps).items()}
        model.likelihood_bound(batch, bound, {k: v for k, v in noise.items() if k != "u_resample"}, lengths, iw_table)
        model.particle_filter(batch, pf, noise, lengths, smc_table)

    iw, smc = iw_table.per_frame(), smc_table.per_frame()
    frames = float(iw_table.counts.sum())
    rows = [("bound", float(iw["iw"]), float(smc["smc"])), ("mean of the samples (ELBO)", float(iw["elbo"]), float(smc["mean"])),
            ("audio", float(iw["audio"]), float(smc["audio"])), ("vision", float(iw["vision"]), float(smc["vision"])),
            ("latent", float(iw["latent"]), float(smc["latent"])), ("effective sample size", float(iw["ess"]), float(smc["ess"]))]
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    lines = [f"# Held-out likelihood: {name}\n\n",
             f"Nats per frame over {int(frames)} frames of {len(wins)} windows; S = {args.samples} samples per window, the posterior observes "
             f"{args.observe}; the particle filter resamples every {args.resample_every} frames where ESS <= {args.threshold} S "
             f"(after {float(smc['resampled']):.4f} of the frames).\n\n",
             "| | importance-weighted (6k) | particle filter (6q) |\n", "|---|---|---|\n"]
    lines += [f"| {what} | {a:.4f} | {b:.4f} |\n" for what, a, b in rows]
    print("".join(lines))
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.with_suffix(".md").write_text("".join(lines))

    def listed(curves: dict[str, torch.Tensor]) -> dict[str, list[float | None]]:
        return {k: [None if x != x else x for x in v.tolist()] for k, v in curves.items()}  # noqa: PLR0124  (NaN: an empty bin)

    out.with_suffix(".json").write_text(json.dumps({
        "samples": args.samples, "resample_every": args.resample_every, "threshold": args.threshold, "observe": args.observe, "frames": frames,
        "windows": len(wins), "iw": {k: float(v) for k, v in iw_table.scalars("loglik").items()},
        "smc": {k: float(v) for k, v in smc_table.scalars("smc").items()}, "iw_by_position": listed(iw_table.curves()),
        "smc_by_position": listed(smc_table.curves())}, indent=2))
    print(f"results in {out.with_suffix('.md')} and {out.with_suffix('.json')}")


if __name__ == "__main__":
    main()
