#!/usr/bin/env python3
"""The latent census of a trained model: per latent level and categorical the code usage, perplexity, unused
classes, KL to the prior, whether it is active, the mutual information with the frame, the aggregate posterior's gap to the aggregate
prior, the switch rate and the dwell time of the sampled class -- plus, per observed subset after the first, its KL from the first
(`cross`).  Printed as text; `--json` writes the same numbers (and the usage per class and the curves by frame position) as JSON.

    python tools/latent_census.py --checkpoint model.ckpt --data-dir data/test [--observe both,audio,vision] [--active-nats 0.01] \\
        [--model mrssm|mmtrssm] [--dims 32,32,4,4,64] [--window 50] [--batch 64] [--seed 0] [--json census.json]

The data are the `.npz` episodes of `tools/word_transitions.py`; the model is built at `--dims deter,hidden,classes,cats,embed` and the
checkpoint loaded by parameter name, as in `tools/held_out_likelihood.py`.  Every episode is cut into windows of `--window` frames (a
shorter tail is kept and runs with its length); each batch of windows is one `model.latent_census` step into one `CensusTable`.
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

COLUMNS = ("perplexity", "unused", "kl", "active", "mi", "prior_gap", "switch_rate", "dwell")


def report(table) -> tuple[str, dict]:  # noqa: ANN001
    """The text and the JSON tree of a `CensusTable`."""
    per, usage, curves = table.per_categorical(), table.usage(), table.curves()
    lines, tree = [], {"observe": list(table.observe), "active_nats": table.active_nats, "steps": table.steps, "levels": {}}

    def clean(x: torch.Tensor):  # noqa: ANN202
        if x.dim():
            return [clean(v) for v in x]
        return float(x) if bool(torch.isfinite(x)) else (None if bool(torch.isnan(x)) else "inf")  # (a dwell time without a switch)

    for i, (name, k, c) in enumerate(table.levels):
        label = name or "latent"
        views = table.views(i)
        level = tree["levels"][label] = {"categoricals": k, "classes": c, "frames": clean(views["frames"]), "groups": {}}
        for g, subset in enumerate(table.observe):
            lines.append(f"level {label} ({k} categoricals of {c} classes), posterior observes {subset}: {int(views['frames'][g])} live frames\n")
            cols = COLUMNS + (("cross",) if g > 0 else ())
            lines.append("  k  " + "".join(f"{col:>12}" for col in cols) + "   usage\n")
            for j in range(k):
                row = "".join(f"{float(per[name][col][g, j]):12.4f}" for col in cols)
                lines.append(f"{j:3d}  {row}   " + " ".join(f"{float(u):.3f}" for u in usage[name][g, j]) + "\n")
            lines.append(f"     active {int(per[name]['active'][g].nansum())} of {k}, unused classes {int(per[name]['unused'][g].nansum())} of {k * c}\n\n")
            level["groups"][subset] = {**{col: clean(per[name][col][g]) for col in (*COLUMNS, "cross", "post_entropy", "prior_entropy")},
                                       "usage": clean(usage[name][g]), "by_position": {p: clean(x[g]) for p, x in curves[name].items()}}
    return "".join(lines), tree


def main() -> None:  # noqa: PLR0914
    ap = argparse.ArgumentParser(description="Code usage, entropies, KL and dwell times of a checkpoint's categorical latent")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--observe", default="both,audio,vision", help="comma-separated subsets out of both, audio, vision; the first is the reference of cross")
    ap.add_argument("--active-nats", type=float, default=0.01)
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the table as JSON to this file")
    args = ap.parse_args()
    if min(args.window, args.batch) < 1:
        ap.error("--window and --batch are >= 1")
    assert torch.cuda.is_available(), "latent_census.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from latent_probe import windows_of
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage
    from word_transitions import build_model, load_episodes

    try:
        census = mt.LatentCensus(tuple(args.observe.split(",")), args.active_nats)
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
    table = None

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
        noise = {k: torch.rand(shape, device=dev, generator=gen) for k, shape in census.noise_shapes(model, len(part), steps).items()}
        table = model.latent_census((action, audio, vision, action, audio, vision), census, noise, lengths, table)

    text, tree = report(table)
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    print(f"Latent census: {name}, {len(wins)} windows of up to {steps} frames, active above {args.active_nats} nats\n\n{text}", end="")
    if args.json:
        out = Path(args.json)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"model": args.model, "windows": len(wins), **tree}, indent=2))
        print(f"JSON in {out}")


if __name__ == "__main__":
    main()
