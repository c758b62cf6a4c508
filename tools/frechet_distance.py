#!/usr/bin/env python3
"""Sample realism by horizon: the Frechet distance between Gaussian fits of feature vectors of the real frames
and of the frames a trained model samples, per stream and horizon bin.

    python tools/frechet_distance.py --checkpoint model.ckpt --data-dir data/test [--classifier mnist_cnn.pt] [--query 10] [--samples 8] \\
        [--features reader|encoder] [--observe both|audio|vision] [--edges 1,2,4,8] [--model mrssm|mmtrssm] [--dims 32,32,4,4,64] \\
        [--window 50] [--batch 64] [--seed 0] [--json frechet.json]

The data are `.npz` episodes as for `tools/latent_census.py`; every episode is cut into windows of `--window` frames (a shorter tail
runs with its length) and each batch of windows is one `model.frechet_distance` step into one `FrechetTable`.  `--features reader`
embeds the vision frames with the digit classifier `tools/train_digit_classifier.py` writes (`--classifier`, required then);
`--features encoder` embeds both modalities with the model's own encoders.  Printed per stream and bin: the distance, its mean and
covariance parts, `tr Sigma_generated / tr Sigma_real` (below 1: blur or collapse) and the rows on either side.
"""

from __future__ import annotations

import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

COLUMNS = ("fd", "mean", "cov", "trace_ratio", "n_real", "n_generated")


def report(table) -> tuple[str, dict]:  # noqa: ANN001
    """The text and the JSON tree of a `FrechetTable`."""
    got = table.compute()
    lines, tree = [], {"features": table.dim, "bins": list(table.bin_names), "streams": {}}
    for stream in table.streams:
        lines.append(f"{stream} ({table.dim} features)\n  bin  " + "".join(f"{c:>14}" for c in COLUMNS) + "\n")
        tree["streams"][stream] = {}
        for j, name in enumerate(table.bin_names):
            row = {c: float(got[stream][c][j]) for c in COLUMNS}
            lines.append(f"{name:>5}  " + "".join(f"{row[c]:14.0f}" if c.startswith("n_") else f"{row[c]:14.5f}" for c in COLUMNS) + "\n")
            tree["streams"][stream][name] = {c: (None if math.isnan(v) else v) for c, v in row.items()}
        lines.append("\n")
    return "".join(lines), tree


def main() -> None:  # noqa: PLR0914
    ap = argparse.ArgumentParser(description="Frechet distance of sampled frames by horizon")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--classifier", default=None, help="state dict of the digit classifier (features=reader)")
    ap.add_argument("--query", type=int, default=10)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--features", choices=("reader", "encoder"), default="reader")
    ap.add_argument("--observe", choices=("both", "audio", "vision"), default="both")
    ap.add_argument("--edges", default="1,2,4,8")
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None, help="write the table as JSON to this file")
    args = ap.parse_args()
    if min(args.window, args.batch) < 1:
        ap.error("--window and --batch are >= 1")
    if args.features == "reader" and not args.classifier:
        ap.error("--features reader needs --classifier")
    assert torch.cuda.is_available(), "frechet_distance.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from latent_probe import windows_of
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage
    from word_transitions import build_model, load_episodes

    try:
        fd = mt.FrechetDistance(args.query, args.samples, args.observe, args.features, tuple(int(e) for e in args.edges.split(",")))
    except ValueError as e:
        ap.error(str(e))
    dev = "cuda:0"
    episodes = load_episodes(Path(args.data_dir))
    if not episodes:
        ap.error("no .npz episodes in --data-dir")
    model = build_model(args.model, tuple(int(x) for x in args.dims.split(",")), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    clf = None
    if args.features == "reader":
        clf = mt.DigitClassifier()
        clf.load_state_dict(torch.load(args.classifier, map_location="cpu", weights_only=True), strict=True)
        clf.to(dev)
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
        noise = {k: torch.rand(shape, device=dev, generator=gen) for k, shape in fd.noise_shapes(model, len(part), steps).items()}
        table = model.frechet_distance((action, audio, vision, action, audio, vision), fd, clf, noise, lengths, table)

    text, tree = report(table)
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    print(f"Frechet distance: {name}, {len(wins)} windows of up to {steps} frames, {fd!r}\n\n{text}", end="")
    if args.json:
        out = Path(args.json)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps({"model": args.model, "windows": len(wins), "config": repr(fd), **tree}, indent=2))
        print(f"JSON in {out}")


if __name__ == "__main__":
    main()
