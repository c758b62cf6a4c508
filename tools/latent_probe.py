#!/usr/bin/env python3
"""Latent quality: linear word probes on the subset posteriors of a trained model -- the accuracy with which a
linear classifier reads the spoken digit out of the latent of the posterior that observes both modalities, audio only or vision only,
per part of the feature, written as `<output>.md` and `<output>.json`.

    python tools/latent_probe.py --checkpoint model.ckpt --train-data-dir data/train --test-data-dir data/test \\
        [--model mrssm|mmtrssm] [--dims 32,32,4,4,64] [--window 50] [--batch 64] [--fit-steps 300] [--lr 1e-2] [--weight-decay 0]

The data are the `.npz` episodes of `tools/word_transitions.py` (`audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `label (T,)` with
-1 = silence, `speaker (T, 6)` one-hot); the model is built at `--dims deter,hidden,classes,cats,embed` and the checkpoint loaded by
parameter name, as there.  Every episode is cut into windows of `--window` frames (a shorter tail is kept and runs with its length).
`model.probe_features` gives the features of the three posteriors of every window ONCE; they are cached on the device and every
part of the feature (`feature`, `deter`, `stoch`; MMTRSSM: `feature`, `higher`, `lower`) is probed in place: `LinearProbe.fit` on the
training windows (`--fit-steps` full-batch AdamW iterations), one evaluation-only step on the test windows.  Silent frames carry no
label and are skipped.  The `.json` also holds the accuracy by frame position inside a window.
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


def windows_of(episodes: list[dict[str, np.ndarray]], steps: int) -> list[tuple[int, int, int]]:
    """``(episode, start, length)`` of every window: consecutive runs of ``steps`` frames, the tail kept with its own length."""
    return [(e, s, min(steps, len(ep["label"]) - s)) for e, ep in enumerate(episodes) for s in range(0, len(ep["label"]), steps)]


def features_of(model, probe, episodes: list[dict[str, np.ndarray]], steps: int, batch: int, dev: str):  # noqa: ANN001, ANN201
    """``x [G, N, Ffull]`` and ``labels [N]`` (int32, -1 on silent frames and past a window's end) of all windows, on the device, and the
    windows' ``(labels [W, steps], lengths [W])`` for the fold by position."""
    from multimodal_mtrssm_amd.probe import frame_labels
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage

    audio_t, vision_t = NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), NormalizeVisionImage()
    wins = windows_of(episodes, steps)
    xs, labs = [], []

    def cut(key: str, e: int, s: int, n: int, *shape: int) -> torch.Tensor:
        out = torch.zeros(steps, *shape)
        out[:n] = torch.from_numpy(np.asarray(episodes[e][key][s : s + n])).float().reshape(n, *shape)
        return out

    for i in range(0, len(wins), batch):
        part = wins[i : i + batch]
        audio = torch.stack([audio_t(cut("audio", e, s, n, 1, 32, 32)) for e, s, n in part]).to(dev)
        vision = torch.stack([vision_t(cut("image", e, s, n, 1, 32, 32)) for e, s, n in part]).to(dev)
        action = torch.stack([cut("speaker", e, s, n, 6) for e, s, n in part]).to(dev)
        lab = torch.full((len(part), steps), -1, dtype=torch.int32)
        for j, (e, s, n) in enumerate(part):
            lab[j, :n] = torch.from_numpy(np.asarray(episodes[e]["label"][s : s + n])).to(torch.int32)
        lengths = torch.tensor([n for _, _, n in part], dtype=torch.int32, device=dev)
        x, valid = model.probe_features((action, audio, vision, action, audio, vision), probe, None, lengths)
        xs.append(x.reshape(x.shape[0], len(part) * steps, -1))
        labs.append(frame_labels(lab.to(dev), valid))
    return torch.cat(xs, dim=1).contiguous(), torch.cat(labs).contiguous()


def main() -> None:
    ap = argparse.ArgumentParser(description="Linear word probes on subset posteriors")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--train-data-dir", required=True)
    ap.add_argument("--test-data-dir", required=True)
    ap.add_argument("--output", default="results/latent_probe")
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--fit-steps", type=int, default=300)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--weight-decay", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if min(args.window, args.batch, args.fit_steps) < 1:
        ap.error("--window, --batch and --fit-steps are >= 1")
    assert torch.cuda.is_available(), "latent_probe.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from word_transitions import build_model, load_episodes

    dev = "cuda:0"
    torch.manual_seed(args.seed)
    train, test = load_episodes(Path(args.train_data_dir)), load_episodes(Path(args.test_data_dir))
    if not train or not test:
        ap.error("no .npz episodes in --train-data-dir or --test-data-dir")
    model = build_model(args.model, tuple(int(x) for x in args.dims.split(",")), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    probe = mt.LatentProbe()
    x_train, y_train = features_of(model, probe, train, args.window, args.batch, dev)
    x_test, y_test = features_of(model, probe, test, args.window, args.batch, dev)
    results: dict[str, dict[str, object]] = {}
    for part, (col0, width) in mt.LatentProbe.layout(model).items():
        linear = mt.LinearProbe(probe.groups, width, 10).to(dev)
        linear.fit(x_train, y_train, args.fit_steps, lr=args.lr, weight_decay=args.weight_decay, col0=col0)
        fitted = linear.step(x_train, y_train, col0=col0, grad=False)
        stats = linear.step(x_test, y_test, col0=col0, grad=False, planes=True)
        w = x_test.shape[1] // args.window
        live = ((y_test >= 0) & (y_test < linear.classes)).reshape(w, args.window)
        table = mt.ProbeTable(probe.groups, args.window, dev, probe.observe)
        table.fold(stats.hit.reshape(-1, w, args.window), stats.nll.reshape(-1, w, args.window), live)
        curves = table.curves()
        results[part] = {
            "columns": [col0, width], "test_frames": float(stats.count[0]), "train_frames": float(fitted.count[0]),
            **{name: {"acc": float(stats.hits[i] / stats.count[i].clamp_min(1.0)), "nll": float(stats.nll_sum[i] / stats.count[i].clamp_min(1.0)),
                      "train_acc": float(fitted.hits[i] / fitted.count[i].clamp_min(1.0)),
                      "acc_by_position": [None if v != v else v for v in curves[name]["acc"].tolist()]}  # noqa: PLR0124  (NaN: an empty bin)
               for i, name in enumerate(probe.observe)}}
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    lines = [f"# Linear word probes: {name}\n\n", "Test accuracy of a linear classifier on the posterior's latent (rows: what the posterior observes).\n\n",
             "| Observes | " + " | ".join(results) + " |\n", "|---|" + "---|" * len(results) + "\n"]
    lines += ["| " + subset + " | " + " | ".join(f"{results[p][subset]['acc']:.4f}" for p in results) + " |\n" for subset in probe.observe]
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.with_suffix(".md").write_text("".join(lines))
    out.with_suffix(".json").write_text(json.dumps(results, indent=2))
    print(f"{x_train.shape[1]} training and {x_test.shape[1]} test frames; results in {out.with_suffix('.md')} and {out.with_suffix('.json')}")


if __name__ == "__main__":
    main()
