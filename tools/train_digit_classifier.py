#!/usr/bin/env python3
"""Train the digit reader on the labelled frames of the evaluation's own episodes and save the state dict that
`tools/word_transitions.py --classifier-checkpoint` loads.

    python tools/train_digit_classifier.py --data-dir data/train --output mnist_cnn.pt [--epochs 5] [--batch-size 64] [--holdout 0.1]
        [--seed 0] [--lr 1e-3] [--dropout 0.5] [--device cuda:0]

The data are `.npz` episodes with `image (T, 1, 32, 32)` in [0, 255] and `label (T,)` (-1 = silence).  Every labelled frame goes through
`NormalizeVisionImage` (the decoder's target range, read with `act = 0`); a seeded `--holdout` share of them is kept out of the fit and
its accuracy printed after every epoch.  The recipe is the evaluation's: Adam at 1e-3, batches of 64, `Dropout(0.5)`, cross-entropy,
5 epochs.  On the GPU every step runs the HIP kernels; `--device cpu` runs the float64 rule (slow: for small sets).

`--modality audio` fits the reader of the AUDIO decode instead (`tools/generation_coherence.py --audio-reader`): the
frames are `audio (T, 32, 32)` mel spectrograms next to the same `label`, mapped through `NormalizeAudioMelSpectrogram(--audio-min,
--audio-max)` (default -80 and 0, the values `tools/word_transitions.py` feeds the model with) to the decoder's target range."""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def load_labelled_frames(folder: Path, modality: str = "vision", audio_min: float = -80.0, audio_max: float = 0.0) -> tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``[N, 1024]`` raw frames in [-1, 1] and int32 ``[N]`` digits of every labelled frame of every episode: ``image`` frames
    through ``NormalizeVisionImage``, or (``modality="audio"``) ``audio`` frames through ``NormalizeAudioMelSpectrogram(audio_min,
    audio_max)``."""
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage

    if modality not in ("vision", "audio"):
        msg = f"modality must be 'vision' or 'audio', got {modality!r}"
        raise ValueError(msg)
    key, shape = ("image", "(T, 1, 32, 32)") if modality == "vision" else ("audio", "(T, 32, 32)")
    frames, labels = [], []
    for path in sorted(folder.glob("*.npz")):
        with np.load(path, allow_pickle=False) as z:
            image, label = np.asarray(z[key]), np.asarray(z["label"]).astype(np.int64)
        if modality == "vision":
            bad = image.shape[0] != label.shape[0] or image.reshape(image.shape[0], -1).shape[1] != 1024  # noqa: PLR2004
        else:
            bad = image.ndim != 3 or image.shape[0] != label.shape[0] or tuple(image.shape[1:]) != (32, 32)  # noqa: PLR2004
        if bad:
            msg = f"{path}: {key} {image.shape} and label {label.shape} are not {shape} and (T,)"
            raise ValueError(msg)
        keep = (label >= 0) & (label < 10)  # noqa: PLR2004
        frames.append(torch.from_numpy(image[keep]).float().reshape(-1, 1024))
        labels.append(torch.from_numpy(label[keep]).to(torch.int32))
    if not frames:
        msg = f"no .npz episodes in {folder}"
        raise ValueError(msg)
    transform = NormalizeVisionImage() if modality == "vision" else NormalizeAudioMelSpectrogram(min_value=audio_min, max_value=audio_max)
    return transform(torch.cat(frames)), torch.cat(labels)


def main() -> None:
    ap = argparse.ArgumentParser(description="Train the digit classifier on episode frames")
    ap.add_argument("--data-dir", required=True, help="folder of .npz episodes (image, label)")
    ap.add_argument("--output", default="mnist_cnn.pt")
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--holdout", type=float, default=0.1, help="share of the labelled frames kept out of the fit")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--modality", choices=("vision", "audio"), default="vision", help="which frames the reader is fitted on")
    ap.add_argument("--audio-min", type=float, default=-80.0, help="--modality audio: the spectrogram value mapped to -1")
    ap.add_argument("--audio-max", type=float, default=0.0, help="--modality audio: the spectrogram value mapped to +1")
    args = ap.parse_args()
    if not 0.0 <= args.holdout < 1.0:
        ap.error("--holdout lies in [0, 1)")
    if args.device.startswith("cuda"):
        assert torch.cuda.is_available(), "train_digit_classifier.py runs its kernels on the MI355X (--device cpu: the float64 rule)"

    import multimodal_mtrssm_amd as mt

    frames, labels = load_labelled_frames(Path(args.data_dir), args.modality, args.audio_min, args.audio_max)
    n = frames.shape[0]
    order = torch.randperm(n, generator=torch.Generator().manual_seed(args.seed))
    held = int(round(args.holdout * n))
    test, train = order[:held], order[held:]
    if train.numel() == 0:
        ap.error(f"{n} labelled frames leave nothing to fit on at --holdout {args.holdout}")
    print(f"{n} labelled frames: {train.numel()} to fit on, {held} held out; digits {torch.bincount(labels.long(), minlength=10).tolist()}")
    torch.manual_seed(args.seed)
    clf = mt.DigitClassifier()
    for layer in (clf.conv1, clf.conv2, clf.fc1, clf.fc2):  # (the constructor's torch initialisation, under the seed)
        layer.reset_parameters()
    clf.to(args.device)
    x_train, y_train = frames[train].to(args.device), labels[train].to(args.device)
    x_test, y_test = frames[test].to(args.device), labels[test].to(args.device)
    with mt.DigitTrainer(clf, lr=args.lr, dropout=args.dropout, seed=args.seed) as trainer:
        for epoch in range(1, args.epochs + 1):
            fit = trainer.fit(x_train, y_train, epochs=1, batch_size=args.batch_size, act=0)
            line = f"epoch {epoch}: train loss {float(fit.nll_sum) / max(float(fit.count), 1.0):.4f} acc {float(fit.hits) / max(float(fit.count), 1.0):.4f}"
            if held:
                ev = trainer.evaluate(x_test, y_test, act=0)
                line += f"; held-out loss {float(ev.nll_sum) / float(ev.count):.4f} acc {float(ev.hits) / float(ev.count):.4f}"
            print(line, flush=True)
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in clf.state_dict().items()}, out)
    check = mt.DigitClassifier()
    check.load_state_dict(torch.load(out, map_location="cpu", weights_only=True), strict=True)
    print(f"saved {out} ({sum(v.numel() for v in check.state_dict().values())} parameters; loads with strict=True)")


if __name__ == "__main__":
    main()
