#!/usr/bin/env python3
"""Word-to-word transition evaluation: the matching rate of sampled futures per spoken digit, next to the
uniform / peak one-hot / random one-hot baselines, written as `<output>.md` and `<output>.json`.

    python tools/word_transitions.py --checkpoint model.ckpt --classifier-checkpoint mnist_cnn.pt --test-data-dir data/test \\
        [--model mrssm|mmtrssm] [--protocol reference|context] [--n-intervals 6] [--n-predictions 10] [--n-frames 10] [--query-length 30]

The flags are the evaluation script's.  For every word 0 .. 9 one interval of `--query-length` frames per speaker is selected (ending
at the word's first occurrence in an episode); ALL words' intervals x predictions run as ONE batch through
`model.word_transitions`; p(w | wa) comes from the label sequences of all episodes.  `--protocol reference` (default) is the script's
own procedure: frame 0 of the interval gives the initial state, the last action is repeated, the first predicted frame is read (so
`--n-frames` changes nothing but is accepted).  `--protocol context` observes the whole interval and reads the next frame.

The test data are `.npz` episodes with `audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `label (T,)` (-1 = silence) and `speaker (T, 6)`
one-hot.  The model is built at `--dims deter,hidden,classes,cats,embed` (default: the reference's default.yaml) and the checkpoint is
loaded by parameter name.  The classifier checkpoint is a state dict of the evaluation's classifier: `tools/train_digit_classifier.py`
writes one from the labelled frames of such episodes, and one trained by the evaluation itself loads as well.
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

MAX_SAMPLES = 16


def load_episodes(folder: Path) -> list[dict[str, np.ndarray]]:
    episodes = []
    for path in sorted(folder.glob("*.npz")):
        with np.load(path, allow_pickle=False) as z:
            episodes.append({k: z[k] for k in ("audio", "image", "label", "speaker")})
    return episodes


def build_model(kind: str, dims: tuple[int, ...], device: str):  # noqa: ANN201
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.factory import decoder_config, encoder_config

    deter, hidden, classes, cats, embed = dims
    frame = (1, 32, 32)
    enc = {"enc_audio": encoder_config(frame, embed), "enc_vision": encoder_config(frame, embed)}
    if kind == "mmtrssm":
        feat = 2 * (deter + classes * cats)
        model = mt.make_mmtrssm(hd=deter, hs=(classes, cats), ld=deter, ls=(classes, cats), hidden=hidden, action=6, embed=embed, **enc,
                                dec_audio=decoder_config(feat, frame), dec_vision=decoder_config(feat, frame))
    else:
        feat = deter + classes * cats
        model = mt.make_mrssm(deter=deter, hidden=hidden, classes=classes, cats=cats, action=6, embed=embed, **enc,
                              dec_audio=decoder_config(feat, frame), dec_vision=decoder_config(feat, frame))
    return model.to(device)


def main() -> None:
    ap = argparse.ArgumentParser(description="Word-to-word transition matching rate")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--classifier-checkpoint", required=True, help="state dict of the digit classifier")
    ap.add_argument("--test-data-dir", required=True)
    ap.add_argument("--output", default="results/word_transitions")
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--protocol", choices=("reference", "context"), default="reference")
    ap.add_argument("--n-intervals", type=int, default=6)
    ap.add_argument("--n-predictions", type=int, default=10)
    ap.add_argument("--n-frames", type=int, default=10)
    ap.add_argument("--query-length", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not 1 <= args.n_predictions <= MAX_SAMPLES:
        ap.error(f"--n-predictions in 1 .. {MAX_SAMPLES} (the futures of one rollout)")
    assert torch.cuda.is_available(), "word_transitions.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import words
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage

    dev = "cuda:0"
    torch.manual_seed(args.seed)
    episodes = load_episodes(Path(args.test_data_dir))
    if not episodes:
        ap.error(f"no .npz episodes in {args.test_data_dir}")
    labels = [e["label"] for e in episodes]
    speakers = [int(np.argmax(e["speaker"][0])) for e in episodes]
    q = args.query_length
    context = args.protocol == "context"
    rows = []  # (word, episode, start): every word's intervals side by side
    for word in words.WORDS:
        for iv in words.select_intervals(labels, speakers, word, args.n_intervals, q):
            if iv["end"] + (1 if context else 0) <= len(labels[iv["file_idx"]]):
                rows.append((word, iv["file_idx"], iv["start"]))
    model = build_model(args.model, tuple(int(x) for x in args.dims.split(",")), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    clf = mt.DigitClassifier()
    clf.load_state_dict(torch.load(args.classifier_checkpoint, map_location="cpu", weights_only=True), strict=True)
    clf.to(dev)
    table = mt.TransitionTable(q + (1 if context else 0), dev)
    if rows:
        steps = table.steps
        audio_t, vision_t = NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), NormalizeVisionImage()
        cut = lambda key, e, s: torch.from_numpy(np.asarray(episodes[e][key][s : s + steps])).float()  # noqa: E731
        audio = torch.stack([audio_t(cut("audio", e, s).reshape(steps, 1, 32, 32)) for _, e, s in rows]).to(dev)
        vision = torch.stack([vision_t(cut("image", e, s).reshape(steps, 1, 32, 32)) for _, e, s in rows]).to(dev)
        action = torch.stack([cut("speaker", e, s) for _, e, s in rows]).to(dev)
        # the row's current word is the word it was selected for (the interval ends at it, or holds it when it comes early)
        lab = torch.full((len(rows), steps), -1, dtype=torch.int32)
        lab[:, q - 1] = torch.tensor([w for w, _, _ in rows], dtype=torch.int32)
        wt = mt.WordTransitions(q, samples=args.n_predictions, protocol=args.protocol)
        model.word_transitions((action, audio, vision, action, audio, vision), lab.to(dev), wt, clf, table=table)
    results = words.results_from_table(table, labels)
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.with_suffix(".md").write_text("# Word-to-word Transition Evaluation Results\n\n" + words.format_results_table(results, model_name=name))
    out.with_suffix(".json").write_text(json.dumps(results, indent=2))
    print(f"{len(rows)} intervals x {args.n_predictions} predictions in one batch; results in {out.with_suffix('.md')} and {out.with_suffix('.json')}")


if __name__ == "__main__":
    main()
