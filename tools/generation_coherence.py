#!/usr/bin/env python3
"""Generation coherence of a trained model: do the generated image and the generated sound say the same digit,
and is it the right one -- per observed subset (`both`, `audio`, `vision`) and horizon, written as `<output>.md` and `<output>.json`.

    python tools/generation_coherence.py --checkpoint model.ckpt --vision-reader mnist_cnn.pt --audio-reader audio_cnn.pt \\
        --test-data-dir data/test [--model mrssm|mmtrssm] [--dims 32,32,4,4,64] [--context 30] [--steps 40] [--samples 10] \\
        [--observe both,audio,vision] [--stride N] [--batch 16] [--seed 0] [--output results/coherence]

The test data are `.npz` episodes as for `tools/word_transitions.py` (`audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `label (T,)` with -1 =
silence, `speaker (T, 6)` one-hot), fed to the model the same way.  Every episode is cut into windows of `--steps` frames, one every
`--stride` frames (default: `--steps`, windows that do not overlap; a tail shorter than `--steps` is dropped); the windows run in batches
of `--batch` through `model.generation_coherence` into ONE `CoherenceTable`: the first `--context` frames of a window are observed (by the
copies of group `audio`: the sound only ...), the rest is generated open loop, `--samples` futures per subset.  The readers are state
dicts of the digit classifier: `tools/train_digit_classifier.py` writes the vision reader, and with `--modality audio` the audio reader
(fit both on frames of the TRAINING episodes, normalised as the model sees them).

Per subset the report holds the five rates (`vision`, `audio`: the decode reads as the frame's label; `agree`: both decodes read the
same digit; `joint`: ... and it is the label; `soft`: sum_k p_vision(k) p_audio(k)) over the horizon bins `obs h1 h2 h4 h8`, Cohen's kappa
of the two readers per phase, the share of failed reads and the 10 x 10 agreement matrix (rows: the digit seen, columns: the digit
heard) of the open-loop phase."""

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

from word_transitions import build_model, load_episodes  # noqa: E402  (the evaluation's episodes and model)

MAX_SAMPLES = 16
BINS = ("obs", "h1", "h2", "h4", "h8")


def windows(lengths: list[int], steps: int, stride: int) -> list[tuple[int, int]]:
    """``(episode, start)`` of every whole window of ``steps`` frames, one every ``stride`` frames."""
    return [(e, s) for e, n in enumerate(lengths) for s in range(0, n - steps + 1, stride)]


def _num(x: torch.Tensor) -> float | None:
    v = float(x)
    return None if v != v else v  # noqa: PLR0124  (NaN: nothing was counted)


def report(table, name: str, context: int, samples: int, n_windows: int) -> tuple[str, dict]:  # noqa: ANN001
    """The text and the JSON tree of a ``CoherenceTable``."""
    from multimodal_mtrssm_amd.coherence import PHASES, PLANES

    views = table.views()
    tree: dict = {"model": name, "context": context, "samples": samples, "steps": table.steps, "windows": n_windows, "observe": list(table.observe),
                  "reads": float(views["counts"].sum()), "groups": {}}
    lines = [f"# Generation coherence: {name}", "",
             f"{n_windows} windows of {table.steps} frames, {context} observed, {samples} sampled futures per subset; "
             f"{int(tree['reads'])} copy-frames read.", ""]
    fmt = lambda v: "  n/a " if v is None else f"{v:6.3f}"  # noqa: E731
    for g, subset in enumerate(table.observe):
        binned = {plane: [_num(x) for x in row] for plane, row in table.binned(g).items()}
        kappa = {phase: _num(table.kappa(g, i)) for i, phase in enumerate(PHASES)}
        failed = {m: {phase: _num(x[i]) for i, phase in enumerate(PHASES)} for m, x in table.failed(g).items()}
        matrix = views["pairs"][g, 1, :10, :10].cpu().tolist()
        tree["groups"][subset] = {"rates": {plane: dict(zip(BINS, row, strict=True)) for plane, row in binned.items()}, "kappa": kappa,
                                  "failed": failed, "open_loop_pairs": matrix, "by_horizon": {p: [_num(x) for x in r] for p, r in table.rates(g).items()}}
        lines += [f"## Observed: {subset}", "", "| rate | " + " | ".join(BINS) + " |", "|---|" + "---|" * len(BINS)]
        lines += [f"| {plane} | " + " | ".join(fmt(v) for v in binned[plane]) + " |" for plane in PLANES]
        lines += ["", f"Cohen's kappa of the two readers: observed {fmt(kappa['obs']).strip()}, open loop {fmt(kappa['open']).strip()}.  Failed reads "
                      f"(vision / audio): observed {fmt(failed['vision']['obs']).strip()} / {fmt(failed['audio']['obs']).strip()}, open loop "
                      f"{fmt(failed['vision']['open']).strip()} / {fmt(failed['audio']['open']).strip()}.", "",
                  "Open loop, digit seen (rows) against digit heard (columns):", "", "| | " + " | ".join(str(d) for d in range(10)) + " |",
                  "|---|" + "---|" * 10]
        lines += [f"| {d} | " + " | ".join(str(int(n)) for n in row) + " |" for d, row in enumerate(matrix)]
        lines.append("")
    return "\n".join(lines), tree


def main() -> None:  # noqa: PLR0914
    ap = argparse.ArgumentParser(description="Generation coherence: both decodes read as digits")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--vision-reader", required=True, help="state dict of the digit classifier fitted on image frames")
    ap.add_argument("--audio-reader", required=True, help="state dict of the digit classifier fitted on audio frames (--modality audio)")
    ap.add_argument("--test-data-dir", required=True)
    ap.add_argument("--output", default="results/coherence")
    ap.add_argument("--model", choices=("mrssm", "mmtrssm"), default="mrssm")
    ap.add_argument("--dims", default="32,32,4,4,64", help="deter,hidden,classes,cats,embed")
    ap.add_argument("--context", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--observe", default="both,audio,vision")
    ap.add_argument("--stride", type=int, default=None, help="frames between window starts (default: --steps)")
    ap.add_argument("--batch", type=int, default=16, help="windows per step")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not 1 <= args.samples <= MAX_SAMPLES:
        ap.error(f"--samples in 1 .. {MAX_SAMPLES} (the futures of one rollout)")
    stride = args.steps if args.stride is None else args.stride
    if args.steps < 1 or stride < 1 or args.batch < 1 or args.context < 1:
        ap.error("--steps, --stride, --batch and --context are at least 1")
    assert torch.cuda.is_available(), "generation_coherence.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage

    dev = "cuda:0"
    try:
        gc = mt.GenerationCoherence(args.context, samples=args.samples, observe=tuple(args.observe.split(",")))
    except ValueError as e:
        ap.error(str(e))
    episodes = load_episodes(Path(args.test_data_dir))
    if not episodes:
        ap.error(f"no .npz episodes in {args.test_data_dir}")
    steps = args.steps
    wins = windows([len(e["label"]) for e in episodes], steps, stride)
    if not wins:
        ap.error(f"no episode holds a window of {steps} frames")
    model = build_model(args.model, tuple(int(x) for x in args.dims.split(",")), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    readers = {}
    for name, path in (("vision", args.vision_reader), ("audio", args.audio_reader)):
        readers[name] = mt.DigitClassifier()
        readers[name].load_state_dict(torch.load(path, map_location="cpu", weights_only=True), strict=True)
        readers[name].to(dev)
    audio_t, vision_t = NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), NormalizeVisionImage()
    cut = lambda key, e, s: torch.from_numpy(np.asarray(episodes[e][key][s : s + steps])).float()  # noqa: E731
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    table = mt.CoherenceTable(gc.groups, steps, dev, gc.observe)
    for i in range(0, len(wins), args.batch):
        part = wins[i : i + args.batch]
        audio = torch.stack([audio_t(cut("audio", e, s).reshape(steps, 1, 32, 32)) for e, s in part]).to(dev)
        vision = torch.stack([vision_t(cut("image", e, s).reshape(steps, 1, 32, 32)) for e, s in part]).to(dev)
        action = torch.stack([cut("speaker", e, s) for e, s in part]).to(dev)
        labels = torch.stack([torch.from_numpy(np.asarray(episodes[e]["label"][s : s + steps]).astype(np.int32)) for e, s in part]).to(dev)
        noise = {k: torch.rand(shape, device=dev, generator=gen) for k, shape in gc.noise_shapes(model, len(part), steps).items()}
        model.generation_coherence((action, audio, vision, action, audio, vision), labels, gc, readers, noise, table=table)
    name = "MoPoE-MMTRSSM" if args.model == "mmtrssm" else "MoPoE-MRSSM"
    text, tree = report(table, name, args.context, args.samples, len(wins))
    tree["scalars"] = {k: _num(v) for k, v in table.scalars("coherence").items()}
    out = Path(args.output)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.with_suffix(".md").write_text(text)
    out.with_suffix(".json").write_text(json.dumps(tree, indent=2))
    print(f"{len(wins)} windows x {gc.groups} subsets x {args.samples} futures; results in {out.with_suffix('.md')} and {out.with_suffix('.json')}")


if __name__ == "__main__":
    main()
