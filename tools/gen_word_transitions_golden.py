#!/usr/bin/env python3
"""Regenerate ``tests/golden/word_transitions.npz``: the results of the reference evaluation's pure bookkeeping functions on seeded
label sequences.

    python tools/gen_word_transitions_golden.py --reference <checkout of the reference project> [--out tests/golden/word_transitions.npz]

The reference's ``evaluation/evaluate_word_transitions_mrssm.py`` is imported by path at run time; nothing of it is copied here.  Its
module-level imports that this machine may lack or that pull in the whole model package (``torchvision``, ``hydra``, its own
``multimodal_rssm`` model and transform modules) are stubbed in ``sys.modules``: the four functions that are run --
``compute_true_distribution``, ``compute_matching_rate``, ``select_intervals_for_word``, ``compute_prediction_distribution`` (and
``compute_baselines`` for its two deterministic entries) -- touch none of them.  The fixture holds inputs and outputs only.
"""

from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import sys
import types
from pathlib import Path

import numpy as np

WORDS = list(range(10))
QUERY, N_INTERVALS = 12, 4
PAD = -9


def _stub(name: str, **attrs: object) -> None:
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sub = ".".join(parts[:i])
        if sub not in sys.modules:
            mod = types.ModuleType(sub)
            mod.__path__ = []  # type: ignore[attr-defined]
            sys.modules[sub] = mod
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference(root: Path) -> types.ModuleType:
    _stub("torchvision", datasets=types.SimpleNamespace(), transforms=types.SimpleNamespace())
    _stub("torchvision.datasets")
    _stub("torchvision.transforms")
    _stub("hydra.utils", instantiate=None)
    _stub("multimodal_rssm.models.mrssm.mopoe_mrssm.core", MoPoE_MRSSM=object)
    _stub("multimodal_rssm.models.transform", NormalizeAudioMelSpectrogram=object, NormalizeVisionImage=object)
    sys.path.insert(0, str(root))
    spec = importlib.util.spec_from_file_location("reference_word_transitions", root / "evaluation" / "evaluate_word_transitions_mrssm.py")
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)  # type: ignore[union-attr]
    return module


def seeded_labels(rng: np.random.Generator, episodes: int, frames: int) -> np.ndarray:
    """Runs of a digit (3 .. 9 frames) separated by silence (0 .. 4 frames); now and then the same digit returns after a silence."""
    out = np.full((episodes, frames), -1, dtype=np.int64)
    for e in range(episodes):
        t, prev = int(rng.integers(0, 4)), -1
        while t < frames:
            digit = prev if prev >= 0 and rng.random() < 0.15 else int(rng.integers(0, 10))  # noqa: PLR2004
            run = int(rng.integers(3, 10))
            out[e, t : t + run] = digit
            t += run + int(rng.integers(0, 5))
            prev = digit
    return out


def edge_labels(frames: int) -> np.ndarray:
    out = np.full((5, frames), -1, dtype=np.int64)  # episode 0: all silence
    out[1, 2:5], out[1, 7:9], out[1, 9:14] = 3, 3, 5  # a repeated word separated by silence collapses: 3 5
    out[2, :] = 7                                     # one word, no successor
    out[3, 0:4], out[3, 4:8], out[3, 30:34] = 5, 3, 8  # 5 3 8; word 8 ends the episode: no successor there
    out[4, frames - 3 :] = 3                          # the word's first occurrence near the end: the interval still fits
    return out


def run(ref: types.ModuleType, labels: np.ndarray, speakers: np.ndarray, rng: np.random.Generator) -> dict[str, np.ndarray]:
    data = []
    for e in range(labels.shape[0]):
        onehot = np.zeros((labels.shape[1], 6), dtype=np.float32)
        onehot[:, speakers[e]] = 1.0
        data.append({"label": labels[e], "speaker": onehot, "audio": np.zeros((labels.shape[1], 1), dtype=np.float32),
                     "image": np.zeros((labels.shape[1], 1), dtype=np.float32)})
    p = np.zeros((10, 11))
    q = np.zeros((10, 11))
    mr = np.zeros(10)
    base = np.zeros((10, 2))
    intervals = np.full((10, N_INTERVALS, 2 + QUERY), PAD, dtype=np.int64)
    predicted = np.full((10, 40), PAD, dtype=np.int64)
    for w in WORDS:
        with contextlib.redirect_stdout(io.StringIO()):
            p_dist = ref.compute_true_distribution(w, data, WORDS)
            chosen = ref.select_intervals_for_word(w, data, n_intervals=N_INTERVALS, query_length=QUERY)
        n = int(rng.integers(0, 41)) if w != 9 else 0  # noqa: PLR2004  (word 9: nothing predicted)
        digits = rng.integers(0, 12, size=n)  # 10 and 11 are not words: failures
        predicted[w, :n] = digits
        q_dist = ref.compute_prediction_distribution([int(d) for d in digits], WORDS)
        p[w] = [p_dist[k] for k in WORDS] + [p_dist["wf"]]
        q[w] = [q_dist[k] for k in WORDS] + [q_dist.get("wf", 0.0)]
        mr[w] = ref.compute_matching_rate(q_dist, p_dist, WORDS)
        b = ref.compute_baselines(p_dist, WORDS, n_random_trials=1)
        base[w] = [b["uniform"], b["peak_onehot"]]
        for i, iv in enumerate(chosen):
            intervals[w, i, 0], intervals[w, i, 1] = iv["file_idx"], iv["speaker_idx"]
            intervals[w, i, 2:] = iv["label"]
    return {"labels": labels, "speakers": speakers, "p": p, "q": q, "mr": mr, "baselines": base, "intervals": intervals, "predicted": predicted}


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--reference", type=Path, required=True, help="root of the reference project's checkout")
    parser.add_argument("--out", type=Path, default=Path(__file__).resolve().parents[1] / "tests" / "golden" / "word_transitions.npz")
    args = parser.parse_args()
    ref = load_reference(args.reference.resolve())
    rng = np.random.default_rng(20240607)
    out: dict[str, np.ndarray] = {"query": np.asarray(QUERY), "n_intervals": np.asarray(N_INTERVALS)}
    sets = {"seeded": (seeded_labels(rng, 14, 90), rng.integers(0, 6, size=14)), "edge": (edge_labels(40), np.asarray([0, 1, 2, 1, 3]))}
    for name, (labels, speakers) in sets.items():
        for k, v in run(ref, labels, speakers.astype(np.int64), rng).items():
            out[f"{name}/{k}"] = v
    args.out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({args.out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
