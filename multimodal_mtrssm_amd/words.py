"""Word-transition matching rate: sampled futures read by the digit classifier.

For every spoken digit ``wa`` futures are sampled from the model, the predicted vision frame is read with ``digits.DigitClassifier``
and the histogram ``q(w | wa)`` is compared with the data's own next-word distribution ``p(w | wa)``:

    MR(wa) = sum_w min(q(w | wa), p(w | wa))          over the ten words and the failure bin "wf"

A *transition step* (``model.word_transitions``) takes a batch ``[B, T]`` with its labels (int ``[B, T]``, -1 = silence), samples ``S``
futures per row in one rollout over ``B * S`` rows, decodes only what is read, and adds ``counts[wa][digit] += 1`` into a
``TransitionTable`` on the device -- ``wa`` is the label of the row's last context frame, a silent row is skipped.  Two protocols:

* ``"context"`` (default): the row observes its first ``query`` frames of both modalities and runs open loop after them --
  ``forecast_skill``'s masked rollout with the same noise contract (``u_post`` shared by a row's copies on the context, ``u_tail[b, s]``
  after it); the vision frame ``read_at`` steps past the context (frame index ``query - 1 + read_at``) is read.
* ``"reference"``: what the evaluation script does -- the initial state comes from frame 0 of the interval, a prior-only rollout
  follows with the interval's LAST action, and the FIRST predicted frame is read.  The other ``query - 1`` frames of the interval are
  not shown to the model at all; that is the script's behaviour and is kept as it is.

With ``by_horizon=True`` (context protocol) every frame of the ``S`` futures is read as well and two planes are folded by horizon with
``mtrssm_horizon_table``: ``hit[b, t]`` = the share of the copies whose digit equals ``labels[b, t]``, ``any[b, t]`` = whether one does;
silent frames are dead (they add nothing to the sums or to the count).

The host functions restate the evaluation's bookkeeping on label sequences (``true_distribution``, ``select_intervals``,
``matching_rate``, ``baselines``, ``format_results_table``); ``tests/golden/word_transitions.npz`` pins them to its results.
"""

from __future__ import annotations

import dataclasses
from collections.abc import Iterable, Sequence

import numpy as np
import torch
from torch import Tensor

from multimodal_mtrssm_amd.digits import CLASSES
from multimodal_mtrssm_amd.skill import MAX_SAMPLES, ForecastSkill, SumTable

WORDS = tuple(range(CLASSES))
BINS = CLASSES + 1          # the ten words and "wf", the failure bin
PROTOCOLS = ("context", "reference")
_HORIZON_ROWS = 3           # hit, any, the live (labelled) frames


class WordTransitions:
    """``WordTransitions(query, samples=S, read_at=r, protocol=..., by_horizon=False)``: see the module's docstring.  ``max_frames``: the
    decoder and the classifier run over chunks of whole rows of at most this many frames."""

    def __init__(self, query: int = 30, samples: int = 10, read_at: int = 1, protocol: str = "context", *, by_horizon: bool = False) -> None:
        if isinstance(query, bool) or not isinstance(query, int) or not 1 <= query < 1 << 31:
            msg = f"query must be an integer 1 <= q < 2^31, got {query!r}"
            raise ValueError(msg)
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
            msg = f"samples must be an integer in 1 .. {MAX_SAMPLES}, got {samples!r}"
            raise ValueError(msg)
        if isinstance(read_at, bool) or not isinstance(read_at, int) or read_at < 1:
            msg = f"read_at must be an integer >= 1 (frames past the context), got {read_at!r}"
            raise ValueError(msg)
        if protocol not in PROTOCOLS:
            msg = f"protocol must be one of {list(PROTOCOLS)}, got {protocol!r}"
            raise ValueError(msg)
        if protocol == "reference" and (read_at != 1 or by_horizon):
            msg = "the reference protocol reads the first predicted frame only: read_at = 1, no by_horizon"
            raise ValueError(msg)
        self.query, self.samples, self.read_at, self.protocol, self.by_horizon = query, samples, read_at, protocol, bool(by_horizon)
        self.skill = ForecastSkill(query, samples=samples)
        self.max_frames = 4096

    def __repr__(self) -> str:
        return (f"WordTransitions({self.query}, samples={self.samples}, read_at={self.read_at}, protocol={self.protocol!r}, "
                f"by_horizon={self.by_horizon})")

    def read_frame(self, steps: int) -> int:
        """The index of the frame that is read in a batch of ``steps`` frames (context protocol)."""
        t = self.query - 1 + self.read_at
        if self.query > steps or t >= steps:
            msg = f"a batch of {steps} frames has no frame {self.read_at} past a context of {self.query}"
            raise ValueError(msg)
        return t

    def plan(self):  # noqa: ANN201
        """The skill's plan (context protocol); reference protocol: its copies with no posterior uniforms, each reads its own
        ``u_prior[b, s]`` ``(B, S, 1, K)`` for the one prior step."""
        plan = self.skill.plan()
        return plan if self.protocol == "context" else dataclasses.replace(plan, post="prior")

    def noise_shapes(self, model, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # noqa: ANN001
        """The uniforms of one step, batch dimension first.  Context protocol: ``ForecastSkill.noise_shapes``.  Reference protocol: the
        initial state's and ``u_prior (B, S, 1, K)`` (MMTRSSM: the ``_l`` / ``_h`` pairs)."""
        return self.plan().noise_shapes(model, batch, steps)


class TransitionTable(SumTable):
    """The accumulated counts of any number of transition steps in ONE fp32 buffer: ``q_counts [10, 11]`` (row = current word,
    column = digit read, column 10 = "wf") and, behind it, ``horizon [2 + 1, T]``: the by-horizon sums of ``hit`` and ``any`` and the
    live (labelled) frames per horizon bin (zeros unless a step ran ``by_horizon``)."""

    def __init__(self, steps: int = 1, device: torch.device | str = "cpu") -> None:
        self.buffer = torch.zeros(CLASSES * BINS + _HORIZON_ROWS * self._checked_steps(steps), dtype=torch.float32, device=device)

    @property
    def steps(self) -> int:
        return (self.buffer.numel() - CLASSES * BINS) // _HORIZON_ROWS

    @property
    def q_counts(self) -> Tensor:
        return self.buffer[: CLASSES * BINS].view(CLASSES, BINS)

    @property
    def horizon(self) -> Tensor:
        return self.buffer[CLASSES * BINS :].view(_HORIZON_ROWS, self.steps)

    def q_distribution(self, word: int) -> dict[int | str, float]:
        """``q(w | word)`` with the key ``"wf"`` for the failure bin; all zeros when nothing was counted."""
        row = self.q_counts[word].double().cpu()
        total = float(row.sum())
        probs = [float(c) / total if total > 0 else 0.0 for c in row.tolist()]
        return {**{w: probs[w] for w in WORDS}, "wf": probs[CLASSES]}

    def accuracy(self) -> dict[str, Tensor]:
        """``hit`` and ``any`` per horizon bin (``[T]`` each: sums over the live frames; NaN for a bin without one) and ``count``."""
        hit, any_, live = self.horizon
        return {"hit": self._mean(hit, live), "any": self._mean(any_, live), "count": live}

    def scalars(self, prefix: str, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, Tensor]:
        """``prefix/{hit,any}/{obs,h1,h2,...}`` over ``SkillTable``'s horizon bins, and ``prefix/reads`` = the futures counted."""
        slices = self._bin_slices(edges)
        hit, any_, live = self.horizon
        out = {f"{prefix}/reads": self.q_counts.sum()}
        for name, row in (("hit", hit), ("any", any_)):
            for label, s in slices:
                out[f"{prefix}/{name}/{label}"] = self._mean(row[s].sum(), live[s].sum())
        return out


# -- the evaluation's bookkeeping on the host --------------------------------------------------------------------------------------------
def digit_sequence(labels: Iterable[int]) -> list[int]:
    """Silence (-1) dropped, repeats collapsed.  The previous digit survives silence: ``3 3 -1 3 5`` is ``3 5``."""
    seq: list[int] = []
    prev = None
    for label in labels:
        d = int(label)
        if d == -1 or d == prev:
            continue
        seq.append(d)
        prev = d
    return seq


def true_distribution(labels: Sequence[Iterable[int]], word: int, word_set: Sequence[int] = WORDS) -> dict[int | str, float]:
    """``p(w | word)`` over the episodes' label sequences: the successors of ``word`` in every collapsed sequence, counted over ALL
    transitions out of ``word`` (a successor outside ``word_set`` counts in the total only); all zeros when ``word`` has no successor."""
    counts: dict[int, int] = {}
    total = 0
    for episode in labels:
        seq = digit_sequence(episode)
        for a, b in zip(seq[:-1], seq[1:], strict=True):
            if a == word:
                if b in word_set:
                    counts[b] = counts.get(b, 0) + 1
                total += 1
    if total == 0:
        return {**{w: 0.0 for w in word_set}, "wf": 0.0}
    return {**{w: counts.get(w, 0) / total for w in word_set}, "wf": 0.0}


def prediction_distribution(predicted: Sequence[int], word_set: Sequence[int] = WORDS) -> dict[int | str, float]:
    """``q(w | wa)`` of a list of read digits; a digit outside ``word_set`` is a failure ("wf").  An empty list gives zeros without
    the "wf" key, as the evaluation does."""
    total = len(predicted)
    if total == 0:
        return {w: 0.0 for w in word_set}
    counts = {w: 0 for w in word_set}
    for d in predicted:
        if d in counts:
            counts[d] += 1
    return {**{w: counts[w] / total for w in word_set}, "wf": (total - sum(counts.values())) / total}


def select_intervals(labels: Sequence[np.ndarray], speakers: Sequence[int], word: int, n_intervals: int = 6, query: int = 30) -> list[dict[str, int]]:
    """One interval of ``query`` frames per speaker, ending at ``word``'s first occurrence in the episode (starting at frame 0 when it
    comes earlier than ``query`` frames in; the first ``query`` frames when the interval would pass the episode's end): a list of
    ``{"file_idx", "speaker_idx", "start", "end"}`` in episode order, at most ``n_intervals``."""
    chosen: list[dict[str, int]] = []
    used: set[int] = set()
    for file_idx, episode in enumerate(labels):
        episode = np.asarray(episode)
        where = np.nonzero(episode == word)[0]
        if where.size == 0:
            continue
        speaker = int(speakers[file_idx])
        if speaker in used:
            continue
        start = max(0, int(where[0]) - query + 1)
        end = start + query
        if end > episode.shape[0]:
            start, end = 0, query
        chosen.append({"file_idx": file_idx, "speaker_idx": speaker, "start": start, "end": end})
        used.add(speaker)
        if len(chosen) >= n_intervals:
            break
    return chosen


def matching_rate(q: dict, p: dict, word_set: Sequence[int] = WORDS) -> float:
    """``sum_w min(q(w), p(w))`` over ``word_set`` in order, then the failure term; a missing key is 0."""
    mr = 0.0
    for w in word_set:
        mr += min(q.get(w, 0.0), p.get(w, 0.0))
    return mr + min(q.get("wf", 0.0), p.get("wf", 0.0))


def baselines(p: dict, word_set: Sequence[int] = WORDS) -> dict[str, float]:
    """The matching rates of three predictors that know nothing of the context: ``uniform`` (1 / |W| each), ``peak_onehot`` (all mass on
    the first most likely word) and ``random_onehot`` -- all mass on a uniformly drawn word, as its EXACT expectation
    ``sum_w p(w) / |W|`` (the evaluation averages 100 ``random.choice`` trials: an unseeded estimate of this number)."""
    n = len(word_set)
    uniform = {**{w: 1.0 / n for w in word_set}, "wf": 0.0}
    peak_word = max(word_set, key=lambda w: p.get(w, 0.0))
    peak = {**{w: 0.0 for w in word_set}, "wf": 0.0}
    peak[peak_word] = 1.0
    expected = 0.0
    for w in word_set:
        expected += min(1.0, p.get(w, 0.0))
    return {"uniform": matching_rate(uniform, p, word_set), "peak_onehot": matching_rate(peak, p, word_set), "random_onehot": expected / n}


def format_results_table(results: dict[int, dict[str, float]], word_set: Sequence[int] = WORDS, model_name: str = "MoPoE-MRSSM") -> str:
    """The evaluation's Markdown table: one row per word with the model's MR and the three baselines."""
    header = f"| Word | {model_name} | Uniform | Peak one-hot | Random one-hot |\n"
    separator = "|-----|---------------|---------|--------------|----------------|\n"
    rows = []
    for word in sorted(word_set):
        r = results.get(word, {})
        rows.append(f"| {word} | {r.get('mopoe', 0.0):.4f} | {r.get('uniform', 0.0):.4f} | {r.get('peak_onehot', 0.0):.4f} | "
                    f"{r.get('random_onehot', 0.0):.4f} |\n")
    return header + separator + "".join(rows)


def results_from_table(table: TransitionTable, labels: Sequence[Iterable[int]], word_set: Sequence[int] = WORDS) -> dict[int, dict[str, float]]:
    """Per word: ``mopoe`` = MR of the table's ``q`` against ``p`` of ``labels`` (0 when nothing was counted for the word) and the baselines."""
    results = {}
    for word in word_set:
        p = true_distribution(labels, word, word_set)
        counted = float(table.q_counts[word].sum()) > 0
        results[word] = {"mopoe": matching_rate(table.q_distribution(word), p, word_set) if counted else 0.0, **baselines(p, word_set)}
    return results


__all__ = ["TransitionTable", "WordTransitions", "baselines", "digit_sequence", "format_results_table", "matching_rate", "prediction_distribution",
           "results_from_table", "select_intervals", "true_distribution"]
