"""CPU: the word-transition bookkeeping against ``tests/golden/word_transitions.npz`` -- the results of the
reference evaluation's own functions on seeded label sequences (``tools/gen_word_transitions_golden.py``) -- its edge cases, the
``TransitionTable`` and the messages of ``WordTransitions`` / ``model.word_transitions``.  Counts are compared with ``==``, ratios to
rtol 1e-12.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import TransitionTable, WordTransitions
from multimodal_mtrssm_amd.words import (
    WORDS,
    baselines,
    digit_sequence,
    format_results_table,
    matching_rate,
    prediction_distribution,
    results_from_table,
    select_intervals,
    true_distribution,
)
from oracle.cases import CASES, build_batch, build_model, with_sizes
from tests.conftest import load_golden, product_from_case

PAD = -9


def _vector(dist: dict) -> list[float]:
    return [dist[w] for w in WORDS] + [dist.get("wf", 0.0)]


@pytest.mark.parametrize("name", ["seeded", "edge"])
def test_host_functions_reproduce_the_golden_fixture(name: str) -> None:
    fx = load_golden("word_transitions")
    labels, speakers = fx[f"{name}/labels"], fx[f"{name}/speakers"]
    query, n_intervals = int(fx["query"]), int(fx["n_intervals"])
    seen_intervals = 0
    for w in WORDS:
        p = true_distribution(labels, w)
        np.testing.assert_allclose(_vector(p), fx[f"{name}/p"][w], rtol=1e-12, atol=0, err_msg=f"p {w}")
        predicted = [int(d) for d in fx[f"{name}/predicted"][w] if d != PAD]
        q = prediction_distribution(predicted)
        np.testing.assert_allclose(_vector(q), fx[f"{name}/q"][w], rtol=1e-12, atol=0, err_msg=f"q {w}")
        assert ("wf" in q) == bool(predicted)  # (an empty list has no failure key, as in the evaluation)
        np.testing.assert_allclose(matching_rate(q, p), fx[f"{name}/mr"][w], rtol=1e-12, atol=0, err_msg=f"mr {w}")
        b = baselines(p)
        np.testing.assert_allclose([b["uniform"], b["peak_onehot"]], fx[f"{name}/baselines"][w], rtol=1e-12, atol=0, err_msg=f"baselines {w}")
        np.testing.assert_allclose(b["random_onehot"], sum(p[k] for k in WORDS) / 10.0, rtol=1e-12, atol=0)
        # the same q through the device table's host view: whole-number counts, then the ratios
        table = TransitionTable(4)
        for d in predicted:
            table.q_counts[w, d if d in WORDS else 10] += 1
        assert float(table.q_counts.sum()) == len(predicted)
        np.testing.assert_allclose(_vector(table.q_distribution(w)), fx[f"{name}/q"][w], rtol=1e-12, atol=0)
        want = fx[f"{name}/intervals"][w]
        got = select_intervals(labels, speakers, w, n_intervals, query)
        assert len(got) == int((want[:, 0] != PAD).sum()), w
        for iv, row in zip(got, want, strict=False):
            assert (iv["file_idx"], iv["speaker_idx"]) == (int(row[0]), int(row[1])) and iv["end"] - iv["start"] == query
            assert labels[iv["file_idx"]][iv["start"] : iv["end"]].tolist() == row[2:].tolist()
            seen_intervals += 1
    assert seen_intervals > 0
    if name == "seeded":
        assert len({int(fx["seeded/intervals"][w, i, 1]) for w in WORDS for i in range(n_intervals) if fx["seeded/intervals"][w, i, 0] != PAD}) > 1
        assert float(fx["seeded/q"][:, 10].max()) > 0 and float(fx["seeded/mr"].max()) > 0  # failures and matches both occur


def test_edge_cases() -> None:
    assert digit_sequence([3, 3, -1, 3, 5, 5, -1, -1, 5, 3]) == [3, 5, 3]  # the previous digit survives silence
    assert digit_sequence([-1, -1, -1]) == [] and digit_sequence([]) == []
    silent = [[-1] * 8, [-1] * 3]
    for w in WORDS:
        p = true_distribution(silent, w)
        assert _vector(p) == [0.0] * 11 and matching_rate({0: 1.0, "wf": 0.0}, p) == 0.0
        assert select_intervals([np.asarray(x) for x in silent], [0, 1], w, 6, 3) == []
    # a word with no successor: it only ever ends a sequence
    p = true_distribution([[1, 1, 2, 2, 7], [7, 7, 7]], 7)
    assert _vector(p) == [0.0] * 11
    assert baselines(p) == {"uniform": 0.0, "peak_onehot": 0.0, "random_onehot": 0.0}
    # a repeated word separated by silence is ONE word: 3 -> 5 once, not 3 -> 3
    p = true_distribution([[3, 3, -1, 3, 5]], 3)
    assert p[5] == 1.0 and p[3] == 0.0
    # a successor outside the word set counts in the total only
    p = true_distribution([[3, 12, 3, 4]], 3)
    assert p[4] == 0.5 and sum(_vector(p)) == 0.5  # noqa: PLR2004
    # the matching rate of a distribution with itself is its mass; the failure bin takes part
    q = {**{w: 0.0 for w in WORDS}, 2: 0.5, "wf": 0.5}
    assert matching_rate(q, q) == 1.0 and matching_rate(q, {**q, "wf": 0.25, 2: 0.75}) == 0.75  # noqa: PLR2004
    # one interval per speaker, in episode order, ending at the word's first occurrence
    episodes = [np.asarray([-1, 4, 4, 2, 2, 2, 4, 4]), np.asarray([2, 2, 4, 4, -1, -1, -1, -1]), np.asarray([-1] * 5 + [2, 2, 2])]
    got = select_intervals(episodes, [0, 0, 1], 2, 6, 3)
    assert got == [{"file_idx": 0, "speaker_idx": 0, "start": 1, "end": 4}, {"file_idx": 2, "speaker_idx": 1, "start": 3, "end": 6}]
    assert select_intervals(episodes, [0, 1, 2], 2, 2, 3)[1] == {"file_idx": 1, "speaker_idx": 1, "start": 0, "end": 3}
    assert select_intervals(episodes, [0, 1, 2], 2, 6, 20)[0] == {"file_idx": 0, "speaker_idx": 0, "start": 0, "end": 20}  # as the evaluation does


def test_results_table_has_the_evaluations_columns() -> None:
    table = TransitionTable(2)
    table.q_counts[3, 5] = 3.0
    table.q_counts[3, 10] = 1.0
    labels = [[3, 3, 5, 5, 3, 4], [3, 5]]
    results = results_from_table(table, labels)
    assert results[3]["mopoe"] == matching_rate({5: 0.75, "wf": 0.25}, {5: 2 / 3, 4: 1 / 3}) == 2 / 3
    assert results[0]["mopoe"] == 0.0 and set(results[3]) == {"mopoe", "uniform", "peak_onehot", "random_onehot"}
    text = format_results_table(results)
    lines = text.splitlines()
    assert lines[0] == "| Word | MoPoE-MRSSM | Uniform | Peak one-hot | Random one-hot |" and lines[1].startswith("|-----|")
    assert len(lines) == 12 and lines[5] == f"| 3 | {2 / 3:.4f} | {results[3]['uniform']:.4f} | {results[3]['peak_onehot']:.4f} | {results[3]['random_onehot']:.4f} |"  # noqa: PLR2004
    assert "MoPoE-MMTRSSM" in format_results_table(results, model_name="MoPoE-MMTRSSM").splitlines()[0]


def test_transition_table_adds_and_reduces_without_a_process_group() -> None:
    a, b = TransitionTable(5), TransitionTable(5)
    assert tuple(a.q_counts.shape) == (10, 11) and tuple(a.horizon.shape) == (3, 5) and a.steps == 5 and a.buffer.numel() == 110 + 15  # noqa: PLR2004
    a.q_counts[2, 3] = 4.0
    b.q_counts[2, 3] = 1.0
    b.q_counts[9, 10] = 2.0
    a.horizon[:, 1] = torch.tensor([1.5, 2.0, 2.0])
    b.horizon[:, 1] = torch.tensor([0.5, 1.0, 2.0])
    b.horizon[2, 0] = 3.0
    assert a.add(b) is a and float(a.q_counts[2, 3]) == 5.0 and float(a.q_counts[9, 10]) == 2.0  # noqa: PLR2004
    assert a.all_reduce() is a and float(a.q_counts.sum()) == 7.0  # noqa: PLR2004  (no process group: a no-op)
    acc = a.accuracy()
    assert acc["hit"].tolist()[:2] == [0.0, 0.5] and acc["any"].tolist()[1] == 0.75 and acc["count"].tolist()[:2] == [3.0, 4.0]  # noqa: PLR2004
    assert bool(acc["hit"][2:].isnan().all())
    scalars = a.scalars("val/words")
    assert set(scalars) == {"val/words/reads"} | {f"val/words/{k}/{n}" for k in ("hit", "any") for n in ("obs", "h1", "h2", "h4", "h8")}
    assert float(scalars["val/words/reads"]) == 7.0 and float(scalars["val/words/hit/h1"]) == 0.5 and float(scalars["val/words/any/obs"]) == 0.0  # noqa: PLR2004
    assert bool(scalars["val/words/hit/h4"].isnan())
    with pytest.raises(ValueError, match="do not add"):
        a.add(TransitionTable(4))
    with pytest.raises(ValueError, match="steps >= 1"):
        TransitionTable(0)
    with pytest.raises(ValueError, match="ascending horizons"):
        a.scalars("x", edges=(2, 1))


def test_messages() -> None:
    for kw, match in (({"query": 0}, "query must be"), ({"query": True}, "query must be"), ({"samples": 17}, "samples must be"),
                      ({"samples": 0}, "samples must be"), ({"read_at": 0}, "read_at must be"), ({"protocol": "prior"}, "protocol must be"),
                      ({"protocol": "reference", "read_at": 2}, "first predicted frame"), ({"protocol": "reference", "by_horizon": True}, "first predicted frame")):
        with pytest.raises(ValueError, match=match):
            WordTransitions(**kw)
    wt = WordTransitions(4, samples=3)
    assert (wt.query, wt.samples, wt.read_at, wt.protocol, wt.by_horizon) == (4, 3, 1, "context", False) and "samples=3" in repr(wt)
    assert wt.read_frame(8) == 4 and WordTransitions(4, samples=1, read_at=4).read_frame(8) == 7  # noqa: PLR2004
    with pytest.raises(ValueError, match="no frame 1 past a context of 4"):
        wt.read_frame(4)
    case = CASES["mrssm_default"]
    model = product_from_case(case, build_model(case), "cpu")
    k = model.transition.distribution_factory.category_size
    assert wt.noise_shapes(model, 5, 8) == {"u_init": (5, k), "u_post": (5, 8, k), "u_tail": (5, 3, 8, k)}
    assert WordTransitions(4, samples=3, protocol="reference").noise_shapes(model, 5, 8) == {"u_init": (5, k), "u_prior": (5, 3, 1, k)}
    mt_case = CASES["mmtrssm_default"]
    assert set(WordTransitions(4, samples=3, protocol="reference").noise_shapes(product_from_case(mt_case, build_model(mt_case), "cpu"), 5, 8)) == {
        "u_init_h", "u_init_l", "u_prior_l", "u_prior_h"}
    clf = mt.DigitClassifier()
    batch = tuple(x[:2, :8] for x in build_batch(with_sizes(case, 2, 8)))
    labels = torch.zeros(2, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="wt must be a WordTransitions"):
        model.word_transitions(batch, labels, mt.ForecastSkill(4), clf)
    with pytest.raises(ValueError, match="classifier must be a DigitClassifier"):
        model.word_transitions(batch, labels, wt, torch.nn.Identity())
    with pytest.raises(ValueError, match="a masked \\(7-tuple\\) batch already says what is seen"):
        model.word_transitions((*batch, torch.ones(2, 8, 2, dtype=torch.bool)), labels, wt, clf)
    with pytest.raises(ValueError, match="labels must be an int32 / int64 tensor of shape \\(2, 8\\)"):
        model.word_transitions(batch, labels[:, :7], wt, clf)
    with pytest.raises(ValueError, match="labels must be an int32"):
        model.word_transitions(batch, labels.float(), wt, clf)
    with pytest.raises(ValueError, match="no context of 9"):
        model.word_transitions(batch, labels, WordTransitions(9, samples=1), clf)
    with pytest.raises(ValueError, match="table must be a TransitionTable of 8 steps"):
        model.word_transitions(batch, labels, wt, clf, table=TransitionTable(7))
    model.state_carry = object()
    with pytest.raises(ValueError, match="does not combine with a set state_carry"):
        model.word_transitions(batch, labels, wt, clf)
