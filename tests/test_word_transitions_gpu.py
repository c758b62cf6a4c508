"""GPU (MI355X): a transition step end to end, on the default-dims models (the smallest configured ones whose
vision frames are 32 x 32), B = 3, T = 8, query = 4, S = 3.

``model.word_transitions`` must give EXACTLY the counts of the slow path built from public pieces: per copy ``forecast_rollout`` under
that copy's rows of the composed noise -> ``decode_state`` -> ``reference_logits`` in float64 -> first maximum -> a Python histogram.
Exactness holds on frames whose float64 top-2 margin is at least ``1e-3 * max |logit|`` (tests/test_digits_gpu.py: the kernels' logits
are within 1e-4 of the scale); the classifier's seed is chosen on the host so that every frame of the batch is such a frame, and the
test asserts that.  Noise is screened on the CPU as in tests/test_forecast_skill_gpu.py, so that no draw sits at a CDF edge.
"""

from __future__ import annotations

import functools

import pytest
import torch

from multimodal_mtrssm_amd import ExpertWeights, TransitionTable, WordTransitions
from oracle.cases import CASES, build_batch, build_model, build_noise, min_margin, with_sizes
from tests.conftest import product_from_case
from tests.test_digits_host import MARGIN, seeded_classifier
from tests.test_modality_mask_oracle import oracle_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, S, Q = 3, 8, 3, 4
MODELS = ["mrssm_default", "mmtrssm_default", "mrssm_default+gate"]


def _wide(x: torch.Tensor) -> torch.Tensor:
    return x.repeat_interleave(S, dim=0)


@functools.lru_cache(maxsize=None)
def _setup(name: str) -> dict:
    """Oracle, batch and skill noise screened on the CPU under the codes of the wide run (row ``b * S + s`` reads its row's context
    draws on ``t < Q`` and draws of its own after) -- tests/test_forecast_skill_gpu.py's setup at this file's sizes."""
    case = with_sizes(CASES[name], B, T)
    oracle = build_model(case)
    batch = build_batch(case)
    wide_batch = tuple(_wide(x) for x in batch)
    codes = (torch.arange(T) < Q).long().mul(3).expand(B * S, T).contiguous()
    best = None
    for seed in range(400, 440):
        noise = build_noise(case, seed, batch=B * S, steps=T)
        for u in noise.values():
            first = _wide(u[::S])
            if u.dim() == 2:  # noqa: PLR2004
                u.copy_(first)
            else:
                u[:, :Q] = first[:, :Q]
        with torch.no_grad():
            out = oracle_step(case, oracle, wide_batch, noise, codes)
        margin = min_margin(case, out, noise)
        if best is None or margin > best[1]:
            best = (noise, margin)
        if margin >= 1e-4:  # noqa: PLR2004
            break
    wide_noise, margin = best
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"  # noqa: PLR2004
    noise = {}
    for k, u in wide_noise.items():
        if k.startswith("u_prior"):
            continue
        noise[k] = u[::S].contiguous()
        if k.startswith("u_post"):
            noise[k.replace("post", "tail")] = u.reshape(B, S, *u.shape[1:]).contiguous()
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "wide_noise": wide_noise}


def _model(name: str):  # noqa: ANN202
    base = name.split("+")[0]
    ref = _setup(base)
    model = product_from_case(ref["case"], ref["oracle"], DEV)
    if name.endswith("+gate"):
        torch.manual_seed(11)
        model.expert_weights = ExpertWeights("gated", ref["case"].dims.embed).to(DEV)
        with torch.no_grad():
            model.expert_weights.weight.normal_(0.0, 0.3)
            model.expert_weights.bias.normal_(0.0, 0.5)
    return model, ref


def _slow_frames(model, ref: dict, batch: tuple) -> torch.Tensor:  # noqa: ANN001
    """float64 ``[B, S, T, 1024]``: the activated vision frames of every copy, from ``forecast_rollout`` + ``decode_state``."""
    wide_noise = {k: v.to(DEV) for k, v in ref["wide_noise"].items()}
    frames = []
    for s in range(S):
        noise_s = {k: v[s::S].contiguous() for k, v in wide_noise.items()}
        with torch.no_grad():
            s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise_s)
            post = model.forecast_rollout(actions=batch[0], observations=(batch[1], batch[2]), context=Q, prev_state=s0, noise=noise_s)
            frames.append(model.decode_state(post)["recon/vision"].reshape(B, T, 1024).double().cpu())
    return torch.stack(frames, dim=1)


def _classifier_for(frames: torch.Tensor, min_digits: int = 3):  # noqa: ANN202
    """A seeded classifier whose ``fc2.bias`` is centred on these frames' mean logits (so that several digits occur), with every frame's
    float64 margin at least ``MARGIN`` of the scale: ``(classifier, digits int64 [..])``."""
    flat = frames.reshape(-1, 1024)  # (decode_state's output is activated: the rule takes it with act = 0)
    for seed in range(5, 25):
        clf = seeded_classifier(seed)
        clf.fc2.bias -= clf.reference_logits(flat, 0).mean(0).float()
        logits = clf.reference_logits(flat, 0)
        top2 = logits.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) >= MARGIN * float(logits.abs().max())).all()):
            digits = clf.first_max(logits).long().reshape(frames.shape[:-1])
            if digits.unique().numel() >= min_digits:
                return clf, digits
    pytest.fail("no classifier seed keeps every frame's margin (the exemption would be needed)")


def _labels(digits: torch.Tensor) -> torch.Tensor:
    """int64 ``[B, T]``: row 1 is silent at the last context frame (skipped); some labels are what copy 0 or copy 2 reads there, some are
    silence, the rest another word."""
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, 10, (B, T), generator=g)
    pick = torch.rand(B, T, generator=g)
    labels = torch.where(pick < 0.35, digits[:, 0], labels)  # noqa: PLR2004
    labels = torch.where((pick >= 0.35) & (pick < 0.55), digits[:, 2], labels)  # noqa: PLR2004
    labels = torch.where(pick > 0.85, torch.full_like(labels, -1), labels)  # noqa: PLR2004
    labels[0, Q - 1], labels[1, Q - 1], labels[2, Q - 1] = 7, -1, 2
    return labels


def _histogram(labels: torch.Tensor, digits: torch.Tensor, frame: int, rows: range = range(B)) -> torch.Tensor:
    want = torch.zeros(10, 11)
    for b in rows:
        word = int(labels[b, Q - 1])
        if word < 0:
            continue
        for s in range(S):
            want[word, int(digits[b, s, frame])] += 1
    return want


def _fold(labels: torch.Tensor, digits: torch.Tensor, onto: torch.Tensor | None = None) -> torch.Tensor:
    """The by-horizon table ``[3, T]`` as a Python fold in fp32, frame by frame in ascending ``(b, t)`` onto the values already there."""
    table = torch.zeros(3, T) if onto is None else onto.clone()
    for b in range(B):
        for t in range(T):
            if int(labels[b, t]) < 0:
                continue
            same = sum(int(digits[b, s, t]) == int(labels[b, t]) for s in range(S))
            h = 0 if t < Q else t - Q + 1
            table[0, h] += torch.tensor(float(same)) / float(S)
            table[1, h] += 1.0 if same else 0.0
            table[2, h] += 1.0
    return table


@pytest.mark.parametrize("name", MODELS)
def test_context_protocol_equals_the_slow_path(name: str) -> None:
    model, ref = _model(name)
    batch = tuple(x.to(DEV) for x in ref["batch"])
    noise = {k: v.to(DEV) for k, v in ref["noise"].items()}
    clf, digits = _classifier_for(_slow_frames(model, ref, batch))
    labels = _labels(digits)
    print(name, "digits read", digits.unique().tolist(), "labels", labels.tolist())
    dclf = seeded_classifier(0)
    dclf.load_state_dict(clf.state_dict())
    dclf.to(DEV)
    wt = WordTransitions(Q, samples=S, by_horizon=True)
    table = model.word_transitions(batch, labels.to(DEV), wt, dclf, noise)
    assert isinstance(table, TransitionTable) and table.steps == T
    want = _histogram(labels, digits, Q)
    assert torch.equal(table.q_counts.cpu(), want) and float(want.sum()) == 2.0 * S and not bool(table.q_counts[:, 10].any())  # noqa: PLR2004
    fold = _fold(labels, digits)
    assert torch.equal(table.horizon.cpu(), fold), (table.horizon.cpu(), fold)
    assert float(fold[2].sum()) == float((labels >= 0).sum()) and 0 < float(fold[0].sum()) < float(fold[1].sum())
    acc = table.accuracy()
    assert torch.equal(acc["count"].cpu(), fold[2]) and set(table.scalars("val/words")) >= {"val/words/hit/obs", "val/words/any/h1", "val/words/reads"}
    # only the read frame decoded: the same counts; int32 labels; a later frame; chunks of one row; accumulation into the table
    plain = model.word_transitions(batch, labels.to(DEV).to(torch.int32), WordTransitions(Q, samples=S), dclf, noise)
    assert torch.equal(plain.q_counts.cpu(), want) and not bool(plain.horizon.any())
    later = model.word_transitions(batch, labels.to(DEV), WordTransitions(Q, samples=S, read_at=3), dclf, noise)
    assert torch.equal(later.q_counts.cpu(), _histogram(labels, digits, Q + 2))
    small = WordTransitions(Q, samples=S, by_horizon=True)
    small.max_frames = 1
    again = model.word_transitions(batch, labels.to(DEV), small, dclf, noise, table=table)
    assert again is table and torch.equal(table.q_counts.cpu(), 2 * want) and torch.equal(table.horizon.cpu(), _fold(labels, digits, fold))
    if name == MODELS[0]:
        # two shards: the tables of rows [0, 2) and [2, 3) add up to the full batch's (no process group needed)
        parts = TransitionTable(T, DEV)
        for rows in (slice(0, 2), slice(2, 3)):
            part = model.word_transitions(tuple(x[rows] for x in batch), labels[rows].to(DEV), wt, dclf, {k: v[rows] for k, v in noise.items()})
            parts.add(part.all_reduce())
        assert torch.equal(parts.buffer.cpu()[:110].reshape(10, 11), want) and torch.equal(parts.horizon.cpu(), fold)
        # without noise the step draws its own: the same number of reads
        drawn = model.word_transitions(batch, labels.to(DEV), wt, dclf)
        assert float(drawn.q_counts.sum()) == 2.0 * S  # noqa: PLR2004


@pytest.mark.parametrize("name", MODELS[:2])
def test_reference_protocol_is_initial_state_and_a_prior_step_with_the_last_action(name: str) -> None:
    model, ref = _model(name)
    batch = tuple(x.to(DEV) for x in ref["batch"])
    wt = WordTransitions(Q, samples=S, protocol="reference")
    g = torch.Generator().manual_seed(9)
    noise = {k: torch.rand(shape, generator=g).to(DEV) for k, shape in wt.noise_shapes(model, B, T).items()}
    frames = []
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        for s in range(S):
            prior_noise = {k: v[:, s].contiguous() for k, v in noise.items() if k.startswith("u_prior")}
            prior = model.rollout_transition(actions=batch[0][:, Q - 1 : Q].contiguous(), prev_state=s0, noise=prior_noise)
            frames.append(model.decode_state(prior)["recon/vision"][:, 0].reshape(B, 1, 1024).double().cpu())
    clf, digits = _classifier_for(torch.stack(frames, dim=1), min_digits=2)  # [B, S, 1]
    labels = _labels(torch.zeros(B, S, T, dtype=torch.int64))
    dclf = seeded_classifier(0)
    dclf.load_state_dict(clf.state_dict())
    dclf.to(DEV)
    table = model.word_transitions(batch, labels.to(DEV), wt, dclf, noise)
    want = _histogram(labels, digits, 0)
    assert torch.equal(table.q_counts.cpu(), want) and float(want.sum()) == 2.0 * S and not bool(table.horizon.any())  # noqa: PLR2004
    with pytest.raises(ValueError, match="must have shape"):
        model.word_transitions(batch, labels.to(DEV), wt, dclf, {k: v[:, :1] if k.startswith("u_prior") else v for k, v in noise.items()})
