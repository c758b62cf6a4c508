"""GPU (MI355X): generation coherence, kernel and end to end.

What is pinned here.  ``mtrssm_coherence_fold`` is the float64 rule on the same fp32 logits: ``pairs``, ``counts`` and the four indicator
sums exactly, the ``soft`` sums to rtol 1e-12 (the project's tolerance for double sums across ``exp`` implementations,
``tests/test_census_gpu.py``), the planes to the project's loss-term tolerance (rtol 2e-5, atol 2e-6) with the rule's zero pattern.  Two
calls agree bitwise, a second call doubles the table exactly, ``planes = NULL`` gives the same table, the sums by horizon are the host's
float64 left fold of the frame sums in the stated order bit for bit, a row's planes depend on that row only.  The shapes: three rows of
three groups with ties, non-finite rows, dead labels and short rows planted; 70 rows of 16 copies over 33 frames (more than one
workgroup, three staged spans per row, the fold across workgroups); a context at and past ``T``; no ``valid``.  A coherence step of
either model class is the rule on the logits its readers returned; its group ``"both"`` is ``forecast_skill``'s rollout bit for bit and
counts the hits ``word_transitions(by_horizon=True)`` counts; ``lengths`` remove exactly the frames past each row's end."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd import CoherenceTable, ForecastSkill, GenerationCoherence, StateCarry, WordTransitions, _lib
from multimodal_mtrssm_amd.coherence import PLANES, group_cells, table_views
from tests.test_coherence_capi import check_c_refusals
from tests.test_coherence_host import coherence_inputs, mixed_valid
from tests.test_digits_host import MARGIN, seeded_classifier
from tests.test_likelihood_gpu import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

OBSERVE = ("both", "audio", "vision")
CASES = [  # (B, G, S, T, context, valid)
    (3, 3, 3, 7, 3, (7, 5, 2)),
    (70, 1, 16, 33, 8, "mixed"),
    (3, 2, 2, 7, 7, (7, 5, 2)),       # context == T: everything is phase 0
    (3, 2, 2, 7, 1 << 20, (7, 5, 2)),  # ... and far past it
    (3, 3, 3, 7, 3, None),
    (2, 4, 1, 17, 1, None),            # four groups of one copy, one frame of context, a span of one frame
]


def _valid(b: int, t: int, valid) -> torch.Tensor | None:  # noqa: ANN001
    if valid is None:
        return None
    return mixed_valid(b, t) if valid == "mixed" else torch.tensor(valid, dtype=torch.int32)


def _host_fold(u: torch.Tensor, b: int, g: int, t: int, context: int) -> torch.Tensor:
    """``[G, 5, T]``: the frame sums ``u [5, B * G, T]`` folded in the stated order, one float64 add per frame."""
    c = min(context, t)
    rows = u.reshape(len(PLANES), b, g, t)
    sums = torch.zeros(g, len(PLANES), t, dtype=torch.float64)
    for row in range(b):
        for i in range(t):
            sums[:, :, 0 if i < c else i - c + 1] += rows[:, row, :, i].T
    return sums


def _assert_against_rule(got_planes, got_table, want_planes, want_table, t: int, what: str) -> None:  # noqa: ANN001, PLR0913
    planes = got_planes.cpu()
    assert planes.dtype == torch.float32 and bool(torch.isfinite(planes).all()), what
    err = (planes.double() - want_planes).abs()
    print(what, "planes: worst abs", float(err.max()), "worst err / (2e-6 + 2e-5 |ref|)", float((err / (2e-6 + 2e-5 * want_planes.abs())).max()))
    np.testing.assert_allclose(planes.double().numpy(), want_planes.numpy(), rtol=2e-5, atol=2e-6, err_msg=f"{what} planes")
    assert torch.equal(planes == 0, want_planes.float() == 0), f"{what}: zero pattern"
    got, want = table_views(got_table.cpu(), t), table_views(want_table, t)
    assert torch.equal(got["pairs"], want["pairs"]) and torch.equal(got["counts"], want["counts"]), f"{what} pairs / counts"
    assert torch.equal(got["sums"][:, :4], want["sums"][:, :4]), f"{what} indicator sums"
    rel = ((got["sums"][:, 4] - want["sums"][:, 4]).abs() / want["sums"][:, 4].abs().clamp_min(1e-300)).max()
    print(what, "soft sums: worst rel", float(rel))
    torch.testing.assert_close(got["sums"][:, 4], want["sums"][:, 4], rtol=1e-12, atol=0.0, msg=f"{what} soft sums")


# 1. the kernel is the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("b", "g", "s", "t", "context", "valid"), CASES)
def test_coherence_kernel_equals_the_float64_rule(b: int, g: int, s: int, t: int, context: int, valid) -> None:  # noqa: ANN001, PLR0913, PLR0914
    lv, la, labels = coherence_inputs(b, g, s, t, seed=b + t)
    valid = _valid(b, t, valid)
    what = f"coherence {(b, g, s, t)} context {context} valid {None if valid is None else valid.tolist()[:4]}"
    want_planes, want_table = GenerationCoherence.reference(lv, la, labels, g, s, context, valid)
    if (b, g, s, t, context) == (3, 3, 3, 7, 3):
        # the inputs alone: every plane is non-zero somewhere, both phases hold reads off the diagonal, the failure bin is hit,
        # a tie of the two largest logits is read somewhere and dead labels are among the frames
        w = table_views(want_table, t)
        assert bool((want_planes.reshape(5, -1) != 0).any(1).all()) and bool((w["sums"].sum((0, 2)) > 0).all())
        pairs = w["pairs"].sum(0)
        off = pairs.clone()
        off.diagonal(dim1=1, dim2=2).zero_()
        assert bool((off.sum((1, 2)) > 0).all()) and bool((pairs.diagonal(dim1=1, dim2=2).sum(1) > 0).all())
        assert float(pairs[:, 10].sum()) > 0 and float(pairs[:, :, 10].sum()) > 0
        top2 = lv.topk(2, dim=-1).values
        assert bool((top2[..., 0] == top2[..., 1]).any()) and bool((labels < 0).any()) and bool((labels > 9).any())  # noqa: PLR2004
    dev = [x.to(DEV) for x in (lv, la, labels)]
    dvalid = None if valid is None else valid.to(DEV)
    planes, table, u = GenerationCoherence.fold(*dev, g, s, context, dvalid, frame_sums=True)
    torch.cuda.synchronize()
    assert tuple(planes.shape) == (5, b * g, t) and tuple(table.shape) == (g, group_cells(t)) and table.dtype == torch.float64
    _assert_against_rule(planes, table, want_planes, want_table, t, what)
    live = (labels >= 0) & (labels <= 9)  # noqa: PLR2004
    if valid is not None:
        live &= torch.arange(t) < valid.clamp(0, t)[:, None]
    assert not bool(planes.cpu().reshape(5, b, g, t)[:, ~live[:, None].expand(b, g, t)].any()), what  # exactly 0 on dead frames
    # the sums by horizon are the float64 left fold of the frame sums in the stated order, bit for bit; the planes are u / S
    assert torch.equal(table_views(table.cpu(), t)["sums"], _host_fold(u.cpu(), b, g, t, context)), what
    assert torch.equal(planes.cpu(), (u.cpu() / float(s)).float()), what
    if context >= t:
        v = table_views(table.cpu(), t)
        assert not bool(v["pairs"][:, 1].any()) and not bool(v["counts"][:, 1:].any()) and not bool(v["sums"][:, :, 1:].any()), what
    # two calls agree bitwise; a second call into the same table doubles it exactly; planes = NULL gives the same table
    planes2, table2 = GenerationCoherence.fold(*dev, g, s, context, dvalid)
    assert torch.equal(planes, planes2) and torch.equal(table, table2), what
    none, table3 = GenerationCoherence.fold(*dev, g, s, context, dvalid, planes=False)
    assert none is None and torch.equal(table, table3), what
    _, twice = GenerationCoherence.fold(*dev, g, s, context, dvalid, table=table2)
    assert twice is table2 and torch.equal(twice, 2.0 * table), what


def test_a_rows_planes_depend_on_that_row_only() -> None:
    b, g, s, t, c = 5, 3, 3, 7, 3
    lv, la, labels = (x.to(DEV) for x in coherence_inputs(b, g, s, t, seed=1))
    valid = torch.tensor([7, 7, 6, 7, 3], dtype=torch.int32, device=DEV)
    planes, _ = GenerationCoherence.fold(lv, la, labels, g, s, c, valid)
    other_v, other_a, _ = coherence_inputs(b, g, s, t, seed=9)
    moved = slice(2 * g * s, 3 * g * s)  # every copy of row 2
    lv2, la2 = lv.clone(), la.clone()
    lv2[moved], la2[moved] = other_v[moved].to(DEV), other_a[moved].to(DEV)
    planes2, _ = GenerationCoherence.fold(lv2, la2, labels, g, s, c, valid)
    keep = torch.ones(b * g, dtype=torch.bool, device=DEV)
    keep[2 * g : 3 * g] = False
    assert torch.equal(planes[:, keep], planes2[:, keep]) and not torch.equal(planes[:, ~keep], planes2[:, ~keep])


def test_c_entry_rejects_bad_arguments_without_a_launch_on_the_device() -> None:
    check_c_refusals(_lib.load())
    lv, la, labels = (x.to(DEV) for x in coherence_inputs(2, 2, 2, 5))
    with pytest.raises(ValueError, match="table must be"):
        GenerationCoherence.fold(lv, la, labels, 2, 2, 3, table=torch.zeros(2, group_cells(5), device=DEV))  # (fp32)
    with pytest.raises(ValueError, match="valid"):
        GenerationCoherence.fold(lv, la, labels, 2, 2, 3, torch.tensor([5, 5], dtype=torch.int32))  # (on the host)
    with pytest.raises(ValueError, match="labels"):
        GenerationCoherence.fold(lv, la, labels.cpu(), 2, 2, 3)


# 2. a coherence step is the rule on what its readers returned ---------------------------------------------------------------------------------
B, T, S, Q = 2, 16, 2, 4


def _reader(seed: int, logits: torch.Tensor) -> torch.nn.Module:
    """A seeded untrained reader, its head centred on ``logits`` (what it reads off this rollout: several digits occur) and scaled so
    that the logits spread by about 2 (the softmax is neither flat nor one-hot)."""
    clf = seeded_classifier(seed)
    flat = logits.reshape(-1, 10).double().cpu()
    gain = 2.0 / float((flat - flat.mean(0)).std())
    clf.fc2.bias.copy_(((clf.fc2.bias.double() - flat.mean(0)) * gain).float())
    clf.fc2.weight.mul_(gain)
    return clf.to(DEV)


@functools.lru_cache(maxsize=None)
def _step(name: str) -> dict:
    """Model, batch, noise, readers and labels of the end-to-end tests, made once: the readers are seeded, centred on a first rollout
    and kept only if every vision logit row of group "both" has a top-2 margin of ``MARGIN`` of the scale (``tests/test_digits_host.py``:
    below it a frame may read either digit when the decode differs in its last bits)."""
    _, model, batch = _setup(name, (B, T))
    gc = GenerationCoherence(Q, samples=S, observe=OBSERVE)
    gen = torch.Generator().manual_seed(11)
    noise = {key: torch.rand(shape, generator=gen).to(DEV) for key, shape in gc.noise_shapes(model, B, T).items()}
    blank = torch.full((B, T), -1, dtype=torch.int32, device=DEV)
    for seed in range(5, 25):
        plain = {"vision": seeded_classifier(seed).to(DEV), "audio": seeded_classifier(seed + 100).to(DEV)}
        first = model.generation_coherence(batch, blank, gc, plain, noise, keep_states=True)
        assert not bool(first.buffer.any())  # (silence everywhere: nothing is counted)
        readers = {"vision": _reader(seed, first.logits[0]), "audio": _reader(seed + 100, first.logits[1])}
        table = model.generation_coherence(batch, blank, gc, readers, noise, keep_states=True)
        zv = table.logits[0].reshape(B, 3 * S, T, 10)[:, :S].double()
        top2 = zv.topk(2, dim=-1).values
        if bool(((top2[..., 0] - top2[..., 1]) >= MARGIN * float(zv.abs().max())).all()):
            break
    else:
        pytest.fail("no reader seed keeps every frame's margin")
    dv, da = table.logits[0].argmax(-1).reshape(B, 3 * S, T).cpu(), table.logits[1].argmax(-1).reshape(B, 3 * S, T).cpu()
    print(name, "reader seed", seed, "vision digits", dv.unique().tolist(), "audio digits", da.unique().tolist())
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, 10, (B, T), generator=g)
    pick = torch.rand(B, T, generator=g)
    labels = torch.where(pick < 0.4, dv[:, 0], labels)  # noqa: PLR2004  (what copy 0 of "both" shows)
    labels = torch.where((pick >= 0.4) & (pick < 0.6), da[:, 1], labels)  # noqa: PLR2004  (what copy 1 of "both" says)
    labels = torch.where(pick > 0.9, torch.full_like(labels, -1), labels)  # noqa: PLR2004
    labels[0, 0], labels[1, T - 1] = int(dv[0, 0, 0]), int(dv[1, 0, T - 1])
    return {"model": model, "batch": batch, "gc": gc, "noise": noise, "readers": readers, "labels": labels.to(torch.int32).to(DEV)}


def _both_against_skill(model, mine, theirs) -> list[tuple[str, torch.Tensor, torch.Tensor]]:  # noqa: ANN001
    """``(key, copies 0 .. S - 1 of every row of a coherence step's states, the skill step's states)`` per state tensor."""
    out = []
    for key in model._FRESH_KEYS:  # noqa: SLF001
        a, b = getattr(mine, key, None), getattr(theirs, key, None)
        if a is not None and b is not None:
            out.append((key, a.reshape(B, 3 * S, *a.shape[1:])[:, :S].reshape(b.shape), b))
    return out


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_group_both_is_forecast_skills_rollout_bit_for_bit(name: str) -> None:
    """With the same noise, group "both"'s states equal ``forecast_skill(..., keep_states=True)``'s bitwise.

    Both steps run the model's encoders themselves; the evaluation rollout pins every GEMM in front of the scan to one reduction slice
    (``linear.ordered_sums``), so no fp32 atomics meet and a row's result does not depend on the run or on the other rows of the launch.
    (Without the pin the embeddings moved by 3e-8 from call to call and ``deter`` differed in 200 to 370 of 2048 entries by 1e-7.)"""
    ref = _step(name)
    model, batch, gc, noise, readers, labels = (ref[k] for k in ("model", "batch", "gc", "noise", "readers", "labels"))
    table = model.generation_coherence(batch, labels, gc, readers, noise, keep_states=True)
    skill_noise = {k: (u[:, :S].contiguous() if "tail" in k else u) for k, u in noise.items()}
    skill = model.forecast_skill(batch, ForecastSkill(Q, samples=S), skill_noise, keep_states=True)
    pairs = _both_against_skill(model, table.states, skill.states)
    for key, mine, theirs in pairs:
        print(name, key, "bitwise equal:", torch.equal(mine, theirs), "worst abs", float((mine - theirs).abs().max()),
              "entries that differ", int((mine != theirs).sum()), "of", mine.numel())
    assert len(pairs) >= 2  # noqa: PLR2004
    for key, mine, theirs in pairs:
        assert torch.equal(mine, theirs), (name, key)


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_group_both_is_the_skills_rollout_from_the_same_inputs(name: str) -> None:
    """The encoders run ONCE (the coherence step's inputs); the rows of group "both" alone, rolled out as a scan of ``B * S`` rows, give
    the scan outputs of the ``B * G * S``-row rollout bit for bit -- and their codes are the skill plan's."""
    ref = _step(name)
    model, batch, gc, noise = (ref[k] for k in ("model", "batch", "gc", "noise"))
    first = lambda x: x.reshape(B, 3 * S, *x.shape[1:])[:, :S].reshape(B * S, *x.shape[1:]).contiguous()  # noqa: E731
    with torch.no_grad():
        wide, _ = model._evaluation_inputs(batch, gc.plan(), noise, None, None)  # noqa: SLF001
        skill_noise = {k: (u[:, :S].contiguous() if "tail" in k else u) for k, u in noise.items()}
        thin, _ = model._evaluation_inputs(batch, ForecastSkill(Q, samples=S).plan(), skill_noise, None, None)  # noqa: SLF001
        assert torch.equal(first(wide["codes"]), thin["codes"]) and all(torch.equal(first(wide["noise"][k]), thin["noise"][k]) for k in model._POST_KEYS)  # noqa: SLF001
        state0 = model._state_like(wide["state0"], {k: first(getattr(wide["state0"], k)) for k in model._FRESH_KEYS})  # noqa: SLF001
        cut_noise = {k: (first(u) if u is not None and u.shape[0] == B * 3 * S else u) for k, u in wide["noise"].items()}
        big = model._rollout_embedded(wide["actions"], wide["audio_embed"], wide["vision_embed"], wide["state0"], wide["noise"], sample_prior=False,  # noqa: SLF001
                                      modality=wide["codes"], expert_log_weights=None)
        small = model._rollout_embedded(first(wide["actions"]), first(wide["audio_embed"]), first(wide["vision_embed"]), state0, cut_noise,  # noqa: SLF001
                                        sample_prior=False, modality=first(wide["codes"]), expert_log_weights=None)
    compared = 0
    for key, x in small.items():
        if torch.is_tensor(x) and x.is_floating_point() and x.shape[0] == B * S:
            compared += 1
            assert torch.equal(first(big[key]), x), (name, key)
    assert compared >= 4  # noqa: PLR2004


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_coherence_step_is_the_rule_on_its_logits(name: str) -> None:  # noqa: PLR0914, PLR0915
    ref = _step(name)
    model, batch, gc, noise, readers, labels = (ref[k] for k in ("model", "batch", "gc", "noise", "readers", "labels"))
    table = model.generation_coherence(batch, labels, gc, readers, noise, keep_states=True)
    torch.cuda.synchronize()
    assert isinstance(table, CoherenceTable) and table.groups == 3 and table.steps == T and table.observe == OBSERVE  # noqa: PLR2004
    assert tuple(table.planes.shape) == (5, B * 3, T) and all(tuple(x.shape) == (B * 3 * S, T, 10) for x in table.logits)
    host = [x.cpu() for x in table.logits]
    want_planes, want_table = GenerationCoherence.reference(*host, labels.cpu(), 3, S, Q)
    _assert_against_rule(table.planes, table.buffer, want_planes, want_table, T, name)
    v = table.views()
    live = float((labels >= 0).sum())
    assert float(v["counts"][0].sum()) == live * S and bool((v["counts"] == v["counts"][0]).all()) and float(v["pairs"].sum()) == 3 * live * S
    soft = table.planes[4].cpu()[(labels.cpu() >= 0).repeat_interleave(3, dim=0)]
    assert soft.unique().numel() >= 2 and bool((soft > 0).all())  # noqa: PLR2004  (soft differs between frames: the comparison says something)
    assert float(v["sums"][:, 0].sum()) > 0 and float(v["sums"][:, 1].sum()) > 0
    scalars = table.scalars("val/coherence")
    assert len(scalars) == 3 * (5 * 5 + 2 + 2) + 1 and float(scalars["val/coherence/reads"]) == 3 * live * S
    # group "both" is forecast_skill's rollout under the same noise (bit for bit: the test above)
    skill_noise = {k: (u[:, :S].contiguous() if "tail" in k else u) for k, u in noise.items()}
    skill = model.forecast_skill(batch, ForecastSkill(Q, samples=S), skill_noise, keep_states=True)
    pairs = _both_against_skill(model, table.states, skill.states)
    assert len(pairs) >= 2  # noqa: PLR2004
    for key, mine, theirs in pairs:
        if key.startswith("stoch"):
            assert torch.equal(mine, theirs), (name, key)
        else:
            torch.testing.assert_close(mine, theirs, rtol=0.0, atol=1e-5, msg=f"{name} {key}")
    # ... and its vision hits by horizon are S x the hit sums of word_transitions(by_horizon=True)
    words = model.word_transitions(batch, labels, WordTransitions(Q, samples=S, by_horizon=True), readers["vision"], skill_noise)
    assert torch.equal(v["sums"][0, 0].cpu(), words.horizon[0].double().cpu() * S), (v["sums"][0, 0], words.horizon[0])
    assert torch.equal(v["counts"][0].cpu(), words.horizon[2].double().cpu() * S)
    # a second step adds into the same table and keeps nothing of the batch.  The kernels' logits are within 1e-4 of their scale M of
    # the float64 rule (tests/test_digits_gpu.py), so two runs' logits differ by d <= 2e-4 M; log p_k = z_k - logsumexp(z) then moves
    # by at most 2 d, a product pv_k pa_k by a factor within 4 d of 1, and so does every sum of them: rtol 8e-4 M
    scale = max(float(x.abs().max()) for x in table.logits)
    full_logits = table.logits
    first = table.buffer.clone()
    again = model.generation_coherence(batch, labels, gc, readers, noise, table=table)
    assert again is table and table.planes is None and table.logits is None and table.states is None
    got, want = table_views((table.buffer - first).cpu(), T), table_views(first.cpu(), T)
    assert torch.equal(got["pairs"], want["pairs"]) and torch.equal(got["counts"], want["counts"]) and torch.equal(got["sums"][:, :4], want["sums"][:, :4])
    print(name, "second step: soft sums worst rel", float(((got["sums"][:, 4] - want["sums"][:, 4]).abs() / want["sums"][:, 4].clamp_min(1e-300)).max()))
    torch.testing.assert_close(got["sums"][:, 4], want["sums"][:, 4], rtol=8e-4 * scale, atol=0.0)
    # chunks of one row (other kernel routes of the decoders) give the same logits within those 2e-4 M, and count the same frames
    small = GenerationCoherence(Q, samples=S, observe=OBSERVE)
    small.max_frames = 1
    chunked = model.generation_coherence(batch, labels, small, readers, noise, keep_states=True)
    for mine, theirs in zip(chunked.logits, full_logits, strict=True):
        print(name, "chunks of one row: logits worst abs / M", float((mine - theirs).abs().max()) / scale)
        torch.testing.assert_close(mine, theirs, rtol=0.0, atol=2e-4 * scale)
    assert torch.equal(chunked.views()["counts"].cpu(), want["counts"]) and float(chunked.views()["pairs"].sum()) == float(want["pairs"].sum())
    # lengths shorter than T remove exactly the frames past each row's end (row 1 ends inside the context)
    lengths = torch.tensor([T - 5, Q - 1], dtype=torch.int32, device=DEV)
    short = model.generation_coherence(batch, labels, gc, readers, noise, lengths=lengths, keep_states=True)
    alive = (torch.arange(T, device=DEV) < lengths[:, None]).repeat_interleave(3, dim=0)
    full = model.generation_coherence(batch, labels, gc, readers, noise, keep_states=True)
    kept_planes = torch.where(alive, full.planes, torch.zeros_like(full.planes))  # (two calls: the encoders move the logits by an ulp)
    assert torch.equal(short.planes[:4], kept_planes[:4]) and torch.equal(short.planes[4] == 0, kept_planes[4] == 0)
    torch.testing.assert_close(short.planes[4], kept_planes[4], rtol=8e-4 * scale, atol=0.0)  # (two runs' logits: the bound above)
    want_short_planes, want_short = GenerationCoherence.reference(*[x.cpu() for x in short.logits], labels.cpu(), 3, S, Q, lengths.cpu())
    _assert_against_rule(short.planes, short.buffer, want_short_planes, want_short, T, f"{name} lengths")
    assert not bool(want_short_planes[:, ~alive.cpu()].any())
    kept = (labels >= 0) & (torch.arange(T, device=DEV) < lengths[:, None])
    assert float(short.views()["counts"][1].sum()) == float(kept.sum()) * S < live * S
    drawn = model.generation_coherence(batch, labels, GenerationCoherence(Q, observe=("audio",)), readers)  # (without noise the step draws its own)
    assert drawn.groups == 1 and float(drawn.views()["counts"].sum()) == live


def test_refusals() -> None:
    ref = _step("mrssm_default")
    model, batch, gc, noise, readers, labels = (ref[k] for k in ("model", "batch", "gc", "noise", "readers", "labels"))
    for bad in ({"vision": readers["vision"]}, {"audio": readers["audio"]}, {"vision": readers["vision"], "audio": None}, readers["vision"]):
        with pytest.raises(ValueError, match="readers must be"):
            model.generation_coherence(batch, labels, gc, bad, noise)
    with pytest.raises(ValueError, match="7-tuple"):
        model.generation_coherence((*batch, torch.ones(B, T, 2, dtype=torch.bool, device=DEV)), labels, gc, readers, noise)
    with pytest.raises(ValueError, match="GenerationCoherence"):
        model.generation_coherence(batch, labels, ForecastSkill(Q), readers, noise)
    with pytest.raises(ValueError, match="labels must be"):
        model.generation_coherence(batch, labels[:, :-1], gc, readers, noise)
    for table in (CoherenceTable(3, T + 1, DEV), CoherenceTable(2, T, DEV), CoherenceTable(3, T)):
        with pytest.raises(ValueError, match="table must be a CoherenceTable of 3 groups and 16 steps"):
            model.generation_coherence(batch, labels, gc, readers, noise, table=table)
    model.state_carry = StateCarry.for_model(model, B)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.generation_coherence(batch, labels, gc, readers, noise)
    finally:
        model.state_carry = None
    _, bench, bench_batch = _setup("mrssm_bench", (2, 3))  # 1 x 128 x 32 audio frames, 1 x 64 x 64 vision frames
    with pytest.raises(ValueError, match="reads 1 x 32 x 32 audio frames, the batch holds"):
        bench.generation_coherence(bench_batch, torch.zeros(2, 3, dtype=torch.int32, device=DEV), gc, readers)
