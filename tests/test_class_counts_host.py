"""Host (no GPU): the oracle-side conditions of ``tests/test_class_counts_gpu.py``, so that a failure there is the kernel's.

For every case of ``tests/class_counts.py``: a screened noise seed exists; the fp32 oracle at head gain 150 agrees with a float64
copy of itself to a tenth of the GPU tolerances on losses and gradients, with identical samples; under constant logit rows the oracle's samples are ``floor(u C)`` and its KL
is 0.0; the head kernel's uniforms keep their margin."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.cases import build_batch, build_model, min_margin
from oracle.ref_model import cat_probs
from tests.class_counts import (CLASS_CASES, HEAD_SHAPES, MASKED_CASES, PARITY_RUNS, SATURATED_CASES, SATURATED_GAIN, TIE_CASES,
                                WIDE_FAMILIES, edge_noise, flatten_heads, float64_copy, floor_index, head_problem, tie_draws)
from tests.config_matrix import SAMPLING_MARGIN, options, screened, with_options

# The probabilities of the fp32 oracle at gain 150: a logit below 64 has an ulp of 2^-18 = 3.8e-6 and comes out of a dot product
# of up to 200 terms, a few ulps from its float64 value; d p = p (1 - p) d logit <= d logit / 4.  Four ulps, over four: 2^-18.
# (Measured: 1.2e-6 at D = H = 200.)  The tenth of the GPU tolerance that losses and gradients keep is out of fp32's reach here.
PROB_BOUND = 2.0**-18

_RUNS = sorted({(case_id, option_set or "") for case_id, option_set, _ in PARITY_RUNS})


def _index(stoch: torch.Tensor, cats: int, classes: int) -> torch.Tensor:
    return stoch.detach().reshape(*stoch.shape[:-1], cats, classes).argmax(-1)


def test_cases_reach_the_general_path() -> None:
    """Every case has a categorical of more than 8 classes or more than 64 categoricals; the wide cases carry one level each way."""
    for case, _family in CLASS_CASES.values():
        d = case.dims
        sizes = [(d.classes, d.cats)] if case.kind == "mrssm" else [(d.ls_classes, d.ls_cats), (d.hs_classes, d.hs_cats)]
        assert any(c > 8 or k > 64 for c, k in sizes), case.name  # noqa: PLR2004
    assert len(CLASS_CASES) == 12  # noqa: PLR2004


@pytest.mark.parametrize(("case_id", "option_set"), _RUNS)
def test_screened_seed_exists(case_id: str, option_set: str) -> None:
    base, _family = CLASS_CASES[case_id]
    case = with_options(base, **options(base, option_set)) if option_set else base
    _noise, margin, seed = screened(case, build_model(case), build_batch(case))  # asserts that a seed qualifies
    print(f"{case_id} {option_set}: seed {seed}, sampling margin {margin:.3e}")
    assert margin >= SAMPLING_MARGIN


@pytest.mark.parametrize("case_id", MASKED_CASES)
def test_masked_weighted_seed_exists(case_id: str) -> None:
    """The masked and weighted runs: a seed keeps the margin ``tests/test_expert_weights_oracle.py`` asks of its own cases."""
    from tests.test_expert_weights_oracle import codes_of, explicit_weights
    from tests.test_expert_weights_oracle import screened as screened_weighted

    case, _family = CLASS_CASES[case_id]
    codes = codes_of("fourway", case.batch, case.steps)
    assert set(codes.flatten().tolist()) == {0, 1, 2, 3}
    lw = explicit_weights(case.batch, case.steps)
    _noise, margin = screened_weighted(case, build_model(case), build_batch(case), codes, lambda _ea, _ev: lw)
    assert margin >= 1e-5, margin  # noqa: PLR2004


@pytest.mark.parametrize("case_id", list(SATURATED_CASES))
def test_saturated_oracle_agrees_with_float64(case_id: str) -> None:
    """At head gain 150 the fp32 oracle stays within a tenth of the GPU tolerances on losses and gradients of a float64 copy of
    itself (losses 2e-6 relative, gradients 2e-5 of a tensor's max, wide 1e-4; samples identical) and its probabilities within
    ``PROB_BOUND``: the GPU bounds of test_saturated_heads_match_oracle rest on the number formats, not on the code under test."""
    case, family = SATURATED_CASES[case_id]
    assert case.head_gain == SATURATED_GAIN
    d = case.dims
    oracle = build_model(case)
    batch = build_batch(case)
    noise, margin, _seed = screened(case, oracle, batch)
    ref = oracle.shared_step(batch, noise)
    ref["loss"].backward()
    oracle64 = float64_copy(oracle)
    oracle64.zero_grad(set_to_none=True)
    ref64 = oracle64.shared_step(tuple(b.double() for b in batch), {k: v.double() for k, v in noise.items()})
    ref64["loss"].backward()
    assert min_margin(case, ref64, {k: v.double() for k, v in noise.items()}) >= 0.9 * margin
    levels = [("", d.cats, d.classes)] if case.kind == "mrssm" else [("_l", d.ls_cats, d.ls_classes), ("_h", d.hs_cats, d.hs_classes)]
    worst_logit, worst_kl, worst_prob = 0.0, 0.0, 0.0
    for sfx, cats, classes in levels:
        for which in ("post", "prior"):
            lg, lg64 = ref[f"_{which}_logits{sfx}"].detach(), ref64[f"_{which}_logits{sfx}"].detach()
            worst_logit = max(worst_logit, float(lg.abs().max()))
            assert float(lg.abs().max()) < 64.0  # noqa: PLR2004
            err = float((cat_probs(lg, cats, classes)[1].double() - cat_probs(lg64, cats, classes)[1]).abs().max())
            worst_prob = max(worst_prob, err)
            assert err <= PROB_BOUND, (which, sfx, err)
            assert torch.equal(_index(ref[f"_{which}_stoch{sfx}"], cats, classes), _index(ref64[f"_{which}_stoch{sfx}"], cats, classes))
    for k in ref:
        if k.startswith("_"):
            continue
        assert np.isfinite(float(ref[k].detach()))
        np.testing.assert_allclose(float(ref[k].detach()), float(ref64[k].detach()), rtol=2e-6, err_msg=k)
        if k.startswith("kl"):
            worst_kl = max(worst_kl, float(ref[k].detach()))
    tol = 0.1 * (1e-3 if family in WIDE_FAMILIES else 2e-4)
    got = dict(oracle.named_parameters())
    worst_grad = 0.0
    for k, p64 in oracle64.named_parameters():
        if p64.grad is None:
            continue
        scale = float(p64.grad.abs().max()) + 1e-12
        err = float((got[k].grad.double() - p64.grad).abs().max()) / scale
        worst_grad = max(worst_grad, err)
        assert err <= tol, (k, err)
    print(f"{case_id}: max|logit| {worst_logit:.1f}, KL {worst_kl:.1f}, worst probability error {worst_prob:.2e}, "
          f"worst gradient error {worst_grad:.2e} of max, margin {margin:.2e}")
    assert worst_logit > 20.0 and worst_kl > 20.0  # saturated indeed  # noqa: PLR2004


@pytest.mark.parametrize("case_id", list(TIE_CASES))
def test_oracle_samples_floor_uc_under_uniform_logits(case_id: str) -> None:
    """Constant logit rows and uniforms on / next to the edges j / C: the oracle's samples are floor(u C), its KL is 0.0."""
    case, _family = TIE_CASES[case_id]
    oracle = flatten_heads(build_model(case))
    noise = edge_noise(case)
    with torch.no_grad():
        ref = oracle.shared_step(build_batch(case), noise)
    for key, stoch, logits, cats, classes in tie_draws(case):
        assert classes & (classes - 1) == 0, "a power of two"
        rows = ref[logits].reshape(*ref[logits].shape[:-1], cats, classes)
        assert float((rows.amax(-1) - rows.amin(-1)).max()) == 0.0, f"{logits}: logit spread"
        assert torch.equal(_index(ref[stoch], cats, classes), floor_index(noise[key], classes)), key
    for k in ref:
        if k.startswith("kl"):
            assert float(ref[k]) == 0.0, k


def test_edge_noise_has_every_kind() -> None:
    """Over a case's draws the four kinds all occur, and an on-edge and a below-edge draw differ in their index."""
    case, _ = TIE_CASES["w256_16x8"]
    u = torch.cat([v.flatten() for v in edge_noise(case).values()])
    c = case.dims.classes
    on_edge = (u * c == torch.floor(u * c)) & (u > 0)
    assert int(on_edge.sum()) > 10 and int((u == 0).sum()) > 10 and int((u == 1.0 - 2.0**-24).sum()) > 10  # noqa: PLR2004
    below = torch.nextafter(u[on_edge], torch.tensor(-1.0))
    assert torch.equal(floor_index(below, c), floor_index(u[on_edge], c) - 1)
    assert int(floor_index(torch.tensor(1.0 - 2.0**-24), c)) == c - 1


@pytest.mark.parametrize(("rows", "cats", "classes"), HEAD_SHAPES)
def test_head_kernel_uniforms_keep_their_margin(rows: int, cats: int, classes: int) -> None:
    pr = head_problem(rows, cats, classes)  # asserts that a seed qualifies
    assert pr["margin"] >= SAMPLING_MARGIN
    assert pr["index"].shape == (rows, cats) and int(pr["index"].max()) < classes
