"""CPU: the reference side of ``tests/test_scan_cotangents_gpu.py`` (``tests/scan_cotangents.py`` holds the problem).

For every case of that file's table: the screening finds a seed, the fp32 oracle draws the float64 reference's samples, the
KL-per-step restatement has ``oracle.ref_model.kl_loss``'s value and gradients, and the float64 reference gives exactly zero
gradients where the GPU test expects exact zeros.  It also measures what the GPU bounds are set from: the error of the fp32
oracle's gradients against its float64 copy, as the largest error over the tensor's largest float64 entry.  The largest such
figure per case is printed and, after a run over all cases, written into ``profiles/scan_cotangent_errors.md``."""

from __future__ import annotations

import functools
import math
import re
from pathlib import Path

import pytest
import torch

from oracle.ref_model import kl_loss
from tests.config_matrix import SAMPLING_MARGIN
from tests.scan_cotangents import (FAMILY_CASES, GRAD_BOUND, HOST_BASELINE, HOST_SINGLE_SETS, Problem, build_problem, kl_per_step, levels,
                                   reference_gradients, relative_error, sample_index)

CASES = [(family, case_id) for family, ids in FAMILY_CASES.items() for case_id in ids]
NOTES = Path(__file__).resolve().parents[1] / "profiles" / "scan_cotangent_errors.md"
_BEGIN, _END = "<!-- host baselines: begin -->", "<!-- host baselines: end -->"


@functools.lru_cache(maxsize=None)
def _problem(case_id: str) -> Problem:
    return build_problem(case_id)


@pytest.fixture(scope="module")
def baselines():  # noqa: ANN201
    """case id -> (family, seed, margin, largest fp32-versus-float64 gradient error, its tensor and set); written to the notes
    file once every case has reported."""
    rows: dict[str, tuple] = {}
    yield rows
    if len(rows) != len(CASES):
        return
    lines = [_BEGIN, "| family | case | seed | sampling margin | largest fp32-oracle error | tensor (set) |", "|---|---|---|---|---|---|"]
    lines += [f"| {fam} | `{cid}` | {seed} | {margin:.1e} | {err:.1e} | `{name}` ({cot}) |"
              for cid, (fam, seed, margin, err, name, cot) in rows.items()]
    lines.append(_END)
    try:
        text = NOTES.read_text()
        block = re.compile(re.escape(_BEGIN) + ".*?" + re.escape(_END), re.DOTALL)
        if block.search(text):
            NOTES.write_text(block.sub(lambda _m: "\n".join(lines), text))
    except OSError as exc:  # a read-only checkout: the figures were printed
        print(f"baselines not written: {exc}")


@pytest.mark.parametrize(("family", "case_id"), CASES, ids=[c for _, c in CASES])
def test_screening_finds_a_seed_and_fp32_draws_the_same_samples(family: str, case_id: str) -> None:
    pr = _problem(case_id)
    assert pr.family == family
    assert pr.margin >= SAMPLING_MARGIN
    out32, _ = reference_gradients(pr.oracle, pr, "all")
    out64, _ = reference_gradients(pr.ref64, pr, "all")
    for sfx, cats, classes in levels(pr.case):
        for which in ("post", "prior"):
            key = f"{which}_stoch{sfx}"
            assert torch.equal(sample_index(out32[key], cats, classes), sample_index(out64[key], cats, classes)), key


@pytest.mark.parametrize("balancing", [True, False])
@pytest.mark.parametrize(("family", "case_id"), CASES, ids=[c for _, c in CASES])
def test_kl_per_step_restates_kl_loss(family: str, case_id: str, balancing: bool) -> None:  # noqa: FBT001
    """The mean over [B, T] of the per-step form has ``kl_loss``'s value and its gradients with respect to both logits, under KL
    balancing (the weights the kernels get) and under the plain KL (weights (1, 1))."""
    from multimodal_mtrssm_amd.distributions import KL_BALANCE_ALPHA

    pr = _problem(case_id)
    out64, _ = reference_gradients(pr.ref64, pr, "all")
    weights = (1.0 - KL_BALANCE_ALPHA, KL_BALANCE_ALPHA) if balancing else (1.0, 1.0)
    for sfx, cats, classes in levels(pr.case):
        grads = []
        for form in ("per_step", "kl_loss"):
            q = out64[f"post_logits{sfx}"].detach().clone().requires_grad_()
            p = out64[f"prior_logits{sfx}"].detach().clone().requires_grad_()
            value = kl_per_step(q, p, cats, classes, weights).mean() if form == "per_step" else kl_loss(q, p, cats, classes, balancing)
            grads.append((value, *torch.autograd.grad(value, [q, p])))
        for got, want in zip(*grads, strict=True):
            torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
        plain = kl_loss(out64[f"post_logits{sfx}"].detach(), out64[f"prior_logits{sfx}"].detach(), cats, classes, False)  # noqa: FBT003
        torch.testing.assert_close(grads[0][0], plain, rtol=1e-12, atol=1e-14)  # the value is the plain KL either way


@pytest.mark.parametrize(("family", "case_id"), CASES, ids=[c for _, c in CASES])
def test_fp32_oracle_gradient_error_against_float64(family: str, case_id: str, baselines: dict) -> None:
    """The measured baseline: for `all` and two single-output sets, every gradient of the fp32 oracle against float64.  The
    family's GPU bound (16 x the family's largest figure, rounded up) must keep at least three bits above this case's figure."""
    pr = _problem(case_id)
    worst = (0.0, "", "")
    for cot in ("all", *HOST_SINGLE_SETS[pr.case.kind]):
        _, g32 = reference_gradients(pr.oracle, pr, cot)
        _, g64 = reference_gradients(pr.ref64, pr, cot)
        compared = 0
        for name, want in g64.items():
            if want is None or float(want.abs().max()) == 0.0:
                assert g32[name] is None or float(g32[name].abs().max()) == 0.0, (cot, name)
                continue
            err = relative_error(g32[name], want)
            compared += 1
            if err > worst[0]:
                worst = (err, name, cot)
        assert compared >= 10, (cot, compared)  # noqa: PLR2004
    print(f"{case_id} ({family}): seed {pr.seed}, margin {pr.margin:.2e}, largest fp32-oracle gradient error {worst[0]:.2e} at {worst[1]} ({worst[2]})")
    baselines[case_id] = (family, pr.seed, pr.margin, *worst)
    assert worst[0] * 8.0 <= GRAD_BOUND[family], (worst, GRAD_BOUND[family])


def test_bounds_follow_from_the_recorded_baselines() -> None:
    """Every family's bound is 16 x its recorded baseline, rounded up to one significant digit."""
    for family, baseline in HOST_BASELINE.items():
        digit, exponent = f"{16.0 * baseline:.12e}".split("e")
        want = float(f"{math.ceil(float(digit) - 1e-9)}e{exponent}")
        assert math.isclose(GRAD_BOUND[family], want, rel_tol=1e-12), (family, baseline, want)


@pytest.mark.parametrize(("family", "case_id"), CASES, ids=[c for _, c in CASES])
def test_first_half_functional_has_zero_late_input_gradients(family: str, case_id: str) -> None:
    """``all_first_half``: the float64 gradients with respect to the actions and embeddings at ``t >= T // 2`` are exactly zero, and
    those before are not: the GPU test's expectation is the reference's."""
    pr = _problem(case_id)
    _, g64 = reference_gradients(pr.ref64, pr, "all_first_half")
    half = pr.case.steps // 2
    assert half >= 1
    for name in ("in/actions", "in/audio_embed", "in/vision_embed"):
        late, early = g64[name][:, half:], g64[name][:, :half]
        assert torch.equal(late, torch.zeros_like(late)), name
        assert float(early.abs().max()) > 0.0, name
