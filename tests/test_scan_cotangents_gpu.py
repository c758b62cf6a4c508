"""GPU (MI355X): the five scan families' reverse-time kernels, one output cotangent pattern at a time, against float64.

The scans are called on their own (``scan.mrssm_posterior_rollout`` / ``scan.mmtrssm_posterior_rollout``) on the random problem
of ``tests/scan_cotangents.py``; a fixed random linear functional reads one output alone (6 sets for MRSSM, 14 for MMTRSSM), all
outputs, all outputs at ``t < T // 2`` only, or all outputs of a rollout without a prior draw.  Each set reaches the BPTT kernel
as its own pattern of null gradient pointers.  Compared with the float64 copy of the oracle: samples exactly; ``deter`` /
``hidden``, the probabilities of every logits output and the KL per step to 1e-5 (the wide families, on three bf16 pieces,
+ 5e-6); the gradients with respect to actions, both embeddings, every initial state tensor (the one-hot samples included),
every parameter, and the expert log-weights of the masked arm, relative to the float64 tensor's largest entry, to

    single-CU MRSSM 2e-5   cluster 2e-5   wide MRSSM 2e-5   single-CU MMTRSSM 9e-6   wide MMTRSSM 2e-5

which is 16 x the largest error of the fp32 oracle against float64 over the family's cases, rounded up to one digit
(``tests/test_scan_cotangents_host.py`` measures it; ``profiles/scan_cotangent_errors.md`` holds the baselines, the reasoning
behind the factor and the largest errors observed on the GPU).  A gradient the reference does not produce, or has exactly zero,
must be None or exactly zero.  The two-piece runs of the wide families use the bounds ``scan.py`` states for two pieces:
probabilities 1.5e-5, the mean KL 1e-4 relative, gradients 1e-3.

The cooperative kernels need the GPU to themselves: run this file in one process."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
from torch import Tensor

from oracle.ref_model import cat_probs
from tests.conftest import product_from_case
from tests.scan_cotangents import (COOPERATIVE, FAMILY_CASES, GRAD_BOUND, MASKED_CASES, ROW_COUNT_RUNS, TWO_PIECE_GRADS, TWO_PIECE_LOSS_RTOL,
                                   TWO_PIECE_PROBS, VALUE_ATOL, WIDE_EXTRA, WIDE_FAMILIES, Problem, build_problem, cast_inputs, case_of,
                                   chosen_outputs, cotangent_sets, functional, levels, masked_sets, reference_gradients,
                                   relative_error, sample_index, state_keys)
from tests.test_config_matrix_gpu import _scan_kernels, lib_loaded  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIECES = 3  # the wide families run on three bf16 pieces per operand: what the value and gradient bounds are stated for


@functools.lru_cache(maxsize=1)  # the cotangent set varies fastest: the runs of a case share its problem, reference and model
def _setup(case_id: str, batch: int | None, steps: int | None, masked: bool) -> tuple[Problem, torch.nn.Module]:  # noqa: FBT001
    pr = build_problem(case_id, batch=batch, steps=steps, masked=masked)
    return pr, product_from_case(pr.case, pr.oracle, DEV)


def _rollout(pr: Problem, model: torch.nn.Module, leaves: dict[str, Tensor], noise: dict[str, Tensor | None]) -> dict[str, Tensor | None]:
    from multimodal_mtrssm_amd import scan

    codes = None if pr.codes is None else pr.codes.to(device=DEV, dtype=torch.int32)
    logw = leaves.get("expert_logw")
    a, ea, ev = leaves["actions"], leaves["audio_embed"], leaves["vision_embed"]
    if pr.case.kind == "mrssm":
        return scan.mrssm_posterior_rollout(model.transition, model.audio_representation, model.vision_representation, a, ea, ev,
                                            leaves["deter"], leaves["stoch"], noise["u_post"], noise["u_prior"],
                                            balancing=bool(model.use_kl_balancing), modality=codes, expert_logw=logw)
    return scan.mmtrssm_posterior_rollout(model, a, ea, ev, {k: leaves[k] for k in state_keys(pr.case)}, noise, modality=codes,
                                          expert_logw=logw)


def run_and_compare(pr: Problem, model: torch.nn.Module, cot: str, pieces: int = PIECES) -> None:  # noqa: PLR0912, PLR0914, PLR0915
    """One forward and backward scan of ``pr`` on the GPU with the functional of ``cot`` against the float64 reference; every
    figure is printed before the first assertion."""
    from multimodal_mtrssm_amd import _lib, scan

    case, family = pr.case, pr.family
    wide = family in WIDE_FAMILIES
    two = wide and pieces == 2  # noqa: PLR2004
    ref_out, ref_grads = reference_gradients(pr.ref64, pr, cot)
    leaves = cast_inputs(pr, torch.float32, DEV)
    noise: dict[str, Tensor | None] = {k: v.to(DEV) for k, v in pr.noise.items()}
    if cot == "no_prior_draw":
        noise = {k: (None if k.startswith("u_prior") else v) for k, v in noise.items()}
    model.zero_grad(set_to_none=True)
    saved = (scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES)
    scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES = True, True, pieces
    _lib.TIMERS.enable()
    try:
        out = _rollout(pr, model, leaves, noise)
        functional(pr, out, cot).backward()
        torch.cuda.synchronize()
        launched = set(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
        scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES = saved
    tag = f"{family} {case.name} B{case.batch} T{case.steps} {'masked ' if pr.codes is not None else ''}{cot} p{pieces if wide else '-'}"

    # (1) the family's forward and BPTT kernels ran, and only those
    fwd, bwd = _scan_kernels(family, case, pieces)
    scans = {k for k in launched if k.startswith(("mtrssm::mrssm_", "mtrssm::mmtrssm_"))}
    assert any(k.startswith(fwd) for k in scans), (fwd, sorted(scans))
    assert any(k.startswith(bwd) for k in scans), (bwd, sorted(scans))
    assert all(k.startswith((fwd, bwd)) for k in scans), sorted(scans)
    if family in COOPERATIVE:
        scan.check_cluster_status()

    problems: list[str] = []
    # (2) samples: one-hot, and the reference's indices
    for sfx, cats, classes in levels(case):
        for which in ("post", "prior"):
            key = f"{which}_stoch{sfx}"
            if out[key] is None:
                assert cot == "no_prior_draw" and which == "prior"
                continue
            s = out[key].detach().reshape(*out[key].shape[:-1], cats, classes)
            if not bool((((s == 0) | (s == 1)).all() & (s.sum(-1) == 1).all()).item()):
                problems.append(f"{key} is not one-hot")
            if not torch.equal(sample_index(out[key], cats, classes), sample_index(ref_out[key], cats, classes)):
                problems.append(f"{key} differs from the reference's samples")
    # (3) values
    atol = TWO_PIECE_PROBS if two else VALUE_ATOL + (WIDE_EXTRA if wide else 0.0)
    figures = []
    for key, want in ref_out.items():
        if out[key] is None or "stoch" in key:
            continue
        got, want = out[key].detach().double().cpu(), want.detach()
        if "logits" in key:
            sfx = key[-2:] if key[-2:] in {"_l", "_h"} else ""
            cats, classes = next((k, c) for s, k, c in levels(case) if s == sfx)
            err = float((cat_probs(got, cats, classes)[1] - cat_probs(want.detach(), cats, classes)[1]).abs().max())
        elif two and key.startswith("kl"):
            err = abs(float(got.mean()) - float(want.mean())) / abs(float(want.mean()))
            figures.append(f"mean {key} {err:.1e}")
            if err > TWO_PIECE_LOSS_RTOL:
                problems.append(f"mean {key}: {err:.3e} relative > {TWO_PIECE_LOSS_RTOL}")
            continue
        elif two:
            continue  # deter / hidden carry no stated bound at two pieces: left to the three-piece run
        else:
            err = float((got - want.detach()).abs().max())
        figures.append(f"{key} {err:.1e}")
        if err > atol:
            problems.append(f"value {key}: {err:.3e} > {atol}")
    print(f"cot-values {tag}: " + ", ".join(figures))
    # (4) gradients
    bound = TWO_PIECE_GRADS if two else GRAD_BOUND[family]
    params = dict(model.named_parameters())
    worst, near, compared = (0.0, ""), [], 0
    for name, want in ref_grads.items():
        got = leaves[name[3:]].grad if name.startswith("in/") else params[name].grad
        if want is None or float(want.abs().max()) == 0.0:
            if got is not None and float(got.abs().max()) != 0.0:
                problems.append(f"grad {name}: the reference has none, the GPU's largest entry is {float(got.abs().max()):.3e}")
            continue
        if got is None:
            problems.append(f"grad {name}: missing on the GPU")
            continue
        err = relative_error(got, want)
        compared += 1
        if err > worst[0]:
            worst = (err, name)
        if err > bound / 2:
            near.append(f"{name} {err:.2e}")
        if not err <= bound:
            problems.append(f"grad {name}: {err:.3e} of its largest entry > {bound}")
    print(f"cot-grads {tag}: {compared} tensors, largest error {worst[0]:.2e} at {worst[1]}, bound {bound}; above half the bound: {near or 'none'}")
    if compared < 8:  # noqa: PLR2004
        problems.append(f"only {compared} gradients compared")
    # (5) exact zeros
    if cot == "all_first_half":
        half = case.steps // 2
        for key in ("actions", "audio_embed", "vision_embed"):
            late = leaves[key].grad[:, half:]
            if not torch.equal(late, torch.zeros_like(late)):
                problems.append(f"grad in/{key} at t >= T // 2 is not exactly zero: {float(late.abs().max()):.3e}")
    if pr.codes is not None:
        off = (pr.codes != 3).to(DEV)  # noqa: PLR2004
        g_lw = leaves["expert_logw"].grad
        if g_lw is None or not torch.equal(g_lw[off], torch.zeros_like(g_lw[off])):
            problems.append("grad in/expert_logw is not exactly zero where not both modalities are present")
        g_ref = ref_grads["in/expert_logw"]
        assert torch.equal(g_ref[pr.codes != 3], torch.zeros_like(g_ref[pr.codes != 3]))  # noqa: PLR2004
    assert not problems, tag + ":\n" + "\n".join(problems)


# ---------------------------------------------------------------------------------------------
# 1. every family's cases x every cotangent set
# ---------------------------------------------------------------------------------------------
RUNS = [(family, case_id, cot) for family, ids in FAMILY_CASES.items() for case_id in ids for cot in cotangent_sets(case_of(case_id)[0])]


@pytest.mark.parametrize(("family", "case_id", "cot"), RUNS, ids=[f"{c}-{s}" for _, c, s in RUNS])
def test_cotangent_set_matches_float64(family: str, case_id: str, cot: str, lib_loaded: None) -> None:  # noqa: F811
    """One cotangent set of one case on its family's own kernels (fast8 and the general categorical block of each family)."""
    pr, model = _setup(case_id, None, None, False)  # noqa: FBT003
    assert pr.family == family and len(chosen_outputs(pr.case, cot)) >= 1
    run_and_compare(pr, model, cot)


# ---------------------------------------------------------------------------------------------
# 2. more rows than one cluster / one row tile takes at once
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("case_id", "batch", "steps"), ROW_COUNT_RUNS, ids=[f"{c}-B{b}" for c, b, _ in ROW_COUNT_RUNS])
def test_row_counts_match_float64(case_id: str, batch: int, steps: int, lib_loaded: None) -> None:  # noqa: F811
    """`all` at B = 70 (a cluster walks two rows; wide MMTRSSM: three row tiles, the last ragged) and B = 37 (wide MRSSM: the second
    row tile is ragged)."""
    pr, model = _setup(case_id, batch, steps, False)  # noqa: FBT003
    run_and_compare(pr, model, "all")


# ---------------------------------------------------------------------------------------------
# 3. the wide families at the shipped two bf16 pieces (an arm check, with the bounds scan.py states for them)
# ---------------------------------------------------------------------------------------------
TWO_PIECE_RUNS = [c for f in ("wide", "mt_wide") for c in FAMILY_CASES[f]]


@pytest.mark.parametrize("case_id", TWO_PIECE_RUNS)
def test_two_pieces_match_float64(case_id: str, lib_loaded: None) -> None:  # noqa: F811
    pr, model = _setup(case_id, None, None, False)  # noqa: FBT003
    run_and_compare(pr, model, "all", pieces=2)


# ---------------------------------------------------------------------------------------------
# 4. the masked and weighted instances
# ---------------------------------------------------------------------------------------------
MASKED_RUNS = [(case_id, cot) for case_id in MASKED_CASES for cot in masked_sets(case_of(case_id)[0])]


@pytest.mark.parametrize(("case_id", "cot"), MASKED_RUNS, ids=[f"{c}-{s}" for c, s in MASKED_RUNS])
def test_masked_weighted_cotangent_set_matches_float64(case_id: str, cot: str, lib_loaded: None) -> None:  # noqa: F811
    """Four-way modality codes and explicit per-step expert weights (``tests/test_expert_weights_oracle.py``'s): the MASKED kernel
    instances, with the gradient of the expert log-weights, exactly zero where not both modalities are present."""
    pr, model = _setup(case_id, None, None, True)  # noqa: FBT003
    assert pr.codes is not None and {0, 1, 2, 3} <= set(np.unique(pr.codes.numpy()).tolist())
    run_and_compare(pr, model, cot)
