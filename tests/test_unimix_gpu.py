"""GPU (MI355X): uniform mixing of the categorical latents inside the five scan families against the
float64 reference of ``tests/unimix_reference.py``.

Same structure as ``tests/test_scan_cotangents_gpu.py`` (the scans called on their own on that file's random problem, a fixed
random linear functional over a chosen set of outputs, three bf16 pieces for the wide families) with ``unimix = eps`` on the
model's factories: samples exactly; ``deter`` / ``hidden``, the probabilities of every logits output and the KL per step to
``VALUE_ATOL`` (wide: ``+ WIDE_EXTRA``); gradients at every input, initial-state tensor and parameter to the family's
``GRAD_BOUND``, relative to the float64 tensor's largest entry (``tests/test_unimix_host.py`` shows that the fp32 reference stays
within the families' ``HOST_BASELINE`` under unimix, so the bounds hold as they are).  Every model here is built with the
``unimix=`` keyword: on a tree without the feature each test fails with a TypeError, and a kernel that ignores the field misses
the values and the gradients.

The cooperative kernels need the GPU to themselves: run this file in one process."""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch
from torch import Tensor

from oracle.cases import CASES, build_batch, build_model, with_sizes
from oracle.ref_model import cat_probs
from oracle.ref_dists import sampling_margin
from tests.config_matrix import SAMPLING_MARGIN, SEEDS
from tests.scan_cotangents import (COOPERATIVE, FAMILY_CASES, GRAD_BOUND, MASKED_CASES, ROW_COUNT_RUNS, VALUE_ATOL, WIDE_EXTRA,
                                   WIDE_FAMILIES, Problem, _draw_noise, cast_inputs, case_of, functional, levels, masked_sets,
                                   relative_error, sample_index, state_keys)
from tests.test_config_matrix_gpu import _scan_kernels, lib_loaded  # noqa: F401  (a fixture)
from tests.unimix_reference import (EPS, EPS_LARGE, build_unimix_problem, kl_bound, prior_rollout, saturated_kl_error, unimix_gradients,
                                    unimix_sets)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PIECES = 3  # the wide families run on three bf16 pieces per operand: what the value and gradient bounds are stated for
# Two runs of ONE model already differ in the last bits wherever the library splits a reduction and lets the slices meet by fp32
# atomics (``linear.py``'s module docstring: every weight gradient, small grids; the encoders' Linear layers): "the same bits" can be
# asked of what the scan kernels write themselves.  Sums that pass such a GEMM are compared to a reordered fp32 sum's error: the
# slices of a split reduction number at most 64, each partial rounded to 2^-24 of the largest.
ATOMIC_ORDER = 64 * 2.0 ** -24
FIRST = {family: ids[0] for family, ids in FAMILY_CASES.items()}  # one case per family


def product(case, oracle_model: torch.nn.Module, unimix: float | None):  # noqa: ANN001, ANN201
    """``tests.conftest.product_from_case`` with the ``unimix`` keyword (None: the keyword is not passed at all)."""
    import multimodal_mtrssm_amd as mt

    d = case.dims
    kw = {} if unimix is None else {"unimix": unimix}
    if case.kind == "mrssm":
        model = mt.make_mrssm(
            deter=d.deter, hidden=d.hidden, classes=d.classes, cats=d.cats, action=d.action, embed=d.embed,
            enc_audio=d.enc_audio, enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision,
            activation=d.activation, init_cells=d.init_cells, kl_coeff=d.kl_coeff, use_kl_balancing=d.use_kl_balancing, **kw)
    else:
        model = mt.make_mmtrssm(
            hd=d.hd, hs=(d.hs_classes, d.hs_cats), ld=d.ld, ls=(d.ls_classes, d.ls_cats), hidden=d.hidden, action=d.action,
            embed=d.embed, enc_audio=d.enc_audio, enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision,
            l_tau=d.l_tau, h_tau=d.h_tau, activation=d.activation, init_cells=d.init_cells, kl_coeff=d.kl_coeff,
            w_kl_h=d.w_kl_h, use_kl_balancing=d.use_kl_balancing, **kw)
    result = model.load_state_dict(oracle_model.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    return model.to(DEV)


@functools.lru_cache(maxsize=1)  # the cotangent set varies fastest: the runs of a case share its problem, reference and model
def _setup(case_id: str, eps: float, batch: int | None, steps: int | None, masked: bool, saturated: bool) -> tuple[Problem, torch.nn.Module]:  # noqa: FBT001, PLR0913
    pr = build_unimix_problem(case_id, eps, batch=batch, steps=steps, masked=masked, saturated=saturated)
    return pr, product(pr.case, pr.oracle, eps)


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


def _run(pr: Problem, model: torch.nn.Module, cot: str) -> tuple[dict[str, Tensor | None], dict[str, Tensor], set[str]]:
    """One forward and backward scan of ``pr`` with the functional of ``cot`` on the family's own kernels: (outputs, input
    leaves, the kernels launched)."""
    from multimodal_mtrssm_amd import _lib, scan

    leaves = cast_inputs(pr, torch.float32, DEV)
    noise: dict[str, Tensor | None] = {k: v.to(DEV) for k, v in pr.noise.items()}
    if cot == "no_prior_draw":
        noise = {k: (None if k.startswith("u_prior") else v) for k, v in noise.items()}
    model.zero_grad(set_to_none=True)
    saved = (scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES)
    scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES = True, True, PIECES
    _lib.TIMERS.enable()
    try:
        out = _rollout(pr, model, leaves, noise)
        functional(pr, out, cot).backward()
        torch.cuda.synchronize()
        launched = set(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
        scan.CLUSTER_SCAN, scan.WIDE_SCAN, scan.WIDE_PIECES = saved
    fwd, bwd = _scan_kernels(pr.family, pr.case, PIECES)
    scans = {k for k in launched if k.startswith(("mtrssm::mrssm_", "mtrssm::mmtrssm_"))}
    assert any(k.startswith(fwd) for k in scans), (fwd, sorted(scans))
    assert any(k.startswith(bwd) for k in scans), (bwd, sorted(scans))
    assert all(k.startswith((fwd, bwd)) for k in scans), sorted(scans)
    if pr.family in COOPERATIVE:
        scan.check_cluster_status()
    return out, leaves, launched


def _check_samples(pr: Problem, out: dict, ref_out: dict, cot: str, problems: list[str]) -> None:
    for sfx, cats, classes in levels(pr.case):
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


def _check_values(pr: Problem, out: dict, ref_out: dict, tag: str, problems: list[str], *, skip_kl: bool = False) -> None:
    atol = VALUE_ATOL + (WIDE_EXTRA if pr.family in WIDE_FAMILIES else 0.0)
    figures = []
    for key, want in ref_out.items():
        if out.get(key) is None or "stoch" in key or (skip_kl and key.startswith("kl")):
            continue
        got, want = out[key].detach().double().cpu(), want.detach()
        if "logits" in key:
            sfx = key[-2:] if key[-2:] in {"_l", "_h"} else ""
            cats, classes = next((k, c) for s, k, c in levels(pr.case) if s == sfx)
            err = float((cat_probs(got, cats, classes)[1] - cat_probs(want, cats, classes)[1]).abs().max())
        else:
            err = float((got - want).abs().max())
        figures.append(f"{key} {err:.1e}")
        if err > atol:
            problems.append(f"value {key}: {err:.3e} > {atol}")
    print(f"unimix-values {tag}: " + ", ".join(figures))


def run_and_compare(pr: Problem, model: torch.nn.Module, cot: str, eps: float) -> None:  # noqa: PLR0912
    """``tests.test_scan_cotangents_gpu.run_and_compare`` against the unimix reference; every figure is printed before the first
    assertion.  The masked arm also demands posterior == prior and KL == 0 exactly on the steps with no modality."""
    case, family = pr.case, pr.family
    assert model.unimix == eps
    ref_out, ref_grads = unimix_gradients(pr.ref64, pr, cot, eps)
    out, leaves, _ = _run(pr, model, cot)
    tag = f"{family} {case.name} B{case.batch} T{case.steps} eps {eps} {'masked ' if pr.codes is not None else ''}{cot}"
    problems: list[str] = []
    _check_samples(pr, out, ref_out, cot, problems)
    _check_values(pr, out, ref_out, tag, problems)
    bound = GRAD_BOUND[family]
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
    print(f"unimix-grads {tag}: {compared} tensors, largest error {worst[0]:.2e} at {worst[1]}, bound {bound}; above half the bound: {near or 'none'}")
    if compared < 8:  # noqa: PLR2004
        problems.append(f"only {compared} gradients compared")
    if pr.codes is not None:
        none = (pr.codes == 0).to(DEV)
        assert bool(none.any())
        for sfx, _cats, _classes in levels(case):
            if not torch.equal(out[f"post_logits{sfx}"][none], out[f"prior_logits{sfx}"][none]):
                problems.append(f"post_logits{sfx} != prior_logits{sfx} on steps with no modality")
            kl = out[f"kl{sfx}"][none]
            if not torch.equal(kl, torch.zeros_like(kl)):
                problems.append(f"kl{sfx} is not exactly 0.0 on steps with no modality: {float(kl.abs().max()):.3e}")
        off = (pr.codes != 3).to(DEV)  # noqa: PLR2004
        g_lw = leaves["expert_logw"].grad
        if g_lw is None or not torch.equal(g_lw[off], torch.zeros_like(g_lw[off])):
            problems.append("grad in/expert_logw is not exactly zero where not both modalities are present")
    assert not problems, tag + ":\n" + "\n".join(problems)


# ---------------------------------------------------------------------------------------------
# 1. values and gradients at eps = 0.01: every family's cases x the cotangent sets
# ---------------------------------------------------------------------------------------------
RUNS = [(family, case_id, cot) for family, ids in FAMILY_CASES.items() for case_id in ids for cot in unimix_sets(case_of(case_id)[0])]


@pytest.mark.parametrize(("family", "case_id", "cot"), RUNS, ids=[f"{c}-{s}" for _, c, s in RUNS])
def test_unimix_matches_float64(family: str, case_id: str, cot: str, lib_loaded: None) -> None:  # noqa: F811
    pr, model = _setup(case_id, EPS, None, None, False, False)  # noqa: FBT003
    assert pr.family == family
    run_and_compare(pr, model, cot, EPS)


# ---------------------------------------------------------------------------------------------
# 2. a larger eps: a wrong (1 - eps) factor or eps / C cannot hide in 1 %
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FIRST))
def test_large_eps_matches_float64(family: str, lib_loaded: None) -> None:  # noqa: F811
    pr, model = _setup(FIRST[family], EPS_LARGE, None, None, False, False)  # noqa: FBT003
    run_and_compare(pr, model, "all", EPS_LARGE)


# ---------------------------------------------------------------------------------------------
# 3. the masked and weighted instances: posterior == prior and KL == 0 exactly where nothing is observed
# ---------------------------------------------------------------------------------------------
MASKED_RUNS = [(case_id, cot) for case_id in MASKED_CASES for cot in masked_sets(case_of(case_id)[0])]


@pytest.mark.parametrize(("case_id", "cot"), MASKED_RUNS, ids=[f"{c}-{s}" for c, s in MASKED_RUNS])
def test_masked_weighted_unimix_matches_float64(case_id: str, cot: str, lib_loaded: None) -> None:  # noqa: F811
    pr, model = _setup(case_id, EPS, None, None, True, False)  # noqa: FBT003
    assert pr.codes is not None and {0, 1, 2, 3} <= set(np.unique(pr.codes.numpy()).tolist())
    run_and_compare(pr, model, cot, EPS)


# ---------------------------------------------------------------------------------------------
# 4. more rows than one cluster / one row tile takes at once
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("case_id", "batch", "steps"), ROW_COUNT_RUNS, ids=[f"{c}-B{b}" for c, b, _ in ROW_COUNT_RUNS])
def test_row_counts_with_unimix_match_float64(case_id: str, batch: int, steps: int, lib_loaded: None) -> None:  # noqa: F811
    pr, model = _setup(case_id, EPS, batch, steps, False, False)  # noqa: FBT003
    run_and_compare(pr, model, "all", EPS)


# ---------------------------------------------------------------------------------------------
# 5. the prior-only scans (and their composed differentiable form)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["mrssm_nonsquare", "mmtrssm_default"])
def test_prior_only_rollout_with_unimix(case_id: str, lib_loaded: None) -> None:  # noqa: F811
    from multimodal_mtrssm_amd import scan

    pr, model = _setup(case_id, EPS, None, None, False, False)  # noqa: FBT003
    case = pr.case
    leaves64 = {k: v.detach() for k, v in cast_inputs(pr, torch.float64).items()}
    want = noise = None
    for seed in SEEDS:  # the open-loop trajectory is another one: its own screening, prior draws only
        noise = _draw_noise(case, seed, case.batch, case.steps)
        with torch.no_grad():
            want = prior_rollout(pr.ref64, case.kind, leaves64, noise, EPS)
        margin = min(float(sampling_margin(cat_probs(want[f"prior_logits{sfx}"], cats, classes)[1], noise[f"u_prior{sfx}"].double()).min())
                     for sfx, cats, classes in levels(case))
        if margin >= SAMPLING_MARGIN:
            break
    else:
        pytest.fail(f"{case_id}: no seed in {SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges of the open-loop trajectory")
    dn = {k: v.to(DEV) for k, v in noise.items()}
    for differentiable in (False, True):
        leaves = cast_inputs(pr, torch.float32, DEV)
        if not differentiable:
            leaves = {k: v.detach() for k, v in leaves.items()}
        with torch.set_grad_enabled(differentiable):
            if case.kind == "mrssm":
                got = scan.mrssm_prior_rollout(model.transition, leaves["actions"], leaves["deter"], leaves["stoch"], dn["u_prior"])
            else:
                got = scan.mmtrssm_prior_rollout(model, leaves["actions"], {k: leaves[k] for k in state_keys(case)}, dn)
        torch.cuda.synchronize()
        assert all(v.requires_grad == differentiable for k, v in got.items() if "logits" in k)
        problems: list[str] = []
        for sfx, cats, classes in levels(case):
            key = f"prior_stoch{sfx}"
            if not torch.equal(sample_index(got[key], cats, classes), sample_index(want[key], cats, classes)):
                problems.append(f"{key} differs from the reference's samples")
            probs = cat_probs(got[f"prior_logits{sfx}"].detach().double().cpu(), cats, classes)[1]
            if float(probs.min()) < EPS / classes * (1.0 - 1e-5):
                problems.append(f"prior probabilities{sfx} below eps / C: {float(probs.min()):.3e}")
        _check_values(pr, got, want, f"prior-only {case_id} {'composed' if differentiable else 'kernel'}", problems)
        assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------------------------
# 6. off means off
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FIRST))
def test_unimix_zero_is_the_default_bit_for_bit(family: str, lib_loaded: None) -> None:  # noqa: F811
    """``unimix=0.0`` passed explicitly against a model built without the keyword: every output of the scan and every gradient the
    reverse scan writes itself (the initial state's) bit for bit; the gradients behind a split-reduction GEMM (the inputs', the
    parameters') to ``ATOMIC_ORDER`` of the tensor's largest entry, the run-to-run difference of one model."""
    pr = build_unimix_problem(FIRST[family], 0.0)
    results = []
    for unimix in (None, 0.0):
        model = product(pr.case, pr.oracle, unimix)
        assert model.unimix == 0.0
        out, leaves, _ = _run(pr, model, "all")
        grads = {f"in/{k}": v.grad for k, v in leaves.items()} | {k: p.grad for k, p in model.named_parameters()}
        results.append(({k: v.detach().clone() for k, v in out.items()}, {k: None if g is None else g.clone() for k, g in grads.items()}))
    (out_a, grads_a), (out_b, grads_b) = results
    assert out_a.keys() == out_b.keys() and grads_a.keys() == grads_b.keys()
    for key in out_a:
        assert torch.equal(out_a[key], out_b[key]), key
    compared = 0
    for key, g in grads_a.items():
        assert (g is None) == (grads_b[key] is None), key
        if g is not None:
            if key[3:] in state_keys(pr.case) and key.startswith("in/"):
                assert torch.equal(g, grads_b[key]), key
            else:
                assert float((g - grads_b[key]).abs().max()) <= ATOMIC_ORDER * float(g.abs().max()), key
            compared += 1
    assert compared >= 10  # noqa: PLR2004


# ---------------------------------------------------------------------------------------------
# 7. saturated heads
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(FIRST))
def test_saturated_heads_are_bounded(family: str, lib_loaded: None) -> None:  # noqa: F811
    """Heads' last layers times 60: the KL per step at most ``K log(C / eps) (1 + 1e-5)``, samples exact, gradients finite, and
    the KL within 16 x the fp32 reference's own error against float64 on the same problem (``tests/test_unimix_host.py`` prints
    that error; ``profiles/unimix_notes.md`` records it)."""
    pr, model = _setup(FIRST[family], EPS, None, None, False, True)  # noqa: FBT003
    ref_out, _ = unimix_gradients(pr.ref64, pr, "all", EPS)
    host_err, scale = saturated_kl_error(pr, EPS)
    out, leaves, _ = _run(pr, model, "all")
    problems: list[str] = []
    _check_samples(pr, out, ref_out, "all", problems)
    for sfx, cats, classes in levels(pr.case):
        kl = out[f"kl{sfx}"].detach().double().cpu()
        bound = kl_bound(cats, classes, EPS) * (1.0 + 1e-5)
        err = float((kl - ref_out[f"kl{sfx}"].detach()).abs().max())
        print(f"unimix-saturated {family} {pr.case.name}{sfx}: KL per step up to {float(kl.max()):.4f} (bound {bound:.4f}); error against "
              f"float64 {err:.2e}, the fp32 reference's {host_err:.2e} on values up to {scale:.1f} (allowed {16.0 * host_err:.2e})")
        if not float(kl.max()) <= bound:
            problems.append(f"kl{sfx} {float(kl.max()):.6f} > {bound:.6f}")
        if not err <= 16.0 * host_err:
            problems.append(f"kl{sfx} error {err:.3e} > 16 x {host_err:.3e}")
    grads = [v.grad for v in leaves.values()] + [p.grad for p in model.parameters()]
    assert sum(g is not None for g in grads) >= 10  # noqa: PLR2004
    for g in grads:
        if g is not None and not bool(torch.isfinite(g).all()):
            problems.append("a gradient is not finite")
            break
    assert not problems, "\n".join(problems)


# ---------------------------------------------------------------------------------------------
# 8. model level
# ---------------------------------------------------------------------------------------------
def _to(noise: dict[str, Tensor], device: str) -> dict[str, Tensor]:
    return {k: v.to(device) for k, v in noise.items()}


def _kl64(post, prior, sfx: str) -> float:  # noqa: ANN001
    q = getattr(post, f"distribution{sfx}").probs.detach().double().cpu()
    p = getattr(prior, f"distribution{sfx}").probs.detach().double().cpu()
    return float((q * (q.log() - p.log())).sum(dim=(-1, -2)).mean())


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_model_step_with_unimix(name: str, lib_loaded: None) -> None:  # noqa: F811
    """``make_*(..., unimix=0.01)`` at the default dims, B = 2, T = 6: the step's ``kl`` (``kl_h``) is the KL of the returned
    states' distributions recomputed in float64 (to ``VALUE_ATOL`` per step, hence on their mean, times the coefficient), every
    probability keeps the floor, and ``initial_state`` does not depend on ``unimix``: from one embedding the two models' initial
    states are the same bits; through the encoders (whose Linear layers meet by atomics) the samples are the same and ``deter`` /
    the head's probabilities agree to ``ATOMIC_ORDER``."""
    from oracle.cases import build_noise

    case = with_sizes(CASES[name], 2, 6)
    oracle = build_model(case)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    noise = _to(build_noise(case), DEV)
    model, plain = product(case, oracle, EPS), product(case, oracle, 0.0)
    d = case.dims
    with torch.no_grad():
        out = model.shared_step(batch, noise)
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        s0_plain = plain.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, prior = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise)
        embed = model._initial_embed((batch[1][:, 0], batch[2][:, 0]), None)  # noqa: SLF001
        head_noise = noise.get("u_init") if case.kind == "mrssm" else noise
        e0, e0_plain = model._initial_from_embed(embed, head_noise), plain._initial_from_embed(embed, head_noise)  # noqa: SLF001
    torch.cuda.synchronize()
    sfxs = [""] if case.kind == "mrssm" else ["_l", "_h"]
    for sfx in sfxs:
        for key in (f"deter{sfx}", f"stoch{sfx}"):
            assert torch.equal(getattr(e0, key), getattr(e0_plain, key)), key
        assert torch.equal(getattr(s0, f"stoch{sfx}"), getattr(s0_plain, f"stoch{sfx}")), sfx
        a, b = getattr(s0, f"deter{sfx}"), getattr(s0_plain, f"deter{sfx}")
        assert float((a - b).abs().max()) <= ATOMIC_ORDER * float(b.abs().max()), sfx
        for key in ("logits", "probs"):
            assert torch.equal(getattr(getattr(e0, f"distribution{sfx}"), key), getattr(getattr(e0_plain, f"distribution{sfx}"), key)), (sfx, key)
        pa, pb = getattr(s0, f"distribution{sfx}").probs, getattr(s0_plain, f"distribution{sfx}").probs
        assert float((pa - pb).abs().max()) <= ATOMIC_ORDER, sfx
    coeff = {"": d.kl_coeff, "_l": d.kl_coeff, "_h": d.kl_coeff * getattr(d, "w_kl_h", 1.0)}
    for (sfx, cats, classes), key in zip(levels(case), ("kl", "kl_h"), strict=False):
        want = _kl64(post, prior, sfx) * coeff[sfx]
        got = float(out[key])
        print(f"unimix-model {name} {key}: {got:.7f}, float64 from the states' distributions {want:.7f}")
        assert abs(got - want) <= VALUE_ATOL * coeff[sfx], (key, got, want)
        assert got <= kl_bound(cats, classes, EPS) * coeff[sfx]
        for state in (post, prior):
            probs = getattr(state, f"distribution{sfx}").probs
            assert float(probs.min()) >= EPS / classes * (1.0 - 1e-5), (key, float(probs.min()))


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_captured_step_with_unimix_matches_eager(name: str, lib_loaded: None) -> None:  # noqa: F811
    """``tests.test_gpu_parity.test_captured_train_step_matches_eager`` with unimix on: a constant kernel argument is captured."""
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd.graph import CapturedTrainStep
    from multimodal_mtrssm_amd.optim import FlatParameters

    case = with_sizes(CASES[name], 2, 6)
    oracle = build_model(case)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    results = {}
    for mode in ("eager", "graph"):
        model = product(case, oracle, EPS)
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(2, 6)
        losses = []
        if mode == "eager":
            for _ in range(3):
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(batch, noise)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append([float(out["loss"]), float(out["kl"])])
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, batch, source, warmup=3)
            for _ in range(3):
                step = cap.step()
                losses.append([float(step["loss"]), float(step["kl"])])
            cap.close()
        scan.check_cluster_status()
        results[mode] = (losses, flat.param.clone())
    np.testing.assert_allclose(results["graph"][0], results["eager"][0], rtol=1e-4)
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_overshoot_step_with_unimix_respects_the_bound(name: str, lib_loaded: None) -> None:  # noqa: F811
    """A step with ``LatentOvershoot(depth=3)``: its rows run as steps with no modality and inherit the mixing, so every KL by
    row and distance is at most ``K log(C / eps)``."""
    import multimodal_mtrssm_amd as mt

    case = with_sizes(CASES[name], 2, 6)
    model = product(case, build_model(case), EPS)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    out = model.shared_step(batch, overshoot=mt.LatentOvershoot(depth=3))
    out["loss"].backward()
    torch.cuda.synchronize()
    assert math.isfinite(float(out["loss"])) and math.isfinite(float(out["overshoot"]))
    terms = model._overshoot_terms_last  # noqa: SLF001
    assert terms is not None and len(terms) == len(levels(case))
    for (sfx, cats, classes), term in zip(levels(case), terms, strict=True):
        plane = term.plane.detach()
        bound = kl_bound(cats, classes, EPS) * (1.0 + 1e-5)
        print(f"unimix-overshoot {name}{sfx}: KL by row and distance up to {float(plane.max()):.4f} (bound {bound:.4f})")
        assert 0.0 < float(plane.max()) <= bound
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())
