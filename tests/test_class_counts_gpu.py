"""GPU (MI355X): the general categorical block of the scans -- class counts above 8 in every scan family, more than 64
categoricals on the single-CU kernels -- the initial-state head kernel on its own, the tie rule of the inverse CDF on exact
arithmetic, and saturated logits (``tests/class_counts.py`` holds the cases, ``tests/test_class_counts_host.py`` checks their
oracle side on the CPU).

Tolerances of the parity runs are those of ``tests/test_config_matrix_gpu.py`` (its docstring), whose comparison they call:
losses 2e-5 relative, values 1e-5 absolute (wide families + 5e-6), samples exact, gradients 2e-4 of the tensor's max (wide
1e-3), the wide families on three bf16 pieces; on the shipped two pieces the bounds ``scan.py`` states for them
(probabilities 1e-5 + 5e-6, losses 1e-4 relative, gradients 1e-3, samples exact)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from oracle.cases import build_batch, build_model
from tests.class_counts import (CLASS_CASES, COOPERATIVE, HEAD_SHAPES, HEAD_USES, MASKED_CASES, PARITY_RUNS, SATURATED_CASES, TIE_CASES,
                                edge_noise, flatten_heads, floor_index, head_functional, head_problem, head_reference_grad,
                                tie_draws)
from tests.config_matrix import options, screened, with_options
from tests.conftest import product_from_case
from tests.test_config_matrix_gpu import _index, _np, _scan_kernels, _to, compare_scan_family, lib_loaded  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _assert_family_ran(launched: set[str], family: str, case, pieces: int) -> None:  # noqa: ANN001
    """The scan kernels among the timed launches are the family's forward and BPTT kernels, and only those."""
    fwd, bwd = _scan_kernels(family, case, pieces)
    scans = {k for k in launched if k.startswith(("mtrssm::mrssm_", "mtrssm::mmtrssm_"))}
    assert any(k.startswith(fwd) for k in scans), (fwd, sorted(scans))
    assert any(k.startswith(bwd) for k in scans), (bwd, sorted(scans))
    assert all(k.startswith((fwd, bwd)) for k in scans), sorted(scans)


# ---------------------------------------------------------------------------------------------
# 1. parity with the oracle at C > 8 and K > 64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("case_id", "option_set", "pieces"), PARITY_RUNS, ids=[f"{c}-{o or 'default'}-p{p}" for c, o, p in PARITY_RUNS])
def test_class_count_matches_oracle(case_id: str, option_set: str | None, pieces: int, lib_loaded: None) -> None:  # noqa: F811
    """``test_scan_family_with_options_matches_oracle``'s comparison at the default options (ELU, KL balancing) and under Tanh with
    plain KL, at class counts above 8: cluster 32 / 64 / 128 / 200, wide MRSSM, single-CU MRSSM and MMTRSSM, wide MMTRSSM with
    either level above 8.  The kernel names show that the cooperative kernels (whose ``C <= 8`` branch then takes the general
    block) ran, and that ``s32_2x70`` and ``w256_2x65`` (more than 64 categoricals) ran on the single-CU kernels alone."""
    base, family = CLASS_CASES[case_id]
    case = with_options(base, **options(base, option_set)) if option_set else base
    oracle = build_model(case)
    batch = build_batch(case)
    noise, _margin, _seed = screened(case, oracle, batch)
    compare_scan_family(case, family, oracle, batch, noise, pieces=pieces)


@pytest.mark.parametrize("case_id", MASKED_CASES)
def test_class_count_masked_weighted_matches_oracle(case_id: str, lib_loaded: None) -> None:  # noqa: F811
    """One masked and weighted run per cooperative family (the ``MASKED`` instantiations hold their own copy of the branch): a
    per-step modality code in {0, 1, 2, 3} and explicit per-step expert weights, built and compared as
    ``tests/test_expert_weights_oracle.py`` does, with its tolerances; the wide families on three bf16 pieces."""
    from multimodal_mtrssm_amd import _lib, scan
    from tests.test_expert_weights_oracle import _close_to_scale, _compare, codes_of, explicit_weights, weighted_step
    from tests.test_expert_weights_oracle import screened as screened_weighted

    case, family = CLASS_CASES[case_id]
    oracle = build_model(case)
    batch = build_batch(case)
    codes = codes_of("fourway", case.batch, case.steps)
    lw = explicit_weights(case.batch, case.steps).requires_grad_()
    lw_of = lambda _ea, _ev: lw  # noqa: E731
    noise, margin = screened_weighted(case, oracle, batch, codes, lw_of)
    assert margin >= 1e-5, margin  # noqa: PLR2004
    ref = weighted_step(case, oracle, batch, noise, codes, lw_of)
    ref["_logw"] = lw
    ref["loss"].backward()
    model = product_from_case(case, oracle, DEV)
    lw_dev = lw.detach().to(DEV).requires_grad_()
    saved = scan.WIDE_PIECES
    scan.WIDE_PIECES = 3
    _lib.TIMERS.enable()
    try:
        _compare(case, oracle, model, batch, noise, codes, ref, lw_dev=lw_dev, masked=True)
        launched = set(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
        scan.WIDE_PIECES = saved
    _assert_family_ran(launched, family, case, 3)
    assert _close_to_scale(lw_dev.grad, lw.grad, "grad expert_log_weights")
    scan.check_cluster_status()


# ---------------------------------------------------------------------------------------------
# 2. the initial-state head kernel on its own
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use", HEAD_USES)
@pytest.mark.parametrize(("rows", "cats", "classes"), HEAD_SHAPES)
def test_categorical_head_kernel(rows: int, cats: int, classes: int, use: str, lib_loaded: None) -> None:  # noqa: F811
    """``core._CategoricalHead`` (one thread per (row, categorical)) against float64 on the CPU: log_softmax, softmax,
    ``oracle.ref_dists.inverse_cdf_index`` and autograd.  Probabilities and log-probabilities to 1e-6 absolute, samples exact,
    the gradient of a fixed random functional to 2e-6 of its max (fp32 expf / logf and sums of at most 33 terms); the functional
    reads every output, the sample alone (``g_l`` null in the backward kernel) or the log-probabilities alone (``g_p`` null)."""
    from multimodal_mtrssm_amd import _lib
    from multimodal_mtrssm_amd.core import _CategoricalHead

    pr = head_problem(rows, cats, classes)
    x = pr["logits"].to(DEV).requires_grad_()
    sample, logp, probs = _CategoricalHead.apply(x, pr["u"].to(DEV), cats, classes)
    assert _lib.load().mtrssm_last_kernel().decode() == "mtrssm::categorical_sample_fwd_kernel"
    assert sample.shape == (rows, cats * classes) and logp.shape == probs.shape == (rows, cats, classes)
    np.testing.assert_allclose(_np(probs), pr["probs"].numpy(), rtol=0, atol=1e-6, err_msg="probs")
    np.testing.assert_allclose(_np(logp), pr["logp"].numpy(), rtol=0, atol=1e-6, err_msg="logp")
    s = _np(sample).reshape(rows, cats, classes)
    assert ((s == 0) | (s == 1)).all() and (s.sum(-1) == 1).all()
    assert (s.argmax(-1) == pr["index"].numpy()).all(), "samples"
    head_functional(sample, logp, probs, pr["weights"], use).backward()
    want = head_reference_grad(pr, use)
    scale = float(want.abs().max())
    np.testing.assert_allclose(_np(x.grad), want.numpy(), rtol=0, atol=2e-6 * scale, err_msg=f"d logits ({use})")


# ---------------------------------------------------------------------------------------------
# 3. the tie rule, exactly
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(TIE_CASES))
def test_uniform_logits_sample_floor_uC(case_id: str, lib_loaded: None) -> None:  # noqa: F811, N802
    """Constant logit rows (last-layer weights of every head zero, biases 0.3) over a power-of-two class count: exp(0) = 1, the
    sum C, 1 / C and the running sums j / C are exact in fp32, in libm and in the hardware exp / rcp, and after the MoPoE mix.
    With uniforms ON the edges j / C, one fp32 number below them, at 0 and at 1 - 2^-24, every posterior and prior sample and
    the initial state's has the index floor(u C) (float64, on the host): an edge belongs to the class above it (``<=``).  Every
    KL is 0.0 exactly.  General block: 16 x 2 and 32 x 1 (cluster), 16 x 8 (wide), 16 x 2 over 4 x 4 (wide MMTRSSM); fast8 and
    single-CU: the 4 x 4, 2 x 8 cases."""
    from multimodal_mtrssm_amd import _lib, scan

    case, family = TIE_CASES[case_id]
    model = product_from_case(case, flatten_heads(build_model(case)), DEV)
    noise = edge_noise(case)
    gbatch, gnoise = tuple(b.to(DEV) for b in build_batch(case)), _to(noise, DEV)
    _lib.TIMERS.enable()
    try:
        with torch.no_grad():
            state0 = model.initial_state((gbatch[1][:, 0], gbatch[2][:, 0]), gnoise)
            post, prior = model.rollout_representation(actions=gbatch[0], observations=(gbatch[1], gbatch[2]), prev_state=state0,
                                                       noise=gnoise)
        out = model.shared_step(gbatch, gnoise)
        out["loss"].backward()
        torch.cuda.synchronize()
        launched = set(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
    _assert_family_ran(launched, family, case, scan.WIDE_PIECES)
    sfx = {"": ""} if case.kind == "mrssm" else {"_l": "_l", "_h": "_h"}
    got = {}
    for s in sfx:
        got[f"_init_stoch{s}" if s else "_stoch0"] = getattr(state0, f"stoch{s}")
        got[f"_post_stoch{s}"] = getattr(post, f"stoch{s}")
        got[f"_prior_stoch{s}"] = getattr(prior, f"stoch{s}")
    for key, stoch, _logits, cats, classes in tie_draws(case):
        want = floor_index(noise[key], classes).numpy()
        index = _index(got[stoch], cats, classes)
        assert (index == want).all(), f"{key}: {int((index != want).sum())} of {want.size} draws off the rule"
    kls = [post.kl_per_step] if case.kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]
    for kl in kls:
        assert torch.equal(kl, torch.zeros_like(kl)), "KL per step"
    for k in out:
        if k.startswith("kl"):
            assert float(out[k].detach()) == 0.0, k
    if family in COOPERATIVE:
        scan.check_cluster_status()


# ---------------------------------------------------------------------------------------------
# 4. saturated logits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(SATURATED_CASES))
def test_saturated_heads_match_oracle(case_id: str, lib_loaded: None) -> None:  # noqa: F811
    """Test 1's comparison with the heads' last-layer gain at 150 instead of 4: max |logit| 27 to 56, KLs of 65 to 118, most
    probabilities of a categorical underflow in ``__expf``.  Same tolerances (the fp32 oracle keeps a tenth of the loss and
    gradient bounds against float64: test_saturated_oracle_agrees_with_float64); every output and gradient is finite."""
    case, family = SATURATED_CASES[case_id]
    oracle = build_model(case)
    batch = build_batch(case)
    noise, _margin, _seed = screened(case, oracle, batch)
    model, out, state0, post, prior = compare_scan_family(case, family, oracle, batch, noise)
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), k
    for name, state in (("state0", state0), ("post", post), ("prior", prior)):
        for attr in ("deter", "stoch", "deter_l", "deter_h", "hidden_l", "hidden_h", "stoch_l", "stoch_h"):
            if hasattr(state, attr):
                assert bool(torch.isfinite(getattr(state, attr)).all()), f"{name}.{attr}"
    kls = [post.kl_per_step] if case.kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]
    for kl in kls:
        assert bool(torch.isfinite(kl).all()), "KL per step"
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), f"grad {k}"
