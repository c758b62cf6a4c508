"""Host side of the option matrix (``tests/config_matrix.py``; oracle only, no GPU): what keeps
``tests/test_config_matrix_gpu.py`` from being vacuous.  Every (case, option set) the GPU file runs builds and trains on the
oracle, the noise screening finds its seed, and each option actually changes what the oracle computes."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from oracle.cases import build_batch, build_model
from tests.config_matrix import (OPTION_SETS, RELU_MARGIN, RELU_VALUES_ONLY, SAMPLING_MARGIN, SCAN_CASES, SEEDS, options,
                                 relu_margin_for, screened, with_options)


@functools.cache
def _prepared(case_id: str, option_set: str):  # noqa: ANN202
    case = with_options(SCAN_CASES[case_id][0], **options(SCAN_CASES[case_id][0], option_set))
    oracle = build_model(case)
    batch = build_batch(case)
    noise, margin, seed = screened(case, oracle, batch, relu_margin_for(case_id, option_set))
    return case, oracle, batch, noise, margin, seed


@pytest.mark.parametrize("option_set", OPTION_SETS)
@pytest.mark.parametrize("case_id", list(SCAN_CASES))
def test_every_run_of_the_matrix_trains_on_the_oracle(case_id: str, option_set: str) -> None:
    """The oracle builds with the options, ``screened`` finds a seed within its 40 tries (for ReLU: one that also keeps every
    ReLU input 2e-5 from the kink, wherever the GPU file compares gradients), and ``shared_step`` + ``backward`` give finite
    losses and a gradient for the scan's parameters."""
    case, oracle, batch, noise, margin, seed = _prepared(case_id, option_set)
    assert case.batch * case.steps <= 45
    assert seed in SEEDS and margin >= SAMPLING_MARGIN
    d = case.dims
    opts = options(case, option_set)
    for k, v in opts.items():
        assert getattr(d, "activation" if k == "activation" else k) == v
    relu = [m for m in oracle.modules() if isinstance(m, torch.nn.ReLU)]
    assert bool(relu) == (option_set == "relu")
    if option_set == "relu":
        assert (relu_margin_for(case_id, option_set) == RELU_MARGIN) == (case_id not in RELU_VALUES_ONLY)
    oracle.zero_grad()
    out = oracle.shared_step(batch, noise)
    out["loss"].backward()
    keys = {k for k in out if not k.startswith("_")}
    assert keys == {"loss", "recon", "recon/audio", "recon/vision", "kl"} | ({"kl_h"} if case.kind == "mmtrssm" else set())
    for k in keys:
        assert torch.isfinite(out[k]), k
    grads = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
    assert len(grads) > 40
    for k, g in grads.items():
        assert torch.isfinite(g).all(), k
    head = "representation.rnn_to_post_projector.0.weight"
    assert float(grads[head].abs().max()) > 0.0


def _f(t: torch.Tensor) -> float:
    return float(t.detach())


def _step(case_id: str, noise: dict, **opts: object):  # noqa: ANN202
    case = with_options(SCAN_CASES[case_id][0], **opts)
    oracle = build_model(case)  # the seeded weights do not depend on the options
    out = oracle.shared_step(build_batch(case), noise)
    out["loss"].backward()
    return out, {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("case_id", ["mrssm_nonsquare", "mmtrssm_default", "mw128"])
def test_kl_options_are_live_in_the_oracle(case_id: str) -> None:
    """At fixed noise and weights: ``kl_coeff = 0.7`` scales both KL terms by 0.7 and ``w_kl_h = 0.3`` scales ``kl_h`` alone by 0.3
    (1e-6 relative); ``use_kl_balancing = False`` leaves every loss value where it was (the two shares of the balanced form
    sum to the plain KL) and changes the gradient of a posterior head."""
    _, _, _, noise, _, _ = _prepared(case_id, "tanh_kl")
    mt = SCAN_CASES[case_id][0].kind == "mmtrssm"
    base, g_base = _step(case_id, noise, activation="Tanh")
    scaled, _ = _step(case_id, noise, activation="Tanh", kl_coeff=0.7)
    np.testing.assert_allclose(_f(scaled["kl"]), 0.7 * _f(base["kl"]), rtol=1e-6)
    np.testing.assert_allclose(_f(scaled["recon"]), _f(base["recon"]), rtol=1e-6)
    assert _f(base["kl"]) > 1e-3
    if mt:
        np.testing.assert_allclose(_f(scaled["kl_h"]), 0.7 * _f(base["kl_h"]), rtol=1e-6)
        high, _ = _step(case_id, noise, activation="Tanh", w_kl_h=0.3)
        np.testing.assert_allclose(_f(high["kl_h"]), 0.3 * _f(base["kl_h"]), rtol=1e-6)
        np.testing.assert_allclose(_f(high["kl"]), _f(base["kl"]), rtol=1e-6)
        assert _f(base["kl_h"]) > 1e-3
    plain, g_plain = _step(case_id, noise, activation="Tanh", use_kl_balancing=False)
    for k in (k for k in base if not k.startswith("_")):
        np.testing.assert_allclose(_f(plain[k]), _f(base[k]), rtol=1e-6, err_msg=k)
    heads = ["representation.rnn_to_post_projector.2.weight", "vision_representation.rnn_to_post_projector.2.weight"]
    if mt:
        heads.append("h_posterior.2.weight")
    for k in heads:
        diff = float((g_plain[k] - g_base[k]).abs().max())
        assert diff > 1e-3 * float(g_base[k].abs().max()), (k, diff)


@pytest.mark.parametrize("case_id", ["mrssm_nonsquare", "mmtrssm_default"])
def test_the_four_activations_give_four_losses(case_id: str) -> None:
    """The activation of the scan's MLPs shapes the prior and the posterior directly: the four KL terms differ pairwise by
    more than 1e-4 relative (a thousand fp32 roundings; the reconstruction terms dominate ``loss`` and hide the difference in its
    low bits, so ``loss`` is only required to take four values)."""
    _, _, _, noise, _, _ = _prepared(case_id, "identity")
    outs = {a: _step(case_id, noise, activation=a)[0] for a in ("Identity", "ReLU", "ELU", "Tanh")}
    assert len({float(o["loss"].detach()) for o in outs.values()}) == 4
    values = sorted(float(o["kl"].detach()) for o in outs.values())
    for lo, hi in zip(values, values[1:]):
        assert hi - lo > 1e-4 * abs(hi), values
