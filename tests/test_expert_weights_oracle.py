"""Weighted MoPoE against an eager CPU restatement, forward and gradients, every scan family.

The restatement is the masked one of ``tests.test_modality_mask_oracle`` with the mixture swapped for
``ExpertWeights.reference_mix``: the three log-weights of a step enter the logsumexp where both modalities are present and
nowhere else.  First pass: explicit weights (a leaf, so ``lw.grad`` is compared too) under a four-way code pattern and with
both modalities everywhere (no mask at all: the host hands the kernels all-"both" codes).  Second pass: a gated and a static
gate with seeded non-zero parameters, the restatement holding the same gate tensors.
"""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch
from torch import Tensor

from multimodal_mtrssm_amd.experts import ExpertWeights
from oracle.cases import CASES, build_batch, build_model, build_noise, min_margin
from oracle.ref_model import cat_probs, kl_loss, st_sample
from tests.conftest import product_from_case
from tests.test_modality_mask_oracle import FAMILIES, IDS, _index, four_way_codes, mask_of, masked_embed0, masked_nll

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATTERNS = ("fourway", "allboth")


def codes_of(pattern: str, B: int, T: int) -> Tensor:  # noqa: N803
    if pattern == "allboth":
        return torch.full((B, T), 3)
    codes = four_way_codes(B, T)
    codes[:, 5:] = 3
    codes[:, 0] = 3
    return codes


def explicit_weights(B: int, T: int) -> Tensor:  # noqa: N803
    return torch.log_softmax(2.0 * torch.randn(B, T, 3, generator=torch.Generator().manual_seed(23)), dim=-1)


def seeded_gate(mode: str, embed: int) -> ExpertWeights:
    gate = ExpertWeights(mode, embed if mode == "gated" else None)
    g = torch.Generator().manual_seed(29)
    with torch.no_grad():
        for p in gate.parameters():
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return gate


def weighted_mrssm_rollout(m, act_in, audio_embed, vision_embed, deter, stoch, noise, codes: Tensor, lw) -> dict[str, Tensor]:  # noqa: ANN001, PLR0913
    """The weighted and masked T loop from a given initial state: the rollout's outputs, each stacked over time."""
    d = m.dims
    keep: dict[str, list[Tensor]] = {k: [] for k in ("deter", "prior_logits", "prior_stoch", "post_logits", "post_stoch")}
    for t in range(act_in.shape[1]):
        deter, prior_logits, prior_stoch = m._prior_step(act_in[:, t], deter, stoch, noise["u_prior"][:, t])  # noqa: SLF001
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter, vision_embed[:, t]], -1))
        post_logits = ExpertWeights.reference_mix(a_logits, v_logits, prior_logits, lw[:, t], codes[:, t])
        stoch = st_sample(cat_probs(post_logits, d.cats, d.classes)[1], noise["u_post"][:, t])
        for k, v in zip(keep, (deter, prior_logits, prior_stoch, post_logits, stoch), strict=True):
            keep[k].append(v)
    return {k: torch.stack(v, dim=1) for k, v in keep.items()}


def weighted_mrssm_step(m, batch, noise, codes: Tensor, lw_of) -> dict[str, Tensor]:  # noqa: ANN001
    d = m.dims
    act_in, audio_in, vision_in, _, audio_tgt, vision_tgt = batch
    audio_embed, vision_embed = m.audio_encoder(audio_in), m.vision_encoder(vision_in)
    lw = lw_of(audio_embed, vision_embed)
    deter = m.init_proj(masked_embed0(audio_embed[:, 0], vision_embed[:, 0], codes[:, 0]))
    logits0 = m.transition.rnn_to_prior_projector(deter)
    stoch = st_sample(cat_probs(logits0, d.cats, d.classes)[1], noise["u_init"])
    roll = weighted_mrssm_rollout(m, act_in, audio_embed, vision_embed, deter, stoch, noise, codes, lw)
    feature = torch.cat([roll["deter"], roll["post_stoch"]], dim=-1)
    mask = mask_of(codes)
    nll_a = masked_nll(m.audio_decoder(feature), audio_tgt, mask[..., 0])
    nll_v = masked_nll(m.vision_decoder(feature), vision_tgt, mask[..., 1])
    kl = kl_loss(roll["post_logits"], roll["prior_logits"], d.cats, d.classes, d.use_kl_balancing) * d.kl_coeff
    out = {"loss": nll_a + nll_v + kl, "recon": nll_a + nll_v, "recon/audio": nll_a, "recon/vision": nll_v, "kl": kl}
    out.update({f"_{k}": v for k, v in roll.items()})
    out["_logits0"] = logits0
    return out


def weighted_mmtrssm_rollout(m, act_in, audio_embed, vision_embed, state0: dict[str, Tensor], noise, codes: Tensor, lw) -> dict[str, Tensor]:  # noqa: ANN001, PLR0913, PLR0914
    """The weighted and masked T loop from a given initial state: the rollout's outputs, each stacked over time."""
    d = m.dims
    deter_l, deter_h, hidden_l, hidden_h = state0["deter_l"], state0["deter_h"], state0["hidden_l"], state0["hidden_h"]
    stoch_l, stoch_h = state0["stoch_l"], state0["stoch_h"]
    names = ("deter_l", "deter_h", "hidden_l", "hidden_h", "prior_logits_l", "prior_logits_h", "prior_stoch_l", "prior_stoch_h",
             "post_logits_l", "post_logits_h", "post_stoch_l", "post_stoch_h")
    keep: dict[str, list[Tensor]] = {k: [] for k in names}
    for t in range(act_in.shape[1]):
        code = codes[:, t]
        deter_l, hidden_l = m.l_rnn(torch.cat([act_in[:, t], stoch_l, stoch_h], dim=-1), deter_l, hidden_l)
        prior_logits_l = m.l_prior(deter_l)
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter_l, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter_l, vision_embed[:, t]], -1))
        post_logits_l = ExpertWeights.reference_mix(a_logits, v_logits, prior_logits_l, lw[:, t], code)  # the lower level only
        new_l = st_sample(cat_probs(post_logits_l, d.ls_cats, d.ls_classes)[1], noise["u_post_l"][:, t])
        deter_h, hidden_h = m.h_rnn(stoch_h, deter_h, hidden_h)
        prior_logits_h = m.h_prior(deter_h)
        post_logits_h = torch.where(code[:, None] == 0, prior_logits_h, m.h_posterior(torch.cat([deter_l, deter_h], dim=-1)))
        new_h = st_sample(cat_probs(post_logits_h, d.hs_cats, d.hs_classes)[1], noise["u_post_h"][:, t])
        prior_stoch_h = st_sample(cat_probs(prior_logits_h, d.hs_cats, d.hs_classes)[1], noise["u_prior_h"][:, t])
        prior_stoch_l = st_sample(cat_probs(prior_logits_l, d.ls_cats, d.ls_classes)[1], noise["u_prior_l"][:, t])
        stoch_l, stoch_h = new_l, new_h
        vals = (deter_l, deter_h, hidden_l, hidden_h, prior_logits_l, prior_logits_h, prior_stoch_l, prior_stoch_h, post_logits_l,
                post_logits_h, stoch_l, stoch_h)
        for k, v in zip(names, vals, strict=True):
            keep[k].append(v)
    return {k: torch.stack(v, dim=1) for k, v in keep.items()}


def weighted_mmtrssm_step(m, batch, noise, codes: Tensor, lw_of) -> dict[str, Tensor]:  # noqa: ANN001, PLR0914
    d = m.dims
    act_in, audio_in, vision_in, _, audio_tgt, vision_tgt = batch
    audio_embed, vision_embed = m.audio_encoder(audio_in), m.vision_encoder(vision_in)
    lw = lw_of(audio_embed, vision_embed)
    h = m.init_proj(masked_embed0(audio_embed[:, 0], vision_embed[:, 0], codes[:, 0]))
    deter_h, deter_l = h[..., : d.hd], h[..., d.hd :]
    hidden_h, hidden_l = deter_h, deter_l
    init_h, init_l = m.h_prior(deter_h), m.l_prior(deter_l)
    stoch_h = st_sample(cat_probs(init_h, d.hs_cats, d.hs_classes)[1], noise["u_init_h"])
    stoch_l = st_sample(cat_probs(init_l, d.ls_cats, d.ls_classes)[1], noise["u_init_l"])
    state0 = {"deter_l": deter_l, "deter_h": deter_h, "hidden_l": hidden_l, "hidden_h": hidden_h, "stoch_l": stoch_l, "stoch_h": stoch_h}
    roll = weighted_mmtrssm_rollout(m, act_in, audio_embed, vision_embed, state0, noise, codes, lw)
    feature = torch.cat([roll["deter_h"], roll["post_stoch_h"], roll["deter_l"], roll["post_stoch_l"]], dim=-1)
    mask = mask_of(codes)
    nll_a = masked_nll(m.audio_decoder(feature), audio_tgt, mask[..., 0])
    nll_v = masked_nll(m.vision_decoder(feature), vision_tgt, mask[..., 1])
    kl_l = kl_loss(roll["post_logits_l"], roll["prior_logits_l"], d.ls_cats, d.ls_classes, d.use_kl_balancing) * d.kl_coeff
    kl_h = kl_loss(roll["post_logits_h"], roll["prior_logits_h"], d.hs_cats, d.hs_classes, d.use_kl_balancing) * (d.kl_coeff * d.w_kl_h)
    out = {"loss": nll_a + nll_v + kl_l + kl_h, "recon": nll_a + nll_v, "recon/audio": nll_a, "recon/vision": nll_v, "kl": kl_l,
           "kl_h": kl_h}
    out.update({f"_{k}": v for k, v in roll.items()})
    out["_init_logits_h"], out["_init_logits_l"] = init_h, init_l
    return out


def weighted_step(case, oracle, batch, noise, codes: Tensor, lw_of) -> dict[str, Tensor]:  # noqa: ANN001, PLR0913
    return (weighted_mrssm_step if case.kind == "mrssm" else weighted_mmtrssm_step)(oracle, batch, noise, codes, lw_of)


def screened(case, oracle, batch, codes: Tensor, lw_of, *, margin: float = 1e-4, first_seed: int = 100, tries: int = 40):  # noqa: ANN001, ANN201, PLR0913
    """``tests.test_modality_mask_oracle.screened`` under the WEIGHTED restatement: every draw keeps ``margin`` from the CDF edges."""
    best = None
    b, t = batch[0].shape[:2]
    for seed in range(first_seed, first_seed + tries):
        noise = build_noise(case, seed, batch=b, steps=t)
        with torch.no_grad():
            out = weighted_step(case, oracle, batch, noise, codes, lw_of)
        m = min_margin(case, out, noise)
        if best is None or m > best[1]:
            best = (noise, m)
        if m >= margin:
            break
    assert best is not None
    return best


def _close_to_scale(got: Tensor, want: Tensor, what: str) -> bool:
    """Within 2e-4 of the tensor's largest entry; False when the reference is all zero (then the result must be too)."""
    scale = float(want.abs().max())
    if scale == 0.0:
        assert float(got.abs().max()) == 0.0, f"{what} must be zero"
        return False
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=0, atol=2e-4 * scale, err_msg=what)
    return True


def _compare(case, oracle, model, batch, noise, codes: Tensor, ref: dict[str, Tensor], *, lw_dev: Tensor | None, masked: bool):  # noqa: ANN001, ANN202, PLR0913, PLR0914
    """Forward (probabilities, samples, KL of empty steps), loss terms and every parameter gradient, with the tolerances of
    ``test_random_four_way_mask_matches_eager_restatement``.  Returns the training step's output dict."""
    d = case.dims
    dbatch = tuple(x.to(DEV) for x in batch)
    dnoise = {k: v.to(DEV) for k, v in noise.items()}
    mask = mask_of(codes).to(DEV) if masked else None
    with torch.no_grad():
        s0 = model.initial_state((dbatch[1][:, 0], dbatch[2][:, 0]), dnoise, modality_mask=None if mask is None else mask[:, 0])
        post, prior = model.rollout_representation(actions=dbatch[0], observations=(dbatch[1], dbatch[2]), prev_state=s0, noise=dnoise,
                                                   modality_mask=mask, expert_log_weights=None if lw_dev is None else lw_dev.detach())
    if case.kind == "mrssm":
        levels = [(post.distribution.probs, post.stoch, prior.distribution.probs, prior.stoch, "", d.cats, d.classes)]
    else:
        levels = [(post.distribution_l.probs, post.stoch_l, prior.distribution_l.probs, prior.stoch_l, "_l", d.ls_cats, d.ls_classes),
                  (post.distribution_h.probs, post.stoch_h, prior.distribution_h.probs, prior.stoch_h, "_h", d.hs_cats, d.hs_classes)]
    for q_probs, q_stoch, p_probs, p_stoch, sfx, cats, classes in levels:
        want_q = cat_probs(ref[f"_post_logits{sfx}"].detach(), cats, classes)[1]
        want_p = cat_probs(ref[f"_prior_logits{sfx}"].detach(), cats, classes)[1]
        np.testing.assert_allclose(q_probs.cpu().numpy(), want_q.numpy(), rtol=0, atol=1e-5, err_msg=f"post probs{sfx}")
        np.testing.assert_allclose(p_probs.cpu().numpy(), want_p.numpy(), rtol=0, atol=1e-5, err_msg=f"prior probs{sfx}")
        assert (_index(q_stoch, cats, classes) == _index(ref[f"_post_stoch{sfx}"], cats, classes)).all(), f"post samples{sfx}"
        assert (_index(p_stoch, cats, classes) == _index(ref[f"_prior_stoch{sfx}"], cats, classes)).all(), f"prior samples{sfx}"
    for kl in ([post.kl_per_step] if case.kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]):
        none = (codes == 0).to(DEV)
        assert torch.equal(kl[none], torch.zeros_like(kl[none]))
    want_table = ExpertWeights.table(_ref_logw(ref), codes)
    np.testing.assert_allclose(model.weights_timeseries.cpu().numpy(), want_table.numpy(), rtol=0, atol=1e-5, err_msg="weights_timeseries")

    out = model.shared_step((*dbatch, mask) if masked else dbatch, dnoise, expert_log_weights=lw_dev)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert set(out) == {k for k in ref if not k.startswith("_")}
    for k in out:
        np.testing.assert_allclose(float(out[k]), float(ref[k]), rtol=1e-4, atol=1e-6, err_msg=k)
    got = dict(model.named_parameters())
    compared = 0
    for k, p in oracle.named_parameters():
        g_ref = p.grad if p.grad is not None else torch.zeros_like(p)
        g_got = got[k].grad
        g_got = torch.zeros_like(got[k]) if g_got is None else g_got
        compared += _close_to_scale(g_got, g_ref, f"grad {k}")
    assert compared > 10
    return out


def _ref_logw(ref: dict[str, Tensor]) -> Tensor:
    return ref["_logw"].detach()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_explicit_weights_match_eager_restatement(name: str, onecu: bool, pattern: str) -> None:  # noqa: FBT001
    case = CASES[name]
    oracle = build_model(case)
    batch = build_batch(case)
    codes = codes_of(pattern, case.batch, case.steps)
    lw = explicit_weights(case.batch, case.steps).requires_grad_()
    lw_of = lambda _ea, _ev: lw  # noqa: E731
    noise, margin = screened(case, oracle, batch, codes, lw_of)
    print(f"{name} {pattern}: sampling margin {margin:.3e}")
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"

    ref = weighted_step(case, oracle, batch, noise, codes, lw_of)
    ref["_logw"] = lw
    ref["loss"].backward()

    model = product_from_case(case, oracle, DEV)
    if onecu:
        model.scan_rows_per_block = 1
    lw_dev = lw.detach().to(DEV).requires_grad_()
    _compare(case, oracle, model, batch, noise, codes, ref, lw_dev=lw_dev, masked=pattern != "allboth")
    assert _close_to_scale(lw_dev.grad, lw.grad, "grad expert_log_weights")
    off = (codes != 3).to(DEV)  # noqa: PLR2004
    assert torch.equal(lw_dev.grad[off], torch.zeros_like(lw_dev.grad[off])), "weights of a step without both modalities got a gradient"
    assert torch.equal(lw.grad[codes != 3], torch.zeros_like(lw.grad[codes != 3]))  # noqa: PLR2004


@pytest.mark.parametrize("mode", ["gated", "static"])
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_gate_matches_eager_restatement(name: str, onecu: bool, mode: str) -> None:  # noqa: FBT001
    case = CASES[name]
    oracle = build_model(case)
    batch = build_batch(case)
    codes = codes_of("fourway", case.batch, case.steps)
    gate = seeded_gate(mode, case.dims.embed)
    seen: dict[str, Tensor] = {}

    def lw_of(ea: Tensor, ev: Tensor) -> Tensor:
        seen["lw"] = gate(ea, ev)
        return seen["lw"]

    noise, margin = screened(case, oracle, batch, codes, lw_of)
    print(f"{name} {mode}: sampling margin {margin:.3e}")
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"

    ref = weighted_step(case, oracle, batch, noise, codes, lw_of)
    ref["_logw"] = seen["lw"]
    ref["loss"].backward()

    model = product_from_case(case, oracle, DEV)
    model.expert_weights = copy.deepcopy(gate).to(DEV)
    model.expert_weights.zero_grad(set_to_none=True)
    if onecu:
        model.scan_rows_per_block = 1
    _compare(case, oracle, model, batch, noise, codes, ref, lw_dev=None, masked=True)
    got = dict(model.expert_weights.named_parameters())
    for k, p in gate.named_parameters():
        assert got[k].grad is not None, f"no gradient at the gate's {k}"
        assert _close_to_scale(got[k].grad, p.grad, f"grad expert_weights.{k}")
