"""Uniform mixing of the categorical latents: the eager reference (helper, no tests) shared by
``tests/test_unimix_host.py`` (oracle only, runs anywhere) and ``tests/test_unimix_gpu.py`` (MI355X).

The rollout loops follow ``OracleMRSSM.rollout_representation`` / ``OracleMMTRSSM.rollout_representation`` line by line, built
from the oracle's own pieces (``mopoe_mix``, ``cat_probs``, ``st_sample`` and the models' submodules), with the transform

    x' = log((1 - eps) softmax(x) + eps / C)        per categorical

after each prior head and after each posterior's logits; at ``eps == 0`` the transform is the identity function (not an
arithmetic no-op: the logits object is returned as it is), so the loops are the oracle's, bit for bit.  The masked and weighted
variants follow ``tests/test_expert_weights_oracle.py``: both present = weighted mix, one = the flat log-softmax of that expert,
none = the prior's RAW logits, and then both sides go through the transform.  The problem, the functional, the KL per step, the
cases and the bounds are those of ``tests/scan_cotangents.py``; the uniforms are screened again on the float64 trajectory WITH
unimix, since the probabilities change."""

from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from oracle.ref_model import cat_probs, mopoe_mix, st_sample
from tests.class_counts import float64_copy
from tests.config_matrix import SAMPLING_MARGIN, SEEDS
from tests.scan_cotangents import (Problem, _draw_noise, build_problem, cast_inputs, functional, kl_per_step, kl_weights, levels,
                                   output_names, state_keys, trajectory_margin)

EPS = 0.01        # the value the issue's measurements were made at
EPS_LARGE = 0.3   # a wrong (1 - eps) factor or eps / C cannot hide in 1 %
HEAD_SCALE = 60.0  # the saturated heads: last layers of every prior and posterior head times this


def unimix(logits: Tensor, cats: int, classes: int, eps: float) -> Tensor:
    """``log((1 - eps) softmax(x) + eps / C)`` per categorical, flat in and out; ``eps == 0``: ``logits`` itself."""
    if eps == 0.0:
        return logits
    probs = cat_probs(logits, cats, classes)[1]
    return ((1.0 - eps) * probs + eps / classes).log().flatten(start_dim=-2)


def kl_bound(cats: int, classes: int, eps: float) -> float:
    """No KL between two mixed distributions of K C-way categoricals exceeds ``K log(C / eps)``: q <= 1 and p >= eps / C."""
    return cats * math.log(classes / eps)


def _reference_mix(a_logits: Tensor, v_logits: Tensor, prior_logits: Tensor, lw: Tensor, code: Tensor) -> Tensor:
    from multimodal_mtrssm_amd.experts import ExpertWeights

    return ExpertWeights.reference_mix(a_logits, v_logits, prior_logits, lw, code)


def mrssm_rollout(m: nn.Module, inputs: dict[str, Tensor], noise: dict[str, Tensor], eps: float, codes: Tensor | None = None,
                  lw: Tensor | None = None) -> dict[str, Tensor]:
    """``OracleMRSSM.rollout_representation`` (``_prior_step`` inlined) with the transform; ``codes`` / ``lw``: the masked and
    weighted loop of ``tests.test_expert_weights_oracle.weighted_mrssm_rollout``."""
    d, tr = m.dims, m.transition
    actions, audio_embed, vision_embed = inputs["actions"], inputs["audio_embed"], inputs["vision_embed"]
    deter, stoch = inputs["deter"], inputs["stoch"]
    keep: dict[str, list[Tensor]] = {k: [] for k in ("deter", "prior_logits", "prior_stoch", "post_logits", "post_stoch")}
    for t in range(actions.shape[1]):
        x = tr.action_state_projector(torch.cat([actions[:, t], stoch], dim=-1))
        deter = tr.rnn_cell(x, deter)
        raw_prior = tr.rnn_to_prior_projector(deter)
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter, vision_embed[:, t]], -1))
        mixed = mopoe_mix(a_logits, v_logits) if codes is None else _reference_mix(a_logits, v_logits, raw_prior, lw[:, t], codes[:, t])
        prior_logits = unimix(raw_prior, d.cats, d.classes, eps)
        post_logits = unimix(mixed, d.cats, d.classes, eps)
        _, prior_probs = cat_probs(prior_logits, d.cats, d.classes)
        prior_stoch = st_sample(prior_probs, noise["u_prior"][:, t])
        _, post_probs = cat_probs(post_logits, d.cats, d.classes)
        stoch = st_sample(post_probs, noise["u_post"][:, t])
        for k, v in zip(keep, (deter, prior_logits, prior_stoch, post_logits, stoch), strict=True):
            keep[k].append(v)
    return {k: torch.stack(v, dim=1) for k, v in keep.items()}


def mmtrssm_rollout(m: nn.Module, inputs: dict[str, Tensor], noise: dict[str, Tensor], eps: float, codes: Tensor | None = None,  # noqa: PLR0914
                    lw: Tensor | None = None) -> dict[str, Tensor]:
    """``OracleMMTRSSM.rollout_representation`` with the transform on all four logits; ``codes`` / ``lw``: the loop of
    ``tests.test_expert_weights_oracle.weighted_mmtrssm_rollout`` (no modality: the higher posterior is the higher prior's raw
    logits, before mixing)."""
    d = m.dims
    actions, audio_embed, vision_embed = inputs["actions"], inputs["audio_embed"], inputs["vision_embed"]
    deter_l, deter_h, hidden_l, hidden_h = inputs["deter_l"], inputs["deter_h"], inputs["hidden_l"], inputs["hidden_h"]
    stoch_l, stoch_h = inputs["stoch_l"], inputs["stoch_h"]
    names = ("deter_l", "deter_h", "hidden_l", "hidden_h", "prior_logits_l", "prior_logits_h", "prior_stoch_l", "prior_stoch_h",
             "post_logits_l", "post_logits_h", "post_stoch_l", "post_stoch_h")
    keep: dict[str, list[Tensor]] = {k: [] for k in names}
    for t in range(actions.shape[1]):
        l_in = torch.cat([actions[:, t], stoch_l, stoch_h], dim=-1)
        deter_l, hidden_l = m.l_rnn(l_in, deter_l, hidden_l)
        raw_prior_l = m.l_prior(deter_l)
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter_l, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter_l, vision_embed[:, t]], -1))
        mixed = mopoe_mix(a_logits, v_logits) if codes is None else _reference_mix(a_logits, v_logits, raw_prior_l, lw[:, t], codes[:, t])
        post_logits_l = unimix(mixed, d.ls_cats, d.ls_classes, eps)
        _, ql = cat_probs(post_logits_l, d.ls_cats, d.ls_classes)
        new_stoch_l = st_sample(ql, noise["u_post_l"][:, t])

        deter_h, hidden_h = m.h_rnn(stoch_h, deter_h, hidden_h)
        raw_prior_h = m.h_prior(deter_h)
        raw_post_h = m.h_posterior(torch.cat([deter_l, deter_h], dim=-1))
        if codes is not None:
            raw_post_h = torch.where(codes[:, t][:, None] == 0, raw_prior_h, raw_post_h)
        post_logits_h = unimix(raw_post_h, d.hs_cats, d.hs_classes, eps)
        _, qh = cat_probs(post_logits_h, d.hs_cats, d.hs_classes)
        new_stoch_h = st_sample(qh, noise["u_post_h"][:, t])

        prior_logits_h = unimix(raw_prior_h, d.hs_cats, d.hs_classes, eps)
        prior_logits_l = unimix(raw_prior_l, d.ls_cats, d.ls_classes, eps)
        _, ph = cat_probs(prior_logits_h, d.hs_cats, d.hs_classes)
        _, pl = cat_probs(prior_logits_l, d.ls_cats, d.ls_classes)
        prior_stoch_h = st_sample(ph, noise["u_prior_h"][:, t])
        prior_stoch_l = st_sample(pl, noise["u_prior_l"][:, t])
        stoch_l, stoch_h = new_stoch_l, new_stoch_h
        vals = (deter_l, deter_h, hidden_l, hidden_h, prior_logits_l, prior_logits_h, prior_stoch_l, prior_stoch_h,
                post_logits_l, post_logits_h, stoch_l, stoch_h)
        for k, v in zip(names, vals, strict=True):
            keep[k].append(v)
    return {k: torch.stack(v, dim=1) for k, v in keep.items()}


def prior_rollout(m: nn.Module, kind: str, inputs: dict[str, Tensor], noise: dict[str, Tensor], eps: float) -> dict[str, Tensor]:
    """``rollout_transition`` of either oracle with the transform after each prior head."""
    d = m.dims
    actions = inputs["actions"]
    if kind == "mrssm":
        tr, deter, stoch = m.transition, inputs["deter"], inputs["stoch"]
        keep: dict[str, list[Tensor]] = {"deter": [], "prior_logits": [], "prior_stoch": []}
        for t in range(actions.shape[1]):
            deter = tr.rnn_cell(tr.action_state_projector(torch.cat([actions[:, t], stoch], dim=-1)), deter)
            logits = unimix(tr.rnn_to_prior_projector(deter), d.cats, d.classes, eps)
            stoch = st_sample(cat_probs(logits, d.cats, d.classes)[1], noise["u_prior"][:, t])
            for k, v in zip(keep, (deter, logits, stoch), strict=True):
                keep[k].append(v)
        return {k: torch.stack(v, dim=1) for k, v in keep.items()}
    deter_l, deter_h, hidden_l, hidden_h = inputs["deter_l"], inputs["deter_h"], inputs["hidden_l"], inputs["hidden_h"]
    stoch_l, stoch_h = inputs["stoch_l"], inputs["stoch_h"]
    names = ("deter_l", "deter_h", "hidden_l", "hidden_h", "prior_logits_l", "prior_logits_h", "prior_stoch_l", "prior_stoch_h")
    keep = {k: [] for k in names}
    for t in range(actions.shape[1]):
        deter_l, hidden_l = m.l_rnn(torch.cat([actions[:, t], stoch_l, stoch_h], dim=-1), deter_l, hidden_l)
        logits_l = unimix(m.l_prior(deter_l), d.ls_cats, d.ls_classes, eps)
        deter_h, hidden_h = m.h_rnn(stoch_h, deter_h, hidden_h)
        logits_h = unimix(m.h_prior(deter_h), d.hs_cats, d.hs_classes, eps)
        stoch_h = st_sample(cat_probs(logits_h, d.hs_cats, d.hs_classes)[1], noise["u_prior_h"][:, t])
        stoch_l = st_sample(cat_probs(logits_l, d.ls_cats, d.ls_classes)[1], noise["u_prior_l"][:, t])
        for k, v in zip(names, (deter_l, deter_h, hidden_l, hidden_h, logits_l, logits_h, stoch_l, stoch_h), strict=True):
            keep[k].append(v)
    return {k: torch.stack(v, dim=1) for k, v in keep.items()}


def unimix_outputs(model: nn.Module, pr: Problem, inputs: dict[str, Tensor], noise: dict[str, Tensor], eps: float) -> dict[str, Tensor]:
    """``tests.scan_cotangents.reference_outputs`` under unimix: the scans' outputs by name, the KL per step included."""
    case = pr.case
    lw = inputs.get("expert_logw") if pr.codes is not None else None
    roll = (mrssm_rollout if case.kind == "mrssm" else mmtrssm_rollout)(model, inputs, noise, eps, pr.codes, lw)
    out = {k: v for k, v in roll.items() if k in output_names(case)}
    w = kl_weights(case)
    for sfx, cats, classes in levels(case):
        out[f"kl{sfx}"] = kl_per_step(roll[f"post_logits{sfx}"], roll[f"prior_logits{sfx}"], cats, classes, w)
    assert set(out) == set(output_names(case))
    return out


def scale_heads(model: nn.Module, kind: str, factor: float = HEAD_SCALE) -> None:
    """Multiply the last layer (weight and bias) of every prior and posterior head by ``factor``: saturated logits."""
    heads = [model.audio_representation.rnn_to_post_projector, model.vision_representation.rnn_to_post_projector]
    heads += [model.transition.rnn_to_prior_projector] if kind == "mrssm" else [model.l_prior, model.h_prior, model.h_posterior]
    with torch.no_grad():
        for head in heads:
            last = [layer for layer in head if isinstance(layer, nn.Linear)][-1]
            last.weight.mul_(factor)
            last.bias.mul_(factor)


def screen(pr: Problem, eps: float) -> Problem:
    """Re-draw ``pr``'s uniforms over ``SEEDS`` until every draw keeps ``SAMPLING_MARGIN`` from every CDF edge on the float64
    trajectory under ``eps`` (the seed may differ from the one ``build_problem`` picked); clears the cached forwards."""
    seen = []
    leaves = {k: v.detach() for k, v in cast_inputs(pr, torch.float64).items()}
    for seed in SEEDS:
        noise = _draw_noise(pr.case, seed, pr.case.batch, pr.case.steps)
        with torch.no_grad():
            out = unimix_outputs(pr.ref64, pr, leaves, noise, eps)
        margin = trajectory_margin(pr, out, noise)
        if margin >= SAMPLING_MARGIN:
            pr.noise, pr.seed, pr.margin = noise, seed, margin
            pr.cache.clear()
            return pr
        seen.append((seed, margin))
    msg = f"{pr.case.name} eps {eps}: no uniforms' seed in {SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges: {seen}"
    raise AssertionError(msg)


def build_unimix_problem(case_id: str, eps: float, *, batch: int | None = None, steps: int | None = None, masked: bool = False,
                         saturated: bool = False) -> Problem:
    """``build_problem`` with the uniforms screened under ``eps``; ``saturated``: the heads' last layers scaled first."""
    pr = build_problem(case_id, batch=batch, steps=steps, masked=masked)
    if saturated:
        scale_heads(pr.oracle, pr.case.kind)
        pr.ref64 = float64_copy(pr.oracle)
    return screen(pr, eps)


def unimix_gradients(model: nn.Module, pr: Problem, cot: str, eps: float) -> tuple[dict[str, Tensor], dict[str, Tensor | None]]:
    """``tests.scan_cotangents.reference_gradients`` under unimix; the forward runs once per (model, eps)."""
    dtype = next(model.parameters()).dtype
    key = ("unimix", dtype, eps)
    if key not in pr.cache:
        leaves = cast_inputs(pr, dtype)
        pr.cache[key] = (leaves, unimix_outputs(model, pr, leaves, pr.noise, eps))
    leaves, out = pr.cache[key]
    named = {f"in/{k}": v for k, v in leaves.items()} | dict(model.named_parameters())
    grads = torch.autograd.grad(functional(pr, out, cot), list(named.values()), retain_graph=True, allow_unused=True)
    return out, dict(zip(named, grads, strict=True))


def saturated_kl_error(pr: Problem, eps: float) -> tuple[float, float]:
    """(largest absolute error of the fp32 reference's KL per step against float64 over the levels of ``pr``, the largest
    float64 KL): what the GPU test's saturated-heads bound is 16 x of, measured on the problem itself."""
    out32, _ = unimix_gradients(pr.oracle, pr, "all", eps)
    out64, _ = unimix_gradients(pr.ref64, pr, "all", eps)
    err = scale = 0.0
    for sfx, _cats, _classes in levels(pr.case):
        err = max(err, float((out32[f"kl{sfx}"].detach().double() - out64[f"kl{sfx}"].detach()).abs().max()))
        scale = max(scale, float(out64[f"kl{sfx}"].detach().max()))
    return err, scale


def unimix_sets(case) -> tuple[str, ...]:  # noqa: ANN001
    """The cotangent sets of the value-and-gradient test: ``all``, every ``kl*``, ``post_logits*``, ``prior_logits*`` and
    ``post_stoch*`` output on its own, and ``no_prior_draw``."""
    singles = tuple(k for k in output_names(case) if k.startswith(("kl", "post_logits", "prior_logits", "post_stoch")))
    return ("all", *singles, "no_prior_draw")


__all__ = ["EPS", "EPS_LARGE", "HEAD_SCALE", "build_unimix_problem", "kl_bound", "mmtrssm_rollout", "mrssm_rollout", "prior_rollout",
           "scale_heads", "screen", "state_keys", "unimix", "unimix_gradients", "unimix_outputs", "unimix_sets"]
