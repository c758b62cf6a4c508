"""The scans' backward per output cotangent (helper, no tests): the problem, the float64 reference, the cotangent sets and the
gradient bounds shared by ``tests/test_scan_cotangents_host.py`` (oracle only, runs anywhere) and
``tests/test_scan_cotangents_gpu.py`` (MI355X).

``_MrssmScan`` and ``_MmtrssmScan`` do not materialise absent output gradients: every subset of the 6 (MRSSM) or 14 (MMTRSSM)
output cotangents reaches the reverse-time kernels as its own pattern of null pointers, and each scan family holds its own copy
of those arms.  Here the scan is called on its own (``scan.mrssm_posterior_rollout`` / ``scan.mmtrssm_posterior_rollout``: no
encoder, decoder or initial-state kernel) on random inputs, a fixed random linear functional reads a chosen set of outputs, and
the gradients with respect to the scan's inputs, its initial state and every parameter are compared with a float64 copy of the
oracle (``profiles/scan_cotangent_errors.md`` holds the measured baselines and how the bounds follow from them)."""

from __future__ import annotations

from dataclasses import dataclass, field, replace

import torch
import torch.nn.functional as F  # noqa: N812
from torch import Tensor, nn

from oracle.cases import Case, build_model
from oracle.ref_dists import sampling_margin
from oracle.ref_model import cat_probs, kl_cat
from tests.class_counts import CLASS_CASES, float64_copy
from tests.config_matrix import SAMPLING_MARGIN, SCAN_CASES, SEEDS

MR_OUTPUTS = ("deter", "prior_logits", "post_logits", "post_stoch", "prior_stoch", "kl")
MT_OUTPUTS = ("deter_l", "deter_h", "hidden_l", "hidden_h", "prior_logits_l", "prior_logits_h", "post_logits_l", "post_logits_h",
              "post_stoch_l", "post_stoch_h", "prior_stoch_l", "prior_stoch_h", "kl_l", "kl_h")
COMBINED_SETS = ("all", "all_first_half", "no_prior_draw")

# family -> the cases that reach each copy of its backward arms (fast8 and the general categorical block)
FAMILY_CASES: dict[str, tuple[str, ...]] = {
    "scan": ("mrssm_nonsquare", "s24x40_12x3"),
    "cluster": ("mrssm_default", "c64", "c128", "mrssm_cfg2dims", "c32_16x2", "c200_9x3"),
    "wide": ("w256", "w32x256", "w256_16x8"),
    "mt_scan": ("mmtrssm_default", "mt32_l12x3_h2x8"),
    "mt_wide": ("mw128", "mw128_l12x3_h2x8", "mw128_l4x4_h16x2"),
}
WIDE_FAMILIES = frozenset({"wide", "mt_wide"})
COOPERATIVE = frozenset({"cluster", "wide", "mt_wide"})
# (case, batch, steps): row counts past one cluster's / one row tile's share, the `all` set only
ROW_COUNT_RUNS = (("mrssm_default", 70, 3), ("w256", 37, 3), ("mw128", 70, 3))
# one masked and weighted case per cooperative family plus one single-CU case
MASKED_CASES = ("mrssm_default", "w256", "mw128", "mrssm_nonsquare")
# the two single-output sets whose fp32-oracle error the host test records next to `all`
HOST_SINGLE_SETS = {"mrssm": ("prior_stoch", "kl"), "mmtrssm": ("prior_stoch_l", "hidden_h")}

# Gradient bounds, relative to the float64 tensor's largest entry: 16 x the largest error of the fp32 oracle against float64
# over the family's cases (tests/test_scan_cotangents_host.py measures it; profiles/scan_cotangent_errors.md holds the table),
# rounded up to one significant digit.
HOST_BASELINE = {"scan": 8.4e-7, "cluster": 1.1e-6, "wide": 1.2e-6, "mt_scan": 5.5e-7, "mt_wide": 6.7e-7}
GRAD_BOUND = {"scan": 2e-5, "cluster": 2e-5, "wide": 2e-5, "mt_scan": 9e-6, "mt_wide": 2e-5}
VALUE_ATOL = 1e-5          # deter / hidden / probabilities / KL per step; the wide families + WIDE_EXTRA (three pieces)
WIDE_EXTRA = 5e-6
TWO_PIECE_PROBS = 1.5e-5   # what scan.py states for two bf16 pieces
TWO_PIECE_GRADS = 1e-3
TWO_PIECE_LOSS_RTOL = 1e-4

_INPUT_SEED, _WEIGHT_SEED, _CODE_T = 4321, 8765, 5


def case_of(case_id: str) -> tuple[Case, str]:
    return SCAN_CASES[case_id] if case_id in SCAN_CASES else CLASS_CASES[case_id]


def output_names(case: Case) -> tuple[str, ...]:
    return MR_OUTPUTS if case.kind == "mrssm" else MT_OUTPUTS


def cotangent_sets(case: Case) -> tuple[str, ...]:
    return (*output_names(case), *COMBINED_SETS)


def masked_sets(case: Case) -> tuple[str, ...]:
    return ("all", "kl", "post_logits") if case.kind == "mrssm" else ("all", "kl_l", "post_logits_l")


def levels(case: Case) -> list[tuple[str, int, int]]:
    """(suffix of the output names, categoricals, classes) per level of latents."""
    d = case.dims
    if case.kind == "mrssm":
        return [("", d.cats, d.classes)]
    return [("_l", d.ls_cats, d.ls_classes), ("_h", d.hs_cats, d.hs_classes)]


def kl_weights(case: Case) -> tuple[float, float]:
    """(w_post, w_prior) as the kernels get them (``kl_w_post`` / ``kl_w_prior``)."""
    from multimodal_mtrssm_amd.scan import MTScanConfig, ScanConfig

    balancing = bool(case.dims.use_kl_balancing)
    if case.kind == "mrssm":
        return ScanConfig(case.dims.cats, case.dims.classes, 0, balancing).kl_weights
    d = case.dims
    return MTScanConfig(d.ls_cats, d.ls_classes, d.hs_cats, d.hs_classes, 0, d.l_tau, d.h_tau, balancing).kl_weights


def kl_per_step(q_logits: Tensor, p_logits: Tensor, cats: int, classes: int, weights: tuple[float, float]) -> Tensor:
    """KL(q || p) per (b, t) as the scans emit it: the plain KL in value; its gradient is that of
    ``w_prior * kl_cat(q.detach(), p) + w_post * kl_cat(q, p.detach())`` (with weights that sum to 1 the two are one expression;
    the plain-KL weights (1, 1) give the plain gradient, and the value is pinned so that they do not give twice the KL)."""
    w_post, w_prior = weights
    ql, qp = cat_probs(q_logits, cats, classes)
    pl, _ = cat_probs(p_logits, cats, classes)
    split = w_prior * kl_cat(ql.detach(), qp.detach(), pl) + w_post * kl_cat(ql, qp, pl.detach())
    if w_post + w_prior == 1.0:
        return split
    return kl_cat(ql, qp, pl).detach() + (split - split.detach())


@dataclass
class Problem:
    case: Case
    family: str
    oracle: nn.Module                       # fp32
    ref64: nn.Module                        # its float64 copy
    inputs: dict[str, Tensor]               # fp32 leaves: actions, audio_embed, vision_embed and the initial state's tensors
    noise: dict[str, Tensor]                # the uniforms, by the scans' names
    weights: dict[str, Tensor]              # output name -> the functional's fixed weights
    seed: int
    margin: float
    codes: Tensor | None = None             # int64 [B, T] modality codes of the masked arm
    logw: Tensor | None = None              # fp32 [B, T, 3] expert log-weights of the masked arm
    cache: dict = field(default_factory=dict)


def _onehot(g: torch.Generator, batch: int, cats: int, classes: int) -> Tensor:
    return F.one_hot(torch.randint(0, classes, (batch, cats), generator=g), classes).float().flatten(start_dim=-2)


def _draw_inputs(case: Case, batch: int, steps: int) -> dict[str, Tensor]:
    d = case.dims
    g = torch.Generator().manual_seed(_INPUT_SEED)
    inputs = {"actions": torch.randn(batch, steps, d.action, generator=g),
              "audio_embed": torch.randn(batch, steps, d.embed, generator=g),
              "vision_embed": torch.randn(batch, steps, d.embed, generator=g)}
    if case.kind == "mrssm":
        inputs["deter"] = 0.5 * torch.randn(batch, d.deter, generator=g)
        inputs["stoch"] = _onehot(g, batch, d.cats, d.classes)
    else:
        for key, width in (("deter_l", d.ld), ("deter_h", d.hd), ("hidden_l", d.ld), ("hidden_h", d.hd)):
            inputs[key] = 0.5 * torch.randn(batch, width, generator=g)
        inputs["stoch_l"] = _onehot(g, batch, d.ls_cats, d.ls_classes)
        inputs["stoch_h"] = _onehot(g, batch, d.hs_cats, d.hs_classes)
    return inputs


def _draw_noise(case: Case, seed: int, batch: int, steps: int) -> dict[str, Tensor]:
    g = torch.Generator().manual_seed(seed)
    out = {}
    for sfx, cats, _classes in levels(case):
        out[f"u_post{sfx}"] = torch.rand(batch, steps, cats, generator=g)
        out[f"u_prior{sfx}"] = torch.rand(batch, steps, cats, generator=g)
    return out


def state_keys(case: Case) -> tuple[str, ...]:
    return ("deter", "stoch") if case.kind == "mrssm" else ("deter_l", "deter_h", "hidden_l", "hidden_h", "stoch_l", "stoch_h")


def reference_outputs(model: nn.Module, pr: Problem, inputs: dict[str, Tensor], noise: dict[str, Tensor]) -> dict[str, Tensor]:
    """The oracle's posterior rollout on ``inputs`` (of ``model``'s dtype) with the scans' output names, the KL per step
    included.  With ``pr.codes`` set, the masked and weighted loop of ``tests/test_expert_weights_oracle.py``."""
    case = pr.case
    state0 = {k: inputs[k] for k in state_keys(case)}
    a, ea, ev = inputs["actions"], inputs["audio_embed"], inputs["vision_embed"]
    if pr.codes is not None:
        from tests.test_expert_weights_oracle import weighted_mmtrssm_rollout, weighted_mrssm_rollout

        lw = inputs["expert_logw"]
        roll = (weighted_mrssm_rollout(model, a, ea, ev, state0["deter"], state0["stoch"], noise, pr.codes, lw) if case.kind == "mrssm"
                else weighted_mmtrssm_rollout(model, a, ea, ev, state0, noise, pr.codes, lw))
    elif case.kind == "mrssm":
        roll = model.rollout_representation(a, ea, ev, state0, noise["u_prior"], noise["u_post"])
    else:
        roll = model.rollout_representation(a, ea, ev, state0, noise)
    out = {k: v for k, v in roll.items() if k in output_names(case)}
    w = kl_weights(case)
    for sfx, cats, classes in levels(case):
        out[f"kl{sfx}"] = kl_per_step(roll[f"post_logits{sfx}"], roll[f"prior_logits{sfx}"], cats, classes, w)
    assert set(out) == set(output_names(case))
    return out


def trajectory_margin(pr: Problem, out: dict[str, Tensor], noise: dict[str, Tensor]) -> float:
    """Smallest |u - cdf| over every draw of the rollout (``oracle.ref_dists.sampling_margin``)."""
    worst = float("inf")
    for sfx, cats, classes in levels(pr.case):
        for which in ("post", "prior"):
            probs = cat_probs(out[f"{which}_logits{sfx}"].detach(), cats, classes)[1]
            worst = min(worst, float(sampling_margin(probs, noise[f"u_{which}{sfx}"].to(probs.dtype)).min()))
    return worst


def cast_inputs(pr: Problem, dtype: torch.dtype, device: str = "cpu") -> dict[str, Tensor]:
    """Fresh leaves of ``pr.inputs`` (and of the expert log-weights of the masked arm), every one with ``requires_grad``."""
    leaves = {k: v.detach().to(device=device, dtype=dtype).requires_grad_() for k, v in pr.inputs.items()}
    if pr.logw is not None:
        leaves["expert_logw"] = pr.logw.detach().to(device=device, dtype=dtype).requires_grad_()
    return leaves


def build_problem(case_id: str, *, batch: int | None = None, steps: int | None = None, masked: bool = False) -> Problem:
    """The problem of a case of ``SCAN_CASES`` / ``CLASS_CASES``: the oracle and its float64 copy, seeded random scan inputs, and
    uniforms re-drawn over ``SEEDS`` until every draw keeps ``SAMPLING_MARGIN`` from every CDF edge on the float64 trajectory."""
    base, family = case_of(case_id)
    case = replace(base, batch=batch or base.batch, steps=steps or base.steps)
    oracle = build_model(case)
    pr = Problem(case, family, oracle, float64_copy(oracle), _draw_inputs(case, case.batch, case.steps), {}, {}, -1, 0.0)
    if masked:
        from tests.test_expert_weights_oracle import codes_of, explicit_weights

        pr.codes = codes_of("fourway", case.batch, case.steps)
        pr.logw = explicit_weights(case.batch, case.steps)
    seen = []
    for seed in SEEDS:
        noise = _draw_noise(case, seed, case.batch, case.steps)
        with torch.no_grad():
            out = reference_outputs(pr.ref64, pr, {k: v.detach() for k, v in cast_inputs(pr, torch.float64).items()}, noise)
        margin = trajectory_margin(pr, out, noise)
        if margin >= SAMPLING_MARGIN:
            pr.noise, pr.seed, pr.margin = noise, seed, margin
            break
        seen.append((seed, margin))
    assert pr.seed >= 0, f"{case_id}: no uniforms' seed in {SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges: {seen}"
    g = torch.Generator().manual_seed(_WEIGHT_SEED)
    pr.weights = {k: torch.randn(out[k].shape, generator=g) for k in output_names(case)}
    return pr


def chosen_outputs(case: Case, cot: str) -> tuple[str, ...]:
    names = output_names(case)
    if cot in names:
        return (cot,)
    if cot == "no_prior_draw":
        return tuple(k for k in names if not k.startswith("prior_stoch"))
    assert cot in {"all", "all_first_half"}, cot
    return names


def functional(pr: Problem, out: dict[str, Tensor], cot: str) -> Tensor:
    """The sum over the chosen outputs of ``(output * weight).sum()``; ``all_first_half`` zeroes the weights at ``t >= T // 2``."""
    total = None
    half = pr.case.steps // 2
    for k in chosen_outputs(pr.case, cot):
        w = pr.weights[k].to(out[k])
        if cot == "all_first_half":
            w = w.clone()
            w[:, half:] = 0.0
        term = (out[k] * w).sum()
        total = term if total is None else total + term
    return total


def reference_gradients(model: nn.Module, pr: Problem, cot: str) -> tuple[dict[str, Tensor], dict[str, Tensor | None]]:
    """(outputs, gradients) of ``model`` (the fp32 oracle or its float64 copy): the gradients of the functional of ``cot`` with
    respect to every input leaf (``in/<name>``) and every parameter (by state-dict name); None where autograd produces none.
    The forward runs once per model and is shared by the cotangent sets."""
    dtype = next(model.parameters()).dtype
    key = ("forward", dtype)
    if key not in pr.cache:
        leaves = cast_inputs(pr, dtype)
        pr.cache[key] = (leaves, reference_outputs(model, pr, leaves, pr.noise))
    leaves, out = pr.cache[key]
    named = {f"in/{k}": v for k, v in leaves.items()} | dict(model.named_parameters())
    grads = torch.autograd.grad(functional(pr, out, cot), list(named.values()), retain_graph=True, allow_unused=True)
    return out, dict(zip(named, grads, strict=True))


def relative_error(got: Tensor, want: Tensor) -> float:
    """Largest error over the reference tensor's largest entry."""
    return float((got.double().cpu() - want.double()).abs().max() / want.double().abs().max())


def sample_index(stoch: Tensor, cats: int, classes: int) -> Tensor:
    return stoch.detach().reshape(*stoch.shape[:-1], cats, classes).argmax(-1).cpu()
