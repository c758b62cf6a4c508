"""The categorical block's general path (helper, no tests): cases with more than 8 classes per categorical and with more than
64 categoricals, shared by ``tests/test_class_counts_host.py`` (oracle only, runs anywhere) and
``tests/test_class_counts_gpu.py`` (MI355X).

``csrc/scan_common.h`` holds the end of every scan's timestep twice: ``cat_block_*_fast8`` (registers, unrolled, C <= 8) and the
general loops ``cat_block_fwd<POST, FAST>`` / ``cat_block_bwd<FAST>``.  The cooperative families pick one at run time by
``C <= 8``; every other case of the suite has 2, 4, 5 or 8 classes, and at most 16 categoricals.  The cases below are the
smallest that reach the general branch of each family (and, past 64 categoricals, the second trip of the ``k += kWave`` lane
loop on the single-CU kernels, which the cooperative predicates must hand the model to).  They stay out of
``oracle.cases.CASES`` (bench.py's view)."""

from __future__ import annotations

import copy
from dataclasses import replace

import torch
from torch import Tensor, nn

from oracle.cases import _SMALL, CASES, Case, _mmtrssm_dims, _mrssm_dims, noise_shapes, with_sizes
from oracle.ref_dists import inverse_cdf_index, sampling_margin
from tests.config_matrix import _A, _V, EXTRA_CASES, SAMPLING_MARGIN, SCAN_CASES

_SA = 32  # hidden of the small MMTRSSM cases


def _mr(name: str, deter: int, hidden: int, classes: int, cats: int, batch: int, steps: int, action: int = 4, embed: int = 32) -> Case:  # noqa: PLR0913
    return Case(name, "mrssm", _mrssm_dims(deter, hidden, classes, cats, action, embed, _A, _V, **_SMALL), batch, steps, _A, _V, query=2)


def _mt(name: str, ld: int, ls: tuple[int, int], hs: tuple[int, int], batch: int, steps: int) -> Case:  # noqa: PLR0913
    return Case(name, "mmtrssm", _mmtrssm_dims(32, hs, ld, ls, _SA, 4, 32, _A, _V, **_SMALL), batch, steps, _A, _V, query=2)


# case id -> (case, scan family it must reach); the families are those of ``tests.config_matrix.SCAN_CASES``
CLASS_CASES: dict[str, tuple[Case, str]] = {
    "c32_16x2": (_mr("c32_16x2", 32, 32, 16, 2, 5, 6), "cluster"),            # S = 32: the cluster BPTT's limit
    "c64_10x3": (_mr("c64_10x3", 64, 64, 10, 3, 5, 6), "cluster"),            # C not a power of two, S = 30
    "c128_32x1": (_mr("c128_32x1", 128, 128, 32, 1, 3, 5), "cluster"),        # K = 1: one live lane
    "c200_9x3": (_mr("c200_9x3", 200, 200, 9, 3, 4, 6), "cluster"),           # the bench's instance, C one past the fast path
    "w256_16x8": (_mr("w256_16x8", 256, 32, 16, 8, 3, 4), "wide"),            # S = 128
    "w32x256_12x5": (_mr("w32x256_12x5", 32, 256, 12, 5, 3, 4), "wide"),      # S = 60: padded to 64 with C > 8
    "s24x40_12x3": (_mr("s24x40_12x3", 24, 40, 12, 3, 5, 6, action=3, embed=20), "scan"),
    "s32_2x70": (_mr("s32_2x70", 32, 32, 2, 70, 3, 5), "scan"),               # K = 70 > 64: the cluster scan must refuse
    "w256_2x65": (_mr("w256_2x65", 256, 32, 2, 65, 3, 4), "scan"),            # K = 65 > 64: the wide scan must refuse
    "mt32_l12x3_h2x8": (_mt("mt32_l12x3_h2x8", 32, (12, 3), (2, 8), 5, 6), "mt_scan"),
    "mw128_l12x3_h2x8": (_mt("mw128_l12x3_h2x8", 128, (12, 3), (2, 8), 5, 4), "mt_wide"),   # lower level general, higher fast
    "mw128_l4x4_h16x2": (_mt("mw128_l4x4_h16x2", 128, (4, 4), (16, 2), 5, 4), "mt_wide"),   # the reverse
}

WIDE_FAMILIES = frozenset({"wide", "mt_wide"})
COOPERATIVE = frozenset({"cluster", "wide", "mt_wide"})

# one Tanh / plain-KL run (``tests.config_matrix.options``) per family
TANH_KL_CASES = ("c64_10x3", "w32x256_12x5", "s24x40_12x3", "mt32_l12x3_h2x8", "mw128_l12x3_h2x8")
# the wide families once more at the shipped two bf16 pieces
TWO_PIECE_CASES = tuple(k for k, (_, fam) in CLASS_CASES.items() if fam in WIDE_FAMILIES)
# one masked and weighted run per cooperative family (the MASKED instantiations hold their own copy of the branch)
MASKED_CASES = ("c32_16x2", "w256_16x8", "mw128_l12x3_h2x8")

# runs of test 1: (case id, option set or None, bf16 pieces of the wide families)
PARITY_RUNS: list[tuple[str, str | None, int]] = (
    [(k, None, 3) for k in CLASS_CASES] + [(k, "tanh_kl", 3) for k in TANH_KL_CASES] + [(k, None, 2) for k in TWO_PIECE_CASES])

# ---------------------------------------------------------------------------------------------
# the tie rule: constant logit rows, uniforms on and next to the CDF's edges
# ---------------------------------------------------------------------------------------------
# every class count here is a power of two: exp(0) = 1, the sum C, 1 / C and the running sum j / C are exact in fp32
TIE_CASES: dict[str, tuple[Case, str]] = {
    "c32_16x2": CLASS_CASES["c32_16x2"],
    "c128_32x1": CLASS_CASES["c128_32x1"],
    "w256_16x8": CLASS_CASES["w256_16x8"],
    "mw128_l4x4_h16x2": CLASS_CASES["mw128_l4x4_h16x2"],
    "mrssm_default": SCAN_CASES["mrssm_default"],        # 4 x 4, cluster: the fast8 path
    "mrssm_nonsquare": SCAN_CASES["mrssm_nonsquare"],    # 2 x 8, single-CU
    "mmtrssm_default": SCAN_CASES["mmtrssm_default"],    # single-CU MMTRSSM
    "w256": (EXTRA_CASES["w256"], "wide"),               # 4 x 4, wide
}
# the second Linear of every head that feeds a categorical (``oracle.cases.build_model``), and of the initial state's projection
TIE_HEADS = ("rnn_to_prior_projector.2.", "rnn_to_post_projector.2.", "l_prior.2.", "h_prior.2.", "h_posterior.2.", "init_proj.2.")
TIE_BIAS = 0.3


def flatten_heads(model: nn.Module) -> nn.Module:
    """``model`` with the last-layer weights of ``TIE_HEADS`` zeroed and their biases at ``TIE_BIAS``: every logit row is constant."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if any(h in name for h in TIE_HEADS):
                p.fill_(TIE_BIAS if name.endswith("bias") else 0.0)
    return model


def _classes_of(case: Case, key: str) -> int:
    d = case.dims
    if case.kind == "mrssm":
        return d.classes
    return d.hs_classes if key.endswith("_h") else d.ls_classes


def edge_noise(case: Case, seed: int = 17) -> dict[str, Tensor]:
    """Uniforms of four kinds, one drawn per element: j / C (on an edge of the uniform CDF), the fp32 number just below it
    (clamped at 0), 0, and 1 - 2^-24 (the largest fp32 below 1); j random in [0, C)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for key, shape in noise_shapes(case, case.batch, case.steps).items():
        classes = _classes_of(case, key)
        j = torch.randint(0, classes, shape, generator=g)
        kind = torch.randint(0, 4, shape, generator=g)
        edge = j.float() / classes
        below = torch.nextafter(edge, torch.tensor(-1.0)).clamp_min(0.0)
        u = torch.where(kind == 0, edge, torch.where(kind == 1, below, torch.where(kind == 2, torch.zeros(()), torch.tensor(1.0 - 2.0**-24))))
        assert u.dtype == torch.float32 and float(u.max()) < 1.0 and float(u.min()) >= 0.0
        out[key] = u
    return out


def tie_draws(case: Case) -> list[tuple[str, str, str, int, int]]:
    """(noise key, oracle output with the one-hot samples, oracle output with the logits, cats, classes) of every draw."""
    d = case.dims
    if case.kind == "mrssm":
        return [("u_init", "_stoch0", "_logits0", d.cats, d.classes), ("u_prior", "_prior_stoch", "_prior_logits", d.cats, d.classes),
                ("u_post", "_post_stoch", "_post_logits", d.cats, d.classes)]
    draws = []
    for lv, cats, classes in (("l", d.ls_cats, d.ls_classes), ("h", d.hs_cats, d.hs_classes)):
        draws += [(f"u_init_{lv}", f"_init_stoch_{lv}", f"_init_logits_{lv}", cats, classes),
                  (f"u_prior_{lv}", f"_prior_stoch_{lv}", f"_prior_logits_{lv}", cats, classes),
                  (f"u_post_{lv}", f"_post_stoch_{lv}", f"_post_logits_{lv}", cats, classes)]
    return draws


def floor_index(u: Tensor, classes: int) -> Tensor:
    """floor(u C) in float64: the index the tie rule gives under a uniform distribution over a power-of-two ``classes``."""
    return torch.floor(u.double() * classes).long()


# ---------------------------------------------------------------------------------------------
# saturated logits
# ---------------------------------------------------------------------------------------------
SATURATED_GAIN = 150.0
SATURATED_CASES: dict[str, tuple[Case, str]] = {
    "c32_16x2": (replace(CLASS_CASES["c32_16x2"][0], head_gain=SATURATED_GAIN), "cluster"),
    "mrssm_cfg2dims": (replace(with_sizes(CASES["mrssm_cfg2dims"], 4, 8), head_gain=SATURATED_GAIN), "cluster"),
    "w256": (replace(EXTRA_CASES["w256"], head_gain=SATURATED_GAIN), "wide"),
    "mw128": (replace(EXTRA_CASES["mw128"], head_gain=SATURATED_GAIN), "mt_wide"),
}


def float64_copy(model: nn.Module) -> nn.Module:
    return copy.deepcopy(model).double()


# ---------------------------------------------------------------------------------------------
# the initial-state head kernel on its own
# ---------------------------------------------------------------------------------------------
# (rows, K, C); the last has rows K = 259: one past a 256-thread block
HEAD_SHAPES = [(1, 1, 1), (3, 5, 2), (7, 3, 9), (4, 16, 16), (2, 2, 33), (37, 7, 12)]
HEAD_SEEDS = range(300, 340)
HEAD_USES = ("all", "sample", "logp")  # which outputs the functional reads: "sample" is the g_l = None arm, "logp" the g_p = None arm


def head_margin(probs: Tensor, u: Tensor) -> float:
    """Smallest |u - cdf| (``oracle.ref_dists.sampling_margin``); a single class has no edge."""
    return float("inf") if probs.shape[-1] == 1 else float(sampling_margin(probs, u).min())


def head_problem(rows: int, cats: int, classes: int) -> dict[str, Tensor | int | float]:
    """Logits ``randn * 3`` and uniforms re-drawn over ``HEAD_SEEDS`` until the float64 margin is ``SAMPLING_MARGIN``; the float64
    log-probabilities, probabilities and inverse-CDF index; fixed random weights of the functional.  Asserts a seed qualifies."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * cats + classes)
    logits = torch.randn(rows, cats * classes, generator=g) * 3.0
    weights = {k: torch.randn(rows, cats, classes, generator=g) for k in ("sample", "logp", "probs")}
    shaped = logits.double().reshape(rows, cats, classes)
    logp, probs = torch.log_softmax(shaped, dim=-1), torch.softmax(shaped, dim=-1)
    seen = []
    for seed in HEAD_SEEDS:
        u = torch.rand(rows, cats, generator=torch.Generator().manual_seed(seed))
        margin = head_margin(probs, u.double())
        if margin >= SAMPLING_MARGIN:
            return {"logits": logits, "u": u, "logp": logp, "probs": probs, "index": inverse_cdf_index(probs, u.double()),
                    "weights": weights, "margin": margin, "seed": seed}
        seen.append((seed, margin))
    msg = f"head {rows, cats, classes}: no seed in {HEAD_SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges: {seen}"
    raise AssertionError(msg)


def head_functional(sample: Tensor, logp: Tensor, probs: Tensor, weights: dict[str, Tensor], use: str) -> Tensor:
    """A fixed linear functional of the head's outputs (``sample`` flat ``[rows, K C]``, the others ``[rows, K, C]``)."""
    w = {k: v.to(sample) for k, v in weights.items()}
    total = sample.new_zeros(())
    if use in {"all", "sample"}:
        total = total + (sample.reshape(logp.shape) * w["sample"]).sum()
    if use in {"all", "logp"}:
        total = total + (logp * w["logp"]).sum()
    if use == "all":
        total = total + (probs * w["probs"]).sum()
    return total


def head_reference_grad(problem: dict, use: str) -> Tensor:
    """d functional / d logits by float64 autograd through log_softmax, softmax and the straight-through sample."""
    x = problem["logits"].double().requires_grad_()
    shaped = x.reshape(problem["probs"].shape)
    logp, probs = torch.log_softmax(shaped, dim=-1), torch.softmax(shaped, dim=-1)
    onehot = torch.nn.functional.one_hot(problem["index"], probs.shape[-1]).double()
    sample = (onehot + (probs - probs.detach())).flatten(start_dim=-2)
    head_functional(sample, logp, probs, problem["weights"], use).backward()
    return x.grad
