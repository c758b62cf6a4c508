"""The option matrix of the scan kernels (helper, no tests): the cases, option sets and noise screening shared by
``tests/test_config_matrix_host.py`` (oracle only, runs anywhere) and ``tests/test_config_matrix_gpu.py`` (MI355X).

Every other GPU parity test runs the model with ELU, KL balancing on, ``kl_coeff = w_kl_h = 1`` and the cluster scan at
D = H in {32, 200}.  The kernels take more: four activations (``_lib.ACT_IDS``), both KL weightings, two loss
coefficients, cluster sizes 64 and 128 and wide scans with D != H.  The cases below reach each scan family at the
smallest batch that still has a ragged row group; they stay out of ``oracle.cases.CASES`` (bench.py's view)."""

from __future__ import annotations

from dataclasses import replace

import torch
from torch import Tensor, nn

from oracle.cases import _SMALL, CASES, Case, _mmtrssm_dims, _mrssm_dims, build_noise, min_margin, with_sizes
from oracle.ref_dists import sampling_margin
from oracle.ref_model import cat_probs

_A, _V = (1, 16, 8), (1, 8, 8)  # frames of the extra cases (embed 32, action 4, the small conv stacks)

EXTRA_CASES: dict[str, Case] = {
    # cluster scan, the template instances no other test launches
    "c64": Case("c64", "mrssm", _mrssm_dims(64, 64, 4, 4, 4, 32, _A, _V, **_SMALL), 5, 6, _A, _V, query=3),
    # S = 30 <= 32: the cluster BPTT kernel too
    "c128": Case("c128", "mrssm", _mrssm_dims(128, 128, 5, 6, 4, 32, _A, _V, **_SMALL), 3, 5, _A, _V, query=2),
    # wide MRSSM scan with D != H, on either side
    "w256": Case("w256", "mrssm", _mrssm_dims(256, 32, 4, 4, 4, 32, _A, _V, **_SMALL), 3, 4, _A, _V, query=2),
    "w32x256": Case("w32x256", "mrssm", _mrssm_dims(32, 256, 4, 4, 4, 32, _A, _V, **_SMALL), 3, 4, _A, _V, query=2),
    # wide MMTRSSM scan below its usual ld = hd = 200, ld != hd
    "mw128": Case("mw128", "mmtrssm", _mmtrssm_dims(32, (2, 8), 128, (4, 4), 32, 4, 32, _A, _V, **_SMALL), 5, 4, _A, _V, query=2),
}

# case id -> (case, scan family it must reach)
SCAN_CASES: dict[str, tuple[Case, str]] = {
    "mrssm_nonsquare": (with_sizes(CASES["mrssm_nonsquare"], 5, 6), "scan"),       # D = 24 != H = 40: the single-CU scan
    "mrssm_default": (with_sizes(CASES["mrssm_default"], 5, 9), "cluster"),        # cluster 32
    "c64": (EXTRA_CASES["c64"], "cluster"),
    "c128": (EXTRA_CASES["c128"], "cluster"),
    "mrssm_cfg2dims": (with_sizes(CASES["mrssm_cfg2dims"], 4, 8), "cluster"),      # cluster 200
    "w256": (EXTRA_CASES["w256"], "wide"),
    "w32x256": (EXTRA_CASES["w32x256"], "wide"),
    "mmtrssm_default": (with_sizes(CASES["mmtrssm_default"], 5, 6), "mt_scan"),    # the single-CU MMTRSSM scan
    "mw128": (EXTRA_CASES["mw128"], "mt_wide"),
}

OPTION_SETS = ("relu", "tanh_kl", "identity")

# ReLU gradients are compared only where a noise seed keeps every ReLU input away from the kink (`screened`).  At
# D = H = 200 (26 k ReLU inputs per step batch, smallest |z| ~ 1e-6) no seed in the 40 tries does: forward values and losses
# only there; the gradients of that size are covered by Tanh and Identity.
RELU_VALUES_ONLY = frozenset({"mrssm_cfg2dims"})

SAMPLING_MARGIN = 1e-4  # oracle.cases.screened_noise's
RELU_MARGIN = 2e-5      # twice the 1e-5 absolute tolerance on forward values: a correct kernel stays on the oracle's side of the kink
SEEDS = range(100, 140)


def options(case: Case, name: str) -> dict:
    """The keyword arguments of ``with_options`` for an option set."""
    if name == "relu":
        return {"activation": "ReLU"}
    if name == "identity":
        return {"activation": "Identity"}
    if name == "tanh_kl":
        kl = {"use_kl_balancing": False, "kl_coeff": 0.7}
        if case.kind == "mmtrssm":
            kl["w_kl_h"] = 0.3
        return {"activation": "Tanh", **kl}
    raise KeyError(name)


def with_options(case: Case, activation: str | None = None, **kl: float | bool) -> Case:
    """``case`` with another activation of the scan's MLPs and / or other KL options (``use_kl_balancing``, ``kl_coeff``,
    ``w_kl_h``); the seeded weights do not depend on either."""
    fields = dict(kl)
    if activation is not None:
        fields["activation"] = activation
    return replace(case, dims=replace(case.dims, **fields))


def relu_margin_for(case_id: str, option_set: str) -> float:
    return RELU_MARGIN if option_set == "relu" and case_id not in RELU_VALUES_ONLY else 0.0


def screened(case: Case, model: nn.Module, batch: tuple[Tensor, ...], relu_margin: float = 0.0) -> tuple[dict[str, Tensor], float, int]:
    """``oracle.cases.screened_noise`` with a second condition and no fallback: the first noise seed in ``SEEDS`` under which
    (1) every categorical draw keeps ``SAMPLING_MARGIN`` from its CDF edges and (2) every input of every ``nn.ReLU`` of the
    oracle keeps ``|z| >= relu_margin`` (forward hooks).  Returns (noise, sampling margin, seed); asserts that a seed qualifies."""
    b, t = batch[0].shape[:2]
    smallest = [float("inf")]

    def hook(_module: nn.Module, inputs: tuple[Tensor, ...], _output: Tensor) -> None:
        smallest[0] = min(smallest[0], float(inputs[0].detach().abs().min()))

    handles = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, nn.ReLU)] if relu_margin > 0 else []
    seen = []
    try:
        for seed in SEEDS:
            noise = build_noise(case, seed, batch=b, steps=t)
            smallest[0] = float("inf")
            with torch.no_grad():
                out = model.shared_step(batch, noise)
            margin = min_margin(case, out, noise)
            if margin >= SAMPLING_MARGIN and smallest[0] >= relu_margin:
                return noise, margin, seed
            seen.append((seed, margin, smallest[0]))
    finally:
        for h in handles:
            h.remove()
    msg = f"{case.name}: no noise seed in {SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges and {relu_margin} from the ReLU kink: {seen}"
    raise AssertionError(msg)


def screened_prior(case: Case, model: nn.Module, actions: Tensor, state0: dict[str, Tensor]) -> tuple[dict[str, Tensor], int]:
    """Uniforms of a prior-only rollout of ``actions.shape[1]`` steps from ``state0``: the first seed in ``SEEDS`` whose every
    draw keeps ``SAMPLING_MARGIN`` from the CDF edges under the oracle.  Returns (noise for ``rollout_transition``, seed)."""
    d = case.dims
    b, n = actions.shape[:2]
    for seed in SEEDS:
        full = build_noise(case, seed, batch=b, steps=n)
        with torch.no_grad():
            if case.kind == "mrssm":
                u = {"u_prior": full["u_trans"]}
                out = model.rollout_transition(actions, state0, u["u_prior"])
                pairs = [(out["prior_logits"], u["u_prior"], d.cats, d.classes)]
            else:
                u = {"u_prior_h": full["u_trans_h"], "u_prior_l": full["u_trans_l"]}
                out = model.rollout_transition(actions, state0, u)
                pairs = [(out["prior_logits_h"], u["u_prior_h"], d.hs_cats, d.hs_classes),
                         (out["prior_logits_l"], u["u_prior_l"], d.ls_cats, d.ls_classes)]
        margin = min(float(sampling_margin(cat_probs(lg, cats, classes)[1], uu).min()) for lg, uu, cats, classes in pairs)
        if margin >= SAMPLING_MARGIN:
            return u, seed
    msg = f"{case.name}: no prior-rollout noise seed in {SEEDS} keeps {SAMPLING_MARGIN} from the CDF edges"
    raise AssertionError(msg)
