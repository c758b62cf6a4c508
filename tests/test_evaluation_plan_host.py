"""CPU: ``evaluation.CopyPlan`` -- what the copies of a row are in an evaluation rollout.

The four plans the config objects build are expanded on a two-row batch (``T = 6``, lengths ``[6, 4]``, three copies) and compared with
wide tensors written out here by hand: the codes and the frame-0 mask of every scan row, the widened uniforms of the three layouts
(``row``, ``copy``, ``tail``) and the row order.  The base codes come from ``Forecast.reference``.  Wrong shapes are refused in the one
wording every evaluator uses, and the ``noise_shapes`` of the five config classes are the dicts their own code spelled out before they
shared one helper.
"""

from __future__ import annotations

import pytest
import torch

from multimodal_mtrssm_amd import EpisodePanel, Forecast, ForecastSkill, LatentProbe, LikelihoodBound, WordTransitions
from multimodal_mtrssm_amd.evaluation import CopyPlan
from oracle.cases import CASES, build_model
from tests.conftest import product_from_case

B, T, S, K = 2, 6, 3, 4
VALID = torch.tensor([6, 4], dtype=torch.int32)
SIZES = {"u_init": K, "u_post": K}


def _base(*contexts: int | None) -> dict:
    """Per context the codes ``[B, T]`` of a row that observes both modalities on it, and the frame-0 mask (both rows are live at 0)."""
    mask0 = torch.ones(B, 2, dtype=torch.bool)
    return {c: (Forecast(T if c is None else c).reference(torch.zeros(B), T, VALID).codes, mask0) for c in contexts}


def _uniforms(*shape: int, seed: int) -> torch.Tensor:
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def test_skill_plan_shares_the_context_and_reads_own_tails() -> None:
    plan = ForecastSkill(2, samples=S, observe="audio").plan()
    assert plan == CopyPlan(S, 1, 2, init="row", post="tail", order="row") and plan.contexts == (2,) and plan.shares_frame0
    u_post, u_tail = _uniforms(B, T, K, seed=1), _uniforms(B, S, T, K, seed=2)
    codes, mask0, noise, spread = plan.expand(_base(2), {"u_post": u_post, "u_tail": u_tail}, {"u_post": K})
    assert codes.dtype == torch.int32 and codes.tolist() == [[1, 1, 0, 0, 0, 0]] * (B * S)
    assert mask0.tolist() == [[True, False]] * (B * S) and plan.first(mask0).tolist() == [[True, False]] * B
    assert tuple(noise["u_post"].shape) == (B * S, T, K) and noise["u_post"].is_contiguous()
    for b in range(B):
        for s in range(S):
            row = noise["u_post"][b * S + s]
            assert torch.equal(row[:2], u_post[b, :2]) and torch.equal(row[2:], u_tail[b, s, 2:]), (b, s)
    x = torch.arange(B * 5.0).reshape(B, 5)
    assert torch.equal(spread(x), torch.stack([x[0], x[0], x[0], x[1], x[1], x[1]]))
    drawn = plan.expand(_base(2), None, {"u_post": K})[2]["u_post"]  # absent uniforms are drawn: the copies still share the context
    assert torch.equal(drawn[0, :2], drawn[2, :2]) and not torch.equal(drawn[0, 2:], drawn[2, 2:])
    # a context longer than T behaves as T: every live frame observed, no tail read
    long = ForecastSkill(9, samples=S).plan()
    codes, _, noise, _ = long.expand(_base(9), {"u_post": u_post, "u_tail": u_tail}, {"u_post": K})
    assert codes.tolist() == [[3] * 6] * S + [[3, 3, 3, 3, 0, 0]] * S and torch.equal(noise["u_post"], u_post.repeat_interleave(S, 0))


def test_likelihood_plan_takes_every_copys_own_uniforms_as_they_lie() -> None:
    plan = LikelihoodBound(samples=S, observe="vision").plan()
    assert plan == CopyPlan(S, 2, None, init="copy", post="copy", order="row") and plan.contexts == (None,)
    u_init, u_post = _uniforms(B, S, K, seed=3), _uniforms(B, S, T, K, seed=4)
    codes, mask0, noise, _ = plan.expand(_base(None), {"u_init": u_init, "u_post": u_post}, SIZES)
    assert codes.tolist() == [[2] * 6] * S + [[2, 2, 2, 2, 0, 0]] * S and mask0.tolist() == [[False, True]] * (B * S)
    assert torch.equal(noise["u_init"], u_init.reshape(B * S, K)) and torch.equal(noise["u_post"], u_post.reshape(B * S, T, K))
    left = plan.expand(_base(None), {}, SIZES)[2]  # absent: left to the consumer's own draw over the wide rows
    assert left.get("u_init") is None and left.get("u_post") is None


def test_probe_plan_gives_every_copy_its_subset_and_the_rows_uniforms() -> None:
    plan = LatentProbe(("both", "audio", "vision")).plan()
    assert plan == CopyPlan(3, (3, 1, 2), None) and not plan.shares_frame0
    u_init, u_post = _uniforms(B, K, seed=5), _uniforms(B, T, K, seed=6)
    codes, mask0, noise, _ = plan.expand(_base(None), {"u_init": u_init, "u_post": u_post}, SIZES)
    assert codes.tolist() == [[3] * 6, [1] * 6, [2] * 6, [3, 3, 3, 3, 0, 0], [1, 1, 1, 1, 0, 0], [2, 2, 2, 2, 0, 0]]
    assert mask0.tolist() == [[True, True], [True, False], [False, True]] * B
    assert torch.equal(noise["u_init"], torch.stack([u_init[0]] * 3 + [u_init[1]] * 3))
    assert torch.equal(noise["u_post"], torch.stack([u_post[0]] * 3 + [u_post[1]] * 3))
    drawn = plan.expand(_base(None), None, SIZES)[2]  # drawn per ROW: the copies of a row share their uniforms
    assert tuple(drawn["u_post"].shape) == (B * 3, T, K) and torch.equal(drawn["u_post"][0], drawn["u_post"][2])
    assert torch.equal(drawn["u_init"][3], drawn["u_init"][5]) and not torch.equal(drawn["u_init"][0], drawn["u_init"][3])


def test_panel_plan_lies_in_copy_order() -> None:
    plan = EpisodePanel(3).plan()
    assert plan == CopyPlan(2, 3, (None, 3), order="copy") and plan.contexts == (None, 3) and plan.shares_frame0
    u_post = _uniforms(B, T, K, seed=7)
    codes, mask0, noise, spread = plan.expand(_base(None, 3), {"u_post": u_post}, {"u_post": K})
    assert codes.tolist() == [[3] * 6, [3, 3, 3, 3, 0, 0], [3, 3, 3, 0, 0, 0], [3, 3, 3, 0, 0, 0]] and codes.is_contiguous()
    assert mask0.tolist() == [[True, True]] * 4
    assert torch.equal(noise["u_post"], torch.cat([u_post, u_post]))
    x = torch.arange(B * 5.0).reshape(B, 5)
    assert torch.equal(spread(x), torch.cat([x, x])) and torch.equal(plan.first(spread(x)), x)
    heard = EpisodePanel(9, observe="audio").plan()  # a query longer than T: both halves observe every live frame
    assert heard.expand(_base(None, 9), None, {})[0].tolist() == [[1] * 6, [1, 1, 1, 1, 0, 0]] * 2


def test_wrong_shapes_are_refused_in_one_wording() -> None:
    row, own, tail = LatentProbe().plan(), LikelihoodBound(samples=S).plan(), ForecastSkill(2, samples=S).plan()
    with pytest.raises(ValueError, match=r"noise\['u_post'\] must have shape \(2, 6, 4\), got \(2, 5, 4\)"):
        row.expand(_base(None), {"u_post": torch.zeros(B, T - 1, K)}, SIZES)
    with pytest.raises(ValueError, match=r"noise\['u_init'\] must have shape \(2, 4\)"):
        row.expand(_base(None), {"u_init": torch.zeros(B, S, K)}, SIZES)
    with pytest.raises(ValueError, match=r"noise\['u_init'\] must have shape \(2, 3, 4\)"):
        own.expand(_base(None), {"u_init": torch.zeros(B, K)}, SIZES)
    with pytest.raises(ValueError, match=r"noise\['u_post'\] must have shape \(2, 3, 6, 4\)"):
        own.expand(_base(None), {"u_post": torch.zeros(B * S, T, K)}, SIZES)
    with pytest.raises(ValueError, match=r"noise\['u_tail'\] must have shape \(2, 3, 6, 4\)"):
        tail.expand(_base(2), {"u_tail": torch.zeros(B, S - 1, T, K)}, {"u_post": K})
    with pytest.raises(ValueError, match=r"noise\['u_post'\] must have shape \(2, 6, 4\)"):
        tail.expand(_base(2), {"u_post": torch.zeros(B, S, T, K)}, {"u_post": K})
    with pytest.raises(ValueError, match=r"noise\['u_prior'\] must have shape \(2, 3, 1, 4\)"):
        WordTransitions(2, samples=S, protocol="reference").plan().uniforms("u_prior", torch.zeros(B, S, K), "copy", B, 1, K)
    for kw in ({"init": "tail"}, {"post": "each"}, {"order": "sample"}, {"bits": (3, 1)}, {"context": (None, 2)}, {"copies": 0}):
        with pytest.raises(ValueError, match="must be one of|one entry per copy"):
            CopyPlan(**{"copies": S, "bits": 3, "context": None, **kw})
    with pytest.raises(ValueError, match="ONE context"):
        CopyPlan(2, 3, (None, 2), post="tail")


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_noise_shapes_are_what_each_config_spelled_out(name: str) -> None:
    case = CASES[name]
    model = product_from_case(case, build_model(case), "cpu")
    b, t, s = 5, 8, 3
    if case.kind == "mrssm":
        k = model.transition.distribution_factory.category_size
        rows = {"u_init": (b, k), "u_post": (b, t, k)}
        skill = {"u_init": (b, k), "u_post": (b, t, k), "u_tail": (b, s, t, k)}
        own = {"u_init": (b, s, k), "u_post": (b, s, t, k)}
        prior = {"u_init": (b, k), "u_prior": (b, s, 1, k)}
    else:
        kl, kh = model.l_dist.category_size, model.h_dist.category_size
        rows = {"u_init_h": (b, kh), "u_init_l": (b, kl), "u_post_l": (b, t, kl), "u_post_h": (b, t, kh)}
        skill = {"u_init_h": (b, kh), "u_init_l": (b, kl), "u_post_l": (b, t, kl), "u_post_h": (b, t, kh),
                 "u_tail_l": (b, s, t, kl), "u_tail_h": (b, s, t, kh)}
        own = {"u_init_h": (b, s, kh), "u_init_l": (b, s, kl), "u_post_l": (b, s, t, kl), "u_post_h": (b, s, t, kh)}
        prior = {"u_init_h": (b, kh), "u_init_l": (b, kl), "u_prior_l": (b, s, 1, kl), "u_prior_h": (b, s, 1, kh)}
    assert ForecastSkill(2, samples=s).noise_shapes(model, b, t) == skill
    assert list(ForecastSkill(2, samples=s).noise_shapes(model, b, t)) == list(skill)  # (a seeded draw goes through them in this order)
    assert LikelihoodBound(samples=s).noise_shapes(model, b, t) == own
    assert LatentProbe().noise_shapes(model, b, t) == rows and EpisodePanel(3).noise_shapes(model, b, t) == rows
    assert WordTransitions(2, samples=s).noise_shapes(model, b, t) == skill
    assert WordTransitions(2, samples=s, protocol="reference").noise_shapes(model, b, t) == prior
    assert rows == {k: v for k, v in model.noise_shapes(b, t).items() if k.startswith(("u_init", "u_post"))}  # the model's own
