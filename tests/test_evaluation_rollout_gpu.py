"""GPU: one evaluation rollout behind every evaluator.

``render_episodes``, ``likelihood_bound`` and ``probe_features`` reach the scan through the same ``_evaluation_rollout`` under three
different ``CopyPlan``s.  Given the same uniforms per row, the rows that observe both modalities on every frame -- the posterior half of
the panels, the one copy of a ``LikelihoodBound(samples=1)`` and the ``"both"`` group of the probes -- are the same rollout: they sample
the same classes, and their ``deter`` agree to 1e-5 (the bound ``test_episode_panel_gpu.test_states_are_the_public_rollouts`` uses for
the same comparison across calls, for the reason written there: the encoders' split reductions meet in fp32 atomics).  The shapes, the
batch and the screened noise are that module's ``_setup``.
"""

from __future__ import annotations

import pytest
import torch

from multimodal_mtrssm_amd import EpisodePanel, LatentProbe, LikelihoodBound
from tests.conftest import product_from_case
from tests.test_episode_panel_gpu import MODELS, B, Q, T, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", MODELS)
def test_three_evaluators_run_the_same_closed_loop_rollout(name: str) -> None:
    ref = _setup(name)
    model = product_from_case(ref["case"], ref["oracle"], DEV)
    batch = tuple(x.to(DEV) for x in ref["batch"])
    noise = {k: v.to(DEV) for k, v in ref["noise"].items()}
    panels = model.render_episodes(batch, EpisodePanel(Q, label=0), noise, keep_states=True).states
    one = model.likelihood_bound(batch, LikelihoodBound(samples=1), {k: u.unsqueeze(1) for k, u in noise.items()}, keep_states=True).states
    x, valid = model.probe_features(batch, LatentProbe(), noise)
    torch.cuda.synchronize()
    assert valid is None and tuple(x.shape[:3]) == (3, B, T)
    if ref["case"].kind == "mrssm":
        deter = model.transition.deterministic_size
        columns = {"deter": (0, deter), "stoch": (deter, x.shape[-1])}
    else:
        hd, hs, ld = model.hd_dim, model.hs_dim, model.ld_dim
        columns = {"deter_h": (0, hd), "stoch_h": (hd, hd + hs), "deter_l": (hd + hs, hd + hs + ld), "stoch_l": (hd + hs + ld, x.shape[-1])}
    for key, (lo, hi) in columns.items():
        a, b, c = getattr(panels, key)[:B], getattr(one, key), x[0, :, :, lo:hi]
        assert tuple(a.shape) == tuple(b.shape) == tuple(c.shape) == (B, T, hi - lo), key
        if key.startswith("stoch"):
            assert torch.equal(a, b) and torch.equal(a, c), key
            continue
        err = max(float((a - b).abs().max()), float((a - c).abs().max()), float((b - c).abs().max()))
        print(name, key, "max |deter difference| between the three rollouts", err)
        assert err <= 1e-5, (key, err)  # noqa: PLR2004
