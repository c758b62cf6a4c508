"""Weighted MoPoE on the GPU: what must NOT change (constant 1/3 weights, a zero-initialised gate, a
modality that is absent everywhere), and that the weights travel wherever the masked rollouts go (rows and prefixes, the
captured step, sharded batches, skill steps).

Tolerances are not chosen here: bitwise where the arithmetic is the same, the rerun yardstick of
``test_modality_dropout_gpu._same_up_to_reruns`` for eager training steps, ``rtol = 1e-4`` of
``test_captured_masked_step_matches_eager`` for graph against eager, ``rtol = 1e-5`` of the data-parallel loss terms, and the
``rtol = 2e-5`` of the skill tables (``test_forecast_skill_gpu._assert_step``).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import conv, linear, scan
from multimodal_mtrssm_amd.experts import LOG_THIRD, ExpertWeights
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from multimodal_mtrssm_amd.parallel import GlobalRowNoise
from multimodal_mtrssm_amd.skill import ForecastSkill
from oracle.cases import CASES, build_batch, build_model, build_noise, with_sizes
from tests.conftest import product_from_case
from tests.test_modality_dropout_gpu import _same_up_to_reruns, _train

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODELS = ["mrssm_cfg2dims", "mmtrssm_cfg3dims"]
# (case, one-CU kernels forced): cluster, one-CU, wide MRSSM; one-CU MMTRSSM twice (default and forced rows_per_block)
FAMILIES = [("mrssm_cfg2dims", False), ("mrssm_cfg2dims", True), ("mrssm_large", False), ("mmtrssm_cfg3dims", False),
            ("mmtrssm_cfg3dims", True)]
FAMILY_IDS = [f"{c}{'-onecu' if f else ''}" for c, f in FAMILIES]
_TENSORS = ("deter", "stoch", "deter_l", "deter_h", "hidden_l", "hidden_h", "stoch_l", "stoch_h", "kl_per_step", "kl_h_per_step")
_DISTS = ("distribution", "distribution_l", "distribution_h")


def _setup(name: str, onecu: bool = False, sizes: tuple[int, int] | None = None):  # noqa: ANN202, FBT001, FBT002
    case = CASES[name] if sizes is None else with_sizes(CASES[name], *sizes)
    model = product_from_case(case, build_model(case), DEV)
    if onecu:
        model.scan_rows_per_block = 1
    batch = tuple(b.to(DEV) for b in build_batch(case))
    noise = {k: v.to(DEV) for k, v in build_noise(case).items()}
    return case, model, batch, noise


def _mask(B: int, T: int, seed: int = 21) -> torch.Tensor:  # noqa: N803
    """All four codes, both modalities at t = 0 and on most steps."""
    m = torch.rand(B, T, 2, generator=torch.Generator().manual_seed(seed)) < 0.7
    m[:, 0] = True
    m[0, 1], m[0, 2], m[0, 3] = torch.tensor([False, False]), torch.tensor([True, False]), torch.tensor([False, True])
    return m.to(DEV)


def _random_logw(B: int, T: int, seed: int = 23) -> torch.Tensor:  # noqa: N803
    return torch.log_softmax(2.0 * torch.randn(B, T, 3, generator=torch.Generator().manual_seed(seed)), dim=-1).to(DEV)


def _seeded_gate(mode: str, embed: int, seed: int = 29) -> ExpertWeights:
    gate = ExpertWeights(mode, embed if mode == "gated" else None)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in gate.parameters():
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return gate.to(DEV)


def _fields(states) -> dict[str, torch.Tensor]:  # noqa: ANN001
    """Every tensor of a (posterior, prior) pair or of one state."""
    out = {}
    for i, st in enumerate(states if isinstance(states, tuple) else (states,)):
        for k in _TENSORS:
            if getattr(st, k, None) is not None:
                out[f"{i}.{k}"] = getattr(st, k)
        for k in _DISTS:
            if getattr(st, k, None) is not None:
                out[f"{i}.{k}.logits"] = getattr(st, k).logits
    return out


def _rollout(model, batch, noise, mask=None, rows=slice(None), steps=slice(None), observations=None, **kw):  # noqa: ANN001, ANN003, ANN202, PLR0913
    sub = lambda x: None if x is None else x[rows][:, steps]  # noqa: E731
    noise = {k: (v[rows] if v.dim() == 2 else v[rows][:, steps]) for k, v in noise.items()}  # noqa: PLR2004
    obs = (batch[1], batch[2]) if observations is None else observations
    obs = tuple(sub(o) for o in obs)
    m = sub(mask)
    first = tuple(None if o is None else o[:, 0] for o in obs)
    s0 = model.initial_state(first, noise, modality_mask=None if m is None else m[:, 0])
    return model.rollout_representation(actions=sub(batch[0]), observations=obs, prev_state=s0, noise=noise, modality_mask=m, **kw)


def _assert_same_bits(got, want, what: str) -> None:  # noqa: ANN001
    got, want = _fields(got), _fields(want)
    assert set(got) == set(want) and len(got) >= 6  # noqa: PLR2004
    differ = []
    for k in want:
        if not torch.equal(got[k], want[k]):
            differ.append(k)
            print(f"{what}: {k} differs by at most {float((got[k] - want[k]).abs().max()):.3e}")
    assert not differ, f"{what}: {differ}"


# 1. constant weights == no weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=FAMILY_IDS)
def test_constant_third_is_the_unweighted_rollout_bit_for_bit(name: str, onecu: bool, monkeypatch: pytest.MonkeyPatch) -> None:  # noqa: FBT001
    """``mrssm_large`` runs with every library GEMM summing in order (``split_r = 1``).  At its default the large model's rollout
    does not rerun bitwise at all, with or without weights: the hoisted 1024-wide GEMMs and the fused input-path GEMM in front of
    the wide scan split their reduction over workgroups and add the slices in arrival order (``linear.py``).  Measured on an
    MI355X, two unweighted runs of ``scan._MrssmScan`` on identical inputs: 2.6e-8 apart (deter), 4.5e-7 (prior logits), 9.5e-7
    (posterior logits), 1.3e-6 (KL per step), samples equal; constant weights against none: the same sizes (3.4e-8 / 7.2e-7 /
    9.5e-7 / 1.3e-6).  With ordered sums both reruns and this comparison are bitwise.  The other families rerun bitwise as they are."""
    if name == "mrssm_large":
        ordered = linear._problem  # noqa: SLF001
        monkeypatch.setattr(linear, "_problem", lambda *a, **kw: ordered(*a, **{**kw, "split_r": 1}))
    case, model, batch, noise = _setup(name, onecu)
    B, T = case.batch, case.steps
    third = torch.full((B, T, 3), LOG_THIRD, dtype=torch.float32, device=DEV)
    mask = _mask(B, T)
    with torch.no_grad():
        want = _rollout(model, batch, noise, mask)
        assert model.weights_timeseries is None  # nothing is reported without weights
        got = _rollout(model, batch, noise, mask, expert_log_weights=third)
        _assert_same_bits(got, want, "masked")
        codes = scan.modality_codes(mask)
        assert torch.equal(model.weights_timeseries, ExpertWeights.table(third, codes))
        # no mask at all: the weighted call runs the masked kernels on all-"both" codes, the plain one the unmasked kernels
        _assert_same_bits(_rollout(model, batch, noise, expert_log_weights=third), _rollout(model, batch, noise), "unmasked")
    scan.check_cluster_status()


@pytest.mark.parametrize("name", MODELS)
def test_constant_third_is_the_unweighted_training_step(name: str) -> None:
    case, model, batch, noise = _setup(name)
    third = torch.full((case.batch, case.steps, 3), LOG_THIRD, dtype=torch.float32, device=DEV)
    mask = _mask(case.batch, case.steps)
    ref, gref = _train(model, batch, noise, modality_mask=mask)
    ref2, gref2 = _train(model, batch, noise, modality_mask=mask)
    got, ggot = _train(model, batch, noise, modality_mask=mask, expert_log_weights=third)
    assert set(got) == set(ref) and set(ggot) == set(gref)
    for k in ref:
        _same_up_to_reruns(got[k], ref[k], ref2[k], k)
    for k in gref:
        _same_up_to_reruns(ggot[k], gref[k], gref2[k], k)


# 2. a zero-initialised gate == no weights ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["static", "gated"])
@pytest.mark.parametrize("name", MODELS)
def test_fresh_gate_is_the_unweighted_model(name: str, mode: str) -> None:
    case, model, batch, noise = _setup(name)
    mask = _mask(case.batch, case.steps)
    with torch.no_grad():
        want = _rollout(model, batch, noise, mask)
    ref, gref = _train(model, batch, noise, modality_mask=mask)
    ref2, gref2 = _train(model, batch, noise, modality_mask=mask)
    model.expert_weights = ExpertWeights(mode, case.dims.embed if mode == "gated" else None).to(DEV)
    with torch.no_grad():
        _assert_same_bits(_rollout(model, batch, noise, mask), want, mode)
    both = scan.modality_codes(mask) == 3  # noqa: PLR2004
    table = model.weights_timeseries
    assert tuple(table.shape) == (case.batch, case.steps, 3) and not table.requires_grad
    np.testing.assert_allclose(table[both].cpu().numpy(), 1.0 / 3.0, rtol=0, atol=1e-7)
    assert torch.equal(table[~both], ExpertWeights.table(None, scan.modality_codes(mask))[~both])
    got, ggot = _train(model, batch, noise, modality_mask=mask)
    for k in ref:
        _same_up_to_reruns(got[k], ref[k], ref2[k], k)
    for k in gref:
        _same_up_to_reruns(ggot[k], gref[k], gref2[k], k)
    new = [k for k in ggot if k.startswith("expert_weights.")]
    assert new and all(bool(torch.isfinite(ggot[k]).all()) for k in new)  # the gate is trained from the first step on
    assert any(float(ggot[k].abs().max()) > 0.0 for k in new)


# 3. rows and prefixes --------------------------------------------------------------------------------------------------------------
# (the families whose rollouts rerun bitwise at their defaults: not the wide one, see test_constant_third_is_the_unweighted_rollout_bit_for_bit)
@pytest.mark.parametrize(("name", "onecu"), [f for f in FAMILIES if f[0] != "mrssm_large"], ids=[i for i in FAMILY_IDS if i != "mrssm_large"])
def test_weighted_rollout_is_row_independent_and_causal(name: str, onecu: bool) -> None:  # noqa: FBT001
    case, model, batch, noise = _setup(name, onecu)
    B, T = case.batch, case.steps
    mask, lw = _mask(B, T), _random_logw(B, T)
    with torch.no_grad():
        full = _fields(_rollout(model, batch, noise, mask, expert_log_weights=lw))
        plain = _fields(_rollout(model, batch, noise, mask))
        assert not torch.equal(full["0.kl_per_step"], plain["0.kl_per_step"])  # the weights do something
        rows = _fields(_rollout(model, batch, noise, mask, rows=slice(0, 2), expert_log_weights=lw[:2].contiguous()))
        for k, v in rows.items():
            assert torch.equal(v, full[k][:2]), f"rows: {k}"
        tp = T - 2
        prefix = _fields(_rollout(model, batch, noise, mask, steps=slice(0, tp), expert_log_weights=lw[:, :tp].contiguous()))
        for k, v in prefix.items():
            assert torch.equal(v, full[k][:, :tp]), f"prefix: {k}"
    scan.check_cluster_status()


def test_weights_need_the_right_shape_on_the_device_too() -> None:
    case, model, batch, noise = _setup("mrssm_cfg2dims")
    with torch.no_grad(), pytest.raises(ValueError, match="expert log-weights"):
        _rollout(model, batch, noise, expert_log_weights=torch.zeros(case.batch, case.steps, 2, device=DEV))
    with torch.no_grad(), pytest.raises(ValueError, match="expert log-weights"):
        _rollout(model, batch, noise, expert_log_weights=torch.zeros(case.batch, case.steps, 3, device=DEV, dtype=torch.float64))


# 4. the captured step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_captured_weighted_masked_step_matches_eager(name: str) -> None:
    """``test_captured_masked_step_matches_eager`` (mode ``masked``: sizes, learning rate, noise seed, criteria) on a gated model,
    three steps with a different mask each."""
    case = with_sizes(CASES[name], 6, 9)
    oracle = build_model(case)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    masks = [_mask(6, 9, seed=40 + i) for i in range(3)]
    results = {}
    for run in ("eager", "graph"):
        model = product_from_case(case, oracle, DEV)
        model.expert_weights = _seeded_gate("gated", case.dims.embed)
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(6, 9)
        losses, tables = [], []
        start = flat.param.clone()
        if run == "eager":
            for i in range(3):
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step((*batch, masks[i]), noise)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v.detach()) for k, v in out.items()})
                tables.append(model.weights_timeseries.clone())
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, (*batch, masks[0]), source, warmup=3, masked=True)
            for i in range(3):
                out = cap.step((*batch, masks[i]))
                losses.append({k: float(v) for k, v in out.items()})
                tables.append(model.weights_timeseries.clone())
            cap.close()
        scan.check_cluster_status()
        gate_moved = (model.expert_weights.weight - _seeded_gate("gated", case.dims.embed).weight).abs()
        assert float((flat.param - start).abs().max()) > 3e-5 and float(gate_moved.detach().max()) > 0.0  # the gate is in the flat step
        results[run] = (losses, flat.param.clone(), tables)
    keys = list(results["eager"][0][0])
    assert list(results["graph"][0][0]) == keys
    for k in keys:
        got, want = [s[k] for s in results["graph"][0]], [s[k] for s in results["eager"][0]]
        print(name, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    diff = (results["graph"][1] - results["eager"][1]).abs()  # (the parameter criterion of that test: absolute, biases start at zero)
    print(name, "param diff max", float(diff.max()), "mean", float(diff.mean()))
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))
    for i in range(3):
        got, want = results["graph"][2][i], results["eager"][2][i]
        assert torch.equal(got == 0, want == 0) and not torch.equal(want, ExpertWeights.table(None, scan.modality_codes(masks[i])))
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=0, err_msg=f"weights_timeseries of step {i}")


# 5. sharding -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_weighted_loss_is_exact_under_row_sharding(name: str) -> None:
    """The gate is per frame: two half batches, each with its rows of the global-row noise, give the full batch's loss terms
    (``rtol = 1e-5``, as ``test_dropout_loss_is_exact_under_data_parallel_sharding``) and its reported weights."""
    case, model, batch, _ = _setup(name)
    B, T = case.batch, case.steps
    model.expert_weights = _seeded_gate("gated", case.dims.embed)
    full_noise = GlobalRowNoise(17, 1, 0, DEV).draw(model.noise_shapes(B, T))
    with torch.no_grad():
        ref = {k: float(v) for k, v in model.shared_step(batch, full_noise).items()}
        table = model.weights_timeseries.clone()
        halves = []
        for r in range(2):
            h = slice(r * B // 2, (r + 1) * B // 2)
            noise = GlobalRowNoise(17, 2, r, DEV).draw(model.noise_shapes(B // 2, T))
            halves.append({k: float(v) for k, v in model.shared_step(tuple(x[h] for x in batch), noise).items()})
            np.testing.assert_allclose(model.weights_timeseries.cpu().numpy(), table[h].cpu().numpy(), rtol=1e-5, atol=0)
    for k, want in ref.items():
        mean = 0.5 * (halves[0][k] + halves[1][k])
        print(f"{k}: one rank {want:.8g} rank-mean {mean:.8g}")
        np.testing.assert_allclose(mean, want, rtol=1e-5, err_msg=k)


# 6. skill steps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_skill_step_repeats_the_gate_of_a_row_for_its_copies(name: str) -> None:
    case, model, batch, noise = _setup(name)
    B, T, S, Q = case.batch, case.steps, 2, 3
    skill = ForecastSkill(Q, samples=S)
    g = torch.Generator().manual_seed(5)
    noise = {k: v for k, v in noise.items() if "init" in k or "post" in k}  # (no prior sample in a skill step)
    noise.update({k: torch.rand(v, generator=g).to(DEV) for k, v in skill.noise_shapes(model, B, T).items() if "tail" in k})
    plain = model.forecast_skill(batch, skill, noise)
    model.expert_weights = _seeded_gate("gated", case.dims.embed)
    table = model.forecast_skill(batch, skill, noise, keep_states=True)
    for k, x in _fields(table.states).items():
        x = x.reshape(B, S, T, -1)
        assert torch.equal(x[:, 1, :Q], x[:, 0, :Q]), k  # the copies share their context trajectory bit for bit
    assert tuple(model.weights_timeseries.shape) == (B * S, T, 3)
    assert torch.equal(model.weights_timeseries[0::S], model.weights_timeseries[1::S])
    assert not bool(model.weights_timeseries[:, Q:].any())  # nothing is observed past the context
    assert not torch.equal(table.buffer, plain.buffer)
    # the same step from explicit per-row weights, repeated by hand, on the model without its gate.  (The gate's GEMM splits its
    # reduction over workgroups, so a second evaluation of it need not be bitwise the first: the tables are compared with the skill
    # tables' own tolerance, the samples of the context -- far from their CDF edges or not -- are not compared.)
    with torch.no_grad():
        conv.begin_step(torch.device(DEV))
        lw = model.expert_weights(*model._encode_both(batch[1], batch[2]))  # noqa: SLF001
    gate, model.expert_weights = model.expert_weights, None
    by_hand = model.forecast_skill(batch, skill, noise, expert_log_weights=lw.repeat_interleave(S, dim=0))
    per_row = model.forecast_skill(batch, skill, noise, expert_log_weights=lw)  # [B, T, 3]: repeated by the step itself
    model.expert_weights = gate
    np.testing.assert_allclose(by_hand.buffer.cpu().numpy(), table.buffer.cpu().numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(per_row.buffer.cpu().numpy(), table.buffer.cpu().numpy(), rtol=2e-5, atol=0)


# 7. a modality that is absent everywhere ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_absent_modality_runs_no_gate(name: str) -> None:
    case, model, batch, noise = _setup(name)
    with torch.no_grad():
        want = _rollout(model, batch, noise, observations=(batch[1], None))
    model.expert_weights = _seeded_gate("gated", case.dims.embed)
    calls = []
    model.expert_weights.register_forward_hook(lambda *_: calls.append(1))
    got = _rollout(model, batch, noise, observations=(batch[1], None))
    _assert_same_bits(got, want, "audio only")
    assert not calls
    table = model.weights_timeseries
    assert torch.equal(table, torch.tensor([1.0, 0.0, 0.0], device=DEV).expand(case.batch, case.steps, 3))
    post = got[0]
    (post.kl_per_step.sum() + (post.stoch if case.kind == "mrssm" else post.stoch_l).sum()).backward()
    for p in model.expert_weights.parameters():
        assert p.grad is None or float(p.grad.abs().max()) == 0.0
    # with both observed the same model does run it
    with torch.no_grad():
        _rollout(model, batch, noise)
    assert calls


# validation logging ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_validation_step_logs_the_mean_weights(name: str) -> None:
    case, model, batch, _ = _setup(name)
    with torch.no_grad():
        assert not any(k.startswith("val/weights/") for k in model.validation_step(batch))
        model.expert_weights = _seeded_gate("static", case.dims.embed)
        logged = model.validation_step(batch)
    want = torch.softmax(model.expert_weights.logits.detach(), dim=-1)
    for i, k in enumerate(("audio", "vision", "fused")):
        np.testing.assert_allclose(float(logged[f"val/weights/{k}"]), float(want[i]), rtol=1e-5)
