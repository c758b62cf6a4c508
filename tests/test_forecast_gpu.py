"""GPU (MI355X): the forecast objective, end to end.

What is pinned here: the sampler kernel is its torch rule bit for bit; a forecast step is the oracle's masked step under the forecast
codes with both modalities reconstructed on every live frame and the KL taken over the observed steps; the open-loop tail is the
reference's ``rollout_transition`` from the last observed posterior; contexts that reach every row's end change nothing; the loss is
exact under data-parallel sharding; the captured step is the eager one.  Tolerances are the project's: loss
terms 2e-5 relative, posterior probabilities and deter 1e-5, samples exact, every gradient 2e-4 of its tensor's largest entry;
captured against eager: losses rtol 1e-4, parameters max 2e-4 / mean 2e-7 at lr 1e-5.  Noise is screened on the CPU under the codes
of the run it feeds (margin 1e-4), so that no draw sits at a CDF edge.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import Forecast, ModalityDropout, StateCarry, scan
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from oracle.cases import CASES, build_batch, build_model, with_sizes
from oracle.ref_model import KL_BALANCE_ALPHA, cat_probs, kl_cat
from tests.test_modality_mask_oracle import oracle_step, screened
from tests.test_ragged_step_gpu import B, FAMILIES, IDS, LOSS_KEYS, VALID, T, _check_grads, _dev, _episode_batch, _model, _np, _padded, _reference, _rows, _train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LO, HI = 1, 6
CONTEXTS = (3, 2, 1)


def centres(contexts: tuple[int, ...] | list[int], lo: int = LO, hi: int = HI) -> torch.Tensor:
    """Uniforms at the centres of the bins that give ``contexts``: ``u = (c - lo + 0.5) / n``."""
    n = hi - lo + 1
    return torch.tensor([(c - lo + 0.5) / n for c in contexts], dtype=torch.float32)


# 1. the kernel is the rule --------------------------------------------------------------------------------------------------------
def _kernel_equals_rule(fc: Forecast, b_global: int, steps: int, world: int, rank: int, *, lengths: bool, md: ModalityDropout | None) -> None:
    g = torch.Generator().manual_seed(b_global + steps)
    u_context = torch.rand(b_global, generator=g)
    u_context[0], u_context[-1] = 0.0, float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))  # the lowest and the top bin
    valid = torch.randint(0, steps + 3, (b_global,), generator=g).to(torch.int32) if lengths else None
    u_mask = None
    if md is not None:
        u_mask = torch.rand(md.noise_shape(b_global, steps), generator=g)
        u_mask[1, 0] = torch.tensor([0.1, 0.2])  # a row that takes the t = 0 fix-up
    want = fc.reference(u_context, steps, valid, u_mask, md)
    on = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    got = fc.sample(on(u_context), steps, on(valid), on(u_mask), md, world=world, rank=rank)
    torch.cuda.synchronize()
    local = b_global // world
    rows = slice(rank * local, (rank + 1) * local)
    assert torch.equal(got.codes.cpu(), want.codes[rows]) and got.codes.dtype == torch.int32
    assert torch.equal(got.mask.cpu(), want.mask[rows])
    assert torch.equal(got.seen_audio.cpu(), want.mask[rows, :, 0].reshape(-1).float())
    assert torch.equal(got.seen_vision.cpu(), want.mask[rows, :, 1].reshape(-1).float())
    assert torch.equal(got.present_audio.cpu(), want.target[rows].reshape(-1).float()) and got.present_vision is got.present_audio
    assert torch.equal(got.live.cpu(), want.observed[rows].reshape(-1).float())
    assert torch.equal(got.mask0.cpu(), want.mask[rows, 0]) and got.mask0.dtype == torch.bool
    assert torch.equal(got.last.cpu(), want.last[rows]) and got.last.dtype == torch.int32
    assert torch.equal(got.counts.cpu(), want.counts)  # the GLOBAL batch's, whatever the slice
    for count, k in ((got.count_audio, 0), (got.count_vision, 0), (got.count_live, 1)):
        assert torch.equal(count.cpu(), want.counts[k] / world)
    assert float(want.counts[1]) < float(want.counts[0])  # (some row runs open loop: u_context[0] = 0 gives the shortest context)


@pytest.mark.parametrize(("world", "rank"), [(1, 0), (5, 3)])
@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("lengths", [False, True], ids=["full", "lengths"])
def test_sampler_kernel_equals_the_rule(lengths: bool, dropout: bool, world: int, rank: int) -> None:  # noqa: FBT001
    md = ModalityDropout(0.4, 0.3, span=2) if dropout else None
    _kernel_equals_rule(Forecast((2, 9)), 5, 7, world, rank, lengths=lengths, md=md)


def test_sampler_kernel_equals_the_rule_past_one_grid() -> None:
    """340 x 50 = 17000 frames, more than 64 workgroups of 256 hold at once: the grid-stride loop and the counts of many workgroups."""
    _kernel_equals_rule(Forecast((10, 50)), 340, 50, 4, 2, lengths=True, md=ModalityDropout(0.2, 0.3, span=3))


# 2. the step is the oracle's masked step, restated -----------------------------------------------------------------------------------
def _kl_steps(q_logits: torch.Tensor, p_logits: torch.Tensor, cats: int, classes: int, balancing: bool) -> torch.Tensor:  # noqa: FBT001
    """``oracle.ref_model.kl_loss`` before its mean: the KL per (b, t)."""
    ql, qp = cat_probs(q_logits, cats, classes)
    pl, _ = cat_probs(p_logits, cats, classes)
    if balancing:
        return KL_BALANCE_ALPHA * kl_cat(ql.detach(), qp.detach(), pl) + (1.0 - KL_BALANCE_ALPHA) * kl_cat(ql, qp, pl.detach())
    return kl_cat(ql, qp, pl)


def _frame_nll(prediction: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    return (0.5 * (target - prediction) ** 2 + 0.5 * math.log(2.0 * math.pi)).flatten(2).sum(-1)


def _forecast_loss(case, oracle, batch, noise, rule) -> dict[str, torch.Tensor]:  # noqa: ANN001
    """The forecast objective from existing pieces: the masked restatement's rollout under the forecast codes, its feature decoded with
    the oracle's decoders, NLL = sum over target frames / live count, KL = sum of the per-step KL over observed steps / observed count."""
    d = case.dims
    roll = oracle_step(case, oracle, batch, noise, rule.codes.long())
    if case.kind == "mrssm":
        feature = torch.cat([roll["_deter"], roll["_post_stoch"]], dim=-1)
        kls = {"kl": (_kl_steps(roll["_post_logits"], roll["_prior_logits"], d.cats, d.classes, d.use_kl_balancing), d.kl_coeff)}
    else:
        feature = torch.cat([roll["_deter_h"], roll["_post_stoch_h"], roll["_deter_l"], roll["_post_stoch_l"]], dim=-1)
        kls = {"kl": (_kl_steps(roll["_post_logits_l"], roll["_prior_logits_l"], d.ls_cats, d.ls_classes, d.use_kl_balancing), d.kl_coeff),
               "kl_h": (_kl_steps(roll["_post_logits_h"], roll["_prior_logits_h"], d.hs_cats, d.hs_classes, d.use_kl_balancing),
                        d.kl_coeff * d.w_kl_h)}
    target, observed = rule.target.float(), rule.observed.float()
    out = {"recon/audio": (_frame_nll(oracle.audio_decoder(feature), batch[4]) * target).sum() / rule.counts[0],
           "recon/vision": (_frame_nll(oracle.vision_decoder(feature), batch[5]) * target).sum() / rule.counts[0]}
    out["recon"] = out["recon/audio"] + out["recon/vision"]
    out["loss"] = out["recon"]
    for key, (steps, coeff) in kls.items():
        assert not bool(steps.detach()[~rule.observed].any()), key  # posterior = prior: the KL is 0 exactly off the context
        out[key] = (steps * observed).sum() / rule.counts[1] * coeff
        out["loss"] = out["loss"] + out[key]
    return out


@functools.lru_cache(maxsize=None)
def _forecast_reference(name: str, valid: tuple[int, ...] | None = VALID, contexts: tuple[int, ...] = CONTEXTS, dropout: bool = False) -> dict:  # noqa: FBT001, FBT002
    """Computed once per model and shared: the rule, the noise screened under its codes, the restated loss terms and their gradients."""
    case = with_sizes(CASES[name], len(contexts), T)
    oracle = build_model(case)
    batch = build_batch(case)
    lens = None if valid is None else torch.tensor(valid, dtype=torch.int32)
    if valid is not None:
        batch = _padded(batch, valid)
    md = u_mask = None
    if dropout:
        md = ModalityDropout(0.4, 0.3, span=2)
        u_mask = torch.rand(md.noise_shape(len(contexts), T), generator=torch.Generator().manual_seed(6))
        u_mask[1, 0] = torch.tensor([0.1, 0.2])  # row 1 takes the t = 0 fix-up (vision)
    u_context = centres(contexts)
    rule = Forecast((LO, HI)).reference(u_context, T, lens, u_mask, md)
    assert rule.context.tolist() == list(contexts)
    noise, margin = screened(case, oracle, batch, rule.codes.long())
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    out = _forecast_loss(case, oracle, batch, noise, rule)
    oracle.zero_grad(set_to_none=True)
    out["loss"].backward()
    grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "rule": rule, "terms": {k: float(v.detach()) for k, v in out.items()},
            "grads": grads, "u_context": u_context, "u_mask": u_mask, "md": md, "lens": lens}


def _forecast_train(model, ref: dict, **kw):  # noqa: ANN001, ANN003, ANN202
    batch, noise = _dev(ref["batch"], ref["noise"])
    noise["u_context"] = ref["u_context"].to(DEV)
    if ref["md"] is not None:
        noise["u_mask"] = ref["u_mask"].to(DEV)
        kw["modality_dropout"] = ref["md"]
    if ref["lens"] is not None:
        kw["lengths"] = ref["lens"].to(DEV)
    return _train(model, batch, noise, forecast=Forecast((LO, HI)), **kw)


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_forecast_step_matches_the_oracle_restatement(name: str, onecu: bool, dropout: bool) -> None:  # noqa: FBT001
    ref = _forecast_reference(name, VALID, CONTEXTS, dropout)
    case, rule = ref["case"], ref["rule"]
    model = _model(name, onecu, ref["oracle"])
    out, grads = _forecast_train(model, ref)
    assert set(out) == set(ref["terms"]) == set(LOSS_KEYS[case.kind])
    for k, want in ref["terms"].items():
        print(name, onecu, dropout, k, float(out[k]), want)
        np.testing.assert_allclose(float(out[k]), want, rtol=2e-5, err_msg=k)
    _check_grads(grads, ref["grads"], least=39)  # (at least 40 tensors compared)
    # the per-step KL is exactly 0 from min(c_b, valid_b) on and non-zero before
    batch, noise = _dev(ref["batch"], ref["noise"])
    mask = rule.mask.to(DEV)
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise, modality_mask=mask[:, 0])
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise, modality_mask=mask)
    kls = [post.kl_per_step] if case.kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]
    for b, (c, n) in enumerate(zip(CONTEXTS, VALID, strict=True)):
        for kl in kls:
            seen = rule.codes[b, : min(c, n)] != 0  # (under dropout a step inside the context may see nothing: KL 0 there as well)
            assert not bool(kl[b, min(c, n):].any()) and bool((kl[b, : min(c, n)].cpu() != 0)[seen].all()) and bool(seen.any()), (b, c, n)


# 3. the tail is the reference's open-loop composition -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_context_noise(name: str, q: int) -> dict:
    """Noise screened under "observe q frames, then nothing" for every row (full-length rows)."""
    ref = _reference(name)
    codes = (torch.arange(T) < q).long().mul(3).expand(B, T).contiguous()
    noise, margin = screened(ref["case"], ref["oracle"], ref["batch"], codes)
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    return noise


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_forecast_rollout_tail_is_rollout_transition_from_the_last_observed_posterior(name: str, onecu: bool) -> None:  # noqa: FBT001
    ref = _reference(name)
    model = _model(name, onecu, ref["oracle"])
    mrssm = ref["case"].kind == "mrssm"
    fields = ("deter", "stoch") if mrssm else ("deter_l", "deter_h", "stoch_l", "stoch_h")
    dists = ("distribution",) if mrssm else ("distribution_l", "distribution_h")
    for q in (*CONTEXTS, T - 1):
        batch, noise = _dev(ref["batch"], _fixed_context_noise(name, q))
        obs = (batch[1], batch[2])
        with torch.no_grad():
            s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
            post, _ = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise)
            tail_noise = {"u_prior": noise["u_post"][:, q:]} if mrssm else {"u_prior_l": noise["u_post_l"][:, q:], "u_prior_h": noise["u_post_h"][:, q:]}
            tail = model.rollout_transition(actions=batch[0][:, q:], prev_state=post[:, q - 1], noise=tail_noise)
        got = model.forecast_rollout(actions=batch[0], observations=obs, context=q, prev_state=s0, noise=noise)
        assert not getattr(got, fields[0]).requires_grad  # (runs under no_grad)
        for want, rows in ((post, slice(0, q)), (tail, slice(q, T))):
            for k in fields:
                a, w = getattr(got, k)[:, rows], getattr(want, k)[:, : rows.stop - rows.start]
                if k.startswith("stoch"):
                    assert torch.equal(a, w), (q, k, rows)
                else:
                    np.testing.assert_allclose(_np(a), _np(w), rtol=0, atol=1e-5, err_msg=f"{k} q {q} {rows}")
            for k in dists:
                a, w = getattr(got, k).probs[:, rows], getattr(want, k).probs[:, : rows.stop - rows.start]
                np.testing.assert_allclose(_np(a), _np(w), rtol=0, atol=1e-5, err_msg=f"{k} q {q} {rows}")
        kls = [got.kl_per_step] if mrssm else [got.kl_per_step, got.kl_h_per_step]
        for kl in kls:
            assert not bool(kl[:, q:].any()) and bool((kl[:, :q] != 0).all())


# 4. contexts that reach every row's end change nothing -------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_contexts_that_reach_the_rows_ends_give_the_closed_loop_step(name: str, onecu: bool) -> None:  # noqa: FBT001
    ref = _reference(name)
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _dev(_padded(ref["batch"], VALID), ref["noise"])
    valid = torch.tensor(VALID, dtype=torch.int32, device=DEV)
    want, want_grads = _train(model, batch, noise, lengths=valid)
    got, grads = _train(model, batch, {**noise, "u_context": centres((6, 5, 1)).to(DEV)}, lengths=valid, forecast=Forecast((LO, HI)))
    assert set(got) == set(want)
    for k in want:
        np.testing.assert_allclose(float(got[k]), float(want[k]), rtol=2e-5, err_msg=k)
    _check_grads(grads, want_grads)
    # without lengths, a context of T frames is the plain step
    full, noise = _dev(ref["batch"], ref["noise"])
    want, want_grads = _train(model, full, noise)
    got, grads = _train(model, full, noise, forecast=Forecast(T))
    for k in want:
        np.testing.assert_allclose(float(got[k]), float(want[k]), rtol=2e-5, err_msg=k)
    _check_grads(grads, want_grads)


# 5. data parallel --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_forecast_loss_is_exact_under_data_parallel_sharding(name: str, onecu: bool) -> None:  # noqa: FBT001
    lens, contexts = [6, 1, 3, 5], (2, 4, 1, 3)
    ref = _forecast_reference(name, tuple(lens), contexts)
    model = _model(name, onecu, ref["oracle"], (4, T))
    batch, noise = _dev(ref["batch"], ref["noise"])
    u_context = ref["u_context"].to(DEV)
    fc = Forecast((LO, HI))
    one, g_one = _train(model, _episode_batch(batch, lens, lens, 0), {**noise, "u_context": u_context}, forecast=fc)
    for k, want in ref["terms"].items():  # (and the one-rank step is the restatement's)
        np.testing.assert_allclose(float(one[k]), want, rtol=2e-5, err_msg=k)
    halves = []
    for r in range(2):
        rows = slice(2 * r, 2 * r + 2)
        sub, sub_noise = _rows(batch, noise, rows, T)
        halves.append(_train(model, _episode_batch(sub, lens[rows], lens, 2 * r), {**sub_noise, "u_context": u_context}, forecast=fc.for_rank(2, r)))
    assert float(halves[0][0]["loss"]) != float(halves[1][0]["loss"])
    for k in one:
        np.testing.assert_allclose(0.5 * (float(halves[0][0][k]) + float(halves[1][0][k])), float(one[k]), rtol=2e-5, err_msg=k)
    mean = {k: 0.5 * (halves[0][1].get(k, 0) + halves[1][1].get(k, 0)) for k in g_one}  # the all-reduced sum scaled by 1 / world
    _check_grads(mean, g_one)
    with pytest.raises(ValueError, match="bound to rank"):
        model.shared_step(_episode_batch(_rows(batch, noise, slice(0, 2), T)[0], lens[:2], lens, 0), {**noise, "u_context": u_context},
                          forecast=fc.for_rank(2, 1))


# 6. captured --------------------------------------------------------------------------------------------------------------------------
CAPTURED = [(n, f, False) for n, f in FAMILIES] + [("mrssm_default", False, True), ("mmtrssm_default", False, True)]


@pytest.mark.parametrize(("name", "onecu", "ragged"), CAPTURED, ids=[*IDS, "mrssm_default-ragged-dropout", "mmtrssm_default-ragged-dropout"])
def test_captured_forecast_step_matches_eager(name: str, onecu: bool, ragged: bool) -> None:  # noqa: FBT001
    """``forecast=`` alone on plain batches, and with ``ragged=True`` and ``modality_dropout=`` in ONE graph, against the eager steps on the
    same uniforms."""
    ref = _reference(name)
    oracle = ref["oracle"]
    fc = Forecast((LO, HI))
    md = ModalityDropout(0.3, 0.3, span=2) if ragged else None
    if ragged:
        valids = [[6, 4, 1], [2, 6, 5]]
        batches = [_episode_batch(_dev(_padded(ref["batch"], v), {})[0], v, v, 0) for v in valids]
    else:
        first = _dev(ref["batch"], {})[0]
        batches = [first, tuple(x.flip(0).contiguous() for x in first)]
    results = {}
    for mode in ("eager", "graph"):
        model = _model(name, onecu, oracle)
        model.forecast, model.modality_dropout = fc, md  # (noise_shapes gains "u_context" and "u_mask")
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(B, T)
        assert "u_context" in shapes and ("u_mask" in shapes) == ragged
        losses = []
        if mode == "eager":
            for eb in batches:
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(eb, noise, forecast=fc, modality_dropout=md)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v.detach()) for k, v in out.items()})
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, batches[0], source, warmup=2, forecast=fc, ragged=ragged, modality_dropout=md)
            for eb in batches:
                losses.append({k: float(v) for k, v in cap.step(eb).items()})
            assert float(opt.state[1]) == 2.0 and opt.steps == 2  # noqa: PLR2004
            assert tuple(cap.uniforms["u_context"].shape) == (B,)
            cap.close()
        scan.check_cluster_status()
        results[mode] = (losses, flat.param.clone())
    for k in results["eager"][0][0]:
        got, want = [s[k] for s in results["graph"][0]], [s[k] for s in results["eager"][0]]
        print(name, onecu, ragged, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    assert results["eager"][0][0]["kl"] != results["eager"][0][1]["kl"]  # the replay read the second batch and fresh contexts
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))  # noqa: PLR2004


# 7. refusals and the model's train / validation surface ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_refusals_and_the_train_and_validation_steps(name: str) -> None:
    ref = _reference(name)
    model = _model(name, False, ref["oracle"])
    batch, noise = _dev(ref["batch"], ref["noise"])
    mask = torch.ones(B, T, 2, dtype=torch.bool, device=DEV)
    fc = Forecast((LO, HI))
    with pytest.raises(ValueError, match="already says what is seen"):
        model.shared_step(batch, noise, modality_mask=mask, forecast=fc)
    with pytest.raises(ValueError, match="already says what is seen"):
        model.shared_step((*batch, mask), noise, forecast=fc)
    with pytest.raises(ValueError, match="open-loop state"):
        model.shared_step(batch, noise, forecast=fc, state_carry=StateCarry.for_model(model, B), reset=torch.ones(B, dtype=torch.bool))
    with pytest.raises(ValueError, match="masked=True"):  # (refused before anything is built or launched)
        CapturedTrainStep(model, None, None, None, (*batch, mask), None, forecast=fc, masked=True)
    # validation_step: the val/* of before, and val/forecast/* of a second step at the fixed context
    plain = model.validation_step(batch)
    model.val_forecast = Forecast(2)
    both = model.validation_step(batch)
    keys = LOSS_KEYS[ref["case"].kind]
    assert set(plain) == {f"val/{k}" for k in keys} and set(both) == set(plain) | {f"val/forecast/{k}" for k in keys}
    assert all(bool(torch.isfinite(v)) for v in both.values()) and float(both["val/forecast/kl"].detach()) > 0.0
    # training_step with model.forecast: contexts drawn on the device, a finite loss with gradients
    model.forecast = fc
    model.zero_grad(set_to_none=True)
    out = model.training_step(batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"])) and set(out) == {"loss"} | {f"train/{k}" for k in keys}
    assert sum(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in model.parameters()) > 40  # noqa: PLR2004
