"""GPU (MI355X): the ELBO schedule -- KL free bits, beta warm-up and modality weights in the scalar epilogue.

What is pinned here: the kernel pair is the torch rule (``beta`` and both gradient planes bit for bit, the summed scalars to the loss
tolerance against the rule in float64); the neutral schedule is the existing epilogue kernels bit for bit; a scheduled step is the
oracle's step with the rule applied to its per-step KLs, plain, with lengths and with a forecast; the loss is exact under data-parallel
sharding; the captured step is the eager one over a warm-up, with the closed-form ``beta`` on every replay; ``FlatAdamW``'s state dict
resumes the schedule.  Tolerances are the project's: loss terms 2e-5 relative, every gradient 2e-4 of its
tensor's largest entry; captured against eager: losses rtol 1e-4, parameters max 2e-4 / mean 2e-7 at lr 1e-5.  Every free-nats threshold
of a model test is chosen on the CPU from the oracle's own per-step KLs, in the widest gap between neighbouring values: no step sits
near it.  The model tests take their families and sizes from ``tests/test_ragged_step_gpu.py`` (``FAMILIES``, ``B``, ``T``, ``VALID``) and share
its cached oracle runs: that module has B = 3, T = 6, so these tests run at T = 6.
"""

from __future__ import annotations

import functools
import itertools
import math

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import ElboSchedule, Forecast, ModalityDropout, StateCarry, scan
from multimodal_mtrssm_amd.core import _ElboCombine, _ElboCombineCounted, _ElboScheduled
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from oracle.cases import CASES, build_batch, build_model, with_sizes
from tests.test_forecast_gpu import CONTEXTS, HI, LO, _frame_nll, _kl_steps, centres
from tests.test_modality_mask_oracle import oracle_step, screened
from tests.test_ragged_step_gpu import B, FAMILIES, IDS, LOSS_KEYS, VALID, T, _check_grads, _dev, _episode_batch, _model, _padded, _reference, _rows, _train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32

WEIGHTS, BETA_START, WARMUP, STEP = (0.5, 2.0), 0.5, 4, 2  # the model tests' schedule: beta = 0.5 + 0.5 * 2 / 4 = 0.75
BETA = 0.75


def below(x: float) -> float:
    return float(torch.nextafter(torch.tensor(x, dtype=F32), torch.tensor(-math.inf)))


def closed_form_beta(start: float, warmup: int, k: int) -> torch.Tensor:
    f = lambda x: torch.tensor(float(x), dtype=F32)  # noqa: E731
    return f(start) + (f(1.0) - f(start)) * torch.clamp(f(k) / f(warmup), max=1.0)


# 1. the kernel is the rule -----------------------------------------------------------------------------------------------------------
def _planes(n: int, free: float, free_h: float, mode: str) -> dict[str, torch.Tensor | None]:
    """Two KL planes in [0, 2) with planted entries -- exactly at the threshold (index 0), one ulp below it (index 1), a dead step far
    above it (index 2) -- and a live plane with its count (``counted``), an all-dead plane with count 0 (``count0``) or none."""
    g = torch.Generator().manual_seed(n)
    kl0, kl1 = torch.rand(n, generator=g) * 2.0, torch.rand(n, generator=g) * 2.0
    live = count = None
    if mode != "plain":
        live = (torch.rand(n, generator=g) < 0.7).float()
    for plane, thr in ((kl0, free), (kl1, free_h)):
        plane[0] = thr
        if n > 1:
            plane[1] = below(thr)
        if n > 2:  # noqa: PLR2004
            plane[2] = 7.0
    if mode == "counted":
        live[:2] = 1.0
        if n > 2:  # noqa: PLR2004
            live[2] = 0.0
        count = live.sum()
    if mode == "count0":
        live.zero_()
        count = torch.zeros(())
    return {"kl0": kl0, "kl1": kl1, "live": live, "count": count}


def _rule64(p: dict, s: ElboSchedule, c0: float, c1: float, nll: tuple[float, float], step: float | None, two: bool) -> dict[str, float]:  # noqa: FBT001
    """The rule in float64 on the fp32 inputs."""
    f = lambda x: float(torch.tensor(x, dtype=F32))  # noqa: E731  (the fp32 value the kernel is handed)
    on = np.ones(p["kl0"].numel(), bool) if p["live"] is None else p["live"].numpy() != 0
    cnt = float(on.size) if p["live"] is None else float(p["count"])
    beta = 1.0 if s.warmup_steps == 0 else f(s.beta_start) + (1.0 - f(s.beta_start)) * min(step / s.warmup_steps, 1.0)
    out = {"recon": f(s.recon_weights[0]) * f(nll[0]) + f(s.recon_weights[1]) * f(nll[1]), "beta": beta}
    for j, (key, free, c) in enumerate((("kl0", s.free_nats, c0), ("kl1", s.free_nats_h, c1))):
        kl = p[key].double().numpy()
        if (j == 1 and not two) or cnt <= 0:
            out[f"k{j}"] = out[f"raw{j}"] = out[f"active{j}"] = 0.0
            continue
        low = p[key].numpy() < np.float32(free)
        out[f"k{j}"] = np.where(low, f(free), kl)[on].sum() / cnt * f(c) * beta
        out[f"raw{j}"] = kl[on].sum() / cnt * f(c)
        out[f"active{j}"] = float((on & ~low).sum()) / cnt
    out["loss"] = out["recon"] + out["k0"] + out["k1"]
    return out


SCHEDULES = [(0, None), (5, 0), (5, 2), (5, 5), (5, 9)]  # (warmup_steps, step): no warm-up with a NULL step, then along the ramp and past it


@pytest.mark.parametrize("mode", ["plain", "counted", "count0"])
@pytest.mark.parametrize("n", [1, 15, 256, 257, 3200])  # one thread, under one wave, exactly one block, one past it, the bench's 64 x 50
def test_kernel_equals_the_rule(n: int, mode: str) -> None:
    c0, c1, nll = 0.8, 0.8 * 0.3, (1234.567, 4321.125)
    for two, free, (warmup, step), weights in itertools.product((False, True), (0.0, 0.7), SCHEDULES, ((1.0, 1.0), (0.25, 3.0))):
        free_h = 0.0 if free == 0.0 else 0.4
        s = ElboSchedule(free, free_h, beta_start=0.25, warmup_steps=warmup, recon_weights=weights)
        p = _planes(n, free, free_h, mode)
        what = (n, mode, two, free, warmup, step, weights)
        runs = {}
        for where in ("cpu", DEV):
            on = lambda x: None if x is None else x.detach().clone().to(where)  # noqa: E731, B023
            a, v = (torch.tensor(x, dtype=F32, device=where, requires_grad=True) for x in nll)
            kl0 = on(p["kl0"]).requires_grad_()
            kl1 = on(p["kl1"]).requires_grad_() if two else None
            step_t = None if step is None else torch.tensor([float(step)], dtype=F32, device=where)
            if where == "cpu":
                t = s.reference(a, v, kl0, c0, kl1, c1, on(p["live"]), on(p["count"]), step_t)
                recon, k0, k1, loss, beta, stats = t.recon, t.k0, t.k1, t.loss, t.beta, torch.stack([t.raw0, t.raw1, t.active0, t.active1])
            else:
                recon, k0, k1, loss, beta, stats = _ElboScheduled.apply(a, v, kl0, kl1, on(p["live"]), on(p["count"]), step_t, s, c0, c1)
            assert not beta.requires_grad and not stats.requires_grad
            (1.5 * loss + 0.5 * k0 + 2.0 * recon + (0.25 * k1 if two else 0.0)).backward()  # every upstream gradient is in play
            runs[where] = {"scalars": [float(x.detach()) for x in (recon, k0, k1, loss)], "beta": beta.detach().cpu(), "stats": stats.detach().cpu().tolist(),
                           "grads": [x.grad.cpu() for x in (a, v, kl0, *([kl1] if two else []))]}
        torch.cuda.synchronize()
        cpu, gpu = runs["cpu"], runs[DEV]
        assert torch.equal(gpu["beta"].reshape(()), cpu["beta"].reshape(())), what
        if warmup:
            assert torch.equal(gpu["beta"].reshape(()), closed_form_beta(0.25, warmup, step)), what
        for got, want in zip(gpu["grads"], cpu["grads"], strict=True):  # g_nll_a, g_nll_v and the planes: bit for bit
            assert torch.equal(got, want), what
        want = _rule64(p, s, c0, c1, nll, step, two)
        for k, got in zip(("recon", "k0", "k1", "loss"), gpu["scalars"], strict=True):
            np.testing.assert_allclose(got, want[k], rtol=2e-5, atol=0, err_msg=f"{k} {what}")
        for k, got in zip(("raw0", "raw1", "active0", "active1"), gpu["stats"], strict=True):
            np.testing.assert_allclose(got, want[k], rtol=2e-5, atol=0, err_msg=f"{k} {what}")
        # the planted entries: the tie passes, one ulp below does not, the dead step above the threshold gets an explicit zero
        g0 = gpu["grads"][2]
        if mode == "count0":
            assert not bool(g0.any()) and gpu["scalars"][1] == 0.0, what
        else:
            assert float(g0[0]) > 0.0, what
            assert n < 2 or float(g0[1]) == 0.0, what  # noqa: PLR2004
            assert n < 3 or (float(g0[2]) == 0.0) == (mode == "counted"), what  # noqa: PLR2004


# 2. the neutral schedule is the existing kernels, bit for bit ----------------------------------------------------------------------------
@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
@pytest.mark.parametrize("two", [False, True], ids=["kl", "kl+kl_h"])
@pytest.mark.parametrize("n", [257, 3200])
def test_neutral_schedule_is_the_existing_epilogue_bitwise(n: int, two: bool, counted: bool) -> None:  # noqa: FBT001
    g = torch.Generator().manual_seed(n + 1)
    base0, base1 = torch.rand(n, generator=g) * 3.0, torch.rand(n, generator=g) * 0.5
    live = (torch.rand(n, generator=g) < 0.7).float().to(DEV)
    count = live.sum() / 2.0  # (what a rank of two is handed)
    c0, c1 = 0.8, 0.8 * 0.3
    runs = []
    for scheduled in (False, True):
        a, v = (torch.tensor(x, dtype=F32, device=DEV, requires_grad=True) for x in (1234.567, 4321.125))
        kl0 = base0.to(DEV).reshape(1, n).requires_grad_()
        kl1 = base1.to(DEV).reshape(1, n).requires_grad_() if two else None
        if scheduled:
            out = _ElboScheduled.apply(a, v, kl0, kl1, live if counted else None, count if counted else None, None, ElboSchedule(), c0, c1)[:4]
        elif counted:
            out = _ElboCombineCounted.apply(a, v, kl0, kl1, live, count, c0, c1)
        else:
            out = _ElboCombine.apply(a, v, kl0, kl1, c0, c1)
        (1.5 * out[3] + 0.5 * out[1] + 2.0 * out[0] + (0.25 * out[2] if two else 0.0)).backward()
        keep = (0, 1, 2, 3) if two else (0, 1, 3)  # (without kl1 the existing kernels leave their third scalar unwritten)
        runs.append(([out[i].detach().clone() for i in keep], [x.grad.clone() for x in (a, v, kl0, *([kl1] if two else []))]))
    torch.cuda.synchronize()
    for got, want in zip(runs[1][0] + runs[1][1], runs[0][0] + runs[0][1], strict=True):
        assert torch.equal(got, want), (got, want)
    assert float(runs[0][0][1]) > 0.0 and bool(runs[0][1][2].any())


# 3. the step is the oracle's step under the rule ------------------------------------------------------------------------------------------
def _threshold(values: np.ndarray, what: str) -> float:
    """The midpoint of the widest gap between neighbouring sorted per-step KLs of the live steps.  The test FAILS unless a live step
    lies on each side and the gap exceeds 1e-3 relative (every step then stays clear of the threshold at the 1e-5 posterior tolerance)."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    assert v.size >= 2, f"{what}: fewer than two live steps"  # noqa: PLR2004
    gaps = np.diff(v)
    i = int(gaps.argmax())
    mid = 0.5 * (v[i] + v[i + 1])
    assert (v < mid).any() and (v > mid).any(), f"{what}: no live step on each side of {mid}"
    assert gaps[i] > 1e-3 * mid, f"{what}: the widest gap {gaps[i]} around {mid} is below 1e-3 relative"
    return float(mid)


def _rule_of(variant: str):  # noqa: ANN202
    """What the step observes, as ``Forecast.reference`` states it: codes, the frames reconstructed, the steps whose KL counts."""
    if variant == "plain":
        return Forecast(T).reference(torch.zeros(B), T), None
    if variant == "lengths":
        lens = torch.tensor(VALID, dtype=torch.int32)
        return Forecast(T).reference(torch.zeros(B), T, lens), lens  # (a context of T frames: codes 3 on every live step)
    return Forecast((LO, HI)).reference(centres(CONTEXTS), T), None


@functools.lru_cache(maxsize=None)
def _scheduled_reference(name: str, variant: str) -> dict:
    """Computed once per model and variant and shared: the oracle's rollout under the variant's codes, the thresholds chosen from its
    per-step KLs, the loss terms under the rule and their gradients."""
    case = with_sizes(CASES[name], B, T)
    d = case.dims
    oracle = build_model(case)
    batch = build_batch(case)
    rule, lens = _rule_of(variant)
    if lens is not None:
        batch = _padded(batch, VALID)
    noise, margin = screened(case, oracle, batch, rule.codes.long())
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
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
    out["recon"] = WEIGHTS[0] * out["recon/audio"] + WEIGHTS[1] * out["recon/vision"]
    out["loss"] = out["recon"]
    free, active = {}, {}
    for key, (steps, coeff) in kls.items():
        free[key] = _threshold(steps.detach()[rule.observed].numpy(), f"{name} {variant} {key}")
        thr = torch.tensor(free[key], dtype=F32)
        out[key] = (torch.where(steps < thr, thr, steps) * observed).sum() / rule.counts[1] * coeff * BETA
        out[f"{key}_raw"] = (steps.detach() * observed).sum() / rule.counts[1] * coeff
        active[key] = float(((steps.detach() >= thr) & rule.observed).sum() / rule.counts[1])
        out["loss"] = out["loss"] + out[key]
    oracle.zero_grad(set_to_none=True)
    out["loss"].backward()
    grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "rule": rule, "lens": lens, "free": free, "active": active,
            "terms": {k: float(v.detach()) for k, v in out.items()}, "grads": grads}


def _schedule(free: dict[str, float], step: int = STEP) -> ElboSchedule:
    return ElboSchedule(free["kl"], free.get("kl_h", 0.0), beta_start=BETA_START, warmup_steps=WARMUP, recon_weights=WEIGHTS).set_step(step, DEV)


@pytest.mark.parametrize("variant", ["plain", "lengths", "forecast"])
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_scheduled_step_is_the_oracles_step_under_the_rule(name: str, onecu: bool, variant: str) -> None:  # noqa: FBT001
    ref = _scheduled_reference(name, variant)
    case = ref["case"]
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _dev(ref["batch"], ref["noise"])
    kw = {}
    if variant == "lengths":
        kw["lengths"] = ref["lens"].to(DEV)
    if variant == "forecast":
        kw["forecast"] = Forecast((LO, HI))
        noise["u_context"] = centres(CONTEXTS).to(DEV)
    s = _schedule(ref["free"])
    out, grads = _train(model, batch, noise, elbo_schedule=s, **kw)
    raw = ("kl_raw",) if case.kind == "mrssm" else ("kl_raw", "kl_h_raw")
    assert list(out) == [k for k in ("recon", "recon/audio", "recon/vision", "kl", "kl_h", "loss") if k in LOSS_KEYS[case.kind]] + list(raw)
    assert set(out) == set(ref["terms"])
    for k, want in ref["terms"].items():
        print(name, onecu, variant, k, float(out[k]), want)
        np.testing.assert_allclose(float(out[k]), want, rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(float(out["loss"]), float(out["recon"]) + sum(float(out[k]) for k in ("kl", "kl_h") if k in out), rtol=1e-6)
    _check_grads(grads, ref["grads"], least=39)
    assert float(s.stats["beta"]) == BETA
    for key, stat in (("kl", "active"), ("kl_h", "active_h")):
        if key in ref["active"]:
            assert 0.0 < ref["active"][key] < 1.0
            np.testing.assert_allclose(float(s.stats[stat]), ref["active"][key], rtol=1e-6, err_msg=stat)  # (a step on each side, counted alike)
    assert float(out["kl"]) != float(out["kl_raw"])


# 4. data parallel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_scheduled_loss_is_exact_under_data_parallel_sharding(name: str, onecu: bool) -> None:  # noqa: FBT001
    lens = [6, 1, 3, 5]
    ref = _reference(name, tuple(lens))
    d = ref["case"].dims
    levels = {"kl": ("", d.cats, d.classes)} if ref["case"].kind == "mrssm" else {"kl": ("_l", d.ls_cats, d.ls_classes), "kl_h": ("_h", d.hs_cats, d.hs_classes)}
    free = {}
    for key, (sfx, cats, classes) in levels.items():  # the oracle's per-step KLs of every row's live steps
        steps = [_kl_steps(r[f"_post_logits{sfx}"], r[f"_prior_logits{sfx}"], cats, classes, d.use_kl_balancing).reshape(-1) for r in ref["rows"]]
        free[key] = _threshold(torch.cat(steps).numpy(), f"{name} {key}")
    model = _model(name, onecu, ref["oracle"], (4, T))
    batch, noise = _dev(_padded(ref["batch"], lens), ref["noise"])
    s = _schedule(free)
    one, g_one = _train(model, _episode_batch(batch, lens, lens, 0), noise, elbo_schedule=s)
    active = float(s.stats["active"])
    assert 0.0 < active < 1.0
    halves, actives = [], []
    for r in range(2):
        rows = slice(2 * r, 2 * r + 2)
        sub, sub_noise = _rows(batch, noise, rows, T)
        halves.append(_train(model, _episode_batch(sub, lens[rows], lens, 2 * r), sub_noise, elbo_schedule=s))
        actives.append(float(s.stats["active"]))
    assert float(halves[0][0]["loss"]) != float(halves[1][0]["loss"])
    for k in one:
        np.testing.assert_allclose(0.5 * (float(halves[0][0][k]) + float(halves[1][0][k])), float(one[k]), rtol=2e-5, err_msg=k)
    np.testing.assert_allclose(0.5 * sum(actives), active, rtol=1e-6)  # the clipping decisions are the same on any rank count
    mean = {k: 0.5 * (halves[0][1].get(k, 0) + halves[1][1].get(k, 0)) for k in g_one}  # the all-reduced sum scaled by 1 / world
    _check_grads(mean, g_one)


# 5. captured ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_captured_scheduled_step_matches_eager_over_the_warm_up(name: str) -> None:
    ref = _reference(name)
    oracle = ref["oracle"]
    first = _dev(ref["batch"], {})[0]
    batches = [first, tuple(x.flip(0).contiguous() for x in first)] * 3
    sref = _scheduled_reference(name, "plain")
    want_beta = [float(closed_form_beta(0.25, 3, k)) for k in range(6)]
    assert want_beta[0] == 0.25 and want_beta[3:] == [1.0, 1.0, 1.0]  # noqa: PLR2004
    results = {}
    for mode in ("eager", "graph"):
        model = _model(name, False, oracle)
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(B, T)
        s = ElboSchedule(sref["free"]["kl"], sref["free"].get("kl_h", 0.0), beta_start=0.25, warmup_steps=3, recon_weights=WEIGHTS)
        losses, betas = [], []
        if mode == "eager":
            s.bind(opt)
            for eb in batches:
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(eb, noise, elbo_schedule=s)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v.detach()) for k, v in out.items()})
                betas.append(float(s.stats["beta"]))
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, batches[0], source, warmup=2, elbo_schedule=s)
            assert float(opt.state[1]) == 0.0 and opt.steps == 0  # (the construction's warm-up steps are put back)
            for eb in batches:
                losses.append({k: float(v) for k, v in cap.step(eb).items()})
                betas.append(float(s.stats["beta"]))
            assert float(opt.state[1]) == 6.0 and opt.steps == 6  # noqa: PLR2004
            cap.close()
            assert s.stats == {}  # (they were tensors of the graph's memory)
        scan.check_cluster_status()
        assert betas == want_beta, (mode, betas)
        results[mode] = (losses, flat.param.clone())
    assert "kl_raw" in results["graph"][0][0]
    for k in results["eager"][0][0]:
        got, want = [x[k] for x in results["graph"][0]], [x[k] for x in results["eager"][0]]
        print(name, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))  # noqa: PLR2004


# 6. resume, and the model's surface -----------------------------------------------------------------------------------------------------------
def test_optimizer_state_dict_resumes_the_schedule() -> None:
    ref = _reference("mrssm_default")
    model = _model("mrssm_default", False, ref["oracle"])
    flat = FlatParameters(model, extra=8)
    opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
    batch = _dev(ref["batch"], {})[0]
    model.elbo_schedule = ElboSchedule(free_nats=0.5, beta_start=0.25, warmup_steps=5).bind(opt)
    betas = []
    for _ in range(2):
        opt.zero_grad()
        out = model.training_step(batch)
        out["loss"].backward()
        opt.step()
        betas.append(float(model.elbo_schedule.stats["beta"]))
    assert list(out) == ["loss", "train/loss", "train/recon", "train/recon/audio", "train/recon/vision", "train/kl", "train/kl_raw"]
    state = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state_dict().items()}
    fresh = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    assert float(fresh.state[1]) == 0.0
    fresh.load_state_dict(state)
    model.elbo_schedule.bind(fresh)
    val = model.validation_step(batch)  # never scheduled: the plain keys, the plain ELBO
    assert set(val) == {f"val/{k}" for k in LOSS_KEYS["mrssm"]}
    np.testing.assert_allclose(float(val["val/loss"]), float(val["val/recon"]) + float(val["val/kl"]), rtol=1e-6)
    fresh.zero_grad()
    model.training_step(batch)["loss"].backward()
    betas.append(float(model.elbo_schedule.stats["beta"]))
    assert betas == [float(closed_form_beta(0.25, 5, k)) for k in range(3)]


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_schedule_combines_with_mask_dropout_and_carry(name: str) -> None:
    """Only the epilogue changes: a modality mask (the uncounted kernel path behind a StepMask) and dropout with a carry run under the
    schedule, and ``loss = recon + kl (+ kl_h)`` with ``recon`` the weighted sum holds in each."""
    ref = _reference(name)
    model = _model(name, False, ref["oracle"])
    batch, noise = _dev(ref["batch"], ref["noise"])
    s = ElboSchedule(free_nats=0.5, free_nats_h=0.2, beta_start=0.0, warmup_steps=4, recon_weights=WEIGHTS).set_step(1, DEV)
    mask = torch.ones(B, T, 2, dtype=torch.bool, device=DEV)
    mask[:, 1:, 0] = False
    carry = StateCarry.for_model(model, B)
    runs = [model.shared_step(batch, noise, modality_mask=mask, elbo_schedule=s),
            model.shared_step(batch, noise, modality_dropout=ModalityDropout(0.3, 0.3, span=2), state_carry=carry, reset=torch.ones(B, dtype=torch.bool),
                              elbo_schedule=s)]
    for out in runs:
        np.testing.assert_allclose(float(out["recon"]), WEIGHTS[0] * float(out["recon/audio"]) + WEIGHTS[1] * float(out["recon/vision"]), rtol=1e-6)
        np.testing.assert_allclose(float(out["loss"]), float(out["recon"]) + sum(float(out[k]) for k in ("kl", "kl_h") if k in out), rtol=1e-6)
        assert float(s.stats["beta"]) == 0.25 and math.isfinite(float(out["loss"])) and float(out["kl_raw"]) > 0.0  # noqa: PLR2004
    runs[1]["loss"].backward()
    torch.cuda.synchronize()
