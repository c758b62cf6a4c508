"""GPU: latent overshooting.

1. the four kernels alone against the float64 rule (``LatentOvershoot.reference`` / ``gather_reference`` / ``scatter_reference``);
2. the ``k = 1`` plane is the closed-loop scan's own KL at frame ``t0 + 1`` (row, action and frame alignment, no restatement involved);
3. ``shared_step(..., overshoot=lo)`` against an expected value built from existing pieces: the oracle's closed-loop run, its prior
   steps rolled from the gathered states, and the torch rule -- every loss term and EVERY gradient;
4. ``detach_state``, the refusal with ``forecast=``, data-parallel halves, captured against eager, ``val_overshoot``.

Tolerances are the project's: values 2e-5 relative, gradients 2e-4 of a tensor's largest entry, the table 1e-12
relative (it is a double).  A flipped one-hot sample forks a trajectory, so the ``u_overshoot`` seeds are screened on the CPU: the first
of 16 whose draws all stay 1e-4 from a CDF edge in the expected run is kept.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import Forecast, LatentOvershoot, OvershootTable
from multimodal_mtrssm_amd.distributions import KL_BALANCE_ALPHA
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from oracle.cases import CASES, build_batch, build_model, with_sizes
from oracle.ref_dists import sampling_margin
from oracle.ref_model import cat_probs, st_sample
from tests.test_forecast_gpu import _frame_nll, _kl_steps
from tests.test_modality_mask_oracle import oracle_step, screened
from tests.test_ragged_step_gpu import B, FAMILIES, IDS, LOSS_KEYS, VALID, T, _check_grads, _dev, _episode_batch, _model, _np, _padded, _train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(4, 4), (6, 5), (8, 2), (16, 8), (3, 11)]  # K x C; the last exercises class counts above 8
GEOMS = [(2, 1, 0), (3, 2, 1), (5, 4, 0), (7, 1, 0)]  # (D, s, o): the depth reaches past T
VALID_GLOBAL = (3, *VALID, 5)  # the rank holds rows 1 .. 3 of five
LO = LatentOvershoot(3, stride=2)


# 1. the kernels alone ---------------------------------------------------------------------------------------------------------------
def _logits(shape: tuple[int, ...], kind: str, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == "saturated":
        x = torch.where(torch.rand(shape, generator=g) < 0.5, -40.0, 40.0) + 0.01 * x  # noqa: PLR2004
    return x


def _kl_case(cats: int, classes: int, geom: tuple[int, int, int], ragged: bool, kind: str, weights: tuple[float, float]) -> None:  # noqa: FBT001, PLR0913, PLR0914
    depth, stride, offset = geom
    lo = LatentOvershoot(depth, stride=stride, offset=offset)
    n, width = lo.rows(T), cats * classes
    post = _logits((B, T, width), kind, 11 * cats + classes)
    os_logits = _logits((B * n, depth, width), kind, 13 * cats + classes + depth)
    if ragged:
        valid, row0 = torch.tensor(VALID_GLOBAL, dtype=torch.int32), 1
    else:
        lo, valid, row0 = lo.for_rank(2, 1), None, B  # rows 3 .. 5 of six
    q64, p64 = post.double().requires_grad_(), os_logits.double().requires_grad_()
    want = lo.reference(q64, p64, cats, valid, row0, weights)
    g_scale = 0.75
    (want.term * g_scale).backward()
    q, p = post.to(DEV).requires_grad_(), os_logits.to(DEV).requires_grad_()
    v = None if valid is None else valid.to(DEV)
    runs = []
    for _ in range(2):
        q.grad = p.grad = None
        got = lo.kl(q, p, cats, v, row0, weights)
        (got.term * g_scale).backward()
        torch.cuda.synchronize()
        runs.append((got.term.detach().clone(), got.plane.clone(), got.table.clone(), got.count.clone(), p.grad.clone(),
                     None if q.grad is None else q.grad.clone()))
    term, plane, table, count, g_os, g_post = runs[0]
    what = f"{cats}x{classes} {geom} ragged={ragged} {kind} {weights}"
    want_term = float(want.term.detach())
    print(what, "term", float(term), want_term, "count", float(count), float(want.count))
    assert float(count) == float(want.count), what
    np.testing.assert_allclose(float(term), want_term, rtol=2e-5, err_msg=what)
    np.testing.assert_allclose(_np(plane), want.plane.numpy(), rtol=2e-5, atol=0, err_msg=what)
    np.testing.assert_allclose(table.cpu().numpy(), want.table.numpy(), rtol=1e-12, atol=0, err_msg=what)
    # dead outputs are exactly 0
    length = torch.full((B,), T) if valid is None else valid[row0 : row0 + B].long().clamp(0, T)
    t0 = torch.tensor(lo.starts(T))
    target = t0.unsqueeze(1) + 1 + torch.arange(depth).unsqueeze(0)
    live = (target.unsqueeze(0) < length.reshape(-1, 1, 1)).reshape(B * n, depth)
    assert not bool(plane.cpu()[~live].any()), what
    trained = live.clone()
    trained[:, 0] = False  # k = 1 is reported, never trained
    assert not bool(g_os.cpu()[~trained].any()), what
    assert bool(g_os.cpu()[trained].any()) or not bool(trained.any()), what
    scale = float(p64.grad.abs().max())
    np.testing.assert_allclose(_np(g_os), p64.grad.float().numpy(), rtol=0, atol=2e-4 * scale, err_msg=f"g_os {what}")
    if weights[1] == 0.0:
        assert g_post is None, what  # (not written at all)
    else:
        scale = float(q64.grad.abs().max())
        np.testing.assert_allclose(_np(g_post), q64.grad.float().numpy(), rtol=0, atol=2e-4 * scale, err_msg=f"g_post {what}")
    for a, b in zip(runs[0], runs[1], strict=True):  # two calls agree bitwise
        assert (a is None and b is None) or torch.equal(a, b), what


@pytest.mark.parametrize("geom", GEOMS, ids=[f"D{d}s{s}o{o}" for d, s, o in GEOMS])
@pytest.mark.parametrize(("cats", "classes"), SHAPES, ids=[f"{k}x{c}" for k, c in SHAPES])
def test_kl_kernels_equal_the_float64_rule(cats: int, classes: int, geom: tuple[int, int, int]) -> None:
    for ragged in (False, True):
        for kind in ("normal", "saturated"):
            for weights in ((1.0, 0.0), (KL_BALANCE_ALPHA, 1.0 - KL_BALANCE_ALPHA)):
                _kl_case(cats, classes, geom, ragged, kind, weights)


def test_kl_kernels_past_one_staging_tile() -> None:
    """K * C above the 512 floats a wave stages (spans of categoricals) and C above them (read in place)."""
    for cats, classes in ((40, 20), (2, 600)):
        _kl_case(cats, classes, (3, 2, 1), True, "normal", (1.0, 1.0))


@pytest.mark.parametrize("geom", GEOMS, ids=[f"D{d}s{s}o{o}" for d, s, o in GEOMS])
def test_gather_and_scatter_are_bit_equal_to_the_select_rule(geom: tuple[int, int, int]) -> None:
    depth, stride, offset = geom
    lo = LatentOvershoot(depth, stride=stride, offset=offset)
    g = torch.Generator().manual_seed(5)
    for widths, actions in (((200, 30), 6), ((5, 8, 3, 12, 7, 16), 3), ((64,), 4)):  # MRSSM's two, MMTRSSM's six; widths off the float4 path
        states = [torch.randn(B, T, w, generator=g) for w in widths]
        acts = torch.randn(B, T, actions, generator=g)
        want_states, want_windows = lo.gather_reference(states, acts)
        dev_states = [x.to(DEV).requires_grad_() for x in states]
        got_states, got_windows = lo.gather(dev_states, acts.to(DEV))
        assert torch.equal(got_windows.cpu(), want_windows)
        tail = [t0 + 1 + j >= T for t0 in lo.starts(T) for j in range(depth)]
        assert not bool(got_windows.cpu().reshape(B, -1, actions)[:, tail].any())  # the zero-filled action tail
        for a, b in zip(got_states, want_states, strict=True):
            assert torch.equal(a.detach().cpu(), b)
        grads = [torch.randn(x.shape, generator=g) for x in want_states]
        torch.autograd.backward(got_states, [x.to(DEV) for x in grads])
        torch.cuda.synchronize()
        for x, full in zip(dev_states, lo.scatter_reference(grads, B, T), strict=True):
            assert torch.equal(x.grad.cpu(), full)
        off = LatentOvershoot(depth, stride=stride, offset=offset, detach_state=True)
        assert not any(x.requires_grad for x in off.gather(dev_states, acts.to(DEV))[0])


# 2. and 3. the step ------------------------------------------------------------------------------------------------------------------
def _levels(case) -> list[tuple[str, int, int]]:  # noqa: ANN001
    d = case.dims
    return [("", d.cats, d.classes)] if case.kind == "mrssm" else [("_l", d.ls_cats, d.ls_classes), ("_h", d.hs_cats, d.hs_classes)]


def _open_loop(case, oracle, roll: dict, actions: torch.Tensor, lo: LatentOvershoot, u: dict[str, torch.Tensor]):  # noqa: ANN001, ANN202
    """The overshoot rows from the oracle's own pieces: its prior step rolled ``D`` times from the closed-loop states at the starts.
    Returns the rows' prior logits per level ``[B * N, D, K * C]`` and the smallest distance of a draw from a CDF edge."""
    d = case.dims
    states = [roll["_" + k] for k in (("deter", "post_stoch") if case.kind == "mrssm" else
                                      ("deter_l", "deter_h", "post_stoch_l", "post_stoch_h", "hidden_l", "hidden_h"))]
    if lo.detach_state:
        states = [x.detach() for x in states]
    starts, windows = lo.gather_reference(states, actions)
    keep: dict[str, list[torch.Tensor]] = {sfx: [] for sfx, _, _ in _levels(case)}
    margin = 1.0
    if case.kind == "mrssm":
        deter, stoch = starts
        for j in range(lo.depth):
            deter, logits, stoch = oracle._prior_step(windows[:, j], deter, stoch, u[""][:, j])  # noqa: SLF001
            margin = min(margin, float(sampling_margin(cat_probs(logits.detach(), d.cats, d.classes)[1], u[""][:, j]).min()))
            keep[""].append(logits)
    else:
        deter_l, deter_h, stoch_l, stoch_h, hidden_l, hidden_h = starts
        for j in range(lo.depth):
            deter_l, hidden_l = oracle.l_rnn(torch.cat([windows[:, j], stoch_l, stoch_h], dim=-1), deter_l, hidden_l)
            logits_l = oracle.l_prior(deter_l)
            deter_h, hidden_h = oracle.h_rnn(stoch_h, deter_h, hidden_h)
            logits_h = oracle.h_prior(deter_h)
            probs_l, probs_h = cat_probs(logits_l, d.ls_cats, d.ls_classes)[1], cat_probs(logits_h, d.hs_cats, d.hs_classes)[1]
            margin = min(margin, float(sampling_margin(probs_l.detach(), u["_l"][:, j]).min()), float(sampling_margin(probs_h.detach(), u["_h"][:, j]).min()))
            stoch_l, stoch_h = st_sample(probs_l, u["_l"][:, j]), st_sample(probs_h, u["_h"][:, j])
            keep["_l"].append(logits_l)
            keep["_h"].append(logits_h)
    return {sfx: torch.stack(v, dim=1) for sfx, v in keep.items()}, margin


def _expected(case, oracle, batch, noise, u_os, lo: LatentOvershoot, lens: torch.Tensor | None) -> dict:  # noqa: ANN001, PLR0913
    """The step's loss terms from existing pieces (float32 oracle, float64 rule), differentiable."""
    d = case.dims
    rule = Forecast(T).reference(torch.zeros(B), T, lens)  # a context that reaches every row's end: the closed-loop (ragged) step
    roll = oracle_step(case, oracle, batch, noise, rule.codes.long())
    if case.kind == "mrssm":
        feature = torch.cat([roll["_deter"], roll["_post_stoch"]], dim=-1)
        kls = {"kl": (_kl_steps(roll["_post_logits"], roll["_prior_logits"], d.cats, d.classes, d.use_kl_balancing), d.kl_coeff)}
    else:
        feature = torch.cat([roll["_deter_h"], roll["_post_stoch_h"], roll["_deter_l"], roll["_post_stoch_l"]], dim=-1)
        kls = {"kl": (_kl_steps(roll["_post_logits_l"], roll["_prior_logits_l"], d.ls_cats, d.ls_classes, d.use_kl_balancing), d.kl_coeff),
               "kl_h": (_kl_steps(roll["_post_logits_h"], roll["_prior_logits_h"], d.hs_cats, d.hs_classes, d.use_kl_balancing),
                        d.kl_coeff * d.w_kl_h)}
    live = rule.target.float()
    out = {"recon/audio": (_frame_nll(oracle.audio_decoder(feature), batch[4]) * live).sum() / rule.counts[0],
           "recon/vision": (_frame_nll(oracle.vision_decoder(feature), batch[5]) * live).sum() / rule.counts[0]}
    out["recon"] = out["recon/audio"] + out["recon/vision"]
    out["loss"] = out["recon"]
    for key, (steps, coeff) in kls.items():
        out[key] = (steps * live).sum() / rule.counts[0] * coeff
        out["loss"] = out["loss"] + out[key]
    os_logits, margin = _open_loop(case, oracle, roll, batch[0], lo, u_os)
    weights = lo.kl_weights(bool(d.use_kl_balancing))
    planes = {}
    for (sfx, cats, _), key, coeff in zip(_levels(case), ("overshoot", "overshoot_h"), (1.0, float(getattr(d, "w_kl_h", 1.0))), strict=False):
        terms = lo.reference(roll["_post_logits" + sfx], os_logits[sfx], cats, lens, 0, weights)
        out[key] = terms.term
        planes[key] = terms
        out["loss"] = out["loss"] + d.kl_coeff * lo.weight * coeff * terms.term
    return {"out": out, "margin": margin, "planes": planes, "roll": roll}


@functools.lru_cache(maxsize=None)
def _overshoot_reference(name: str, ragged: bool, detach: bool = False) -> dict:  # noqa: FBT001, FBT002
    """Computed once per model and shared: the closed-loop noise screened under the step's codes, the ``u_overshoot`` seed screened in
    the expected run (the first of 16 that keeps 1e-4 from every CDF edge), the expected terms and their gradients."""
    case = with_sizes(CASES[name], B, T)
    oracle = build_model(case)
    batch = build_batch(case)
    lens = torch.tensor(VALID, dtype=torch.int32) if ragged else None
    if ragged:
        batch = _padded(batch, VALID)
    lo = LatentOvershoot(LO.depth, stride=LO.stride, detach_state=detach)
    codes = Forecast(T).reference(torch.zeros(B), T, lens).codes.long()
    noise, margin = screened(case, oracle, batch, codes)
    assert margin >= 1e-5, f"no noise seed keeps the closed-loop draws away from the CDF edges (best {margin})"
    n = lo.rows(T)
    found = None
    for seed in range(300, 316):
        g = torch.Generator().manual_seed(seed)
        u_os = {sfx: torch.rand(B, n, lo.depth, cats, generator=g) for sfx, cats, _ in _levels(case)}
        flat = {sfx: u.reshape(B * n, lo.depth, -1) for sfx, u in u_os.items()}
        with torch.no_grad():
            m = _expected(case, oracle, batch, noise, flat, lo, lens)["margin"]
        if m >= 1e-4:  # noqa: PLR2004
            found = (seed, m, u_os, flat)
            break
    assert found is not None, "none of 16 u_overshoot seeds keeps every draw 1e-4 from a CDF edge"
    print(f"{name} ragged={ragged}: u_overshoot seed {found[0]}, margin {found[1]:.3e}")
    exp = _expected(case, oracle, batch, noise, found[3], lo, lens)
    oracle.zero_grad(set_to_none=True)
    exp["out"]["loss"].backward()
    grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "lens": lens, "lo": lo, "u_os": found[2],
            "terms": {k: float(v.detach()) for k, v in exp["out"].items()}, "grads": grads, "planes": exp["planes"], "roll": exp["roll"]}


def _step_noise(ref: dict) -> tuple[tuple, dict]:
    batch, noise = _dev(ref["batch"], ref["noise"])
    for sfx, u in ref["u_os"].items():
        noise["u_overshoot" + sfx] = u.to(DEV)
    return batch, noise


def _step_kw(ref: dict) -> dict:
    return {} if ref["lens"] is None else {"lengths": ref["lens"].to(DEV)}


def test_the_screen_finds_a_seed_on_the_cpu() -> None:
    """The screening runs on the host alone; it prints the margin it found."""
    for name in ("mrssm_default", "mmtrssm_default"):
        for ragged in (False, True):
            assert _overshoot_reference(name, ragged)["u_os"]


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_overshoot_step_matches_the_expected_value_from_existing_pieces(name: str, onecu: bool, ragged: bool) -> None:  # noqa: FBT001
    ref = _overshoot_reference(name, ragged)
    case = ref["case"]
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _step_noise(ref)
    out, grads = _train(model, batch, noise, overshoot=ref["lo"], **_step_kw(ref))
    extra = ("overshoot",) if case.kind == "mrssm" else ("overshoot", "overshoot_h")
    assert tuple(out) == (*[k for k in ("recon", "recon/audio", "recon/vision", "kl", "kl_h", "loss") if k in LOSS_KEYS[case.kind]], *extra)
    for k, want in ref["terms"].items():
        print(name, onecu, ragged, k, float(out[k]), want)
        np.testing.assert_allclose(float(out[k]), want, rtol=2e-5, err_msg=k)
    _check_grads(grads, ref["grads"])
    # the planes: the kernel's against the rule's on the oracle's logits; dead terms exactly 0
    for got, want in zip(model._overshoot_terms_last, ref["planes"].values(), strict=True):  # noqa: SLF001
        np.testing.assert_allclose(_np(got.plane), want.plane.numpy(), rtol=2e-5, atol=2e-6)
        assert torch.equal(got.plane.cpu() == 0, want.plane == 0)
        np.testing.assert_allclose(got.table.cpu().numpy()[1], want.table.numpy()[1], rtol=0, atol=0)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_the_first_distance_is_the_closed_loop_scans_own_kl(name: str, onecu: bool, ragged: bool) -> None:  # noqa: FBT001
    ref = _overshoot_reference(name, ragged)
    lo, lens = ref["lo"], ref["lens"]
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _step_noise(ref)
    kw = _step_kw(ref)
    with torch.no_grad():
        model.shared_step(batch, noise, overshoot=lo, **kw)
        terms = model._overshoot_terms_last  # noqa: SLF001
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise, **kw)
    kls = [post.kl_per_step] if ref["case"].kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]
    t0 = torch.tensor(lo.starts(T))
    length = torch.full((B,), T) if lens is None else lens.long()
    live = (t0.unsqueeze(0) + 1) < length.unsqueeze(1)  # [B, N]
    assert bool(live.any())
    for got, kl in zip(terms, kls, strict=True):
        first = got.plane[:, 0].reshape(B, -1).cpu()
        want = kl.cpu()[:, t0 + 1]
        np.testing.assert_allclose(first[live].numpy(), want[live].numpy(), rtol=2e-5, atol=0)
        assert not bool(first[~live].any())


# 4. further checks ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_detached_start_states_leave_the_posterior_heads_to_the_plain_step(name: str) -> None:
    ref = _overshoot_reference(name, False, True)
    model = _model(name, False, ref["oracle"])
    batch, noise = _step_noise(ref)
    out, grads = _train(model, batch, noise, overshoot=ref["lo"])
    for k, want in ref["terms"].items():
        np.testing.assert_allclose(float(out[k]), want, rtol=2e-5, err_msg=k)
    _check_grads(grads, ref["grads"])
    plain_out, plain = _train(model, batch, noise)
    np.testing.assert_allclose(float(plain_out["kl"]), float(out["kl"]), rtol=2e-5)
    heads = [k for k in plain if "rnn_to_post_projector" in k or "h_posterior" in k]
    assert heads
    for k in heads:  # the posterior is a fixed target and nothing flows back into the start states
        scale = float(plain[k].abs().max())
        np.testing.assert_allclose(_np(grads[k]), _np(plain[k]), rtol=0, atol=2e-4 * scale, err_msg=k)


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_refusals_train_step_and_validation_table(name: str) -> None:
    ref = _overshoot_reference(name, True)
    lo, case = ref["lo"], ref["case"]
    model = _model(name, False, ref["oracle"])
    batch, noise = _step_noise(ref)
    with pytest.raises(ValueError, match="forecast"):
        model.shared_step(batch, noise, forecast=Forecast(3), overshoot=lo)
    with pytest.raises(ValueError, match="LatentOvershoot"):
        model.shared_step(batch, noise, overshoot=3)
    with pytest.raises(ValueError, match="offset"):
        model.shared_step(batch, noise, overshoot=LatentOvershoot(2, offset=T - 1))
    plain_shapes = dict(model.noise_shapes(B, T))
    model.overshoot = lo
    shapes = model.noise_shapes(B, T)
    new = {k: v for k, v in shapes.items() if k not in plain_shapes}
    sizes = [cats for _, cats, _ in _levels(case)]
    assert list(new.values()) == [(B, lo.rows(T), lo.depth, k) for k in sizes] and all(k.startswith("u_overshoot") for k in new)
    assert {k: shapes[k] for k in plain_shapes} == plain_shapes
    logged = model.training_step(batch)
    assert "train/overshoot" in logged and ("train/overshoot_h" in logged) == (case.kind == "mmtrssm")
    model.overshoot = None
    # validation: the table is the kernel-alone rule's on the step's own logits
    model.val_overshoot = lo
    ragged_batch = _episode_batch(batch, list(VALID), list(VALID), 0)
    torch.manual_seed(3)
    model.validation_step(ragged_batch)
    terms = model._overshoot_terms_last  # noqa: SLF001
    table = model.overshoot_table
    assert isinstance(table, OvershootTable) and table.levels == len(sizes)
    for level, got in enumerate(terms):
        assert torch.equal(table.buffer[level], got.table)
    live = [sum(1 for n in VALID for t0 in lo.starts(T) if t0 + k < n) for k in range(1, lo.depth + 1)]
    assert table.buffer[0, 1].tolist() == [float(x) for x in live]
    model.validation_step(ragged_batch)
    assert table.buffer[0, 1].tolist() == [2.0 * x for x in live]
    logged = model.on_validation_epoch_end()
    want = {f"val/overshoot/kl_d{k}" for k in range(1, lo.depth + 1)}
    if case.kind == "mmtrssm":
        want |= {f"val/overshoot/kl_h_d{k}" for k in range(1, lo.depth + 1)}
    assert want <= set(logged) and model.overshoot_table is None
    assert all(bool(torch.isfinite(logged[k])) for k in want)


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_overshoot_loss_is_exact_under_data_parallel_sharding(name: str, onecu: bool) -> None:  # noqa: FBT001
    """Two half-batches with global-row noise reproduce the full batch's loss terms (B = 4: rows 0 .. 1 and 2 .. 3)."""
    valid = (6, 4, 1, 5)
    case = with_sizes(CASES[name], 4, T)
    oracle = build_model(case)
    model = _model(name, onecu, oracle, (4, T))
    batch = tuple(x.to(DEV) for x in _padded(build_batch(case), valid))
    g = torch.Generator(device=DEV).manual_seed(9)
    model.overshoot = LO
    noise = {k: torch.rand(s, generator=g, device=DEV) for k, s in sorted(model.noise_shapes(4, T).items())}
    model.overshoot = None
    with torch.no_grad():
        full = model.shared_step(_episode_batch(batch, list(valid), list(valid), 0), noise, overshoot=LO)
        halves = []
        for rank in range(2):
            rows = slice(2 * rank, 2 * rank + 2)
            part = _episode_batch(tuple(x[rows] for x in batch), list(valid[rows]), list(valid), 2 * rank)
            halves.append(model.shared_step(part, {k: v[rows] for k, v in noise.items()}, overshoot=LO.for_rank(2, rank)))
    for k in full:
        mean = 0.5 * (float(halves[0][k]) + float(halves[1][k]))
        print(name, onecu, k, float(full[k]), mean)
        np.testing.assert_allclose(mean, float(full[k]), rtol=2e-5, err_msg=k)


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_captured_overshoot_step_matches_eager(name: str, onecu: bool) -> None:  # noqa: FBT001
    """Three steps of the graph against three eager steps from the same weights, optimizer state and noise stream, at the tolerances
    ``test_ragged_step_gpu.py`` states for captures (losses 1e-4 relative; parameters: largest difference below 2e-4, mean below 2e-7,
    at its lr = 1e-5 and clip_norm = 10)."""
    ref = _overshoot_reference(name, False)
    batch, _ = _dev(ref["batch"], ref["noise"])
    runs = []
    for captured in (False, True):
        model = _model(name, onecu, ref["oracle"])
        flat = FlatParameters(model, extra=8)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        dp = mt.FlatDataParallel(flat)
        source = dp.noise_source(21)
        losses = []
        if captured:
            step = CapturedTrainStep(model, flat, opt, dp, batch, source, warmup=2, overshoot=LO)
            with pytest.raises(ValueError, match="forecast"):
                CapturedTrainStep(model, flat, opt, dp, batch, source, overshoot=LO, forecast=Forecast(3))
            for _ in range(3):
                losses.append({k: float(v) for k, v in step.step(batch).items()})
            step.close()
        else:
            model.overshoot = LO
            shapes = model.noise_shapes(B, T)
            model.overshoot = None
            for _ in range(3):
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(batch, noise, overshoot=LO)
                out["loss"].backward()
                logs = dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v) for k, v in logs.items()})
        torch.cuda.synchronize()
        runs.append((losses, flat.param.detach().clone()))
    (eager, p0), (graph, p1) = runs
    for a, b in zip(eager, graph, strict=True):
        assert list(a) == list(b)
        for k in a:
            np.testing.assert_allclose(b[k], a[k], rtol=1e-4, err_msg=k)
    diff = (p1 - p0).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))  # noqa: PLR2004


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_overshoot_composes_with_dropout_schedule_carry_and_the_weighted_model(name: str) -> None:
    """Under modality dropout, lengths, an ELBO schedule in its warm-up, a state carry and a learned gate at once, the step's existing
    terms are those of the same step without the overshoot (same uniforms), the new keys come last, and
    ``loss = that step's loss + kl_coeff * weight * beta * (overshoot + w_kl_h * overshoot_h)``."""
    ref = _overshoot_reference(name, True)
    case, d = ref["case"], ref["case"].dims
    model = _model(name, False, ref["oracle"])
    model.expert_weights = mt.ExpertWeights("gated", model.audio_representation.obs_embed_size).to(DEV)
    with torch.no_grad():
        for p in model.expert_weights.parameters():
            p.normal_(0.0, 0.5, generator=torch.Generator(device=DEV).manual_seed(2))
    batch, noise = _step_noise(ref)
    md = mt.ModalityDropout(0.4, 0.3, span=2)
    noise["u_mask"] = torch.rand(md.noise_shape(B, T), generator=torch.Generator().manual_seed(6)).to(DEV)
    lo = LatentOvershoot(LO.depth, stride=LO.stride, weight=0.5, balanced=True)
    outs = []
    for overshoot in (None, lo):
        schedule = mt.ElboSchedule(free_nats=0.05, beta_start=0.25, warmup_steps=8).set_step(2, DEV)
        carry = mt.StateCarry.for_model(model, B)
        kw = {"modality_dropout": md, "elbo_schedule": schedule, "state_carry": carry, "reset": torch.ones(B, dtype=torch.bool),
              "lengths": ref["lens"].to(DEV), "overshoot": overshoot}
        out, grads = _train(model, batch, noise, **kw)
        outs.append((out, grads, float(schedule.stats["beta"]), model.weights_timeseries.clone()))
    (plain, _, beta0, w0), (both, grads, beta, w1) = outs
    assert 0.25 < beta == beta0 < 1.0  # noqa: PLR2004
    assert tuple(w1.shape) == (B, T, 3)  # the reported weights stay the closed-loop step's, not the overshoot rows'
    np.testing.assert_allclose(_np(w1), _np(w0), rtol=2e-5, atol=1e-7)
    extra = ("overshoot",) if case.kind == "mrssm" else ("overshoot", "overshoot_h")
    assert tuple(both) == (*plain, *extra)
    for k in plain:
        if k != "loss":
            np.testing.assert_allclose(float(both[k]), float(plain[k]), rtol=2e-5, err_msg=k)
    term = float(both["overshoot"]) + (float(d.w_kl_h) * float(both["overshoot_h"]) if case.kind == "mmtrssm" else 0.0)
    assert term > 0.0
    np.testing.assert_allclose(float(both["loss"]), float(plain["loss"]) + float(d.kl_coeff) * lo.weight * beta * term, rtol=2e-5)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and any("expert_weights" in k for k in grads)
