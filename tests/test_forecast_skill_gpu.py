"""GPU (MI355X): forecast skill by horizon, end to end.

What is pinned here: the scorer kernel is the float64 rule (rtol 1e-5: non-negative addends, at most 16 sequential adds per lane and an
8-level tree, about 28 * 2^-24 = 1.7e-6, plus room for the device Tanh; ``spread`` -- a difference of near-equal numbers when the
samples agree -- additionally atol 1e-6 * mean), bitwise reproducible, exactly 0 on dead frames and consistent with the NLL kernel; the
table kernel is the fp32 torch fold bit for bit; a skill step is the composition of the existing public pieces (``forecast_rollout``
per sample with the composed noise, ``decode_state``, the float64 rule) to the project's loss-term tolerance, rtol 2e-5 (DESIGN.md
section 2), with the copies of a row sharing their context trajectory exactly; ``validation_step`` keeps its ``val/*`` draws.  Noise is
screened on the CPU under the codes of the run it feeds (margin 1e-4), so that no draw sits at a CDF edge.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import ForecastSkill, SkillTable
from oracle.cases import CASES, build_batch, build_model, build_noise, min_margin, with_sizes
from tests.conftest import product_from_case
from tests.test_forecast_skill_host import HOST_COUNTS, HOST_Q, HOST_SUMS, HOST_VALID, host_planes
from tests.test_modality_mask_oracle import oracle_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, T, S, Q = 2, 6, 4, 2
MODELS = ["mrssm_default", "mmtrssm_default"]
BITS = {"both": 3, "audio": 1, "vision": 2}
COUNTS = [float(B * Q)] + [float(B)] * (T - Q) + [0.0] * (Q - 1)  # frames per bin of one step: the last horizon is T - Q


# 1. the scorer is the rule ----------------------------------------------------------------------------------------------------------
def _assert_planes(got, want, what) -> None:  # noqa: ANN001
    mean = want.mean.numpy()
    for name in ("mean", "ens", "best"):
        np.testing.assert_allclose(getattr(got, name).cpu().numpy(), getattr(want, name).numpy(), rtol=1e-5, atol=0, err_msg=f"{name} {what}")
    err = np.abs(got.spread.cpu().double().numpy() - want.spread.numpy())
    bound = 1e-5 * np.abs(want.spread.numpy()) + 1e-6 * mean
    print(what, "spread worst err / bound", float((err / np.maximum(bound, 1e-300)).max()) if bound.max() > 0 else 0.0)
    assert bool((err <= bound).all()), f"spread {what}: {float(err.max())}"


@pytest.mark.parametrize("shape", [(3, 1, 5, 4), (2, 2, 3, 1036), (2, 5, 3, 1024), (1, 16, 2, 4096), (70, 2, 40, 4)], ids=str)
def test_scorer_kernel_equals_the_float64_rule(shape: tuple[int, int, int, int]) -> None:
    b, s, t, e = shape
    g = torch.Generator().manual_seed(sum(shape))
    pred = torch.randn(b, s, t, e, generator=g) * 1.5
    target = torch.rand(b, t, e, generator=g) * 2.0 - 1.0
    ragged = torch.randint(0, t + 2, (b,), generator=g).to(torch.int32)
    if b > 1:
        ragged[0], ragged[-1] = t + 3, 0  # a value above T (the whole row is live) and a row with no live frame
        ragged_cases = [ragged]
    else:  # (one row cannot hold both)
        ragged_cases = [torch.tensor([t + 3], dtype=torch.int32), torch.zeros(1, dtype=torch.int32)]
    dpred, dtarget = pred.to(DEV), target.to(DEV)
    for act in (0, 3):
        for valid in (None, *ragged_cases):
            what = f"{shape} act {act} valid {None if valid is None else valid.tolist()[:6]}"
            want = ForecastSkill.reference(pred.double(), target.double(), valid, act)
            got = ForecastSkill.score(dpred, dtarget, None if valid is None else valid.to(DEV), act, se_samples=True)
            again = ForecastSkill.score(dpred, dtarget, None if valid is None else valid.to(DEV), act, se_samples=True)
            torch.cuda.synchronize()
            _assert_planes(got, want, what)
            np.testing.assert_allclose(got.se_samples.cpu().numpy(), want.se_samples.numpy(), rtol=1e-5, atol=0, err_msg=what)
            assert torch.equal(got.best, got.se_samples.min(1).values), what
            for a, w in zip(got, again, strict=True):
                assert torch.equal(a, w), what  # two runs agree bitwise
            if s == 1:
                assert not bool(got.spread.any()) and torch.equal(got.mean, got.ens) and torch.equal(got.mean, got.best), what
            if valid is not None:
                dead = ~(torch.arange(t) < valid[:, None]).to(DEV)
                for plane in got[:4]:
                    assert not bool(plane[dead].any()), what
                assert not bool(got.se_samples[dead[:, None].expand(b, s, t)].any()), what
                assert bool(dead.any()) == (int(valid.min()) < t)
            else:  # the frame mean of `mean`, plus the constant, is the NLL kernel's value on the same data
                nll = mt.likelihood(dpred, dtarget[:, None].expand(b, s, t, e).contiguous(), event_ndims=1, out_act=act)
                mine = float(got.mean.double().mean()) + 0.5 * e * math.log(2.0 * math.pi)
                print(what, "nll", float(nll), mine)
                np.testing.assert_allclose(mine, float(nll), rtol=1e-5, err_msg=what)
    # without se_samples the planes are the same bits
    bare = ForecastSkill.score(dpred, dtarget, None, 3)
    full = ForecastSkill.score(dpred, dtarget, None, 3, se_samples=True)
    assert bare.se_samples is None and all(torch.equal(a, w) for a, w in zip(bare[:4], full[:4], strict=True))


# 2. the table kernel is the fold ------------------------------------------------------------------------------------------------------
def test_table_kernel_equals_the_fp32_fold_bit_for_bit() -> None:
    context, valid = torch.tensor(HOST_Q, dtype=torch.int32), torch.tensor(HOST_VALID, dtype=torch.int32)
    table = SkillTable(7, DEV)
    ForecastSkill.table_add(host_planes().to(DEV), context.to(DEV), valid.to(DEV), table.sums[:2], table.counts)
    assert table.counts.tolist() == HOST_COUNTS and table.sums[:2].tolist() == HOST_SUMS and not bool(table.sums[2:].any())
    # B = 300, T = 50: random contexts and lengths, two batches accumulating in one buffer, with and without lengths
    g = torch.Generator().manual_seed(8)
    b, t = 300, 50
    want_sums, want_counts = torch.zeros(8, t), torch.zeros(t)
    got = SkillTable(t, DEV)
    for lengths in (True, False):
        planes = torch.rand(8, b, t, generator=g) * 30.0
        context = torch.randint(1, t + 5, (b,), generator=g).to(torch.int32)
        valid = torch.randint(0, t + 3, (b,), generator=g).to(torch.int32) if lengths else None
        ForecastSkill.reference_table(planes, context, valid, want_sums, want_counts)
        ForecastSkill.table_add(planes.to(DEV), context.to(DEV), None if valid is None else valid.to(DEV), got.sums, got.counts)
        torch.cuda.synchronize()
        assert torch.equal(got.counts.cpu(), want_counts) and torch.equal(got.sums.cpu(), want_sums), lengths
    assert float(want_counts[0]) > 1000 and float(want_counts[t - 1]) > 0  # noqa: PLR2004


# 3. the skill step is the composition of the public pieces ----------------------------------------------------------------------------
def _wide(x: torch.Tensor) -> torch.Tensor:
    return x.repeat_interleave(S, dim=0)


@functools.lru_cache(maxsize=None)
def _setup(name: str, observe: str = "both", q: int = Q) -> dict:
    """Computed once per model and shared: the oracle, a batch and skill noise screened on the CPU under the codes of the wide run it
    feeds -- row ``b * S + s`` reads its row's context draws on ``t < q`` and draws of its own after."""
    case = with_sizes(CASES[name], B, T)
    oracle = build_model(case)
    batch = build_batch(case)
    wide_batch = tuple(_wide(x) for x in batch)
    codes = (torch.arange(T) < q).long().mul(BITS[observe]).expand(B * S, T).contiguous()
    best = None
    for seed in range(300, 340):
        noise = build_noise(case, seed, batch=B * S, steps=T)
        for k, u in noise.items():  # the copies of a row share the initial draw and the context's draws
            first = _wide(u[::S])
            if u.dim() == 2:  # noqa: PLR2004
                u.copy_(first)
            else:
                u[:, : min(q, T)] = first[:, : min(q, T)]
        with torch.no_grad():
            out = oracle_step(case, oracle, wide_batch, noise, codes)
        margin = min_margin(case, out, noise)
        if best is None or margin > best[1]:
            best = (noise, margin)
        if margin >= 1e-4:  # noqa: PLR2004
            break
    wide_noise, margin = best
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    noise = {}
    for k, u in wide_noise.items():
        if k.startswith("u_prior"):
            continue
        noise[k] = u[::S].contiguous()  # u_init*, u_post*: the row's own (its tail part is never read)
        if k.startswith("u_post"):
            noise[k.replace("post", "tail")] = u.reshape(B, S, *u.shape[1:]).contiguous()
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "wide_noise": wide_noise}


def _model(name: str, ref: dict):  # noqa: ANN202
    return product_from_case(ref["case"], ref["oracle"], DEV)


def _dev(ref: dict) -> tuple[tuple, dict]:
    return tuple(x.to(DEV) for x in ref["batch"]), {k: v.to(DEV) for k, v in ref["noise"].items()}


def _state_fields(kind: str) -> tuple[tuple[str, ...], tuple[str, ...]]:
    return (("deter",), ("stoch",)) if kind == "mrssm" else (("deter_l", "deter_h"), ("stoch_l", "stoch_h"))


def _composed(model, ref: dict, batch: tuple, q: int, lengths: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:  # noqa: ANN001
    """The planes ``[8, B, T]`` and the table ``[9, T]`` in float64 from existing public pieces: per sample ``forecast_rollout`` under that
    sample's rows of the composed noise, ``decode_state``, then the rule."""
    wide_noise = {k: v.to(DEV) for k, v in ref["wide_noise"].items()}
    obs = (batch[1], batch[2])
    recon: dict[str, list[torch.Tensor]] = {"recon/audio": [], "recon/vision": []}
    for s in range(S):
        noise_s = {k: v[s::S].contiguous() for k, v in wide_noise.items()}
        with torch.no_grad():
            s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise_s)
            post = model.forecast_rollout(actions=batch[0], observations=obs, context=q, prev_state=s0, noise=noise_s, lengths=lengths)
            dec = model.decode_state(post)
        for k in recon:
            recon[k].append(dec[k].flatten(2).double().cpu())
    valid = None if lengths is None else lengths.cpu()
    planes = []
    for k, tgt in (("recon/audio", batch[4]), ("recon/vision", batch[5])):
        got = ForecastSkill.reference(torch.stack(recon[k], dim=1), tgt.flatten(2).double().cpu(), valid, 0)
        planes += list(got[:4])
    planes = torch.stack(planes)
    sums, counts = torch.zeros(8, T, dtype=torch.float64), torch.zeros(T, dtype=torch.float64)
    ForecastSkill.reference_table(planes, torch.full((B,), q, dtype=torch.int32), valid, sums, counts)
    return planes, torch.cat([sums, counts[None]])


def _assert_step(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Rows (audio, vision) x (mean, ens, best, spread) of the planes ``[8, B, T]`` or of the table's sums ``[8, T]``: rtol 2e-5, the
    project's loss-term tolerance.  ``spread`` additionally gets the scorer's atol of 1e-6 * mean: on the context the copies of a row
    decode to the same values, the float64 rule gives exactly 0 there, and fp32's left fold ``((y + y) + y) + y`` rounds at ``3 y``, so
    ``ybar`` misses ``y`` by up to an ulp -- a difference of near-equal numbers whose error scales with the frame's error, not with 0."""
    got, want = got.cpu().double().numpy(), want.double().numpy()
    for j in (0, 4):
        for r in range(3):
            np.testing.assert_allclose(got[j + r], want[j + r], rtol=2e-5, atol=0, err_msg=f"{what} row {j + r}")
        err, bound = np.abs(got[j + 3] - want[j + 3]), 2e-5 * np.abs(want[j + 3]) + 1e-6 * want[j]
        assert bool((err <= bound).all()), f"{what} spread row {j + 3}: worst {float(err.max())}"


@pytest.mark.parametrize("name", MODELS)
def test_skill_step_is_the_composition_of_the_public_pieces(name: str) -> None:
    ref = _setup(name)
    kind = ref["case"].kind
    model = _model(name, ref)
    batch, noise = _dev(ref)
    skill = ForecastSkill(Q, samples=S)
    table = model.forecast_skill(batch, skill, noise, keep_states=True)
    torch.cuda.synchronize()
    assert isinstance(table, SkillTable) and tuple(table.buffer.shape) == (9, T) and tuple(table.planes.shape) == (8, B, T)
    deters, stochs = _state_fields(kind)
    differ = False
    for k in (*deters, *stochs):
        x = getattr(table.states, k).reshape(B, S, T, -1)
        assert not x.requires_grad
        for s in range(1, S):
            assert torch.equal(x[:, s, :Q], x[:, 0, :Q]), (k, s)  # the copies share their context trajectory bit for bit
            differ = differ or not torch.equal(x[:, s, Q:], x[:, 0, Q:])
    assert differ  # ... and part ways somewhere on the tail
    want_planes, want_table = _composed(model, ref, batch, Q)
    rel = (table.planes.cpu().double() - want_planes).abs() / want_planes.abs().clamp_min(1e-30)
    print(name, "planes worst rel (mean, ens, best rows)", float(rel[[0, 1, 2, 4, 5, 6]].max()), "spread on the context", float(table.planes[[3, 7], :, :Q].max()))
    _assert_step(table.planes, want_planes, "planes")
    _assert_step(table.sums, want_table[:8], "table")
    assert torch.equal(table.counts.cpu().double(), want_table[8])
    assert table.counts.tolist() == COUNTS
    assert bool((table.planes[3][:, Q:] > 0).any()) and bool((table.planes[7][:, Q:] > 0).any())  # the tails' decodes differ: spread
    # a second step adds into the same table; chunks of one row at a time change nothing
    small = ForecastSkill(Q, samples=S)
    small.max_frames = 1
    again = model.forecast_skill(batch, small, noise, table=table)
    assert again is table and table.states is None and table.planes is None  # (nothing of a batch stays on the accumulator)
    assert torch.equal(table.counts.cpu(), 2.0 * want_table[8].float())
    _assert_step(table.sums, 2.0 * want_table[:8], "two steps")
    # without noise the step draws its own
    drawn = model.forecast_skill(batch, skill)
    assert bool(torch.isfinite(drawn.buffer).all()) and torch.equal(drawn.counts.cpu(), want_table[8].float())


@pytest.mark.parametrize("q", [6, 9])
@pytest.mark.parametrize("name", MODELS)
def test_a_context_of_the_whole_row_fills_only_bin_zero(name: str, q: int) -> None:
    ref = _setup(name, "both", q)
    model = _model(name, ref)
    batch, noise = _dev(ref)
    table = model.forecast_skill(batch, ForecastSkill(q, samples=S), noise)
    assert table.counts.tolist() == [float(B * T)] + [0.0] * (T - 1) and not bool(table.sums[:, 1:].any())
    assert bool(table.curves()["audio"]["mean"][1:].isnan().all())
    # bin 0 is the closed-loop reconstruction error: every copy is the plain posterior rollout under the row's own draws
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise)
        dec = model.decode_state(post)
    for j, (k, tgt) in enumerate((("recon/audio", batch[4]), ("recon/vision", batch[5]))):
        err = (0.5 * (tgt.double() - dec[k].double()) ** 2).flatten(2).sum(-1)
        for row in (0, 1, 2):  # mean, ens, best: the copies are equal, so all three are the one closed-loop error
            np.testing.assert_allclose(float(table.sums[4 * j + row, 0]), float(err.sum()), rtol=2e-5, err_msg=f"{k} {row}")
        assert float(table.sums[4 * j + 3, 0]) <= 1e-6 * float(err.sum())  # noqa: PLR2004  (no spread)


# 4. cross-modal: observe audio, predict vision -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_observing_audio_only_is_the_masked_rollout(name: str) -> None:
    ref = _setup(name, "audio")
    kind = ref["case"].kind
    model = _model(name, ref)
    batch, noise = _dev(ref)
    table = model.forecast_skill(batch, ForecastSkill(Q, samples=S, observe="audio"), noise, keep_states=True)
    wide_noise = {k: v.to(DEV) for k, v in ref["wide_noise"].items()}
    mask = torch.zeros(B * S, T, 2, dtype=torch.bool, device=DEV)
    mask[:, :Q, 0] = True  # audio on the context, nothing after
    wide = tuple(_wide(x) for x in batch)
    with torch.no_grad():
        s0 = model.initial_state((wide[1][:, 0], wide[2][:, 0]), wide_noise, modality_mask=mask[:, 0])
        post, _ = model.rollout_representation(actions=wide[0], observations=(wide[1], wide[2]), prev_state=s0, noise=wide_noise, modality_mask=mask)
    deters, stochs = _state_fields(kind)
    for k in stochs:
        assert torch.equal(getattr(table.states, k), getattr(post, k)), k
    for k in deters:
        np.testing.assert_allclose(getattr(table.states, k).cpu().numpy(), getattr(post, k).cpu().numpy(), rtol=0, atol=1e-5, err_msg=k)
    assert table.counts.tolist() == COUNTS and bool(torch.isfinite(table.buffer).all())
    both = model.forecast_skill(batch, ForecastSkill(Q, samples=S), noise)
    assert not torch.equal(both.sums[4, 0], table.sums[4, 0])  # vision's bin 0 is now a cross-modal reconstruction


# 5. lengths ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_lengths_cut_the_counts_and_dead_frames_add_nothing(name: str) -> None:
    ref = _setup(name)
    model = _model(name, ref)
    batch, noise = _dev(ref)
    lengths = torch.tensor([6, 3], dtype=torch.int32, device=DEV)
    table = model.forecast_skill(batch, ForecastSkill(Q, samples=S), noise, lengths=lengths, keep_states=True)
    h, live = ForecastSkill.horizon(torch.full((B,), Q, dtype=torch.int32), lengths.cpu(), T)
    want = torch.bincount(h[live], minlength=T).float()
    assert torch.equal(table.counts.cpu(), want) and want.tolist() == [4.0, 2.0, 1.0, 1.0, 1.0, 0.0]
    assert not bool(table.planes[:, 1, 3:].any()) and bool((table.planes[[0, 4], 0] != 0).all()) and bool((table.planes[[0, 4], 1, :3] != 0).all())
    want_planes, want_table = _composed(model, ref, batch, Q, lengths)
    _assert_step(table.planes, want_planes, "planes")
    _assert_step(table.sums, want_table[:8], "table")
    assert torch.equal(table.counts.cpu().double(), want_table[8])


# 6. validation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_validation_step_keeps_its_draws_and_the_epoch_end_logs_the_skill(name: str) -> None:
    ref = _setup(name)
    model = _model(name, ref)
    batch, _ = _dev(ref)
    torch.manual_seed(5)
    plain = model.validation_step(batch)
    assert model.skill_table is None and model.on_validation_epoch_end() == {}
    model.val_skill = ForecastSkill(Q, samples=S)
    torch.manual_seed(5)
    both = model.validation_step(batch)
    assert set(both) == set(plain)
    for k, v in plain.items():
        # the skill step runs after the existing work: the same draws, so the same values -- up to the order of the NLL kernels' float
        # atomics, which differs from run to run in the last bits (a changed draw flips samples and moves every term far more than the
        # project's loss-term tolerance)
        np.testing.assert_allclose(float(both[k]), float(v), rtol=2e-5, err_msg=k)
    model.validation_step(batch)
    assert isinstance(model.skill_table, SkillTable) and model.skill_table.counts.tolist() == [2.0 * c for c in COUNTS]
    logged = model.on_validation_epoch_end()
    assert model.skill_table is None
    assert set(logged) == {f"val/skill/{m}/{k}/{n}" for m in ("audio", "vision") for k in ("mean", "ens", "best", "spread")
                           for n in ("obs", "h1", "h2", "h4", "h8")}
    for m in ("audio", "vision"):
        for n in ("obs", "h1", "h2", "h4"):
            vals = {k: float(logged[f"val/skill/{m}/{k}/{n}"]) for k in ("mean", "ens", "best", "spread")}
            assert all(math.isfinite(v) for v in vals.values()) and max(vals["best"], vals["ens"]) <= vals["mean"] * (1.0 + 1e-6), (m, n, vals)
            np.testing.assert_allclose(vals["ens"] + vals["spread"], vals["mean"], rtol=1e-4, err_msg=f"{m} {n}")
        assert math.isnan(float(logged[f"val/skill/{m}/mean/h8"]))  # T = 6: no frame 8 steps past the context
    assert model.on_validation_epoch_end() == {}
