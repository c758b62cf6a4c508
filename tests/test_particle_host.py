"""CPU: the particle-filter likelihood -- the float64 rule against values written out by hand and against a
plain-Python loop, its reduction to the importance-weighted bound at ``threshold = 0``, the ancestors of equal and of collapsed
weights, ragged rows, the replay of given ancestors, the unbiasedness of the estimator, the configuration's refusals and uniforms, the
table, the non-GPU route of ``fold`` / ``gather`` and the argument refusals of the two C-ABI entries (which return before any launch).
Nothing here launches a kernel.  ``check_particle_refusals`` is shared with ``tests/test_particle_gpu.py``."""

from __future__ import annotations

import ctypes as C
import math

import pytest
import torch

from multimodal_mtrssm_amd import LikelihoodBound, ParticleFilter, ParticleTable, StateCarry, _lib
from multimodal_mtrssm_amd.particle import PLANES, TABLE_ROWS
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case
from tests.test_likelihood_host import HOST_B, HOST_EVENTS, HOST_S, HOST_T, HOST_VALID, bound_inputs


def uniforms(b: int, t: int, seed: int = 5) -> torch.Tensor:
    return torch.rand(b, t, generator=torch.Generator().manual_seed(seed))


def brute_force(ratio: torch.Tensor, valid, u: torch.Tensor, c: int, threshold: float):  # noqa: ANN001, ANN201
    """The rule in plain Python floats, one row and one frame at a time (latent term only): planes ``[8, B, T]`` and ancestors."""
    b_, s_, t_ = ratio.shape
    segs = list(range(0, t_, c))
    out = torch.zeros(8, b_, t_, dtype=torch.float64)
    anc = torch.arange(s_, dtype=torch.int32).reshape(1, s_, 1).repeat(b_, 1, len(segs))
    for b in range(b_):
        n = t_ if valid is None else max(0, int(valid[b]))
        lw, base, prev = [0.0] * s_, 0.0, 0.0
        for t in range(min(n, t_)):
            l = [float(ratio[b, s, t]) for s in range(s_)]
            lw = [x + y for x, y in zip(lw, l, strict=True)]
            top = max(lw)
            w = [math.exp(x - top) for x in lw]
            sum_w = 0.0
            for x in w:
                sum_w += x
            now = base + (top + math.log(sum_w)) - math.log(s_)
            ess = sum_w * sum_w / sum(x * x for x in w)
            out[0, b, t], out[1, b, t], out[4, b, t], out[5, b, t], out[7, b, t] = now - prev, sum(l) / s_, sum(l) / s_, ess, now
            prev = now
            if (t + 1) % c == 0 and t + 1 < t_ and t + 1 < n and ess <= threshold * s_:
                out[6, b, t] = 1.0
                prefix, run = [], 0.0
                for x in w:
                    run += x
                    prefix.append(run)
                for i in range(s_):
                    target = ((float(u[b, t]) + i) / s_) * sum_w
                    anc[b, i, t // c] = min(s_ - 1, sum(1 for x in prefix if x <= target))
                base, lw = now, [0.0] * s_
    return out, anc


# -- 1. the rule ---------------------------------------------------------------------------------------------------------------------------
def test_the_rule_by_hand() -> None:
    """``S = 2, T = 3, c = 1``, always resampling; the per-frame weights are (1, 3), (2, 2), (4, 1), so ``Z = 2 * 2 * 2.5``."""
    ratio = torch.tensor([[[1.0, 2.0, 4.0], [3.0, 2.0, 1.0]]], dtype=torch.float64).log()  # (float64: the logs are exact to 1e-16)
    u = torch.tensor([[0.9, 0.25, 0.5]])
    planes, anc, margin = ParticleFilter.reference(None, None, ratio, resample_every=1, threshold=1.0, u_resample=u)
    assert planes.dtype == torch.float64 and tuple(planes.shape) == (8, 1, 3) and anc.dtype == torch.int32 and tuple(anc.shape) == (1, 2, 3)
    ln = math.log
    want = {
        "smc": [ln(2.0), ln(2.0), ln(2.5)],
        "mean": [ln(3.0) / 2, ln(2.0), ln(4.0) / 2],
        "audio": [0.0] * 3,
        "vision": [0.0] * 3,
        "latent": [ln(3.0) / 2, ln(2.0), ln(4.0) / 2],
        "ess": [16.0 / 10.0, 2.0, 25.0 / 17.0],
        "resampled": [1.0, 1.0, 0.0],
        "smc_prefix": [ln(2.0), ln(4.0), ln(10.0)],
    }
    for p, name in enumerate(PLANES):
        torch.testing.assert_close(planes[p, 0], torch.tensor(want[name], dtype=torch.float64), rtol=0, atol=1e-12, msg=name)
    # frame 0: w = (1/3, 1), c = (1/3, 4/3), targets (0.45, 0.95) * 4/3 = (0.6, 1.2667): both take slot 1.  frame 1: w = (1, 1),
    # c = (1, 2), targets (0.25, 1.25): the identity.  frame 2 ends the last segment: never resampled
    assert anc[0].tolist() == [[1, 0, 0], [1, 1, 1]]
    assert margin == pytest.approx(min(0.6 - 1 / 3, 4 / 3 - 0.95 * 4 / 3) / (4 / 3), rel=1e-6)  # (u is fp32: 0.9 is not exact)


@pytest.mark.parametrize("c", [1, 2, 3, HOST_T])
@pytest.mark.parametrize("threshold", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("s", [1, 2, 5, 16])
def test_reference_equals_the_brute_force_loop(s: int, threshold: float, c: int) -> None:
    for kind in ("normal", "wide", "equal"):
        ratio = bound_inputs(s, kind)[2] * 3.0
        for valid in (torch.tensor(HOST_VALID, dtype=torch.int32), None):
            u = uniforms(HOST_B, HOST_T)
            got, anc, margin = ParticleFilter.reference(None, None, ratio, valid, resample_every=c, threshold=threshold, u_resample=u)
            want, want_anc = brute_force(ratio, valid, u, c, threshold)
            assert margin >= 1e-9, (s, kind, margin)  # noqa: PLR2004
            torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)
            assert torch.equal(anc, want_anc), (s, kind, c, threshold)
            assert torch.equal(got[6], want[6])


@pytest.mark.parametrize("kind", ["normal", "wide", "equal"])
@pytest.mark.parametrize("s", HOST_S)
def test_threshold_zero_is_the_importance_weighted_bound(s: int, kind: str) -> None:
    inputs = bound_inputs(s, kind)
    for valid in (torch.tensor(HOST_VALID, dtype=torch.int32), None):
        want = LikelihoodBound.reference(*inputs, valid, *HOST_EVENTS)
        for c in (1, 2, HOST_T):
            got, anc, margin = ParticleFilter.reference(*inputs, valid, *HOST_EVENTS, resample_every=c, threshold=0.0)
            assert margin == math.inf and not bool(got[6].any())
            assert torch.equal(anc, torch.arange(s, dtype=torch.int32).reshape(1, s, 1).expand_as(anc))
            for mine, theirs in ((0, 0), (2, 2), (3, 3), (4, 4), (5, 5), (7, 6)):  # the same arithmetic in the same order
                assert torch.equal(got[mine], want[theirs]), (s, kind, c, mine)
            # plane 1 is the mean of the frame's l, the bound's elbo the difference of two running means: equal up to their rounding
            torch.testing.assert_close(got[1], want[1], rtol=0, atol=1e-12 * float(want[7].abs().max()))


def test_one_particle_has_smc_equal_to_mean() -> None:
    inputs = bound_inputs(1, "normal")
    got, _, _ = ParticleFilter.reference(*inputs, None, *HOST_EVENTS, resample_every=2, threshold=1.0, u_resample=uniforms(HOST_B, HOST_T))
    torch.testing.assert_close(got[0], got[1], rtol=0, atol=1e-12 * float(got[7].abs().max()))
    assert bool((got[5] == 1.0).all()) and got[6, :, 1].tolist() == [1.0] * HOST_B  # ess = 1 <= 1 * S: resampled, onto itself


# -- 2. ancestors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 5, 16])
def test_equal_weights_give_identity_ancestors(s: int) -> None:
    ratio = bound_inputs(s, "equal")[2]
    got, anc, margin = ParticleFilter.reference(None, None, ratio, resample_every=1, threshold=1.0, u_resample=uniforms(HOST_B, HOST_T))
    assert bool((got[6, :, :-1] == 1.0).all()) and not bool(got[6, :, -1].any())  # ess = S <= S: every segment but the last
    assert torch.equal(anc, torch.arange(s, dtype=torch.int32).reshape(1, s, 1).expand_as(anc))
    assert margin >= 1e-9  # noqa: PLR2004


@pytest.mark.parametrize("s", [2, 5, 16])
def test_a_collapsed_row_takes_every_ancestor_from_the_best_slot(s: int) -> None:
    g = torch.Generator().manual_seed(s)
    ratio = torch.rand(4, s, 3, generator=g)
    best = torch.tensor([0, s - 1, s // 2, 1])
    ratio[torch.arange(4), best, 0] += 50.0  # a spread of 50 nats: the others weigh e^-50
    got, anc, _ = ParticleFilter.reference(None, None, ratio, resample_every=1, threshold=0.5, u_resample=uniforms(4, 3))
    assert got[6, :, 0].tolist() == [1.0] * 4 and bool((got[5, :, 0] < 1.0 + 1e-9).all())  # noqa: PLR2004
    assert torch.equal(anc[:, :, 0], best.to(torch.int32).reshape(4, 1).expand(4, s))


def test_ragged_rows_never_resample_at_their_end_and_dead_frames_are_zero() -> None:
    s, t = 4, 8
    ratio = bound_inputs(s, "wide", b=6, t=t)[2]
    valid = torch.tensor([8, 5, 4, 1, 0, 11], dtype=torch.int32)
    for c in (1, 2, 4):
        got, anc, _ = ParticleFilter.reference(None, None, ratio, valid, resample_every=c, threshold=1.0, u_resample=uniforms(6, t))
        live = torch.arange(t) < valid[:, None]
        assert not bool(got[:, ~live].any())
        for b in range(6):
            for j, t0 in enumerate(range(0, t, c)):
                end = t0 + c - 1
                may = end + 1 < t and end + 1 < int(valid[b])
                assert float(got[6, b, min(end, t - 1)]) == float(may), (c, b, j)
                if not may:
                    assert anc[b, :, j].tolist() == list(range(s)), (c, b, j)
        assert not bool(got[6, torch.arange(6), (valid.clamp(1, t) - 1).long()].any())  # nothing at a row's last live frame


def test_ancestors_replay() -> None:
    inputs = bound_inputs(5, "normal")
    u = uniforms(HOST_B, HOST_T)
    planes, anc, margin = ParticleFilter.reference(*inputs, None, *HOST_EVENTS, resample_every=2, threshold=1.0, u_resample=u)
    assert margin < math.inf and bool(planes[6].any())
    given = anc.flip(1)
    again, back, none = ParticleFilter.reference(*inputs, None, *HOST_EVENTS, resample_every=2, threshold=1.0, ancestors=given)
    assert torch.equal(again, planes) and torch.equal(back, given) and none == math.inf  # the inputs are the slots', as given
    with pytest.raises(ValueError, match="ancestors"):
        ParticleFilter.reference(*inputs, None, *HOST_EVENTS, resample_every=2, threshold=1.0, ancestors=given[:, :, :1])


def test_the_estimator_is_unbiased() -> None:
    """``l ~ N(0, 0.25^2)`` i.i.d.: ``E exp(l) = exp(0.25^2 / 2)`` per frame, and ``E Z = exp(T 0.25^2 / 2)`` whatever is resampled."""
    n, s, t, sigma = 20_000, 4, 8, 0.25
    g = torch.Generator().manual_seed(2024)
    ratio = (torch.randn(n, s, t, generator=g, dtype=torch.float64) * sigma).to(torch.float32)
    u = torch.rand(n, t, generator=g)
    planes, _, margin = ParticleFilter.reference(None, None, ratio, resample_every=1, threshold=1.0, u_resample=u)
    assert bool((planes[6, :, :-1] == 1.0).all()) and margin >= 0.0
    z = torch.exp(planes[7, :, t - 1])
    mean, stderr, want = float(z.mean()), float(z.std() / math.sqrt(n)), math.exp(t * sigma * sigma / 2.0)
    print("Z mean", mean, "want", want, "standard error", stderr)
    assert abs(mean - want) <= 5.0 * stderr
    assert float(planes[7, :, t - 1].mean()) < math.log(want)  # log Z is a lower bound in expectation


# -- 3. the configuration and the table -----------------------------------------------------------------------------------------------------
def test_config_validation() -> None:
    pf = ParticleFilter(4)
    assert (pf.samples, pf.resample_every, pf.threshold, pf.observe, pf.score, pf.latent, pf.max_frames) == (4, 1, 0.5, "both", ("audio", "vision"),
                                                                                                             True, 4096)
    assert "resample_every=1" in repr(pf) and pf.group is None and pf.segments(5) == [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]
    assert ParticleFilter(2, 3, 1, "audio", ("vision",), False).segments(7) == [(0, 3), (3, 6), (6, 7)]  # noqa: FBT003
    for bad in (0, 17, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="samples"):
            ParticleFilter(bad)
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="resample_every"):
            ParticleFilter(2, bad)
    for bad in (-0.1, 1.5, float("nan"), "1", None, True):
        with pytest.raises(ValueError, match="threshold"):
            ParticleFilter(2, 1, bad)
    with pytest.raises(ValueError, match="observe"):
        ParticleFilter(2, observe="all")
    with pytest.raises(ValueError, match="score"):
        ParticleFilter(2, score="audio")
    with pytest.raises(ValueError, match="nothing to score"):
        ParticleFilter(2, score=(), latent=False)
    plan = pf.plan()
    assert (plan.copies, plan.bits, plan.context, plan.init, plan.post, plan.order) == (4, 3, None, "copy", "copy", "row")
    bound = pf.for_group("g")
    assert bound is not pf and bound.group == "g" and pf.group is None and bound.resample_every == 1


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


def test_noise_shapes_put_the_batch_first(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    pf = ParticleFilter(3, 2)
    shapes = pf.noise_shapes(model, 5, 7)
    assert shapes == LikelihoodBound(3).noise_shapes(model, 5, 7) | {"u_resample": (5, 7)}
    assert all(shape[0] == 5 for shape in shapes.values())
    d = case.dims
    if case.kind == "mrssm":
        assert shapes == {"u_init": (5, 3, d.cats), "u_post": (5, 3, 7, d.cats), "u_resample": (5, 7)}


def test_particle_step_refuses_masked_batches_and_a_set_carry(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    b, t = batch[0].shape[:2]
    pf = ParticleFilter(2)
    with pytest.raises(ValueError, match="masked"):
        model.particle_filter((*batch, torch.ones(b, t, 2, dtype=torch.bool)), pf)
    with pytest.raises(ValueError, match="must be a ParticleFilter"):
        model.particle_filter(batch, LikelihoodBound(2))
    with pytest.raises(ValueError, match="ParticleTable"):
        model.particle_filter(batch, pf, table=ParticleTable(t + 1))
    model.state_carry = StateCarry.for_model(model, b, "cpu")
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.particle_filter(batch, pf)
    finally:
        model.state_carry = None
    assert model.val_particle is None and model.particle_table is None


def test_table_folds_by_frame_position() -> None:
    s = 4
    inputs = bound_inputs(s, "normal")
    valid = torch.tensor(HOST_VALID, dtype=torch.int32)
    planes, _, _ = ParticleFilter.reference(*inputs, valid, *HOST_EVENTS, resample_every=2, threshold=1.0, u_resample=uniforms(HOST_B, HOST_T))
    planes = planes.to(torch.float32)
    table = ParticleTable(HOST_T)
    assert tuple(table.buffer.shape) == (8, HOST_T) and ParticleTable.ROWS == 7 == len(TABLE_ROWS) and table.ancestors is None and table.inputs is None  # noqa: PLR2004
    assert table.fold(planes, valid) is table
    live = torch.arange(HOST_T) < valid[:, None]
    assert torch.equal(table.counts, live.sum(0).float())
    torch.testing.assert_close(table.sums, planes[:7].sum(1), rtol=1e-6, atol=1e-6)
    curves, per, scalars = table.curves(), table.per_frame(), table.scalars("val/smc")
    assert list(curves) == list(per) == list(TABLE_ROWS) == ["smc", "mean", "audio", "vision", "latent", "ess", "resampled"]
    assert set(scalars) == {f"val/smc/{k}" for k in TABLE_ROWS}
    assert bool(torch.isnan(curves["smc"][int(valid.max()) :]).all()) and bool(torch.isfinite(curves["smc"][: int(valid.max())]).all())
    torch.testing.assert_close(per["smc"], planes[0].sum() / live.sum(), rtol=1e-5, atol=0)
    assert 0.0 < float(per["resampled"]) < 1.0 and float(per["smc"]) >= float(per["mean"])
    assert bool(torch.isnan(ParticleTable(3).per_frame()["ess"]))
    with pytest.raises(ValueError, match="planes"):
        table.fold(planes[:6], valid)
    table.add(ParticleTable(HOST_T).fold(planes, valid))
    assert torch.equal(table.counts, 2.0 * live.sum(0).float())


# -- 4. the non-GPU route of fold / gather and the refusals -----------------------------------------------------------------------------------
def test_cpu_route_of_fold_chains_the_carry_into_the_reference() -> None:
    s, c = 5, 3
    inputs = bound_inputs(s, "normal")
    valid, u = torch.tensor(HOST_VALID, dtype=torch.int32), uniforms(HOST_B, HOST_T)
    want, want_anc, _ = ParticleFilter.reference(*inputs, valid, *HOST_EVENTS, resample_every=c, threshold=1.0, u_resample=u)
    carry = ParticleFilter.new_carry(HOST_B, s)
    assert carry.dtype == torch.float64 and tuple(carry.shape) == (HOST_B, s + 2) and not bool(carry.any())
    for j, t0 in enumerate(range(0, HOST_T, c)):
        t1 = min(HOST_T, t0 + c)
        last = t1 == HOST_T
        planes, anc = ParticleFilter.fold(*(x[:, :, t0:t1] for x in inputs), valid, None if last else u[:, t1 - 1], t0, 1.0, last, carry, *HOST_EVENTS)
        assert planes.dtype == torch.float32 and anc.dtype == torch.int32
        assert torch.equal(planes, want[:, :, t0:t1].to(torch.float32)) and torch.equal(anc, want_anc[:, :, j])
    torch.testing.assert_close(carry[:, s + 1], want[7][torch.arange(HOST_B), (valid.clamp(1, HOST_T) - 1).long()] * (valid > 0), rtol=0, atol=0)


def test_cpu_route_of_gather_is_index_select() -> None:
    b, s, steps = 3, 4, 2
    g = torch.Generator().manual_seed(1)
    last = [torch.randn(b * s, steps, w, generator=g) for w in (3, 8)]
    anc = torch.randint(0, s, (b, s), generator=g).to(torch.int32)
    got = ParticleFilter.gather(last, anc)
    rows = (torch.arange(b)[:, None] * s + anc.long()).reshape(-1)
    for x, y in zip(last, got, strict=True):
        assert torch.equal(y, x[:, -1].index_select(0, rows))


def test_python_entries_refuse_bad_arguments() -> None:
    s = 4
    inputs = bound_inputs(s, "normal")
    carry = ParticleFilter.new_carry(HOST_B, s)
    u = uniforms(HOST_B, HOST_T)[:, 0]
    with pytest.raises(ValueError, match="at least one"):
        ParticleFilter.fold(None, None, None, None, u, 0, 0.5, False, carry)  # noqa: FBT003
    with pytest.raises(ValueError, match="threshold"):
        ParticleFilter.fold(*inputs, None, u, 0, 1.5, False, carry, *HOST_EVENTS)  # noqa: FBT003
    with pytest.raises(ValueError, match="carry"):
        ParticleFilter.fold(*inputs, None, u, 0, 0.5, False, carry.float(), *HOST_EVENTS)  # noqa: FBT003
    with pytest.raises(ValueError, match="carry"):
        ParticleFilter.fold(*inputs, None, u, 0, 0.5, False, carry[:, :-1], *HOST_EVENTS)  # noqa: FBT003
    with pytest.raises(ValueError, match="uniforms"):
        ParticleFilter.fold(*inputs, None, None, 0, 0.5, False, carry, *HOST_EVENTS)  # noqa: FBT003
    with pytest.raises(ValueError, match="frames"):
        ParticleFilter.fold(*inputs, None, u, -1, 0.5, False, carry, *HOST_EVENTS)  # noqa: FBT003
    with pytest.raises(ValueError, match="planes"):
        ParticleFilter.fold(*inputs, None, u, 0, 0.5, False, carry, *HOST_EVENTS, planes=torch.empty(8, HOST_B, HOST_T + 1))  # noqa: FBT003
    with pytest.raises(ValueError, match="ancestor"):
        ParticleFilter.fold(*inputs, None, u, 0, 0.5, False, carry, *HOST_EVENTS, ancestor=torch.empty(HOST_B, s, dtype=torch.int64))  # noqa: FBT003
    with pytest.raises(ValueError, match="u_resample"):
        ParticleFilter.reference(*inputs, None, *HOST_EVENTS, resample_every=1, threshold=0.5)
    last = [torch.zeros(HOST_B * s, 2, 3)]
    with pytest.raises(ValueError, match="ancestor"):
        ParticleFilter.gather(last, torch.zeros(HOST_B, s, dtype=torch.int64))
    with pytest.raises(ValueError, match="scan output"):
        ParticleFilter.gather(last, torch.zeros(HOST_B + 1, s, dtype=torch.int32))
    with pytest.raises(ValueError, match="state table"):
        ParticleFilter.gather(last * 7, torch.zeros(HOST_B, s, dtype=torch.int32))
    with pytest.raises(ValueError, match="out"):
        ParticleFilter.gather(last, torch.zeros(HOST_B, s, dtype=torch.int32), out=[torch.zeros(HOST_B * s, 4)])


def check_particle_refusals(lib) -> None:  # noqa: ANN001
    """Every refusal of the two C entries returns -1 before a launch, so the pointers are never read: any non-null address serves
    (64 is 16-byte aligned)."""
    p, no = 64, None
    fold, gather = lib.mtrssm_particle_fold, lib.mtrssm_particle_gather

    def f(**kw):  # noqa: ANN003, ANN202
        a = {"se_audio": p, "se_vision": p, "log_ratio": p, "valid": p, "u": p, "u_stride": 7, "t0": 0, "B": 3, "S": 4, "c": 2, "E_a": 96, "E_v": 40,
             "threshold": 0.5, "last": 0, "carry": p, "planes": p, "ancestor": p} | kw
        return fold(a["se_audio"], a["se_vision"], a["log_ratio"], a["valid"], a["u"], a["u_stride"], a["t0"], a["B"], a["S"], a["c"], a["E_a"],
                    a["E_v"], a["threshold"], a["last"], a["carry"], a["planes"], a["ancestor"], None)

    bad = [{"carry": no}, {"planes": no}, {"ancestor": no}, {"se_audio": no, "se_vision": no, "log_ratio": no}, {"u": no}, {"u_stride": 0},
           {"B": 0}, {"c": 0}, {"t0": -1}, {"E_a": 0}, {"E_v": -1}, {"S": 0}, {"S": 17}, {"threshold": -0.01}, {"threshold": 1.01},
           {"threshold": float("nan")}, {"last": 2}, {"last": -1}, {"B": 1 << 24}, {"B": 1 << 12, "c": 1 << 12}, {"t0": 1 << 30}, {"planes": 66},
           {"carry": 68}, {"valid": 65}, {"u": 62}]
    for kw in bad:
        assert f(**kw) == -1, kw
        assert lib.mtrssm_last_error(), kw

    def table(count: int = 2, width: int = 4, src: int | None = p, dst: int | None = 128):  # noqa: ANN202
        t = _lib.StateTable()
        t.count = count
        for k in range(max(0, min(count, _lib.STATE_MAX))):
            t.width[k], t.src[k], t.dst[k] = width, src, dst
        return t

    anc = p
    assert gather(None, anc, 3, 4, 2, None) == -1
    assert gather(C.byref(table()), None, 3, 4, 2, None) == -1
    assert gather(C.byref(table()), 66, 3, 4, 2, None) == -1  # a misaligned ancestor
    for kw in ({"count": 0}, {"count": 7}, {"width": 0}, {"src": None}, {"dst": None}, {"src": 128}, {"src": 66}, {"dst": 130}):
        assert gather(C.byref(table(**kw)), anc, 3, 4, 2, None) == -1, kw
    for b, s, steps in ((0, 4, 2), (3, 0, 2), (3, 17, 2), (3, 4, 0), (1 << 20, 16, 1 << 10)):
        assert gather(C.byref(table()), anc, b, s, steps, None) == -1, (b, s, steps)


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_particle_refusals(_lib.load())
