"""CPU: the forecast objective -- the rule's torch restatement on hand-built uniforms, the argument and
combination refusals, the model's noise shapes, and the new C-ABI entry (declared, bound, rejecting bad arguments without a launch).
Nothing here launches a kernel."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import Forecast, ModalityDropout, StateCarry, _lib
from multimodal_mtrssm_amd.dropout import ragged_reference
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.parallel import FlatDataParallel, GlobalRowNoise
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()
BELOW_ONE = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))  # the largest fp32 below 1.0


def centres(contexts: list[int], lo: int, hi: int) -> torch.Tensor:
    """Uniforms at the centres of the bins that give ``contexts``: ``u = (c - lo + 0.5) / n``."""
    n = hi - lo + 1
    return torch.tensor([(c - lo + 0.5) / n for c in contexts], dtype=torch.float32)


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


# -- the rule ---------------------------------------------------------------------------------------------------------------------
def test_context_lengths_from_bin_centres_and_the_top_clamp() -> None:
    t = 7
    fc = Forecast((2, 9))  # hi > T: rows with c_b >= 7 are plain closed-loop rows
    want = [2, 3, 4, 5, 6, 7, 8, 9]
    got = fc.reference(centres(want, 2, 9), t)
    assert got.context.tolist() == want and got.context.dtype == torch.int32
    assert got.observed.sum(dim=1).tolist() == [min(c, t) for c in want]
    assert bool(got.target.all()) and got.last.tolist() == [t - 1] * 8 and got.last.dtype == torch.int32
    for b, c in enumerate(want):
        assert got.codes[b].tolist() == [3] * min(c, t) + [0] * (t - min(c, t))
    assert got.counts.tolist() == [8.0 * t, float(sum(min(c, t) for c in want))]
    # the bin edges: u = k / n opens bin k; the fp32 value just below 1.0 lands in the top bin, never past it
    edges = fc.reference(torch.tensor([0.0, 0.125, 0.25, BELOW_ONE], dtype=torch.float32), t)
    assert edges.context.tolist() == [2, 3, 4, 9]
    for lo, hi in ((1, 3), (1, 6), (2, 50), (1, 1000), (7, (1 << 31) - 1)):
        top = Forecast((lo, hi)).reference(torch.tensor([BELOW_ONE, 0.0, 1.0]), t)  # (1.0 is no uniform of [0, 1): the clamp's case)
        assert top.context[1:].tolist() == [lo, hi] and hi - 128 <= int(top.context[0]) <= hi, (lo, hi)
        assert int(top.context[0]) == hi or hi > 1 << 24, (lo, hi)  # (the top bin itself while float(n) is exact)
    assert Forecast(4).reference(torch.tensor([0.0, 0.5, BELOW_ONE]), t).context.tolist() == [4, 4, 4]  # fixed: u is irrelevant


def test_lengths_cut_the_context_and_dead_steps_have_code_zero() -> None:
    t = 6
    fc = Forecast((1, 6))
    valid = torch.tensor([6, 4, 1, 0, 9, 2], dtype=torch.int32)  # (9 is clamped to the 6 steps)
    want = [3, 2, 1, 2, 6, 5]  # row 5: valid 2 < c_b 5
    got = fc.reference(centres(want, 1, 6), t, valid)
    live = ragged_reference(valid, None, t).live
    assert torch.equal(got.target, live) and got.last.tolist() == [5, 3, 0, -1, 5, 1]
    assert got.observed.sum(dim=1).tolist() == [3, 2, 1, 0, 6, 2]
    assert got.codes.tolist() == [[3, 3, 3, 0, 0, 0], [3, 3, 0, 0, 0, 0], [3, 0, 0, 0, 0, 0], [0] * 6, [3] * 6, [3, 3, 0, 0, 0, 0]]
    assert bool((got.codes[~got.observed] == 0).all())  # the tail and the dead steps
    assert got.counts.tolist() == [float(got.target.sum()), float(got.observed.sum())] == [19.0, 14.0]
    assert torch.equal(got.mask, torch.stack([got.observed, got.observed], dim=-1))


def test_dropout_fix_up_applies_inside_the_context() -> None:
    t = 6
    md = ModalityDropout(0.5, 0.5, span=2)
    u = torch.rand(md.noise_shape(4, t), generator=torch.Generator().manual_seed(3))
    u[0, 0] = torch.tensor([0.2, 0.1])  # both below p at t = 0: the fix-up gives row 0 audio
    u[1, 0] = torch.tensor([0.1, 0.2])  # ... and row 1 vision
    u[2] = 0.9  # nothing dropped
    u[3, 0] = torch.tensor([0.1, 0.2])  # a dead row: the fix-up is ANDed away
    valid = torch.tensor([6, 5, 6, 0], dtype=torch.int32)
    fc = Forecast((1, 6))
    got = fc.reference(centres([4, 1, 3, 2], 1, 6), t, valid, u, md)
    plain = md.reference(u, t)
    assert torch.equal(got.mask, plain & got.observed.unsqueeze(-1))
    assert got.codes[0, 0] == 1 and got.codes[1].tolist() == [2, 0, 0, 0, 0, 0] and got.codes[2].tolist() == [3, 3, 3, 0, 0, 0]
    assert not bool(got.codes[3].any()) and not bool(got.codes[0, 4:].any())
    # every live frame stays a target, dropped or not; the counts are plane sums and know nothing of the dropout
    assert got.target.sum(dim=1).tolist() == [6, 5, 6, 0]
    assert got.counts.tolist() == [float(got.target.sum()), float(got.observed.sum())] == [17.0, 8.0]
    assert bool((got.codes[0, :4] != 3).any())  # something inside the context is dropped
    with pytest.raises(ValueError, match="come together"):
        fc.reference(centres([4, 1, 3, 2], 1, 6), t, valid, u)
    with pytest.raises(ValueError, match="rows"):
        fc.reference(centres([4, 1, 3], 1, 6), t, None, u, md)


def test_a_context_of_the_whole_row_is_the_plain_step() -> None:
    b, t = 3, 5
    got = Forecast(t).reference(torch.rand(b, generator=torch.Generator().manual_seed(1)), t)
    assert bool((got.codes == 3).all()) and bool(got.target.all()) and bool(got.observed.all())
    assert got.counts.tolist() == [float(b * t)] * 2 and got.last.tolist() == [t - 1] * b
    # ... and with lengths, contexts that reach every row's end give the ragged rule
    valid = torch.tensor([5, 3, 1], dtype=torch.int32)
    rag = ragged_reference(valid, None, t)
    got = Forecast((1, 5)).reference(centres([5, 4, 1], 1, 5), t, valid)
    assert torch.equal(got.codes, rag.codes) and torch.equal(got.target, rag.live) and torch.equal(got.observed, rag.live)
    assert got.counts.tolist() == [float(rag.counts[2])] * 2 and torch.equal(got.last, rag.last)


# -- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", [0, -1, (0, 3), (4, 3), (1, 1 << 31), 2.0, (1.0, 3), True, (1, 2, 3), "3", None])
def test_forecast_rejects_bad_contexts(context) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="context"):
        Forecast(context)


def test_forecast_surface() -> None:
    fc = Forecast((2, 5))
    assert (fc.lo, fc.hi, fc.world, fc.rank, fc.fixed) == (2, 5, 1, 0, False) and Forecast(3).fixed
    assert repr(fc) == "Forecast((2, 5))" and repr(Forecast(3)) == "Forecast(3)" and Forecast([2, 5]).hi == 5  # noqa: PLR2004
    bound = fc.for_rank(4, 3)
    assert (bound.world, bound.rank, bound.lo, bound.hi) == (4, 3, 2, 5) and (fc.world, fc.rank) == (1, 0)
    assert fc.noise_shape(6) == (6,)
    for world, rank in ((0, 0), (2, 2), (2, -1)):
        with pytest.raises(ValueError, match="rank"):
            fc.for_rank(world, rank)
    with pytest.raises(ValueError, match="float32"):
        fc.reference(torch.zeros(3, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="float32"):
        fc.reference(torch.zeros(3, 1), 4)
    with pytest.raises(ValueError, match="steps"):
        fc.reference(torch.zeros(3), 0)
    with pytest.raises(ValueError, match="int32"):
        fc.reference(torch.zeros(3), 4, torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="rows"):
        fc.reference(torch.zeros(3), 4, torch.tensor([1, 2], dtype=torch.int32))
    with pytest.raises(ValueError, match="multiple of world"):
        fc.sample(torch.zeros(3), 4, world=2, rank=0)
    flat = type("Flat", (), {"param": torch.zeros(1)})()
    assert FlatDataParallel(flat).forecast(fc).world == 1


def test_step_refuses_a_mask_a_carry_and_unbound_uniforms(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool)
    fc = Forecast((1, case.steps))
    with pytest.raises(ValueError, match="already says what is seen"):
        model.shared_step(batch, modality_mask=mask, forecast=fc)
    with pytest.raises(ValueError, match="already says what is seen"):
        model.shared_step((*batch, mask), forecast=fc)
    with pytest.raises(ValueError, match="open-loop state"):
        model.shared_step(batch, forecast=fc, state_carry=StateCarry.for_model(model, case.batch), reset=torch.ones(case.batch, dtype=torch.bool))
    with pytest.raises(ValueError, match="Forecast"):
        model.shared_step(batch, forecast=3)
    with pytest.raises(ValueError, match="valid_global"):  # lengths= is one rank's own rows: a rank-bound forecast needs the batch's
        model.shared_step(batch, {"u_context": torch.rand(2 * case.batch)}, forecast=fc.for_rank(2, 0),
                          lengths=torch.full((case.batch,), case.steps, dtype=torch.int32))
    with pytest.raises(ValueError, match="u_context"):  # more than one rank: the uniforms of the GLOBAL batch must be given
        model.shared_step(batch, forecast=fc.for_rank(2, 0))
    with pytest.raises(ValueError, match="rows"):
        model.shared_step(batch, {"u_context": torch.rand(case.batch)}, forecast=fc.for_rank(2, 0))
    with pytest.raises(ValueError, match="bound to rank"):
        model.shared_step(batch, {"u_context": torch.rand(2 * case.batch)}, forecast=fc.for_rank(2, 0),
                          modality_dropout=ModalityDropout(0.3, 0.3).for_rank(2, 1))
    with pytest.raises(ValueError, match="u_mask"):
        model.shared_step(batch, {"u_context": torch.rand(2 * case.batch)}, forecast=fc.for_rank(2, 0),
                          modality_dropout=ModalityDropout(0.3, 0.3).for_rank(2, 0))
    with pytest.raises(ValueError, match="context"):
        model.forecast_rollout(actions=batch[0], observations=(batch[1], batch[2]), context=0, prev_state=None)
    with pytest.raises(TypeError, match="tuple"):
        model.forecast_rollout(actions=batch[0], observations=batch[1], context=2, prev_state=None)


def test_captured_step_refuses_masked_and_carry_with_forecast(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool)
    fc = Forecast((1, case.steps))
    with pytest.raises(ValueError, match="masked=True"):
        CapturedTrainStep(model, None, None, None, (*batch, mask), None, forecast=fc, masked=True)
    with pytest.raises(ValueError, match="open-loop state"):
        CapturedTrainStep(model, None, None, None, batch, None, forecast=fc, state_carry=StateCarry.for_model(model, case.batch))
    with pytest.raises(ValueError, match="Forecast"):
        CapturedTrainStep(model, None, None, None, batch, None, forecast=(1, 3))
    dp = type("DP", (), {"world": 1, "rank": 0})()
    with pytest.raises(ValueError, match="6-tuple"):
        CapturedTrainStep(model, None, None, dp, (*batch, mask), None, forecast=fc)


# -- model surface ----------------------------------------------------------------------------------------------------------------
def test_noise_shapes_gain_u_context_only_with_a_forecast(cpu_model) -> None:  # noqa: ANN001
    _, model = cpu_model
    assert model.forecast is None and model.val_forecast is None
    shapes = model.noise_shapes(6, 9)
    assert "u_context" not in shapes
    model.forecast = Forecast((2, 9))
    try:
        with_fc = model.noise_shapes(6, 9)
        model.modality_dropout = ModalityDropout(0.2, 0.2, span=4)
        with_both = model.noise_shapes(6, 9)
    finally:
        model.forecast = model.modality_dropout = None
    assert with_fc == {**shapes, "u_context": (6,)} and list(with_fc)[:-1] == list(shapes)
    assert with_both == {**shapes, "u_mask": (6, 3, 2), "u_context": (6,)}
    assert model.noise_shapes(6, 9) == shapes
    model.val_forecast = Forecast(3)  # validation only: the training step's uniforms are unchanged
    try:
        assert model.noise_shapes(6, 9) == shapes
    finally:
        model.val_forecast = None


def test_global_row_noise_keeps_u_context_whole_and_other_draws_as_before() -> None:
    shapes = {"u_init": (2, 3), "u_post": (2, 4, 3)}
    plain = GlobalRowNoise(5, 2, 1, "cpu").draw(shapes)
    ranks = [GlobalRowNoise(5, 2, r, "cpu").draw({**shapes, "u_context": (2,)}) for r in (0, 1)]
    assert tuple(ranks[0]["u_context"].shape) == (4,) and torch.equal(ranks[0]["u_context"], ranks[1]["u_context"])
    assert tuple(ranks[0]["u_post"].shape) == (2, 4, 3) and not torch.equal(ranks[0]["u_post"], ranks[1]["u_post"])
    whole = GlobalRowNoise(5, 1, 0, "cpu").draw({"u_init": (4, 3), "u_post": (4, 4, 3), "u_context": (4,)})  # the same job on one rank
    assert torch.equal(whole["u_context"], ranks[0]["u_context"])
    for k in shapes:
        assert torch.equal(torch.cat([ranks[0][k], ranks[1][k]]), whole[k]), k
    assert torch.equal(GlobalRowNoise(5, 2, 1, "cpu").draw(shapes)["u_post"], plain["u_post"])  # without the key: the draws of before


def test_training_and_validation_steps_pass_the_forecast_on(cpu_model, monkeypatch: pytest.MonkeyPatch) -> None:  # noqa: ANN001
    case, model = cpu_model
    seen = []
    monkeypatch.setattr(model, "shared_step", lambda batch, **kw: seen.append(kw) or {"loss": torch.zeros(()), "kl": torch.ones(())})
    model.forecast, model.val_forecast = Forecast((2, 4)), Forecast(3)
    try:
        train = model.training_step(build_batch(case))
        val = model.validation_step(build_batch(case))
    finally:
        model.forecast = model.val_forecast = None
    assert seen[0]["forecast"].hi == 4 and "forecast" not in seen[1] and seen[2] == {"forecast": seen[2]["forecast"]}  # noqa: PLR2004
    assert seen[2]["forecast"].fixed and set(train) == {"loss", "train/loss", "train/kl"}
    assert set(val) == {"val/loss", "val/kl", "val/forecast/loss", "val/forecast/kl"}
    seen.clear()
    assert set(model.validation_step(build_batch(case))) == {"val/loss", "val/kl"} and len(seen) == 1  # without: as before


# -- C-ABI ------------------------------------------------------------------------------------------------------------------------
def test_sampler_is_declared_exported_and_bound() -> None:
    lib = _lib.load()
    assert re.search(r"\bint mtrssm_step_mask_forecast\(", HEADER)
    assert "mtrssm_step_mask_forecast" in _lib.SYMBOLS and len(_lib.SYMBOLS["mtrssm_step_mask_forecast"][1]) == 21  # noqa: PLR2004
    assert lib.mtrssm_step_mask_forecast is not None
    nm = __import__("subprocess").run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mtrssm_step_mask_forecast\b", nm)


def test_sampler_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    call = lib.mtrssm_step_mask_forecast
    outs = (p,) * 8
    assert call(None, None, None, 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5, *outs, None) == -1 and b"step_mask_forecast: null" in lib.mtrssm_last_error()
    assert call(None, None, p, 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5, p, p, p, None, p, p, p, p, None) == -1  # no target plane
    assert call(None, None, p, 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5, *outs[:7], None, None) == -1  # no counts
    for args in [
        (None, None, p, 0, 7, 1, 0.0, 0.0, 1, 7, 0, 5),            # empty global batch
        (None, None, p, 5, 0, 1, 0.0, 0.0, 1, 7, 0, 5),            # no steps
        (None, None, p, 5, 7, 0, 0.0, 0.0, 1, 7, 0, 5),            # span 0
        (None, None, p, 5, 7, 1, 0.0, 0.0, 1, 7, 4, 2),            # the slice leaves the batch
        (None, None, p, 5, 7, 1, 0.0, 0.0, 1, 7, -1, 2),           # negative first row
        (None, None, p, 5, 7, 1, 0.0, 0.0, 0, 7, 0, 5),            # lo = 0: frame 0 must be observed
        (None, None, p, 5, 7, 1, 0.0, 0.0, 4, 3, 0, 5),            # hi < lo
        (None, None, p, 5, 7, 1, 0.0, 0.0, 1, 1 << 31, 0, 5),      # hi does not fit 31 bits
        (None, p, p, 5, 7, 1, 1.0, 0.0, 1, 7, 0, 5),               # p = 1 with dropout uniforms
        (None, p, p, 5, 7, 1, 0.0, float("nan"), 1, 7, 0, 5),
        (None, None, p, 1 << 20, 16, 1, 0.0, 0.0, 1, 7, 0, 5),     # 2^24 frames: the fp32 counts would stop being exact
        (None, C.c_void_p(68), p, 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5),  # u_mask is read as float2
        (C.c_void_p(66), None, p, 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5),  # valid is read as int32
        (None, None, C.c_void_p(66), 5, 7, 1, 0.0, 0.0, 1, 7, 0, 5),
    ]:
        assert call(*args, *outs, None) == -1, args
        assert b"step_mask_forecast" in lib.mtrssm_last_error()
