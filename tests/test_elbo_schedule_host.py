"""CPU: the ELBO schedule -- validation, the rule's torch statement on hand-made planes, the neutral schedule
against the plain eager epilogue, beta over the warm-up, the train / validation surface, ``bind`` as a view, and the new C-ABI pair
(declared, bound, rejecting bad arguments without a launch).  Nothing here launches a kernel."""

from __future__ import annotations

import math

import pytest
import torch

from multimodal_mtrssm_amd import ElboSchedule, Forecast, _lib
from multimodal_mtrssm_amd.core import _elbo
from multimodal_mtrssm_amd.dropout import StepMask
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

F32 = torch.float32


def f32(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=F32)


def below(x: float) -> float:
    return float(torch.nextafter(f32(x), f32(-math.inf)))


def _counted(live: torch.Tensor, count: float) -> StepMask:
    z = torch.zeros(1)
    return StepMask(z, z, z, z, z, z, live=live, count_live=f32(count))


# -- validation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kwargs", [
    {"free_nats": -0.1}, {"free_nats": math.inf}, {"free_nats": math.nan}, {"free_nats_h": -1.0}, {"free_nats_h": math.nan}, {"free_nats": "1"},
    {"beta_start": -0.01}, {"beta_start": 1.01}, {"beta_start": math.nan},
    {"warmup_steps": -1}, {"warmup_steps": 2.0}, {"warmup_steps": True}, {"warmup_steps": 1 << 24},
    {"recon_weights": (1.0, -1.0)}, {"recon_weights": (math.inf, 1.0)}, {"recon_weights": (math.nan, 1.0)}, {"recon_weights": (1.0,)}, {"recon_weights": 1.0},
])
def test_invalid_schedules_are_refused(kwargs: dict) -> None:
    with pytest.raises(ValueError):  # noqa: PT011
        ElboSchedule(**kwargs)


def test_valid_edges_and_the_missing_step() -> None:
    s = ElboSchedule(free_nats=0.0, free_nats_h=3.5, beta_start=0.0, warmup_steps=(1 << 24) - 1, recon_weights=(0.0, 2.0))
    assert (s.free_nats_h, s.beta_start, s.warmup_steps, s.recon_weights) == (3.5, 0.0, (1 << 24) - 1, (0.0, 2.0))
    with pytest.raises(ValueError, match="bind"):  # a warm-up without bind / set_step
        s.reference(f32(1.0), f32(1.0), torch.ones(4), 1.0)
    with pytest.raises(ValueError, match="bind"):
        _elbo(f32(1.0), f32(1.0), torch.ones(4), 1.0, schedule=s)
    with pytest.raises(ValueError, match="2\\^24"):
        s.set_step(-1)
    with pytest.raises(ValueError, match="FlatAdamW"):
        s.bind(object())
    with pytest.raises(ValueError, match="ElboSchedule"):
        _elbo(f32(1.0), f32(1.0), torch.ones(4), 1.0, schedule="free bits")
    assert ElboSchedule().reference(f32(1.0), f32(2.0), torch.ones(4), 1.0).beta.item() == 1.0  # no warm-up: no step needed


# -- the rule on hand-made planes ---------------------------------------------------------------------------------------------------
def test_rule_on_hand_made_planes() -> None:
    """free = 0.7: entry 0 far above, 1 exactly at the threshold (passes), 2 one ulp below it (clipped), 3 far below, 4 dead but above
    the threshold (no sum, no gradient), 5 live and above.  Four live entries counted as ``count = 4`` (entry 2 of the higher plane
    is at ITS threshold)."""
    free, free_h = 0.7, 0.25
    kl0 = torch.tensor([2.0, free, below(free), 0.1, 5.0, 1.5], dtype=F32, requires_grad=True)
    kl1 = torch.tensor([0.5, 0.1, free_h, 0.0, 9.0, below(free_h)], dtype=F32, requires_grad=True)
    live = torch.tensor([1.0, 1.0, 1.0, 1.0, 0.0, 1.0])
    a, v = f32(3.0).requires_grad_(), f32(4.0).requires_grad_()
    s = ElboSchedule(free, free_h, beta_start=0.5, warmup_steps=4, recon_weights=(0.5, 2.0)).set_step(2)
    c0, c1 = 0.8, 0.8 * 0.5
    t = s.reference(a, v, kl0, c0, kl1, c1, live, f32(5.0))
    assert t.beta.item() == 0.75
    assert t.recon.item() == 0.5 * 3.0 + 2.0 * 4.0
    f = float(f32(free))
    fh = float(f32(free_h))
    want0 = (2.0 + f + f + f + 1.5) / 5.0 * float(f32(c0)) * 0.75
    want1 = (0.5 + fh + fh + fh + fh) / 5.0 * float(f32(c1)) * 0.75
    assert t.k0.item() == pytest.approx(want0, rel=1e-6) and t.k1.item() == pytest.approx(want1, rel=1e-6)
    assert t.loss.item() == pytest.approx(9.5 + want0 + want1, rel=1e-6)
    assert t.raw0.item() == pytest.approx((2.0 + f + below(free) + 0.1 + 1.5) / 5.0 * float(f32(c0)), rel=1e-6)
    assert t.raw1.item() == pytest.approx((0.5 + 0.1 + fh + 0.0 + below(free_h)) / 5.0 * float(f32(c1)), rel=1e-6)
    assert t.active0.item() == pytest.approx(3 / 5) and t.active1.item() == pytest.approx(2 / 5)
    assert not any(x.requires_grad for x in (t.beta, t.raw0, t.raw1, t.active0, t.active1))
    t.loss.backward()
    g0 = float(f32(1.0) * f32(c0) * f32(0.75) / f32(5.0))
    g1 = float(f32(1.0) * f32(c1) * f32(0.75) / f32(5.0))
    assert kl0.grad.tolist() == [g0, g0, 0.0, 0.0, 0.0, g0]  # the tie passes, one ulp below does not, the dead step gets 0
    assert kl1.grad.tolist() == [g1, 0.0, g1, 0.0, 0.0, 0.0]
    assert a.grad.item() == 0.5 and v.grad.item() == 2.0
    # gradients of the separate terms: g_recon reaches the NLLs only, g_k0 its own plane only
    kl0.grad = kl1.grad = a.grad = v.grad = None
    t = s.reference(a, v, kl0, c0, kl1, c1, live, f32(5.0))
    (3.0 * t.recon + 2.0 * t.k0).backward()
    g0 = float(f32(2.0) * f32(c0) * f32(0.75) / f32(5.0))
    assert kl0.grad.tolist() == [g0, g0, 0.0, 0.0, 0.0, g0] and not bool(kl1.grad.any()) and a.grad.item() == 1.5 and v.grad.item() == 6.0


def test_torch_where_and_clamp_pass_the_gradient_at_the_tie() -> None:
    """What the rule's tie is modelled on."""
    for clip in (lambda x: torch.where(x < 0.7, f32(0.7), x), lambda x: torch.clamp(x, min=0.7)):
        x = torch.tensor([0.7, below(0.7)], dtype=F32, requires_grad=True)
        clip(x).sum().backward()
        assert x.grad.tolist() == [1.0, 0.0]


def test_count_zero_gives_zero_terms_and_explicit_zero_gradients() -> None:
    kl0 = torch.tensor([2.0, 3.0], requires_grad=True)
    a, v = f32(3.0).requires_grad_(), f32(4.0).requires_grad_()
    t = ElboSchedule(0.5).reference(a, v, kl0, 1.0, None, 0.0, torch.zeros(2), f32(0.0))
    assert [x.item() for x in (t.k0, t.k1, t.raw0, t.active0, t.loss)] == [0.0, 0.0, 0.0, 0.0, 7.0]
    t.loss.backward()
    assert kl0.grad.tolist() == [0.0, 0.0] and a.grad.item() == 1.0
    nan = ElboSchedule(0.5).reference(a, v, torch.tensor([math.nan, 1.0]), 1.0)  # a NaN stays a NaN
    assert math.isnan(nan.k0.item()) and math.isnan(nan.loss.item())


# -- the neutral schedule is the plain epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("counted", [False, True], ids=["plain", "counted"])
@pytest.mark.parametrize("two", [False, True], ids=["kl", "kl+kl_h"])
def test_neutral_schedule_equals_no_schedule_exactly(two: bool, counted: bool) -> None:  # noqa: FBT001
    n = 257
    results = []
    for schedule in (None, ElboSchedule()):
        kl0 = torch.rand(n, generator=torch.Generator().manual_seed(4)).mul(3.0).reshape(1, n).requires_grad_()
        kl1 = torch.rand(n, generator=torch.Generator().manual_seed(5)).reshape(1, n).requires_grad_() if two else None
        a, v = f32(1234.567).requires_grad_(), f32(4321.125).requires_grad_()
        live = (torch.rand(n, generator=torch.Generator().manual_seed(6)) < 0.7).float()
        sm = _counted(live, float(live.sum())) if counted else None
        out = _elbo(a, v, kl0, 0.8, kl1, 0.8 * 0.3, step_mask=sm, schedule=schedule)
        out[3].backward()
        results.append(([x.detach().clone() for x in out], [x.grad.clone() for x in (a, v, kl0, *([kl1] if two else []))]))
    for got, want in zip(results[1][0], results[0][0], strict=True):
        assert torch.equal(got, want), (got, want)
    for got, want in zip(results[1][1], results[0][1], strict=True):
        assert torch.equal(got, want)
    assert float(results[0][0][1]) > 0.0


# -- beta over the warm-up -----------------------------------------------------------------------------------------------------------
def test_beta_is_the_closed_form_and_saturates_at_exactly_one() -> None:
    s = ElboSchedule(beta_start=0.25, warmup_steps=5)
    got = []
    for k in range(8):
        s.set_step(k)
        got.append(s.reference(f32(0.0), f32(0.0), torch.ones(3), 1.0).beta)
    want = [f32(0.25) + (f32(1.0) - f32(0.25)) * torch.clamp(f32(float(k)) / f32(5.0), max=1.0) for k in range(8)]
    assert all(torch.equal(g, w) for g, w in zip(got, want, strict=True))
    assert [float(b) for b in got[5:]] == [1.0, 1.0, 1.0] and float(got[0]) == 0.25 and all(float(x) < float(y) for x, y in zip(got[:5], got[1:6], strict=True))
    assert [float(b) for b in got[:5]] == pytest.approx([0.25 + 0.75 * k / 5 for k in range(5)], rel=1e-6)
    k0 = s.set_step(2).reference(f32(0.0), f32(0.0), torch.full((3,), 2.0), 0.5).k0
    assert torch.equal(k0, f32(6.0) / f32(3.0) * f32(0.5) * got[2])  # s / N * c * beta, each rounded on its own
    assert s.stats == {}  # (reference alone records nothing; _elbo does)
    _elbo(f32(0.0), f32(0.0), torch.full((3,), 2.0), 0.5, schedule=s)
    assert set(s.stats) == {"beta", "active", "kl_raw"} and torch.equal(s.stats["beta"], got[2]) and float(s.stats["kl_raw"]) == 1.0


# -- the model's surface ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_default"])
def test_training_step_uses_the_schedule_and_validation_step_ignores_it(name: str, monkeypatch: pytest.MonkeyPatch) -> None:
    case = CASES[name]
    model = product_from_case(case, build_model(case), "cpu")
    assert model.elbo_schedule is None
    seen = []
    monkeypatch.setattr(model, "shared_step", lambda batch, **kw: seen.append(kw) or {"loss": torch.zeros(()), "kl": torch.ones(())})
    before = dict(model.noise_shapes(3, 5))
    model.elbo_schedule = ElboSchedule(free_nats=1.0, warmup_steps=10)
    assert model.noise_shapes(3, 5) == before  # no draw is added
    model.training_step(build_batch(case))
    model.validation_step(build_batch(case))
    assert seen[0]["elbo_schedule"] is model.elbo_schedule and len(seen) == 2  # noqa: PLR2004
    assert seen[1].get("elbo_schedule") is None  # val/loss stays the plain ELBO
    model.val_forecast = Forecast(3)
    seen.clear()
    model.validation_step(build_batch(case))
    assert len(seen) == 2 and all(kw.get("elbo_schedule") is None for kw in seen)  # noqa: PLR2004


# -- bind is a view -----------------------------------------------------------------------------------------------------------------------
class _Opt:
    """The part of ``FlatAdamW`` the schedule reads: ``state`` = [lr, steps taken, 1 - b1^t, sqrt(1 - b2^t)] in device memory."""

    def __init__(self) -> None:
        self.state = torch.tensor([1e-3, 0.0, 0.0, 0.0], dtype=F32)


def test_bind_is_a_view_of_the_optimizer_state() -> None:
    opt = _Opt()
    s = ElboSchedule(beta_start=0.0, warmup_steps=4)
    assert s.bind(opt) is s
    step = s.step_on(torch.device("cpu"))
    assert step.data_ptr() == opt.state[1:2].data_ptr() and step.shape == (1,)
    betas = []
    for k in (0.0, 1.0, 3.0, 9.0):
        opt.state[1] = k  # what the optimizer step does on the device
        betas.append(float(s.reference(f32(0.0), f32(0.0), torch.ones(2), 1.0).beta))
    assert betas == [0.0, 0.25, 0.75, 1.0]
    other = _Opt()  # what FlatAdamW.load_state_dict leaves: the steps taken, restored
    other.state[1] = 2.0
    assert float(s.bind(other).reference(f32(0.0), f32(0.0), torch.ones(2), 1.0).beta) == 0.5
    s.set_step(1)  # an own tensor again: the optimizer's is not written
    own = s.step_on(torch.device("cpu"))
    assert s.set_step(3, "cpu").step_on(torch.device("cpu")) is own and s.set_step(1).step_on(torch.device("cpu")) is own  # filled, not replaced
    assert ElboSchedule._same_device(torch.device("cpu"), torch.device("cpu", 0)) and not ElboSchedule._same_device(torch.device("cpu"), torch.device("cuda"))  # noqa: SLF001
    assert float(other.state[1]) == 2.0 and float(s.reference(f32(0.0), f32(0.0), torch.ones(2), 1.0).beta) == 0.25


# -- C-ABI ------------------------------------------------------------------------------------------------------------------------------
def test_the_new_entries_reject_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    p = 1 << 20  # (never dereferenced: every call below returns before a launch)
    par = _lib.ElboSchedule(1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0)
    assert [n for n, _ in _lib.ElboSchedule._fields_] == ["c0", "c1", "free0", "free1", "w_a", "w_v", "beta_start", "warmup"]  # noqa: SLF001
    assert lib.mtrssm_elbo_schedule_fwd(None, p, p, None, None, None, None, 4, par, p, p, p, p, p, p, None) == -1
    assert lib.mtrssm_elbo_schedule_fwd(p, p, p, None, None, None, None, 0, par, p, p, p, p, p, p, None) == -1
    assert lib.mtrssm_elbo_schedule_fwd(p, p, p, None, None, None, None, 4, par, p, p, p, p, None, p, None) == -1  # no beta
    assert lib.mtrssm_elbo_schedule_fwd(p, p, p, None, p, None, None, 4, par, p, p, p, p, p, p, None) == -1  # live without count
    assert b"come together" in lib.mtrssm_last_error()
    warm = _lib.ElboSchedule(1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.5, 5.0)
    assert lib.mtrssm_elbo_schedule_fwd(p, p, p, None, None, None, None, 4, warm, p, p, p, p, p, p, None) == -1  # a warm-up without step
    assert b"step" in lib.mtrssm_last_error()
    huge = _lib.ElboSchedule(1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.5, float(1 << 24))
    assert lib.mtrssm_elbo_schedule_fwd(p, p, p, None, None, None, p, 4, huge, p, p, p, p, p, p, None) == -1
    assert lib.mtrssm_elbo_schedule_bwd(None, None, None, p, None, None, None, None, p, 4, par, p, p, p, None, None) == -1  # no kl0
    assert lib.mtrssm_elbo_schedule_bwd(None, None, None, p, p, None, None, None, None, 4, par, p, p, p, None, None) == -1  # no stored beta
    assert lib.mtrssm_elbo_schedule_bwd(None, None, None, p, p, None, None, None, p, 4, par, p, p, p, p, None) == -1  # g_kl1 without kl1
    assert lib.mtrssm_elbo_schedule_bwd(None, None, None, p, p, None, None, p, p, 4, par, p, p, p, None, None) == -1  # count without live
