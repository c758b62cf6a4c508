"""CPU: held-out likelihood -- the bound's rule and the latent log-ratio's rule in torch (float64) against
brute-force loops, their properties, the table's fold by frame position and naming, the argument refusals of the Python surface and of
the two C-ABI entries (which return before any launch), and the non-GPU route of ``log_ratio`` / ``bound``.  Nothing here launches a
kernel.  The shapes and inputs (``bound_inputs``, ``ratio_inputs``) are shared with ``tests/test_likelihood_gpu.py``."""

from __future__ import annotations

import math

import pytest
import torch

from multimodal_mtrssm_amd import LikelihoodBound, LikelihoodTable, StateCarry, _lib
from multimodal_mtrssm_amd.likelihood import PLANES, TABLE_ROWS
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HOST_B, HOST_T = 3, 7
HOST_VALID = (7, 3, 0)
HOST_S = (1, 2, 16)
HOST_EVENTS = (96, 40)  # E of audio and vision in the kernel-level cases
RATIO_SHAPES = ((4, 4), (6, 5), (8, 2), (3, 11))  # (K, C)
RATIO_LEAD = (6, 5)


def bound_inputs(s: int, kind: str = "normal", b: int = HOST_B, t: int = HOST_T, seed: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 ``(se_audio, se_vision, log_ratio)`` ``[B, S, T]``.  ``normal``: errors of a few nats; ``wide``: log-weights spread over
    hundreds of nats (the bound tracks the best sample, ESS goes to 1); ``equal``: every sample of a row carries the same numbers."""
    g = torch.Generator().manual_seed(100 * s + seed)
    scale = {"normal": 3.0, "wide": 400.0, "equal": 3.0}[kind]
    rows = 1 if kind == "equal" else s
    se_a = torch.rand(b, rows, t, generator=g) * scale + 40.0
    se_v = torch.rand(b, rows, t, generator=g) * scale + 10.0
    ratio = -torch.rand(b, rows, t, generator=g) * (scale / 3.0)
    return tuple(x.expand(b, s, t).contiguous() for x in (se_a, se_v, ratio))


def ratio_inputs(cats: int, classes: int, gain: float = 1.0, lead: tuple[int, ...] = RATIO_LEAD) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 ``(post_logits, prior_logits, stoch)`` ``[*lead, K * C]``, the sample a one-hot per categorical."""
    g = torch.Generator().manual_seed(1000 * cats + classes)
    post = torch.randn(*lead, cats * classes, generator=g) * gain
    prior = torch.randn(*lead, cats * classes, generator=g) * gain
    idx = torch.randint(0, classes, (*lead, cats), generator=g)
    stoch = torch.nn.functional.one_hot(idx, classes).to(torch.float32).reshape(*lead, cats * classes)
    return post, prior, stoch


def brute_force(se_a, se_v, ratio, valid, e_a: int, e_v: int) -> torch.Tensor:  # noqa: ANN001
    """The quantity of DESIGN.md 6k in plain Python floats (float64), one frame at a time."""
    ref = next(x for x in (se_a, se_v, ratio) if x is not None)
    b_, s_, t_ = ref.shape
    out = torch.zeros(8, b_, t_, dtype=torch.float64)
    for b in range(b_):
        n = t_ if valid is None else max(0, min(t_, int(valid[b])))
        cum = [0.0] * s_
        l_prev = m_prev = 0.0
        for t in range(n):
            a = [0.0 if se_a is None else -float(se_a[b, s, t]) - 0.5 * e_a * math.log(2.0 * math.pi) for s in range(s_)]
            v = [0.0 if se_v is None else -float(se_v[b, s, t]) - 0.5 * e_v * math.log(2.0 * math.pi) for s in range(s_)]
            r = [0.0 if ratio is None else float(ratio[b, s, t]) for s in range(s_)]
            for s in range(s_):
                cum[s] += (a[s] + v[s]) + r[s]
            top = max(cum)
            w = [math.exp(c - top) for c in cum]
            l_now = top + math.log(sum(w)) - math.log(s_)
            m_now = sum(cum) / s_
            vals = (l_now - l_prev, m_now - m_prev, sum(a) / s_, sum(v) / s_, sum(r) / s_, sum(w) ** 2 / sum(x * x for x in w), l_now, m_now)
            for p, x in enumerate(vals):
                out[p, b, t] = x
            l_prev, m_prev = l_now, m_now
    return out


# -- 1. the bound's rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "wide", "equal"])
@pytest.mark.parametrize("s", HOST_S)
def test_reference_equals_the_brute_force_loop(s: int, kind: str) -> None:
    se_a, se_v, ratio = bound_inputs(s, kind)
    for valid in (torch.tensor(HOST_VALID, dtype=torch.int32), None):
        got = LikelihoodBound.reference(se_a, se_v, ratio, valid, *HOST_EVENTS)
        want = brute_force(se_a, se_v, ratio, valid, *HOST_EVENTS)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(PLANES), HOST_B, HOST_T)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-9)  # (atol: planes 0 / 1 are differences of prefixes of ~1e3 nats)
        iw, elbo, audio, vision, latent, ess, iw_prefix, elbo_prefix = got
        assert bool((iw_prefix >= elbo_prefix - 1e-9).all())  # Jensen
        torch.testing.assert_close(elbo, audio + vision + latent, rtol=0, atol=1e-12 * float(elbo_prefix.abs().max()))
        assert bool((ess >= 1.0 - 1e-12)[ess != 0].all()) and bool((ess <= s + 1e-12).all())
        if valid is not None:
            dead = ~(torch.arange(HOST_T) < valid[:, None])
            assert bool(dead.any()) and not bool(got[:, dead].any())  # exactly 0 on dead frames
            assert bool((got[5][~dead] >= 1.0 - 1e-12).all())
        if s == 1:
            assert torch.equal(iw, elbo) and torch.equal(iw_prefix, elbo_prefix) and bool((ess[ess != 0] == 1.0).all())
        if kind == "wide" and s > 1:
            # sums of seven errors spread over 400 nats each: the best two of <= 16 samples lie many nats apart and the best one carries
            # the weight (1.01 is a second-best weight of 0.005, a gap of 5.3 nats)
            assert float(ess[0, -1]) < 1.01  # noqa: PLR2004
            assert float((iw_prefix - elbo_prefix)[0, -1]) > 50.0  # noqa: PLR2004
        if kind == "equal":
            live = ess != 0
            assert bool((ess[live] == float(s)).all())  # exactly S
            torch.testing.assert_close(iw, elbo, rtol=0, atol=1e-12 * float(elbo_prefix.abs().max()))


@pytest.mark.parametrize("s", [2, 16])
def test_equal_samples_of_dyadic_numbers_give_iw_equal_to_elbo_bitwise(s: int) -> None:
    ratio = -(torch.randint(0, 64, (HOST_B, 1, HOST_T), generator=torch.Generator().manual_seed(s)).to(torch.float32) / 8.0)
    got = LikelihoodBound.reference(None, None, ratio.expand(HOST_B, s, HOST_T).contiguous())  # (every sum over s is exact)
    assert torch.equal(got[0], got[1]) and torch.equal(got[6], got[7]) and bool((got[5] == float(s)).all())
    assert torch.equal(got[4], ratio[:, 0].double()) and not bool(got[2].any()) and not bool(got[3].any())


def test_each_term_toggles() -> None:
    se_a, se_v, ratio = bound_inputs(4)
    valid = torch.tensor(HOST_VALID, dtype=torch.int32)
    full = LikelihoodBound.reference(se_a, se_v, ratio, valid, *HOST_EVENTS)
    for off in range(3):
        args = [se_a, se_v, ratio]
        args[off] = None
        got = LikelihoodBound.reference(*args, valid, *HOST_EVENTS)
        want = brute_force(*args, valid, *HOST_EVENTS)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-9)
        assert not bool(got[2 + off].any())  # the plane of a term that is off is 0 ...
        for on in range(3):
            if on != off:
                assert torch.equal(got[2 + on], full[2 + on])  # ... and the others are what they were
        torch.testing.assert_close(got[1], got[2] + got[3] + got[4], rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="at least one"):
        LikelihoodBound.reference(None, None, None)


# -- 2. the latent log-ratio's rule ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("cats", "classes"), RATIO_SHAPES)
def test_reference_ratio_equals_log_softmax_and_gather(cats: int, classes: int) -> None:
    for gain in (1.0, 30.0):  # (30: saturated heads)
        post, prior, stoch = ratio_inputs(cats, classes, gain)
        got = LikelihoodBound.reference_ratio(post, prior, stoch, cats, classes)
        assert got.dtype == torch.float64 and tuple(got.shape) == RATIO_LEAD and bool(torch.isfinite(got).all())
        idx = stoch.reshape(*RATIO_LEAD, cats, classes).argmax(-1, keepdim=True)
        lq = torch.log_softmax(post.double().reshape(*RATIO_LEAD, cats, classes), -1).gather(-1, idx)
        lp = torch.log_softmax(prior.double().reshape(*RATIO_LEAD, cats, classes), -1).gather(-1, idx)
        torch.testing.assert_close(got, (lp - lq).sum((-1, -2)), rtol=1e-12, atol=1e-12)
        assert float(got.abs().max()) > (10.0 if gain > 1.0 else 0.1)
        same = LikelihoodBound.reference_ratio(post, post.clone(), stoch, cats, classes)
        assert not bool(same.any())  # identical logits: exactly 0


def test_reference_ratio_takes_the_first_class_above_one_half() -> None:
    post, prior = torch.tensor([[0.0, 1.0, 2.0]]), torch.tensor([[2.0, 1.0, 0.0]])
    two = LikelihoodBound.reference_ratio(post, prior, torch.tensor([[0.0, 1.0, 1.0]]), 1, 3)
    one = LikelihoodBound.reference_ratio(post, prior, torch.tensor([[0.0, 1.0, 0.0]]), 1, 3)
    none = LikelihoodBound.reference_ratio(post, prior, torch.zeros(1, 3), 1, 3)
    zero = LikelihoodBound.reference_ratio(post, prior, torch.tensor([[1.0, 0.0, 0.0]]), 1, 3)
    assert torch.equal(two, one) and torch.equal(none, zero) and float(one) == 0.0 and float(zero) == 2.0  # noqa: PLR2004


# -- 3. the table ------------------------------------------------------------------------------------------------------------------------
def test_table_folds_by_frame_position() -> None:
    valid = torch.tensor(HOST_VALID, dtype=torch.int32)
    live = torch.arange(HOST_T) < valid[:, None]
    p, b, t = torch.meshgrid(torch.arange(8), torch.arange(HOST_B), torch.arange(HOST_T), indexing="ij")
    planes = torch.where(live, (100 * p + 10 * b + t + 1).to(torch.float32), torch.zeros(()))  # whole numbers: exact in fp32
    table = LikelihoodTable(HOST_T)
    assert tuple(table.buffer.shape) == (7, HOST_T) and table.buffer.dtype == torch.float32 and table.planes is None and table.states is None
    assert table.fold(planes, valid) is table
    assert table.counts.tolist() == [2.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0]  # context = 1: bin h is frame t
    assert torch.equal(table.sums, planes[:6].sum(1))
    for name, row in table.curves().items():
        assert torch.equal(row, planes[TABLE_ROWS.index(name)].sum(0) / table.counts)
    table.fold(planes[:6])  # (the first six planes are enough; no lengths: every frame is live, the dead ones add their zeros)
    assert table.counts.tolist() == [5.0, 5.0, 5.0, 4.0, 4.0, 4.0, 4.0]
    other = LikelihoodTable(HOST_T).fold(planes, valid)
    before = table.buffer.clone()
    assert table.add(other) is table and torch.equal(table.buffer, before + other.buffer)
    per = table.per_frame()
    assert tuple(per) == TABLE_ROWS
    for i, name in enumerate(TABLE_ROWS):
        assert float(per[name]) == pytest.approx(float(table.sums[i].sum()) / float(table.counts.sum()), rel=1e-6)
    scalars = table.scalars("val/loglik")
    assert set(scalars) == {f"val/loglik/{k}" for k in ("iw", "elbo", "audio", "vision", "latent", "ess", "gap")}
    assert float(scalars["val/loglik/gap"]) == pytest.approx(float(per["iw"]) - float(per["elbo"]), rel=1e-6)
    assert all(math.isnan(float(v)) for v in LikelihoodTable(4).scalars("x").values()) and bool(LikelihoodTable(4).curves()["iw"].isnan().all())
    assert table.all_reduce() is table  # (no process group: a no-op)
    with pytest.raises(ValueError, match="steps"):
        LikelihoodTable(0)
    with pytest.raises(ValueError, match="do not add"):
        table.add(LikelihoodTable(HOST_T + 1))
    with pytest.raises(ValueError, match="planes"):
        table.fold(planes[:5])


# -- 4. refusals and surface --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [0, 17, -1, 2.0, True, None])
def test_bad_sample_counts_are_refused(samples) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="samples"):
        LikelihoodBound(samples)


@pytest.mark.parametrize("observe", ["all", "Audio", "", None, 3])
def test_bad_observe_is_refused(observe) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="observe"):
        LikelihoodBound(2, observe)


@pytest.mark.parametrize("score", ["audio", ("audio", "audio"), ("sound",), (3,)])
def test_bad_score_is_refused(score) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="score"):
        LikelihoodBound(2, score=score)


def test_bound_surface() -> None:
    with pytest.raises(ValueError, match="nothing to score"):
        LikelihoodBound(2, score=(), latent=False)
    with pytest.raises(ValueError, match="latent"):
        LikelihoodBound(2, latent=1)
    lb = LikelihoodBound(samples=4, observe="audio", score=("vision",), latent=False)
    assert (lb.samples, lb.observe, lb.score, lb.latent, lb.bits, lb.max_frames, lb.group) == (4, "audio", ("vision",), False, 1, 4096, None)
    assert lb.observed("cpu").tolist() == [True, False]
    default = LikelihoodBound()
    assert (default.samples, default.observe, default.score, default.latent, default.bits) == (1, "both", ("audio", "vision"), True, 3)
    assert LikelihoodBound(2, score=("vision", "audio")).score == ("audio", "vision")
    bound = lb.for_group("group")
    assert bound is not lb and bound.group == "group" and lb.group is None and bound.samples == 4  # noqa: PLR2004
    assert repr(lb) == "LikelihoodBound(samples=4, observe='audio', score=('vision',), latent=False)"


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


def test_noise_shapes_put_the_batch_first(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    shapes = LikelihoodBound(samples=3).noise_shapes(model, 4, 6)
    if case.kind == "mrssm":
        k = case.dims.cats
        assert shapes == {"u_init": (4, 3, k), "u_post": (4, 3, 6, k)}
    else:
        kl, kh = case.dims.ls_cats, case.dims.hs_cats
        assert shapes == {"u_init_h": (4, 3, kh), "u_init_l": (4, 3, kl), "u_post_l": (4, 3, 6, kl), "u_post_h": (4, 3, 6, kh)}
    assert all(s[0] == 4 for s in shapes.values())  # noqa: PLR2004  (GlobalRowNoise slices the first extent)


def test_likelihood_step_refuses_masked_batches_and_a_set_carry(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    b, t = batch[0].shape[:2]
    lb = LikelihoodBound(samples=2)
    assert model.val_likelihood is None and model.likelihood_table is None and model.on_validation_epoch_end() == {}
    with pytest.raises(ValueError, match="masked"):
        model.likelihood_bound((*batch, torch.ones(b, t, 2, dtype=torch.bool)), lb)
    with pytest.raises(ValueError, match="LikelihoodBound"):
        model.likelihood_bound(batch, 2)
    model.state_carry = StateCarry.for_model(model, b)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.likelihood_bound(batch, lb)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="LikelihoodTable"):
        model.likelihood_bound(batch, lb, table=LikelihoodTable(t + 1))


def test_python_entries_refuse_bad_arguments() -> None:
    se_a, se_v, ratio = bound_inputs(2)
    with pytest.raises(ValueError, match="share one"):
        LikelihoodBound.bound(se_a, se_v[:, :1], ratio, None, *HOST_EVENTS)
    with pytest.raises(ValueError, match="1 <= S <= 16"):
        LikelihoodBound.bound(None, None, torch.zeros(2, 17, 3))
    with pytest.raises(ValueError, match="valid"):
        LikelihoodBound.bound(se_a, se_v, ratio, torch.tensor(HOST_VALID), *HOST_EVENTS)  # (int64)
    with pytest.raises(ValueError, match="event size"):
        LikelihoodBound.bound(se_a, None, ratio, None, 0, 0)
    with pytest.raises(ValueError, match="2\\^24"):
        LikelihoodBound.reference(None, None, torch.zeros(1 << 12, 1, 1 << 12, device="meta"))
    with pytest.raises(ValueError, match="out must be"):
        LikelihoodBound.bound(se_a, se_v, ratio, None, *HOST_EVENTS, out=torch.zeros(6, HOST_B, HOST_T))
    post, prior, stoch = ratio_inputs(4, 4)
    with pytest.raises(ValueError, match="K, C >= 1"):
        LikelihoodBound.log_ratio(post, prior, stoch, 0, 16)
    with pytest.raises(ValueError, match="logits must be"):
        LikelihoodBound.log_ratio(post, prior, stoch, 4, 5)
    with pytest.raises(ValueError, match="share a shape"):
        LikelihoodBound.log_ratio(post, prior[:3], stoch, 4, 4)
    with pytest.raises(ValueError, match="accumulate"):
        LikelihoodBound.log_ratio(post, prior, stoch, 4, 4, accumulate=True)
    with pytest.raises(ValueError, match="2\\^31"):
        LikelihoodBound.reference_ratio(*(torch.zeros(1 << 20, 1 << 11, device="meta"),) * 3, 1 << 5, 1 << 6)


def check_c_refusals(lib) -> None:  # noqa: ANN001
    """Every ``-1`` return of the two entry points; each call returns before a launch (also run on the GPU machine)."""
    ok = 0x10000  # never dereferenced
    good = {"post": ok, "prior": ok, "stoch": ok, "rows": 30, "K": 6, "C": 5, "acc": 0, "out": ok}

    def ratio(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_latent_log_ratio(a["post"], a["prior"], a["stoch"], a["rows"], a["K"], a["C"], a["acc"], a["out"], None)

    for name in ("post", "prior", "stoch", "out"):
        assert ratio(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
        assert ratio(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("rows", "K", "C"):
        assert ratio(**{name: 0}) == -1 and ratio(**{name: -3}) == -1 and b"latent_log_ratio" in lib.mtrssm_last_error(), name
    assert ratio(acc=2) == -1 and ratio(acc=-1) == -1
    assert ratio(rows=1 << 20, K=1 << 6, C=1 << 5) == -1 and b"2^31" in lib.mtrssm_last_error()  # rows * K * C = 2^31
    assert ratio(rows=1 << 40, K=1 << 40, C=2) == -1  # (the product overflows 64 bits)

    bgood = {"a": ok, "v": ok, "r": ok, "valid": None, "B": 3, "S": 4, "T": 7, "ea": 96, "ev": 40, "planes": ok}

    def bound(**kw) -> int:  # noqa: ANN003
        a = {**bgood, **kw}
        return lib.mtrssm_iw_bound(a["a"], a["v"], a["r"], a["valid"], a["B"], a["S"], a["T"], a["ea"], a["ev"], a["planes"], None)

    assert bound(planes=None) == -1 and b"null" in lib.mtrssm_last_error()
    assert bound(a=None, v=None, r=None) == -1 and b"null" in lib.mtrssm_last_error()
    for name in ("a", "v", "r", "valid", "planes"):
        assert bound(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("B", "T", "ea", "ev"):
        assert bound(**{name: 0}) == -1 and bound(**{name: -3}) == -1 and b"iw_bound" in lib.mtrssm_last_error(), name
    for s in (0, 17, -1):
        assert bound(S=s) == -1 and b"samples" in lib.mtrssm_last_error(), s
    assert bound(B=1 << 12, T=1 << 12) == -1 and b"2^24" in lib.mtrssm_last_error()
    assert bound(B=1 << 40, T=1 << 40) == -1


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


# -- 5. the non-GPU route -----------------------------------------------------------------------------------------------------------------
def test_cpu_route_of_log_ratio_and_bound_is_the_reference() -> None:
    post, prior, stoch = ratio_inputs(6, 5)
    want = LikelihoodBound.reference_ratio(post, prior, stoch, 6, 5)
    got = LikelihoodBound.log_ratio(post, prior, stoch, 6, 5)
    assert got.dtype == torch.float32 and torch.equal(got, want.float())
    twice = LikelihoodBound.log_ratio(post, prior, stoch, 6, 5, out=got.clone(), accumulate=True)
    assert torch.equal(twice, (want.float().double() + want).float())
    se_a, se_v, ratio = bound_inputs(4)
    valid = torch.tensor(HOST_VALID, dtype=torch.int32)
    planes = LikelihoodBound.bound(se_a, se_v, ratio, valid, *HOST_EVENTS)
    assert planes.dtype == torch.float32 and torch.equal(planes, LikelihoodBound.reference(se_a, se_v, ratio, valid, *HOST_EVENTS).float())
    out = torch.empty(8, HOST_B, HOST_T)
    assert LikelihoodBound.bound(None, se_v, None, None, 0, HOST_EVENTS[1], out=out) is out
    assert torch.equal(out, LikelihoodBound.reference(None, se_v, None, None, 0, HOST_EVENTS[1]).float())
