"""GPU (MI355X): held-out likelihood, kernels and end to end.

What is pinned here.  Both kernels compute in double and round once, so each is the float64 rule on the same fp32 inputs within
``|got - ref| <= 1e-6 * max(1, |ref|)``, bitwise reproducible, a row's result independent of the batch around it, exactly 0 on dead
frames and -- at ``S = 1`` -- ``iw == elbo`` bit for bit.  A likelihood step is the composition of the public pieces
(``initial_state``, ``rollout_representation``, ``decode_state`` on the ``B * S`` repeated rows with the same uniforms, then the
float64 rule on the host): the data planes and the prefixes to the project's loss-term tolerance, rtol 2e-5 (an error in ``se`` moves
``L[t]`` and ``M[t]`` by at most the same relative amount), the latent plane within ``1e-6 * max(1, |x|)``, planes 0 / 1 through their
running sums against planes 6 / 7, the ESS in ``[1, S]`` only (it is exponentially sensitive to ``se``: pinned at kernel level).  At
``S = 1`` with ``shared_step``'s uniforms the audio / vision planes are ``shared_step``'s ``recon/*``.  ``validation_step`` keeps its
``val/*`` values bit for bit; that test runs at frame counts whose NLL sums fit ONE workgroup (<= 1024 elements per modality),
because the NLL kernels add their workgroups' partial sums with float atomics whose order is free from run to run.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import ExpertWeights, LikelihoodBound, LikelihoodTable, StateCarry, _lib
from oracle.cases import CASES, build_batch, build_model, build_noise, with_sizes
from tests.conftest import product_from_case
from tests.test_likelihood_host import HOST_B, HOST_EVENTS, HOST_S, HOST_T, HOST_VALID, RATIO_SHAPES, bound_inputs, check_c_refusals, ratio_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, T = 3, 6
LENGTHS = (6, 4, 1)


def _close(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """``|got - ref| <= 1e-6 * max(1, |ref|)``: the kernels' bound."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    err, bound = (got - want).abs(), 1e-6 * want.abs().clamp_min(1.0)
    print(what, "worst err / bound", float((err / bound).max()))
    assert bool((err <= bound).all()), f"{what}: worst {float(err.max())} at ref {float(want.flatten()[int((err / bound).argmax())])}"


# 1. the log-ratio kernel is the rule ----------------------------------------------------------------------------------------------------
# the issue's four (K, C) pairs, then one per other path of the launch: a row wider than the LDS tile walked in spans of whole
# categoricals (40 x 20 = 800 > 512), a categorical wider than the tile walked class by class (C = 600), and one class
@pytest.mark.parametrize(("cats", "classes"), [*RATIO_SHAPES, (40, 20), (2, 600), (5, 1)])
def test_log_ratio_kernel_equals_the_float64_rule(cats: int, classes: int) -> None:
    for gain in (1.0, 30.0):  # (30: saturated heads)
        post, prior, stoch = ratio_inputs(cats, classes, gain)
        want = LikelihoodBound.reference_ratio(post, prior, stoch, cats, classes)
        dpost, dprior, dstoch = post.to(DEV), prior.to(DEV), stoch.to(DEV)
        got = LikelihoodBound.log_ratio(dpost, dprior, dstoch, cats, classes)
        again = LikelihoodBound.log_ratio(dpost, dprior, dstoch, cats, classes)
        torch.cuda.synchronize()
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(post.shape[:-1]) and bool(torch.isfinite(got).all())
        _close(got, want, f"ratio {cats}x{classes} gain {gain}")
        assert torch.equal(got, again)
        same = LikelihoodBound.log_ratio(dpost, dpost.clone(), dstoch, cats, classes)
        assert not bool(same.any()), (cats, classes, gain)  # identical logits: exactly 0
        # accumulate: a second level's sum joins the first before the one rounding
        post2, prior2, stoch2 = ratio_inputs(cats, classes, 0.5 * gain)
        both = LikelihoodBound.log_ratio(post2.to(DEV), prior2.to(DEV), stoch2.to(DEV), cats, classes, out=got.clone(), accumulate=True)
        want2 = LikelihoodBound.reference_ratio(post2, prior2, stoch2, cats, classes)
        _close(both, got.cpu().double() + want2, f"accumulate {cats}x{classes} gain {gain}")
        # a row's result depends on that row only: the last rows alone, in a launch of another shape
        tail = LikelihoodBound.log_ratio(dpost[-1, -2:].contiguous(), dprior[-1, -2:].contiguous(), dstoch[-1, -2:].contiguous(), cats, classes)
        assert torch.equal(tail, got[-1, -2:]), (cats, classes, gain)


# 2. the bound kernel is the rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "wide", "equal"])
@pytest.mark.parametrize("s", HOST_S)
def test_bound_kernel_equals_the_float64_rule(s: int, kind: str) -> None:
    inputs = bound_inputs(s, kind)
    dev = [x.to(DEV) for x in inputs]
    valid = torch.tensor(HOST_VALID, dtype=torch.int32)
    for lengths in (valid, None):
        dvalid = None if lengths is None else lengths.to(DEV)
        for off in (None, 0, 1, 2):  # every term on, then each of the three inputs nulled in turn
            host, args = list(inputs), list(dev)
            if off is not None:
                host[off] = args[off] = None
            what = f"bound S {s} {kind} valid {None if lengths is None else lengths.tolist()} off {off}"
            want = LikelihoodBound.reference(*host, lengths, *HOST_EVENTS)
            got = LikelihoodBound.bound(*args, dvalid, *HOST_EVENTS)
            again = LikelihoodBound.bound(*args, dvalid, *HOST_EVENTS)
            torch.cuda.synchronize()
            assert got.dtype == torch.float32 and tuple(got.shape) == (8, HOST_B, HOST_T)
            _close(got, want, what)  # every plane
            assert torch.equal(got, again), what  # two calls agree bitwise
            if off is not None:
                assert not bool(got[2 + off].any()), what
            if lengths is not None:
                dead = ~(torch.arange(HOST_T) < lengths[:, None]).to(DEV)
                assert not bool(got[:, dead].any()), what  # exactly 0 on dead frames
            if s == 1:
                assert torch.equal(got[0], got[1]) and torch.equal(got[6], got[7]), what
            assert bool((got[6] >= got[7]).all()), what  # Jensen survives the one rounding: fp32 rounding is monotone
            live = got[5] != 0
            assert bool((got[5][live] >= 1.0).all()) and bool((got[5] <= float(s)).all()), what


def test_bound_kernel_row_independence() -> None:
    """The same row in a different batch gives the same bits: alone, and as row 17 of 20 (a second workgroup, another DPP row)."""
    s = 5
    se_a, se_v, ratio = (x.to(DEV) for x in bound_inputs(s, "normal", b=20, t=9, seed=3))
    valid = torch.randint(0, 11, (20,), generator=torch.Generator().manual_seed(4)).to(torch.int32)
    valid[17] = 7
    valid = valid.to(DEV)
    full = LikelihoodBound.bound(se_a, se_v, ratio, valid, *HOST_EVENTS)
    want = LikelihoodBound.reference(se_a.cpu(), se_v.cpu(), ratio.cpu(), valid.cpu(), *HOST_EVENTS)
    _close(full, want, "bound B 20")
    for row in (0, 15, 16, 17, 19):
        one = LikelihoodBound.bound(se_a[row : row + 1], se_v[row : row + 1], ratio[row : row + 1], valid[row : row + 1], *HOST_EVENTS)
        assert torch.equal(one[:, 0], full[:, row]), row
    moved = LikelihoodBound.bound(se_a[15:19].contiguous(), se_v[15:19].contiguous(), ratio[15:19].contiguous(), valid[15:19].contiguous(), *HOST_EVENTS)
    assert torch.equal(moved, full[:, 15:19])


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


# 3. the likelihood step is the composition of the public pieces -------------------------------------------------------------------------------
def _seeded_gate(embed: int, seed: int = 29) -> ExpertWeights:
    gate = ExpertWeights("gated", embed)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in gate.parameters():
            p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return gate


@functools.lru_cache(maxsize=None)
def _setup(name: str, sizes: tuple[int, int] = (B, T)):  # noqa: ANN202
    """Model (``make_mrssm`` / ``make_mmtrssm`` at the case's dims with the oracle's weights; ``weighted``: a
    ``WeightedMoPoE_MRSSM`` with a seeded gate) and batch on the device, made once and shared."""
    weighted = name == "weighted"
    case = with_sizes(CASES["mrssm_default" if weighted else name], *sizes)
    if weighted:
        d = case.dims
        model = mt.make_mrssm(deter=d.deter, hidden=d.hidden, classes=d.classes, cats=d.cats, action=d.action, embed=d.embed,
                              enc_audio=d.enc_audio, enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision,
                              activation=d.activation, init_cells=d.init_cells, kl_coeff=d.kl_coeff, use_kl_balancing=d.use_kl_balancing,
                              expert_weights="gated")
        assert isinstance(model, mt.WeightedMoPoE_MRSSM)
        model.load_state_dict(build_model(case).state_dict(), strict=False)
        model.expert_weights = _seeded_gate(d.embed)
        model = model.to(DEV)
    else:
        model = product_from_case(case, build_model(case), DEV)
    batch = tuple(x.to(DEV) for x in build_batch(case))
    return case, model, batch


def _noise(model, bound: LikelihoodBound, b: int, t: int, seed: int = 11) -> dict[str, torch.Tensor]:  # noqa: ANN001
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(shape, generator=g).to(DEV) for k, shape in bound.noise_shapes(model, b, t).items()}


def _levels(case) -> list[tuple[str, int, int]]:  # noqa: ANN001
    d = case.dims
    if case.kind == "mrssm":
        return [("", d.cats, d.classes)]
    return [("_l", d.ls_cats, d.ls_classes), ("_h", d.hs_cats, d.hs_classes)]


def _composed(case, model, batch, bound: LikelihoodBound, noise: dict[str, torch.Tensor], lengths: torch.Tensor | None) -> torch.Tensor:  # noqa: ANN001, PLR0913, PLR0914
    """The planes ``[8, B, T]`` in float64 from public pieces: ``initial_state``, ``rollout_representation`` and ``decode_state`` on the
    ``B * S`` repeated rows (row ``b * S + s``) under the same uniforms, then the float64 rule on the host."""
    b, t = batch[0].shape[:2]
    s = bound.samples
    wide = tuple(x.repeat_interleave(s, dim=0) for x in batch)
    wide_noise = {k: v.reshape(b * s, *v.shape[2:]).contiguous() for k, v in noise.items()}
    live = torch.ones(b, t, dtype=torch.bool) if lengths is None else torch.arange(t) < lengths.cpu()[:, None]
    mask = (live[:, :, None] & torch.tensor([bool(bound.bits & 1), bool(bound.bits & 2)])).repeat_interleave(s, dim=0).to(DEV)
    with torch.no_grad():
        s0 = model.initial_state((wide[1][:, 0], wide[2][:, 0]), wide_noise, modality_mask=mask[:, 0])
        post, prior = model.rollout_representation(actions=wide[0], observations=(wide[1], wide[2]), prev_state=s0, noise=wide_noise,
                                                   modality_mask=mask)
        dec = model.decode_state(post)
    se, events = [None, None], [0, 0]
    for j, (key, tgt) in enumerate((("recon/audio", batch[4]), ("recon/vision", batch[5]))):
        if key.split("/")[1] in bound.score:
            y = dec[key].flatten(2).double().cpu().reshape(b, s, t, -1)
            se[j] = (0.5 * (tgt.flatten(2).double().cpu()[:, None] - y) ** 2).sum(-1)
            events[j] = y.shape[-1]
    ratio = None
    if bound.latent:
        ratio = torch.zeros(b * s, t, dtype=torch.float64)
        for suffix, cats, classes in _levels(case):
            q, p, z = (getattr(post, f"distribution{suffix}").logits, getattr(prior, f"distribution{suffix}").logits, getattr(post, f"stoch{suffix}"))
            ratio = ratio + LikelihoodBound.reference_ratio(q.flatten(-2).cpu(), p.flatten(-2).cpu(), z.cpu(), cats, classes)
        ratio = ratio.reshape(b, s, t)
    return LikelihoodBound.reference(se[0], se[1], ratio, None if lengths is None else lengths.cpu(), *events)


def _assert_step(table: LikelihoodTable, want: torch.Tensor, s: int, lengths: torch.Tensor | None, what: str, *, latent_only: bool = False) -> None:  # noqa: PLR0913
    got = table.planes.cpu().double()
    b, t = got.shape[1:]
    live = torch.ones(b, t, dtype=torch.bool) if lengths is None else torch.arange(t) < lengths.cpu()[:, None]
    assert not bool(got[:, ~live].any()), what
    rel = ((got - want).abs() / want.abs().clamp_min(1e-30))[:, live]
    print(what, "worst rel of planes 2, 3, 6, 7:", [float(rel[p].max()) for p in (2, 3, 6, 7)], "plane 4 worst abs:",
          float((got[4] - want[4]).abs().max()), "of", float(want[4].abs().max()))
    for p in (2, 3, 6, 7):
        if latent_only and p in (6, 7):  # no data term: a prefix is a sum of <= T latent terms, each within the latent plane's bound
            err, bound = (got[p] - want[p]).abs(), t * 1e-6 * want[p].abs().clamp_min(1.0)
            assert bool((err <= bound).all()), f"{what} plane {p}: worst {float(err.max())}"
            continue
        np.testing.assert_allclose(got[p].numpy(), want[p].numpy(), rtol=2e-5, atol=0, err_msg=f"{what} plane {p}")
    _close(got[4], want[4], f"{what} plane 4")
    # planes 0 / 1 through their running sums: <= T + 1 fp32 roundings of numbers no larger than the prefix, (T + 1) * 2^-24 < 1e-6
    for inc, prefix in ((0, 6), (1, 7)):
        run = torch.where(live, got[inc].cumsum(1), torch.zeros(()).double())
        np.testing.assert_allclose(run.numpy(), got[prefix].numpy(), rtol=1e-6, atol=0, err_msg=f"{what} plane {inc} vs {prefix}")
    ess = table.planes[5].cpu()
    assert bool((ess[live] >= 1.0).all()) and bool((ess[live] <= float(s)).all()), what
    assert bool((got[6] >= got[7]).all()), what
    if s == 1:
        assert torch.equal(table.planes[0], table.planes[1]) and torch.equal(table.planes[6], table.planes[7]), what
    # the table: counts exact, the sums by frame position
    assert torch.equal(table.counts.cpu(), live.sum(0).float()), what
    sums = table.sums.cpu().double()
    for p in (2, 3):
        np.testing.assert_allclose(sums[p].numpy(), want[p].sum(0).numpy(), rtol=2e-5, atol=0, err_msg=f"{what} table row {p}")
    for p in (0, 1, 4, 5):  # (the fold of this step's own planes: b <= 3 fp32 adds)
        np.testing.assert_allclose(sums[p].numpy(), got[p].sum(0).numpy(), rtol=1e-6, atol=1e-6, err_msg=f"{what} table row {p}")


STEP_CASES = [(name, s, observe) for name in ("mrssm_default", "mmtrssm_default") for s in (1, 4) for observe in ("both", "audio")]
STEP_CASES.append(("weighted", 4, "both"))  # one WeightedMoPoE_MRSSM


@pytest.mark.parametrize(("name", "s", "observe"), STEP_CASES)
def test_likelihood_step_is_the_composition_of_the_public_pieces(name: str, s: int, observe: str) -> None:
    case, model, batch = _setup(name)
    bound = LikelihoodBound(samples=s, observe=observe)
    noise = _noise(model, bound, B, T)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    table = model.likelihood_bound(batch, bound, noise, lengths=lengths, keep_states=True)
    torch.cuda.synchronize()
    assert isinstance(table, LikelihoodTable) and tuple(table.buffer.shape) == (7, T) and tuple(table.planes.shape) == (8, B, T)
    want = _composed(case, model, batch, bound, noise, lengths)
    _assert_step(table, want, s, lengths, f"{name} S {s} {observe}")
    if name == "weighted":
        assert model.weights_timeseries is not None and not bool(torch.allclose(model.weights_timeseries[0, 0], torch.full((3,), 1 / 3, device=DEV)))
    if s > 1:  # the copies of a row part ways: each has its own draws
        x = table.states.stoch.reshape(B, s, T, -1) if case.kind == "mrssm" else table.states.stoch_l.reshape(B, s, T, -1)
        assert not torch.equal(x[:, 0], x[:, 1])
    # a second step adds into the same table; chunks of one row at a time change nothing
    small = LikelihoodBound(samples=s, observe=observe)
    small.max_frames = 1
    first = table.buffer.clone()
    again = model.likelihood_bound(batch, small, noise, lengths=lengths, table=table)
    assert again is table and table.planes is None and table.states is None
    assert torch.equal(table.counts, 2.0 * first[6])
    # (decoders over another batch shape round differently in the last bits: the loss-term tolerance again, 1e-6 on the latent row,
    # which no decoder touches; the ESS row moves exponentially with se and only keeps its range)
    np.testing.assert_allclose(table.sums[:4].cpu().numpy(), 2.0 * first[:4].cpu().numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(table.sums[4].cpu().numpy(), 2.0 * first[4].cpu().numpy(), rtol=1e-6, atol=1e-6)
    assert bool((table.sums[5] >= table.counts).all()) and bool((table.sums[5] <= float(s) * table.counts).all())


def test_term_toggles_and_the_conditional_estimate() -> None:
    """``score=("vision",), latent=False, observe="audio"``: ``log (1 / S) sum_s p(x_v | z_s)``, ``z_s ~ q(z | x_a)``; and latent only."""
    case, model, batch = _setup("mrssm_default")
    for bound in (LikelihoodBound(samples=4, observe="audio", score=("vision",), latent=False), LikelihoodBound(samples=4, score=(), latent=True),
                  LikelihoodBound(samples=2, observe="vision", score=("audio",))):
        noise = _noise(model, bound, B, T, seed=13)
        table = model.likelihood_bound(batch, bound, noise, keep_states=True)  # (no lengths: every frame is live)
        want = _composed(case, model, batch, bound, noise, None)
        _assert_step(table, want, bound.samples, None, repr(bound), latent_only=not bound.score)
        for p, on in ((2, "audio" in bound.score), (3, "vision" in bound.score), (4, bound.latent)):
            assert bool(table.planes[p].any()) == on, (repr(bound), p)
    drawn = model.likelihood_bound(batch, LikelihoodBound(samples=3))  # without noise the step draws its own
    assert bool(torch.isfinite(drawn.buffer).all()) and drawn.counts.tolist() == [float(B)] * T and drawn.planes is None


# 4. tie to the trained objective ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_one_sample_with_the_steps_uniforms_gives_the_steps_reconstruction_terms(name: str) -> None:
    case, model, batch = _setup(name)
    noise = {k: v.to(DEV) for k, v in build_noise(case).items() if k.startswith(("u_init", "u_post"))}
    with torch.no_grad():
        step = model.shared_step(batch, noise)
    mine = {k: v.unsqueeze(1) for k, v in noise.items()}  # (B, 1, K) and (B, 1, T, K): S = 1
    table = model.likelihood_bound(batch, LikelihoodBound(samples=1), mine, keep_states=True)
    torch.cuda.synchronize()
    for p, key in ((2, "recon/audio"), (3, "recon/vision")):
        got = -float(table.planes[p].double().sum()) / (B * T)
        print(name, key, got, float(step[key]))
        np.testing.assert_allclose(got, float(step[key]), rtol=2e-5, err_msg=key)


# 5. validation -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_cfg3dims"])
def test_validation_step_keeps_its_values_and_the_epoch_end_logs_the_likelihood(name: str) -> None:
    """B = 2, T = 4 frames of 16 x 8 audio and 8 x 8 vision: 1024 and 512 elements, one NLL workgroup each (see the module docstring)."""
    case, model, batch = _setup(name, (2, 4))
    bound = LikelihoodBound(samples=3)
    try:
        torch.manual_seed(5)
        plain = model.validation_step(batch)
        direct = model.likelihood_bound(batch, bound)
        model.validation_step(batch)
        model.likelihood_bound(batch, bound, table=direct)
        assert model.likelihood_table is None and model.on_validation_epoch_end() == {}
        model.val_likelihood = bound
        torch.manual_seed(5)
        both = model.validation_step(batch)
        assert set(both) == set(plain)
        for k, v in plain.items():
            assert torch.equal(both[k], v), (k, float(both[k]), float(v))  # bitwise: the likelihood step runs after everything else
        model.validation_step(batch)
        assert isinstance(model.likelihood_table, LikelihoodTable) and model.likelihood_table.counts.tolist() == [4.0] * 4
        logged = model.on_validation_epoch_end()
        assert model.likelihood_table is None and model.on_validation_epoch_end() == {}
        want = direct.scalars("val/loglik")
        assert set(logged) == set(want) == {f"val/loglik/{k}" for k in ("iw", "elbo", "audio", "vision", "latent", "ess", "gap")}
        for k, v in want.items():
            assert torch.equal(logged[k], v), (k, float(logged[k]), float(v))
        assert float(logged["val/loglik/gap"]) >= 0.0 and 1.0 <= float(logged["val/loglik/ess"]) <= 3.0  # noqa: PLR2004
        np.testing.assert_allclose(float(logged["val/loglik/elbo"]),
                                   float(logged["val/loglik/audio"] + logged["val/loglik/vision"] + logged["val/loglik/latent"]), rtol=1e-5)
    finally:
        model.val_likelihood = None
        model.likelihood_table = None


# 6. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_likelihood_step_refuses_masked_batches_and_a_set_carry() -> None:
    _, model, batch = _setup("mrssm_default")
    bound = LikelihoodBound(samples=2)
    with pytest.raises(ValueError, match="masked"):
        model.likelihood_bound((*batch, torch.ones(B, T, 2, dtype=torch.bool, device=DEV)), bound)
    model.state_carry = StateCarry.for_model(model, B)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.likelihood_bound(batch, bound)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="shape"):
        model.likelihood_bound(batch, bound, {"u_post": torch.rand(B, T, case_cats(model), device=DEV)})


def case_cats(model) -> int:  # noqa: ANN001
    return model.transition.distribution_factory.category_size
