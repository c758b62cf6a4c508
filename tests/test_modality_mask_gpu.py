"""Missing-modality rollouts and training on the GPU (DESIGN.md "Missing modalities").

Anchors: a mask with both modalities everywhere is today's path; a step with no modality is ``rollout_transition``'s step
fed with the posterior uniforms; an absent modality has no influence on anything and gets no gradient.
"""

from __future__ import annotations

import math

import pytest
import torch

from multimodal_mtrssm_amd.objective import likelihood
from oracle.cases import CASES, build_batch, build_model, build_noise
from tests.conftest import product_from_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (case, one-CU kernels forced): cluster, wide, one-CU and both MMTRSSM forms
FAMILIES = [
    ("mrssm_cfg2dims", False),
    ("mrssm_bench", False),
    ("mrssm_large", False),
    ("mrssm_nonsquare", False),
    ("mrssm_cfg2dims", True),
    ("mmtrssm_cfg3dims", False),
    ("mmtrssm_default", True),
]
IDS = [f"{c}{'-onecu' if f else ''}" for c, f in FAMILIES]


def _setup(name: str, force_onecu: bool):  # noqa: ANN202, FBT001
    case = CASES[name]
    model = product_from_case(case, build_model(case), DEV)
    if force_onecu:
        model.scan_rows_per_block = 1
    batch = tuple(b.to(DEV) for b in build_batch(case))
    noise = {k: v.to(DEV) for k, v in build_noise(case).items()}
    return case, model, batch, noise


def _train(model, batch, noise, **kw):  # noqa: ANN001, ANN003, ANN202
    model.zero_grad(set_to_none=True)
    out = model.shared_step(batch, noise, **kw)
    out["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items()}, grads


def _same_up_to_reruns(got: torch.Tensor, ref: torch.Tensor, ref2: torch.Tensor, what: str, *, exact: bool = True) -> None:
    """``exact``: bitwise when the unmasked path itself reruns bitwise.  Otherwise (and always for parameter gradients, whose
    reductions over B*T are not ordered the same across the two autograd graphs) within the rerun spread, floored at 2e-5 of
    the tensor's scale (the conv encoders' backward reruns differ by ~1e-5 of it)."""
    if exact and torch.equal(ref, ref2):
        assert torch.equal(got, ref), what
        return
    scale = float(ref.abs().max()) + 1e-12
    spread = float((ref2 - ref).abs().max())
    assert float((got - ref).abs().max()) <= max(4 * spread, 2e-5 * scale), what


def _mr(case) -> bool:  # noqa: ANN001
    return case.kind == "mrssm"


def _state_fields(case) -> tuple[str, ...]:  # noqa: ANN001
    return ("deter", "stoch") if _mr(case) else ("deter_l", "deter_h", "hidden_l", "hidden_h", "stoch_l", "stoch_h")


def _probs(case, state) -> list[torch.Tensor]:  # noqa: ANN001
    if _mr(case):
        return [state.distribution.probs]
    return [state.distribution_l.probs, state.distribution_h.probs]


def _kls(case, post) -> list[torch.Tensor]:  # noqa: ANN001
    return [post.kl_per_step] if _mr(case) else [post.kl_per_step, post.kl_h_per_step]


# 1. all present == no mask ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_all_present_equals_no_mask(name: str, onecu: bool) -> None:  # noqa: FBT001
    case, model, batch, noise = _setup(name, onecu)
    ones = torch.ones(case.batch, case.steps, 2, dtype=torch.bool, device=DEV)
    obs = (batch[1], batch[2])
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        s0b = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)  # (the conv encoders' reruns need not be bitwise)
        s0m = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise, modality_mask=ones[:, 0])
        for f in _state_fields(case):
            _same_up_to_reruns(getattr(s0m, f), getattr(s0, f), getattr(s0b, f), f)
        post, prior = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise)
        post2, prior2 = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise)
        postm, priorm = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise, modality_mask=ones)
    for f in _state_fields(case):
        _same_up_to_reruns(getattr(postm, f), getattr(post, f), getattr(post2, f), f)
    for i, (a, a2, b) in enumerate(zip(_probs(case, post) + _probs(case, prior) + _kls(case, post),
                                       _probs(case, post2) + _probs(case, prior2) + _kls(case, post2),
                                       _probs(case, postm) + _probs(case, priorm) + _kls(case, postm), strict=True)):
        _same_up_to_reruns(b, a, a2, f"rollout output {i}")
    ref, gref = _train(model, batch, noise)
    ref2, gref2 = _train(model, batch, noise)
    got, ggot = _train(model, batch, noise, modality_mask=ones)
    got7, ggot7 = _train(model, (*batch, ones), noise)  # the 7-tuple batch of the data pipeline
    assert set(got) == set(ref) == set(got7)
    assert set(ggot) == set(gref) == set(ggot7)
    for k in ref:
        # (the NLL sums end in fp32 atomics of several workgroups: a rerun may differ in the last bits)
        _same_up_to_reruns(got[k], ref[k], ref2[k], k, exact=False)
        _same_up_to_reruns(got7[k], ref[k], ref2[k], k, exact=False)
    for k in gref:
        _same_up_to_reruns(ggot[k], gref[k], gref2[k], k, exact=False)
        _same_up_to_reruns(ggot7[k], gref[k], gref2[k], k, exact=False)


# 2. observe q steps, then nothing == rollout_representation up to q, then rollout_transition ---------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_observe_then_imagine_is_one_masked_rollout(name: str, onecu: bool) -> None:  # noqa: FBT001
    case, model, batch, noise = _setup(name, onecu)
    q = min(case.query, case.steps - 1)
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool, device=DEV)
    mask[:, q:] = False
    obs = (batch[1], batch[2])
    upost = ("u_post",) if _mr(case) else ("u_post_l", "u_post_h")
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        postm, _ = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise, modality_mask=mask)
        head_noise = {k: noise[k][:, :q] for k in upost}
        post, _ = model.rollout_representation(actions=batch[0][:, :q], observations=(batch[1][:, :q], batch[2][:, :q]), prev_state=s0,
                                               noise=head_noise)
        tail_noise = {k.replace("post", "prior"): noise[k][:, q:] for k in upost}
        trans = model.rollout_transition(actions=batch[0][:, q:], prev_state=post[:, q - 1], noise=tail_noise)
    for f in _state_fields(case):
        a, b, c = getattr(postm, f), getattr(post, f), getattr(trans, f)
        if f.startswith("stoch"):
            assert torch.equal(a[:, :q], b), f
            assert torch.equal(a[:, q:], c), f
        else:
            torch.testing.assert_close(a[:, :q], b, rtol=0, atol=1e-5)
            torch.testing.assert_close(a[:, q:], c, rtol=0, atol=1e-5)
    for a, b, c in zip(_probs(case, postm), _probs(case, post), _probs(case, trans), strict=True):
        torch.testing.assert_close(a[:, :q], b, rtol=0, atol=1e-5)
        torch.testing.assert_close(a[:, q:], c, rtol=0, atol=1e-5)
    for kl in _kls(case, postm):
        assert torch.equal(kl[:, q:], torch.zeros_like(kl[:, q:]))
        assert bool((kl[:, :q] != 0).any())


# 4. isolation of an absent modality --------------------------------------------------------------------------------------
def _audio_params(model) -> dict[str, torch.nn.Parameter]:  # noqa: ANN001
    mods = {"audio_encoder": model.audio_encoder, "audio_representation": model.audio_representation.rnn_to_post_projector}
    return {f"{m}.{n}": p for m, mod in mods.items() for n, p in mod.named_parameters()}


@pytest.mark.parametrize(("name", "onecu"), [FAMILIES[0], FAMILIES[3], FAMILIES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_absent_audio_has_no_influence_and_no_gradient(name: str, onecu: bool) -> None:  # noqa: FBT001
    case, model, batch, noise = _setup(name, onecu)
    mask = torch.zeros(case.batch, case.steps, 2, dtype=torch.bool, device=DEV)
    mask[..., 1] = True
    out1, g1 = _train(model, batch, noise, modality_mask=mask)
    audio_params = _audio_params(model)
    for n, p in audio_params.items():
        assert p.grad is None or not bool(p.grad.any()), n
    perturbed = list(batch)
    perturbed[1] = batch[1] + torch.randn_like(batch[1])
    out2, g2 = _train(model, tuple(perturbed), noise, modality_mask=mask)
    for k in out1:
        assert torch.equal(out1[k], out2[k]), k
    assert set(g1) == set(g2)
    for k in g1:  # (weight-gradient GEMMs split their B*T reduction over fp32 atomics: equal up to the arrival order)
        assert float((g1[k] - g2[k]).abs().max()) <= 1e-6 * (float(g1[k].abs().max()) + 1e-12), k

    # observations=(audio, None): the vision encoder is never called; same states as the mask with vision absent
    def boom(*_args, **_kw) -> None:  # noqa: ANN002, ANN003
        raise AssertionError("the vision encoder ran for an absent modality")

    mask_a = torch.zeros_like(mask)
    mask_a[..., 0] = True
    with torch.no_grad():
        s_ref = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise, modality_mask=mask_a[:, 0])
        p_ref, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s_ref, noise=noise,
                                                modality_mask=mask_a)
        handle = model.vision_encoder.register_forward_hook(boom)
        try:
            s0 = model.initial_state((batch[1][:, 0], None), noise)
            post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], None), prev_state=s0, noise=noise)
        finally:
            handle.remove()
    for f in _state_fields(case):
        assert torch.equal(getattr(s0, f), getattr(s_ref, f)), f
        assert torch.equal(getattr(post, f), getattr(p_ref, f)), f


# 5. masked NLL kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 3])
@pytest.mark.parametrize(("B", "T", "event_shape"), [
    (2, 8, (1, 16, 8)),  # quads only, one frame per quad
    (2, 8, (3, 5, 7)),   # frames straddle quads
    (1, 3, (3, 5, 7)),   # n % 4 = 3: the scalar tail loops
    (1, 1, (1, 3, 3)),   # two quads and a tail
])
def test_masked_nll_matches_eager(act: int, B: int, T: int, event_shape: tuple[int, ...]) -> None:  # noqa: N803
    # (at most 2 workgroups at these sizes: the fp32 atomics of the sum add in a fixed order)
    g = torch.Generator(device=DEV).manual_seed(7)
    pred = torch.randn(B, T, *event_shape, device=DEV, generator=g)
    tgt = torch.rand(B, T, *event_shape, device=DEV, generator=g) * 2 - 1
    mask = torch.rand(B, T, device=DEV, generator=g) < 0.6
    mask[0, 0] = True
    event = math.prod(event_shape)

    p = pred.clone().requires_grad_()
    out = likelihood(p, tgt, 3, out_act=act, frame_mask=mask)
    out.backward()
    pe = pred.clone().requires_grad_()
    pa = torch.tanh(pe) if act else pe
    per_frame = (0.5 * (tgt - pa) ** 2).flatten(2).sum(-1) + 0.5 * math.log(2 * math.pi) * event
    ref = per_frame[mask].sum() / mask.sum()
    ref.backward()
    torch.testing.assert_close(out, ref.detach(), rtol=2e-6, atol=0)
    torch.testing.assert_close(p.grad, pe.grad, rtol=0, atol=1e-6 * float(pe.grad.abs().max()))
    assert not bool(p.grad[~mask].any())

    # every frame present: bitwise the unmasked kernel
    p1 = pred.clone().requires_grad_()
    p2 = pred.clone().requires_grad_()
    o1 = likelihood(p1, tgt, 3, out_act=act, frame_mask=torch.ones(B, T, dtype=torch.bool, device=DEV))
    o2 = likelihood(p2, tgt, 3, out_act=act)
    o1.backward()
    o2.backward()
    assert torch.equal(o1, o2)
    assert torch.equal(p1.grad, p2.grad)

    # no frame present: 0 and a zero gradient
    p0 = pred.clone().requires_grad_()
    o0 = likelihood(p0, tgt, 3, out_act=act, frame_mask=torch.zeros(B, T, dtype=torch.bool, device=DEV))
    o0.backward()
    assert float(o0) == 0.0
    assert not bool(p0.grad.any())


# 6. shared_step with a random mask; compute_reconstruction_loss ------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_cfg2dims", "mmtrssm_cfg3dims"])
def test_masked_step_recon_matches_compute_reconstruction_loss(name: str) -> None:
    case, model, batch, noise = _setup(name, False)
    g = torch.Generator(device=DEV).manual_seed(3)
    mask = torch.rand(case.batch, case.steps, 2, device=DEV, generator=g) < 0.6
    mask[:, 0, 0] = True
    mask[0, 1:3] = False  # some steps with no modality at all
    out = model.shared_step((*batch, mask), noise)
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise, modality_mask=mask[:, 0])
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise,
                                               modality_mask=mask)
        recon = model.compute_reconstruction_loss(model.decode_state(post), model.get_targets_from_batch(batch), mask)
    for k in ("recon/audio", "recon/vision"):
        torch.testing.assert_close(recon[k], out[k].detach(), rtol=1e-4, atol=0)
    torch.testing.assert_close(recon["recon"], out["recon"].detach(), rtol=1e-4, atol=0)
    # each term by hand from the decoder output: frames of the present modality only
    rec = model.decode_state(post)
    for j, k in enumerate(("recon/audio", "recon/vision")):
        tgt = model.get_targets_from_batch(batch)[k]
        per_frame = (0.5 * (tgt - rec[k].detach()) ** 2).flatten(2).sum(-1) + 0.5 * math.log(2 * math.pi) * tgt[0, 0].numel()
        m = mask[..., j]
        torch.testing.assert_close(out[k].detach(), per_frame[m].sum() / m.sum(), rtol=1e-4, atol=0)
    kls = _kls(case, post)
    assert torch.equal(kls[0][0, 1:3], torch.zeros_like(kls[0][0, 1:3]))
    kl_key = "kl"
    torch.testing.assert_close(out[kl_key].detach(), kls[0].mean() * float(model.kl_coeff), rtol=1e-5, atol=0)
    out["loss"].backward()  # the masked backward runs
    for n, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), n


def test_compute_reconstruction_loss_no_mask_runs() -> None:
    """The reference's signature (no mask) returns the summed term too (it raised NameError before)."""
    case, model, batch, noise = _setup("mrssm_cfg2dims", False)
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise)
        recon = model.compute_reconstruction_loss(model.decode_state(post), model.get_targets_from_batch(batch))
        out = model.shared_step(batch, noise)
    assert set(recon) == {"recon", "recon/audio", "recon/vision"}
    for k in recon:
        torch.testing.assert_close(recon[k], out[k], rtol=1e-4, atol=0)
