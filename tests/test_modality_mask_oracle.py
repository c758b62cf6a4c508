"""Masked MoPoE against an eager CPU restatement (DESIGN.md "Missing modalities"), forward and gradients.

The restatement below is the oracle's T loop (``oracle.ref_model``) with the masked mixture of the contract written out in
plain autograd: ``torch.where`` picks, per (b, t), the three-expert mixture, one expert's flat log-softmax or the prior's raw
logits, so the gradients of the unpicked branches are exactly zero and a "none" step's posterior gradient lands on the prior
logits.  A random mask with all four codes runs through every scan family; probabilities, samples, loss terms and every
parameter gradient are compared.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch
from torch import Tensor

from oracle.cases import CASES, build_batch, build_model, build_noise, min_margin
from oracle.ref_model import cat_probs, kl_loss, mopoe_mix, st_sample
from tests.conftest import product_from_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# (case, one-CU kernels forced): golden dims of both models, the bench frame sizes, and every scan family
FAMILIES = [
    ("mrssm_cfg2dims", False),    # cluster
    ("mrssm_default", False),     # cluster, D = 200
    ("mrssm_nonsquare", False),   # one-CU
    ("mrssm_cfg2dims", True),     # one-CU forced
    ("mrssm_large", False),       # wide
    ("mrssm_bench", False),       # B = 2, T = 50, real frame sizes
    ("mmtrssm_cfg3dims", False),
    ("mmtrssm_default", False),
    ("mmtrssm_default", True),
]
IDS = [f"{c}{'-onecu' if f else ''}" for c, f in FAMILIES]


def four_way_codes(B: int, T: int) -> Tensor:  # noqa: N803
    """Codes (bit 0 audio, bit 1 vision) with all four values in every row past t = 0; t = 0 observes something."""
    g = torch.Generator().manual_seed(11)
    codes = torch.randint(0, 4, (B, T), generator=g)
    codes[:, 1:5] = torch.tensor([0, 1, 2, 3])[: min(4, T - 1)]
    codes[:, 0] = torch.arange(B) % 3 + 1
    return codes


def mask_of(codes: Tensor) -> Tensor:
    return torch.stack([(codes & 1) != 0, (codes & 2) != 0], dim=-1)


def masked_mix(a_logits: Tensor, v_logits: Tensor, prior_logits: Tensor, code: Tensor) -> Tensor:
    """The contract's table: both -> MoPoE mix, one -> that expert's flat log-softmax, none -> the prior's raw logits."""
    c = code[:, None]
    both = mopoe_mix(a_logits, v_logits)
    la, lv = torch.log_softmax(a_logits, dim=-1), torch.log_softmax(v_logits, dim=-1)
    return torch.where(c == 3, both, torch.where(c == 1, la, torch.where(c == 2, lv, prior_logits)))  # noqa: PLR2004


def masked_embed0(ea: Tensor, ev: Tensor, code0: Tensor) -> Tensor:
    c = code0[:, None]
    return torch.where(c == 3, (ea + ev) / 2.0, torch.where(c == 1, ea, ev))  # noqa: PLR2004


def masked_nll(prediction: Tensor, target: Tensor, present: Tensor) -> Tensor:
    per_frame = (0.5 * (target - prediction) ** 2 + 0.5 * math.log(2.0 * math.pi)).flatten(2).sum(-1)
    if not bool(present.any()):
        return (per_frame * 0.0).sum()
    return per_frame[present].sum() / present.sum()


def oracle_mrssm_step(m, batch: tuple[Tensor, ...], noise: dict[str, Tensor], codes: Tensor) -> dict[str, Tensor]:  # noqa: ANN001
    d = m.dims
    act_in, audio_in, vision_in, _, audio_tgt, vision_tgt = batch
    audio_embed, vision_embed = m.audio_encoder(audio_in), m.vision_encoder(vision_in)
    deter = m.init_proj(masked_embed0(audio_embed[:, 0], vision_embed[:, 0], codes[:, 0]))
    logits0 = m.transition.rnn_to_prior_projector(deter)
    stoch = st_sample(cat_probs(logits0, d.cats, d.classes)[1], noise["u_init"])
    keep: dict[str, list[Tensor]] = {k: [] for k in ("deter", "prior_logits", "prior_stoch", "post_logits", "post_stoch")}
    for t in range(act_in.shape[1]):
        deter, prior_logits, prior_stoch = m._prior_step(act_in[:, t], deter, stoch, noise["u_prior"][:, t])  # noqa: SLF001
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter, vision_embed[:, t]], -1))
        post_logits = masked_mix(a_logits, v_logits, prior_logits, codes[:, t])
        stoch = st_sample(cat_probs(post_logits, d.cats, d.classes)[1], noise["u_post"][:, t])
        for k, v in zip(keep, (deter, prior_logits, prior_stoch, post_logits, stoch), strict=True):
            keep[k].append(v)
    roll = {k: torch.stack(v, dim=1) for k, v in keep.items()}
    feature = torch.cat([roll["deter"], roll["post_stoch"]], dim=-1)
    mask = mask_of(codes)
    nll_a = masked_nll(m.audio_decoder(feature), audio_tgt, mask[..., 0])
    nll_v = masked_nll(m.vision_decoder(feature), vision_tgt, mask[..., 1])
    kl = kl_loss(roll["post_logits"], roll["prior_logits"], d.cats, d.classes, d.use_kl_balancing) * d.kl_coeff
    out = {"loss": nll_a + nll_v + kl, "recon": nll_a + nll_v, "recon/audio": nll_a, "recon/vision": nll_v, "kl": kl}
    out.update({f"_{k}": v for k, v in roll.items()})
    out["_logits0"] = logits0
    return out


def oracle_mmtrssm_step(m, batch: tuple[Tensor, ...], noise: dict[str, Tensor], codes: Tensor) -> dict[str, Tensor]:  # noqa: ANN001, PLR0914
    d = m.dims
    act_in, audio_in, vision_in, _, audio_tgt, vision_tgt = batch
    audio_embed, vision_embed = m.audio_encoder(audio_in), m.vision_encoder(vision_in)
    h = m.init_proj(masked_embed0(audio_embed[:, 0], vision_embed[:, 0], codes[:, 0]))
    deter_h, deter_l = h[..., : d.hd], h[..., d.hd :]
    hidden_h, hidden_l = deter_h, deter_l
    init_h, init_l = m.h_prior(deter_h), m.l_prior(deter_l)
    stoch_h = st_sample(cat_probs(init_h, d.hs_cats, d.hs_classes)[1], noise["u_init_h"])
    stoch_l = st_sample(cat_probs(init_l, d.ls_cats, d.ls_classes)[1], noise["u_init_l"])
    names = ("deter_l", "deter_h", "hidden_l", "hidden_h", "prior_logits_l", "prior_logits_h", "prior_stoch_l", "prior_stoch_h",
             "post_logits_l", "post_logits_h", "post_stoch_l", "post_stoch_h")
    keep: dict[str, list[Tensor]] = {k: [] for k in names}
    for t in range(act_in.shape[1]):
        code = codes[:, t]
        deter_l, hidden_l = m.l_rnn(torch.cat([act_in[:, t], stoch_l, stoch_h], dim=-1), deter_l, hidden_l)
        prior_logits_l = m.l_prior(deter_l)
        a_logits = m.audio_representation.rnn_to_post_projector(torch.cat([deter_l, audio_embed[:, t]], -1))
        v_logits = m.vision_representation.rnn_to_post_projector(torch.cat([deter_l, vision_embed[:, t]], -1))
        post_logits_l = masked_mix(a_logits, v_logits, prior_logits_l, code)
        new_l = st_sample(cat_probs(post_logits_l, d.ls_cats, d.ls_classes)[1], noise["u_post_l"][:, t])
        deter_h, hidden_h = m.h_rnn(stoch_h, deter_h, hidden_h)
        prior_logits_h = m.h_prior(deter_h)
        post_logits_h = torch.where(code[:, None] == 0, prior_logits_h, m.h_posterior(torch.cat([deter_l, deter_h], dim=-1)))
        new_h = st_sample(cat_probs(post_logits_h, d.hs_cats, d.hs_classes)[1], noise["u_post_h"][:, t])
        prior_stoch_h = st_sample(cat_probs(prior_logits_h, d.hs_cats, d.hs_classes)[1], noise["u_prior_h"][:, t])
        prior_stoch_l = st_sample(cat_probs(prior_logits_l, d.ls_cats, d.ls_classes)[1], noise["u_prior_l"][:, t])
        stoch_l, stoch_h = new_l, new_h
        vals = (deter_l, deter_h, hidden_l, hidden_h, prior_logits_l, prior_logits_h, prior_stoch_l, prior_stoch_h, post_logits_l,
                post_logits_h, stoch_l, stoch_h)
        for k, v in zip(names, vals, strict=True):
            keep[k].append(v)
    roll = {k: torch.stack(v, dim=1) for k, v in keep.items()}
    feature = torch.cat([roll["deter_h"], roll["post_stoch_h"], roll["deter_l"], roll["post_stoch_l"]], dim=-1)
    mask = mask_of(codes)
    nll_a = masked_nll(m.audio_decoder(feature), audio_tgt, mask[..., 0])
    nll_v = masked_nll(m.vision_decoder(feature), vision_tgt, mask[..., 1])
    kl_l = kl_loss(roll["post_logits_l"], roll["prior_logits_l"], d.ls_cats, d.ls_classes, d.use_kl_balancing) * d.kl_coeff
    kl_h = kl_loss(roll["post_logits_h"], roll["prior_logits_h"], d.hs_cats, d.hs_classes, d.use_kl_balancing) * (d.kl_coeff * d.w_kl_h)
    out = {"loss": nll_a + nll_v + kl_l + kl_h, "recon": nll_a + nll_v, "recon/audio": nll_a, "recon/vision": nll_v, "kl": kl_l,
           "kl_h": kl_h}
    out.update({f"_{k}": v for k, v in roll.items()})
    out["_init_logits_h"], out["_init_logits_l"] = init_h, init_l
    return out


def oracle_step(case, oracle, batch, noise, codes) -> dict[str, Tensor]:  # noqa: ANN001
    return (oracle_mrssm_step if case.kind == "mrssm" else oracle_mmtrssm_step)(oracle, batch, noise, codes)


def screened(case, oracle, batch, codes, *, margin: float = 1e-4, first_seed: int = 100, tries: int = 40):  # noqa: ANN001, ANN201
    """``oracle.cases.screened_noise`` under the MASKED restatement: every draw keeps ``margin`` from the CDF edges."""
    best = None
    b, t = batch[0].shape[:2]
    for seed in range(first_seed, first_seed + tries):
        noise = build_noise(case, seed, batch=b, steps=t)
        with torch.no_grad():
            out = oracle_step(case, oracle, batch, noise, codes)
        m = min_margin(case, out, noise)
        if best is None or m > best[1]:
            best = (noise, m)
        if m >= margin:
            break
    assert best is not None
    return best


def _index(stoch: Tensor, cats: int, classes: int) -> np.ndarray:
    return stoch.detach().reshape(*stoch.shape[:-1], cats, classes).argmax(-1).cpu().numpy()


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_random_four_way_mask_matches_eager_restatement(name: str, onecu: bool) -> None:  # noqa: FBT001, PLR0914, PLR0915
    case = CASES[name]
    d = case.dims
    oracle = build_model(case)
    batch = build_batch(case)
    codes = four_way_codes(case.batch, case.steps)
    noise, margin = screened(case, oracle, batch, codes)
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"

    ref = oracle_step(case, oracle, batch, noise, codes)
    ref["loss"].backward()

    model = product_from_case(case, oracle, DEV)
    if onecu:
        model.scan_rows_per_block = 1
    dbatch = tuple(x.to(DEV) for x in batch)
    dnoise = {k: v.to(DEV) for k, v in noise.items()}
    mask = mask_of(codes).to(DEV)

    # forward: probabilities and samples of both rollouts, per step
    with torch.no_grad():
        s0 = model.initial_state((dbatch[1][:, 0], dbatch[2][:, 0]), dnoise, modality_mask=mask[:, 0])
        post, prior = model.rollout_representation(actions=dbatch[0], observations=(dbatch[1], dbatch[2]), prev_state=s0,
                                                   noise=dnoise, modality_mask=mask)
    if case.kind == "mrssm":
        levels = [(post.distribution.probs, post.stoch, prior.distribution.probs, prior.stoch, "", d.cats, d.classes)]
    else:
        levels = [(post.distribution_l.probs, post.stoch_l, prior.distribution_l.probs, prior.stoch_l, "_l", d.ls_cats, d.ls_classes),
                  (post.distribution_h.probs, post.stoch_h, prior.distribution_h.probs, prior.stoch_h, "_h", d.hs_cats, d.hs_classes)]
    for q_probs, q_stoch, p_probs, p_stoch, sfx, cats, classes in levels:
        want_q = cat_probs(ref[f"_post_logits{sfx}"].detach(), cats, classes)[1]
        want_p = cat_probs(ref[f"_prior_logits{sfx}"].detach(), cats, classes)[1]
        np.testing.assert_allclose(q_probs.cpu().numpy(), want_q.numpy(), rtol=0, atol=1e-5, err_msg=f"post probs{sfx}")
        np.testing.assert_allclose(p_probs.cpu().numpy(), want_p.numpy(), rtol=0, atol=1e-5, err_msg=f"prior probs{sfx}")
        assert (_index(q_stoch, cats, classes) == _index(ref[f"_post_stoch{sfx}"], cats, classes)).all(), f"post samples{sfx}"
        assert (_index(p_stoch, cats, classes) == _index(ref[f"_prior_stoch{sfx}"], cats, classes)).all(), f"prior samples{sfx}"
    kls = [post.kl_per_step] if case.kind == "mrssm" else [post.kl_per_step, post.kl_h_per_step]
    for kl in kls:
        none = (codes == 0).to(DEV)
        assert torch.equal(kl[none], torch.zeros_like(kl[none]))

    # loss terms and every parameter gradient of the masked training step
    out = model.shared_step((*dbatch, mask), dnoise)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert set(out) == {k for k in ref if not k.startswith("_")}
    for k in out:
        np.testing.assert_allclose(float(out[k]), float(ref[k]), rtol=1e-4, atol=1e-6, err_msg=k)
    got = dict(model.named_parameters())
    compared = 0
    for k, p in oracle.named_parameters():
        g_ref = p.grad if p.grad is not None else torch.zeros_like(p)
        g_got = got[k].grad
        g_got = torch.zeros_like(got[k]) if g_got is None else g_got
        scale = float(g_ref.abs().max())
        if scale == 0.0:
            assert float(g_got.abs().max()) == 0.0, f"grad {k} must be zero"
            continue
        np.testing.assert_allclose(g_got.cpu().numpy(), g_ref.numpy(), rtol=0, atol=2e-4 * scale, err_msg=f"grad {k}")
        compared += 1
    assert compared > 10
