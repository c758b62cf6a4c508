"""CPU: uniform mixing of the categorical latents, the reference side of ``tests/test_unimix_gpu.py``
(``tests/unimix_reference.py`` holds the loops) and the host plumbing.

1. at ``eps = 0`` the reference loops are the oracle's rollouts, bit for bit, for every case of ``FAMILY_CASES``;
2. at ``eps = 0.01`` every case finds a seed, fp32 draws float64's samples and the fp32 reference's gradients (``all``) stay within
   the family's ``HOST_BASELINE`` of float64's: the GPU bounds of ``tests/scan_cotangents.py`` hold as they are;
3. with the heads' last layers scaled by 60 every KL per step is at most ``K log(C / eps)`` (above 100 without unimix), every mixed
   probability at least ``eps / C``, and the fp32 reference's KL error against float64 (what the GPU test's saturated bound is 16 x
   of) is printed;
4. the factory, the model property, the range check and the state dict;
5. the C ABI rejects ``unimix`` outside ``[0, 1)`` before anything else, and dims built without the field carry 0."""

from __future__ import annotations

import ctypes as C
import functools
import math

import pytest
import torch

from oracle.cases import CASES
from oracle.ref_model import cat_probs
from tests.config_matrix import SAMPLING_MARGIN
from tests.conftest import product_from_case
from tests.scan_cotangents import FAMILY_CASES, HOST_BASELINE, Problem, build_problem, cast_inputs, levels, relative_error, sample_index
from tests.unimix_reference import (EPS, build_unimix_problem, kl_bound, saturated_kl_error, unimix_gradients,
                                    unimix_outputs)

ALL_CASES = [(family, case_id) for family, ids in FAMILY_CASES.items() for case_id in ids]
SATURATED = [(family, ids[0]) for family, ids in FAMILY_CASES.items()]


@functools.lru_cache(maxsize=None)
def _problem(case_id: str) -> Problem:
    return build_unimix_problem(case_id, EPS)


# ---------------------------------------------------------------------------------------------
# 1. eps = 0: the oracle's own rollout
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("family", "case_id"), ALL_CASES, ids=[c for _, c in ALL_CASES])
def test_reference_at_eps_zero_is_the_oracle_bit_for_bit(family: str, case_id: str) -> None:
    pr = build_problem(case_id)
    assert pr.family == family
    leaves = {k: v.detach() for k, v in cast_inputs(pr, torch.float32).items()}
    state0 = {k: leaves[k] for k in leaves if k not in {"actions", "audio_embed", "vision_embed"}}
    a, ea, ev = leaves["actions"], leaves["audio_embed"], leaves["vision_embed"]
    with torch.no_grad():
        got = unimix_outputs(pr.oracle, pr, leaves, pr.noise, 0.0)
        want = (pr.oracle.rollout_representation(a, ea, ev, state0, pr.noise["u_prior"], pr.noise["u_post"]) if pr.case.kind == "mrssm"
                else pr.oracle.rollout_representation(a, ea, ev, state0, pr.noise))
    compared = 0
    for key, value in got.items():
        if key.startswith("kl"):
            continue
        assert torch.equal(value, want[key]), key
        compared += 1
    assert compared == (5 if pr.case.kind == "mrssm" else 12)


# ---------------------------------------------------------------------------------------------
# 2. eps = 0.01: seeds, samples, the fp32 reference's gradient error
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("family", "case_id"), ALL_CASES, ids=[c for _, c in ALL_CASES])
def test_seed_samples_and_fp32_gradient_error_at_eps(family: str, case_id: str) -> None:
    pr = _problem(case_id)
    assert pr.margin >= SAMPLING_MARGIN
    out32, g32 = unimix_gradients(pr.oracle, pr, "all", EPS)
    out64, g64 = unimix_gradients(pr.ref64, pr, "all", EPS)
    for sfx, cats, classes in levels(pr.case):
        for which in ("post", "prior"):
            key = f"{which}_stoch{sfx}"
            assert torch.equal(sample_index(out32[key], cats, classes), sample_index(out64[key], cats, classes)), key
    worst, compared = (0.0, ""), 0
    for name, want in g64.items():
        if want is None or float(want.abs().max()) == 0.0:
            assert g32[name] is None or float(g32[name].abs().max()) == 0.0, name
            continue
        err = relative_error(g32[name], want)
        compared += 1
        if err > worst[0]:
            worst = (err, name)
    print(f"unimix {case_id} ({family}): seed {pr.seed}, margin {pr.margin:.2e}, largest fp32-reference gradient error {worst[0]:.2e} at {worst[1]}")
    assert compared >= 10  # noqa: PLR2004
    assert worst[0] <= HOST_BASELINE[family], (worst, HOST_BASELINE[family])


# ---------------------------------------------------------------------------------------------
# 3. saturated heads: the KL is bounded at its source
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("family", "case_id"), SATURATED, ids=[c for _, c in SATURATED])
def test_saturated_heads_kl_is_bounded(family: str, case_id: str) -> None:
    pr = build_unimix_problem(case_id, EPS, saturated=True)
    leaves = {k: v.detach() for k, v in cast_inputs(pr, torch.float64).items()}
    with torch.no_grad():
        mixed = unimix_outputs(pr.ref64, pr, leaves, pr.noise, EPS)
        raw = unimix_outputs(pr.ref64, pr, leaves, pr.noise, 0.0)
    for sfx, cats, classes in levels(pr.case):
        bound = kl_bound(cats, classes, EPS)
        kl, kl_raw = mixed[f"kl{sfx}"], raw[f"kl{sfx}"]
        print(f"unimix saturated {case_id}{sfx}: KL per step {float(kl.min()):.2f} .. {float(kl.max()):.2f} <= {bound:.2f}; "
              f"without unimix {float(kl_raw.min()):.1f} .. {float(kl_raw.max()):.1f}")
        assert float(kl.max()) <= bound
        # (the unbounded tail is the largest step: one step of a rollout may well have a small KL, saturated or not)
        assert float(kl_raw.max()) > 100.0  # noqa: PLR2004
        for which in ("post", "prior"):
            probs = cat_probs(mixed[f"{which}_logits{sfx}"], cats, classes)[1]
            # (the float64 softmax of the stored log-probabilities re-rounds the mixed value: one part in 1e12 of slack)
            assert float(probs.min()) >= EPS / classes * (1.0 - 1e-12), (which, sfx)
    err, scale = saturated_kl_error(pr, EPS)
    print(f"unimix saturated {case_id} ({family}): fp32-reference KL error against float64 {err:.2e} on values up to {scale:.1f}")
    assert err < 1e-3  # noqa: PLR2004  (a sanity check of the measurement; the GPU test's bound is 16 x the figure itself)


# ---------------------------------------------------------------------------------------------
# 4. factory, model property, state dict
# ---------------------------------------------------------------------------------------------
def test_factory_probabilities_follow_the_formula() -> None:
    import multimodal_mtrssm_amd as mt

    cats, classes, eps = 5, 6, 0.25
    logits = 4.0 * torch.randn(7, cats * classes, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    plain = mt.MultiOneHotFactory(class_size=classes, category_size=cats)
    mixed = mt.MultiOneHotFactory(classes, cats, unimix=eps)
    assert plain.unimix == 0.0 and mixed.unimix == eps
    want = (1.0 - eps) * torch.softmax(logits.reshape(7, cats, classes), dim=-1) + eps / classes
    dist = mixed(logits)
    torch.testing.assert_close(dist.probs, want, rtol=1e-13, atol=1e-15)
    torch.testing.assert_close(dist.probs.sum(-1), torch.ones(7, cats, dtype=torch.float64), rtol=1e-13, atol=0)
    torch.testing.assert_close(dist.logits, want.log(), rtol=1e-12, atol=1e-13)
    assert float(dist.probs.min()) >= eps / classes
    assert torch.equal(plain(logits).probs, mixed.unmixed(logits).probs)  # the scans' outputs and the initial head: as they are
    assert torch.equal(plain(logits).probs, mt.MultiOneHotFactory(classes, cats, unimix=0.0)(logits).probs)
    assert list(mixed.state_dict()) == [] and list(mixed.parameters()) == [] and list(mixed.buffers()) == []


def _models(unimix: float | None):  # noqa: ANN202
    import multimodal_mtrssm_amd as mt

    kw = {} if unimix is None else {"unimix": unimix}
    d = CASES["mrssm_nonsquare"].dims
    mr = mt.make_mrssm(deter=d.deter, hidden=d.hidden, classes=d.classes, cats=d.cats, action=d.action, embed=d.embed,
                       enc_audio=d.enc_audio, enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision, **kw)
    d = CASES["mmtrssm_default"].dims
    mm = mt.make_mmtrssm(hd=d.hd, hs=(d.hs_classes, d.hs_cats), ld=d.ld, ls=(d.ls_classes, d.ls_cats), hidden=d.hidden, action=d.action,
                         embed=d.embed, enc_audio=d.enc_audio, enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision, **kw)
    return mr, mm


def _factories(model) -> list:  # noqa: ANN001
    found = [model.transition.distribution_factory, model.audio_representation.distribution_factory,
             model.representation.distribution_factory, model.vision_representation.distribution_factory]
    return found + ([model.l_dist, model.h_dist] if hasattr(model, "l_dist") else [])


def test_model_unimix_reaches_every_factory_and_adds_no_state() -> None:
    from multimodal_mtrssm_amd import scan

    for plain, mixed in zip(_models(None), _models(0.01), strict=True):
        assert plain.unimix == 0.0 and all(f.unimix == 0.0 for f in _factories(plain))
        assert mixed.unimix == 0.01 and all(f.unimix == 0.01 for f in _factories(mixed))  # noqa: PLR2004
        assert list(plain.state_dict()) == list(mixed.state_dict())
        assert [n for n, _ in plain.named_buffers()] == [n for n, _ in mixed.named_buffers()]
        plain.unimix = 0.2
        assert plain.unimix == 0.2 and all(f.unimix == 0.2 for f in _factories(plain))  # noqa: PLR2004
        assert list(plain.state_dict()) == list(mixed.state_dict())
        for bad in (1.0, -0.1, float("nan"), 1.5):
            with pytest.raises(ValueError, match="unimix"):
                plain.unimix = bad
        assert plain.unimix == 0.2  # noqa: PLR2004  (a rejected value changes nothing)
        plain.vision_representation.distribution_factory.unimix = 0.1  # factories that disagree: the scans refuse
        with pytest.raises(ValueError, match="unimix"):
            _ = plain.unimix
        with pytest.raises(ValueError, match="unimix"):
            scan.unimix_of(*_factories(plain))
    import multimodal_mtrssm_amd as mt

    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="unimix"):
            mt.MultiOneHotFactory(4, 4, unimix=bad)
        with pytest.raises(ValueError, match="unimix"):
            _models(bad)


def test_eager_heads_apply_the_factory_transform() -> None:
    """``Representation.forward`` (the eager per-step API) returns the mixed distribution of its head's logits."""
    case = CASES["mrssm_nonsquare"]
    from oracle.cases import build_model

    model = product_from_case(case, build_model(case), "cpu")
    d = case.dims
    g = torch.Generator().manual_seed(5)
    from multimodal_mtrssm_amd.state import State

    deter = torch.randn(3, d.deter, generator=g)
    embed = torch.randn(3, d.embed, generator=g)
    prior = State(deter=deter, distribution=model.transition.distribution_factory.unmixed(torch.zeros(3, d.stoch)), stoch=torch.zeros(3, d.stoch))
    raw = model.audio_representation(embed, prior).distribution.probs
    model.unimix = 0.3
    mixed = model.audio_representation(embed, prior).distribution.probs
    torch.testing.assert_close(mixed, 0.7 * raw + 0.3 / d.classes, rtol=1e-5, atol=1e-7)


# ---------------------------------------------------------------------------------------------
# 5. the C ABI
# ---------------------------------------------------------------------------------------------
def test_capi_rejects_unimix_out_of_range_before_anything_else() -> None:
    from multimodal_mtrssm_amd import _lib

    lib = _lib.load()
    mr = _lib.MrssmDims(2, 4, 8, 8, 2, 2, 2, 1, 0.2, 0.8, 0, 0)
    mt = _lib.MmtrssmDims(2, 4, 8, 8, 8, 2, 2, 2, 2, 2, 1, 2.0, 4.0, 0.5, 0.75, 0.2, 0.8, 0, 0)
    assert mr.unimix == 0.0 and mt.unimix == 0.0  # positional construction without the field
    assert C.sizeof(_lib.MrssmDims) == 13 * 4 and C.sizeof(_lib.MmtrssmDims) == 20 * 4
    null = None
    calls = {
        "mrssm_rollout_fwd": lambda d: lib.mtrssm_mrssm_rollout_fwd(C.byref(d), C.byref(_lib.MrssmFwdWeights()), C.byref(_lib.MrssmFwdIO()), null),
        "mrssm_rollout_bwd": lambda d: lib.mtrssm_mrssm_rollout_bwd(C.byref(d), C.byref(_lib.MrssmBwdWeights()), C.byref(_lib.MrssmBwdIO()), null),
        "mrssm_rollout_fwd_cluster": lambda d: lib.mtrssm_mrssm_rollout_fwd_cluster(C.byref(d), C.byref(_lib.MrssmClusterWeights()),
                                                                                    C.byref(_lib.MrssmFwdIO()), null, 0, null),
        "mrssm_rollout_bwd_cluster": lambda d: lib.mtrssm_mrssm_rollout_bwd_cluster(C.byref(d), C.byref(_lib.MrssmClusterWeights()),
                                                                                    C.byref(_lib.MrssmBwdIO()), null, 0, null),
        "mrssm_rollout_fwd_wide": lambda d: lib.mtrssm_mrssm_rollout_fwd_wide(C.byref(d), C.byref(_lib.MrssmClusterWeights()),
                                                                              C.byref(_lib.MrssmFwdIO()), 3, null, 0, null),
        "mrssm_rollout_bwd_wide": lambda d: lib.mtrssm_mrssm_rollout_bwd_wide(C.byref(d), C.byref(_lib.MrssmClusterWeights()),
                                                                              C.byref(_lib.MrssmBwdIO()), 3, null, 0, null),
    }
    mt_calls = {
        "mmtrssm_rollout_fwd": lambda d: lib.mtrssm_mmtrssm_rollout_fwd(C.byref(d), C.byref(_lib.MmtrssmFwdWeights()), C.byref(_lib.MmtrssmFwdIO()), null),
        "mmtrssm_rollout_bwd": lambda d: lib.mtrssm_mmtrssm_rollout_bwd(C.byref(d), C.byref(_lib.MmtrssmBwdWeights()), C.byref(_lib.MmtrssmBwdIO()), null),
        "mmtrssm_rollout_fwd_wide": lambda d: lib.mtrssm_mmtrssm_rollout_fwd_wide(C.byref(d), C.byref(_lib.MmtrssmFwdWeights()),
                                                                                  C.byref(_lib.MmtrssmFwdIO()), 3, null, 0, null),
        "mmtrssm_rollout_bwd_wide": lambda d: lib.mtrssm_mmtrssm_rollout_bwd_wide(C.byref(d), C.byref(_lib.MmtrssmBwdWeights()),
                                                                                  C.byref(_lib.MmtrssmBwdIO()), 3, null, 0, null),
    }
    kernel_before = lib.mtrssm_last_kernel()
    for dims, table in ((mr, calls), (mt, mt_calls)):
        for name, call in table.items():
            dims.unimix = 0.0
            assert call(dims) != 0 and b"unimix" not in lib.mtrssm_last_error(), name  # (null pointers or unsupported dims: its usual error)
            for bad in (1.0, -0.1, float("nan"), 2.0):
                dims.unimix = bad
                assert call(dims) == -1, (name, bad)  # MTRSSM_EINVAL
                assert b"unimix" in lib.mtrssm_last_error(), (name, bad, lib.mtrssm_last_error())
            dims.unimix = math.nextafter(1.0, 0.0)  # the largest float below 1 rounds to 1.0f: rejected as well
            assert call(dims) == -1 and b"unimix" in lib.mtrssm_last_error(), name
            dims.unimix = 0.5
            assert call(dims) != 0 and b"unimix" not in lib.mtrssm_last_error(), name
    assert lib.mtrssm_last_kernel() == kernel_before  # nothing was launched


def test_supported_functions_ignore_unimix() -> None:
    from multimodal_mtrssm_amd import _lib

    lib = _lib.load()
    for unimix in (0.0, 0.01, 5.0):
        large = _lib.MrssmDims(32, 100, 1024, 1024, 16, 8, 2, 1, 0.2, 0.8, 0, 0, unimix)
        base = _lib.MrssmDims(32, 100, 1024, 1024, 16, 8, 2, 1, 0.2, 0.8, 0, 0)
        assert lib.mtrssm_mrssm_wide_supported(C.byref(large), 3) == lib.mtrssm_mrssm_wide_supported(C.byref(base), 3)
        assert lib.mtrssm_mrssm_wide_workspace_bytes(C.byref(large), 3) == lib.mtrssm_mrssm_wide_workspace_bytes(C.byref(base), 3)
        assert lib.mtrssm_mrssm_cluster_supported(C.byref(large)) == lib.mtrssm_mrssm_cluster_supported(C.byref(base))
