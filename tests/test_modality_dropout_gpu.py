"""Modality dropout on the GPU: the sampler kernel against its torch restatement, dropout steps against
explicit-mask steps, masked steps inside the captured hipGraph against the eager sequence, data-parallel exactness of the loss.

Tolerances are not chosen here.  Eager comparisons use the rerun yardstick of ``test_modality_mask_gpu.py`` (restated below),
graph-vs-eager the criteria of ``test_gpu_parity.test_captured_train_step_matches_eager``, the data-parallel loss terms the
``rtol = 1e-5`` of ``test_gpu_parity.test_bench_model_full_batch_properties``.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import ModalityDropout, scan
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from multimodal_mtrssm_amd.parallel import GlobalRowNoise
from oracle.cases import CASES, build_batch, build_model, build_noise, with_sizes
from tests.conftest import product_from_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _setup(name: str, sizes: tuple[int, int] | None = None):  # noqa: ANN202
    case = CASES[name] if sizes is None else with_sizes(CASES[name], *sizes)
    model = product_from_case(case, build_model(case), DEV)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    noise = {k: v.to(DEV) for k, v in build_noise(case).items()}
    return case, model, batch, noise


def _train(model, batch, noise, **kw):  # noqa: ANN001, ANN003, ANN202
    model.zero_grad(set_to_none=True)
    out = model.shared_step(batch, noise, **kw)
    out["loss"].backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items()}, grads


def _same_up_to_reruns(got: torch.Tensor, ref: torch.Tensor, ref2: torch.Tensor, what: str) -> None:
    """The yardstick of ``test_modality_mask_gpu._same_up_to_reruns`` (its ``exact=False`` form, the one it applies to loss terms
    and parameter gradients): within four times the spread of a rerun of the reference itself, floored at 2e-5 of the tensor's
    scale (the conv encoders' backward reruns differ by ~1e-5 of it)."""
    scale = float(ref.abs().max()) + 1e-12
    spread = float((ref2 - ref).abs().max())
    err = float((got - ref).abs().max())
    print(f"{what}: err {err:.3e} rerun spread {spread:.3e} scale {scale:.3e}")
    assert err <= max(4 * spread, 2e-5 * scale), what


def _u_mask(md: ModalityDropout, B: int, T: int, seed: int) -> torch.Tensor:  # noqa: N803
    """Seeded uniforms (host generator: the same numbers wherever the test runs) whose first rows are built by hand so that
    the t = 0 fix-up certainly fires: both below p with audio larger, with vision larger, and a tie."""
    u = torch.rand(md.noise_shape(B, T), generator=torch.Generator().manual_seed(seed))
    pa, pv = md.p_audio, md.p_vision
    if pa > 0 and pv > 0:
        lo = min(pa, pv)
        hand = [(0.5 * lo, 0.25 * lo), (0.25 * lo, 0.5 * lo), (0.5 * lo, 0.5 * lo)]
        for b, (a, v) in enumerate(hand[:B]):
            u[b, 0, 0], u[b, 0, 1] = a, v
    return u.to(DEV)


# 1. the sampler kernel == the rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64])
@pytest.mark.parametrize("T", [1, 6, 50])
def test_sampler_matches_reference_exactly(B: int, T: int) -> None:  # noqa: N803
    fired = 0
    for span in (1, 4, 7):
        for p in ((0.0, 0.0), (0.3, 0.3), (0.9, 0.9), (0.3, 0.9), (0.9, 0.0)):
            md = ModalityDropout(*p, span=span)
            u = _u_mask(md, B, T, seed=1000 * B + 10 * T + span)
            ref = md.reference(u, T)
            plain = (u[:, torch.arange(T, device=DEV) // span] >= torch.tensor(p, device=DEV))
            fired += int((ref[:, 0] != plain[:, 0]).any())
            assert bool(ref[:, 0].any(dim=-1).all())
            want_counts = ref.sum(dim=(0, 1)).to(torch.float32)
            for world in ((1, 2) if B % 2 == 0 else (1,)):
                local = B // world
                for rank in range(world):
                    s = md.sample(u, T, world=world, rank=rank)
                    rows = ref[rank * local : (rank + 1) * local]
                    what = f"B {B} T {T} span {span} p {p} rank {rank}/{world}"
                    assert s.codes.dtype == torch.int32 and torch.equal(s.codes, scan.modality_codes(rows)), what
                    assert torch.equal(s.present_audio, rows[..., 0].reshape(-1).float()), what
                    assert torch.equal(s.present_vision, rows[..., 1].reshape(-1).float()), what
                    assert s.mask0.dtype == torch.bool and torch.equal(s.mask0, rows[:, 0]), what
                    assert torch.equal(s.counts, want_counts), what  # the GLOBAL counts, the same on every rank
                    assert torch.equal(s.mask, rows), what
                    sm = s.step_mask()
                    assert float(sm.count_audio) == float(want_counts[0]) / world and float(sm.count_vision) == float(want_counts[1]) / world
            if p == (0.0, 0.0):
                assert bool(ref.all())
    assert fired >= 3  # the hand-built rows took the fix-up branch (every span, both p > 0)


# 2. p = (0, 0) is the unmasked step -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_cfg2dims", "mmtrssm_cfg3dims"])
def test_zero_probability_is_the_unmasked_step(name: str) -> None:
    _, model, batch, noise = _setup(name)
    ref, gref = _train(model, batch, noise)
    ref2, gref2 = _train(model, batch, noise)
    got, ggot = _train(model, batch, noise, modality_dropout=ModalityDropout(0.0, 0.0, span=3))
    assert set(got) == set(ref) and set(ggot) == set(gref)
    for k in ref:
        _same_up_to_reruns(got[k], ref[k], ref2[k], k)
    for k in gref:
        _same_up_to_reruns(ggot[k], gref[k], gref2[k], k)


# 3. eager dropout step == eager step fed the explicit mask --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_cfg2dims", "mmtrssm_cfg3dims"])
def test_dropout_step_is_the_explicit_mask_step(name: str) -> None:
    case, model, batch, noise = _setup(name)
    md = ModalityDropout(0.3, 0.4, span=2)
    u = _u_mask(md, case.batch, case.steps, seed=5)
    mask = md.reference(u, case.steps)
    assert not bool(mask.all()) and bool((~mask.any(dim=-1)).any())  # something is dropped, some step has no modality
    ref, gref = _train(model, batch, noise, modality_mask=mask)
    ref2, gref2 = _train(model, batch, noise, modality_mask=mask)
    got, ggot = _train(model, batch, {**noise, "u_mask": u}, modality_dropout=md)
    assert set(got) == set(ref) and set(ggot) == set(gref)
    for k in ref:
        _same_up_to_reruns(got[k], ref[k], ref2[k], k)
    for k in gref:
        _same_up_to_reruns(ggot[k], gref[k], gref2[k], k)
    # without noise["u_mask"] the step draws its own uniforms and runs
    out = model.shared_step(batch, noise, modality_dropout=md)
    assert bool(torch.isfinite(out["loss"]))


# 4. masked steps in the captured graph == the eager sequence ---------------------------------------------------------------------------
def _random_masks(steps: int, B: int, T: int, seed: int) -> list[torch.Tensor]:  # noqa: N803
    g = torch.Generator().manual_seed(seed)
    masks = []
    for _ in range(steps):
        m = torch.rand(B, T, 2, generator=g) < 0.6
        m[:, 0, 0] = True
        masks.append(m.to(DEV))
    return masks


@pytest.mark.parametrize("mode", ["dropout", "masked"])
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default", "mrssm_cfg2dims"])
def test_captured_masked_step_matches_eager(name: str, mode: str) -> None:
    """As ``test_captured_train_step_matches_eager`` (same cases, sizes, learning rate, seed, five steps, same criteria), with
    a different modality mask every step: sampled inside the graph (``dropout``) or handed in with the batch (``masked``)."""
    case = with_sizes(CASES[name], 6, 9)
    oracle = build_model(case)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    md = ModalityDropout(0.4, 0.3, span=2)
    masks = _random_masks(5, 6, 9, seed=21)
    results = {}
    for run in ("eager", "graph"):
        model = product_from_case(case, oracle, DEV)
        if mode == "dropout":
            model.modality_dropout = md
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(6, 9)
        assert ("u_mask" in shapes) == (mode == "dropout")
        losses = []
        start = flat.param.clone()
        if run == "eager":
            for i in range(5):
                noise = source.draw(shapes)
                opt.zero_grad()
                if mode == "dropout":
                    out = model.shared_step(batch, noise, modality_dropout=md)
                else:
                    out = model.shared_step((*batch, masks[i]), noise)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v) for k, v in out.items()})
        else:
            if mode == "dropout":
                cap = CapturedTrainStep(model, flat, opt, dp, batch, source, warmup=3, modality_dropout=md)
            else:
                cap = CapturedTrainStep(model, flat, opt, dp, (*batch, masks[0]), source, warmup=3, masked=True)
            for i in range(5):
                out = cap.step() if mode == "dropout" else cap.step((*batch, masks[i]))
                losses.append({k: float(v) for k, v in out.items()})
            assert float(opt.state[1]) == 5.0 and opt.steps == 5
            with pytest.raises(ValueError, match="6-tuple|7-tuple"):  # the other kind of batch: refused, nothing replayed
                cap.step((*batch, masks[0]) if mode == "dropout" else batch)
            assert float(opt.state[1]) == 5.0
            cap.close()
        scan.check_cluster_status()
        moved = (flat.param - start).abs()
        assert float(moved.max()) > 3e-5
        results[run] = (losses, flat.param.clone())
    keys = list(results["eager"][0][0])
    assert list(results["graph"][0][0]) == keys
    for k in keys:
        got, want = [s[k] for s in results["graph"][0]], [s[k] for s in results["eager"][0]]
        print(name, mode, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    audio = [s["recon/audio"] for s in results["eager"][0]]
    assert len(set(audio)) == 5  # a different mask (and noise) every step
    diff = (results["graph"][1] - results["eager"][1]).abs()
    print(name, mode, "param diff max", float(diff.max()), "mean", float(diff.mean()))
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))


def _audio_grads(model) -> dict[str, torch.Tensor]:  # noqa: ANN001
    mods = {"audio_encoder": model.audio_encoder, "audio_head": model.audio_representation.rnn_to_post_projector}
    return {f"{m}.{n}": p.grad for m, mod in mods.items() for n, p in mod.named_parameters()}


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_a_replay_reads_the_mask_of_its_step(name: str) -> None:
    """``masked=True``: replays with audio everywhere, at t = 0 only, nowhere, and everywhere again.  The gradient buffer after
    a replay is that step's.  A parameter gradient cannot separate the t = 0 frames' share from the later frames', so "exactly
    zero" is asserted where the whole contribution must vanish: audio at no step (vision keeps t = 0 valid) gives the audio
    encoder and the audio posterior head exactly zero gradient, as in the eager ``test_absent_audio_has_no_influence_and_no_
    gradient``; the t = 0-only replay keeps a non-zero one (the initial embedding and the t = 0 scan step) and changes
    ``recon/audio``'s divisor to B frames."""
    case = with_sizes(CASES[name], 6, 9)
    model = product_from_case(case, build_model(case), DEV)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
    every = torch.ones(6, 9, 2, dtype=torch.bool, device=DEV)
    first_only = every.clone()
    first_only[:, 1:, 0] = False
    nowhere = every.clone()
    nowhere[..., 0] = False
    cap = CapturedTrainStep(model, flat, opt, dp, (*batch, every), dp.noise_source(seed=3), warmup=2, masked=True)
    seen = []
    for mask in (every, first_only, nowhere, every):
        out = cap.step((*batch, mask))
        torch.cuda.synchronize()
        seen.append((float(out["recon/audio"]), {k: g.clone() for k, g in _audio_grads(model).items()}))
    cap.close()
    for i in (0, 1, 3):
        assert seen[i][0] > 0.0
        assert any(bool(g.any()) for g in seen[i][1].values()), i
        for part in ("audio_encoder", "audio_head"):
            assert any(bool(g.any()) for k, g in seen[i][1].items() if k.startswith(part)), (i, part)
    assert seen[2][0] == 0.0  # no audio frame: the term is 0
    for k, g in seen[2][1].items():
        assert not bool(g.any()), k
    # fewer audio steps, smaller audio-head gradient: t = 0 alone is one of nine scan steps
    head = [sum(float(g.abs().sum()) for k, g in s[1].items() if k.startswith("audio_head")) for s in seen]
    assert head[1] < head[0] and head[1] < head[3]


def test_invalid_first_frame_raises_before_any_replay() -> None:
    case = with_sizes(CASES["mrssm_default"], 6, 9)
    model = product_from_case(case, build_model(case), DEV)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
    good = torch.ones(6, 9, 2, dtype=torch.bool, device=DEV)
    cap = CapturedTrainStep(model, flat, opt, dp, (*batch, good), dp.noise_source(seed=3), warmup=2, masked=True)
    cap.step((*batch, good))
    torch.cuda.synchronize()
    before, count = flat.param.clone(), float(opt.state[1])
    bad = good.clone()
    bad[4, 0] = False  # row 4 observes nothing at t = 0
    with pytest.raises(ValueError, match="t = 0"):
        cap.step((*batch, bad))
    torch.cuda.synchronize()
    assert float(opt.state[1]) == count == 1.0 and opt.steps == 1
    assert torch.equal(flat.param, before)
    assert torch.equal(cap.mask, good)  # the refused mask never reached the graph's buffer
    cap.step((*batch, good))
    assert float(opt.state[1]) == 2.0
    cap.close()


# 5. data-parallel exactness of the masked loss ---------------------------------------------------------------------------------------
DP_SEED = 3  # ModalityDropout(0.5, 0.3, span=10), B = 64, T = 50: reference() on the host gives 823 / 722 audio frames per half


@pytest.mark.parametrize("name", ["mrssm_bench"])
def test_dropout_loss_is_exact_under_data_parallel_sharding(name: str) -> None:
    """B = 64 on one rank against its two 32-row halves, each run as rank r of 2 (``GlobalRowNoise(world=2, rank=r)``,
    ``for_rank(2, r)``): the rank-mean of every loss term equals the single-rank term by the ``rtol = 1e-5`` of
    ``test_bench_model_full_batch_properties``, and the gradients summed over the halves and scaled by 1 / 2 equal the
    single-rank gradients.  (That test compares scalars only; for gradient tensors, whose B*T reductions end in fp32 atomics,
    the rerun yardstick above is the project's measure of "equal".)  With today's per-rank counts -- the same masks handed in as
    explicit masks -- the same comparison must FAIL: the halves' audio present-frame counts differ by 13 %."""
    case, model, batch, _ = _setup(name, (64, 50))
    md = ModalityDropout(0.5, 0.3, span=10)
    u = torch.rand(md.noise_shape(64, 50), generator=torch.Generator().manual_seed(DP_SEED)).to(DEV)
    mask = md.reference(u, 50)
    counts = [mask[h].sum(dim=(0, 1)).tolist() for h in (slice(0, 32), slice(32, 64))]
    print("present frames per half (audio, vision):", counts)
    assert abs(counts[0][0] - counts[1][0]) > 0.05 * (counts[0][0] + counts[1][0]) / 2  # audio: visibly different halves
    shapes_full, shapes_half = model.noise_shapes(64, 50), model.noise_shapes(32, 50)
    full_noise = {**GlobalRowNoise(17, 1, 0, DEV).draw(shapes_full), "u_mask": u}
    ref, gref = _train(model, batch, full_noise, modality_dropout=md)
    ref2, gref2 = _train(model, batch, full_noise, modality_dropout=md)
    exact, today = [], []
    for r, h in enumerate((slice(0, 32), slice(32, 64))):
        noise = GlobalRowNoise(17, 2, r, DEV).draw(shapes_half)
        sub = tuple(x[h] for x in batch)
        exact.append(_train(model, sub, {**noise, "u_mask": u}, modality_dropout=md.for_rank(2, r)))
        today.append(_train(model, sub, noise, modality_mask=mask[h]))
    for k in ref:
        mean = 0.5 * (float(exact[0][0][k]) + float(exact[1][0][k]))
        print(f"{k}: one rank {float(ref[k]):.8g} rank-mean {mean:.8g} per-rank-count mean "
              f"{0.5 * (float(today[0][0][k]) + float(today[1][0][k])):.8g}")
        np.testing.assert_allclose(mean, float(ref[k]), rtol=1e-5, err_msg=k)
    for k in gref:
        _same_up_to_reruns(0.5 * (exact[0][1][k] + exact[1][1][k]), gref[k], gref2[k], k)
    # today's normalisation is NOT the global batch's step.  Each half's reconstruction gradient comes out scaled by
    # global count / (2 * its own count) = 1 +- 6.5 % for audio at this seed (823 / 722 frames), far outside the yardstick.  The
    # loss TERMS move much less: the rank-mean of per-rank means is off by (m0 - m1) (c1 - c0) / (2 (c0 + c1)), and the halves'
    # mean NLLs m0, m1 of a freshly initialised model differ by only ~2e-4 of their size (measured: recon/audio off by 6e-6
    # relative, inside rtol = 1e-5), so the comparison as a whole is what must fail, and the gradients are where it must.
    failed = []
    for k in ref:
        mean = 0.5 * (float(today[0][0][k]) + float(today[1][0][k]))
        if abs(mean - float(ref[k])) > 1e-5 * abs(float(ref[k])):
            failed.append(k)
    for k in gref:
        got = 0.5 * (today[0][1][k] + today[1][1][k])
        scale, spread = float(gref[k].abs().max()) + 1e-12, float((gref2[k] - gref[k]).abs().max())
        if float((got - gref[k]).abs().max()) > max(4 * spread, 2e-5 * scale):
            failed.append(k)
    print("per-rank counts: outside the criterion:", len(failed), "of", len(ref) + len(gref), failed[:6])
    assert any(k.startswith("audio_decoder") for k in failed)
    assert any(k.startswith("vision_decoder") for k in failed) or counts[0][1] == counts[1][1]
