"""GPU: the episode panel kernel and ``render_episodes``.

What is pinned here: ``mtrssm_episode_panel`` gives ``EpisodePanel.reference``'s bytes (computed on the CPU) with zero differences allowed
-- on the reference callback's fixture, on a small case built to break it (unequal frame sizes, RGB, every column kind, odd row
lengths, a tail of the flat video, frame numbers gaining a digit, per-row contexts and lengths, unseen modalities, values beyond
[-1, 1], NaN, every quantisation boundary) and at the bench's frame sizes, where the grid strides.  At model level: the prior column is
the posterior column on the context, the observation column is the rule applied to the targets, the video is the rule applied to the
decoded frames, the states are the public rollouts' under the same noise (samples exact, ``deter`` to 1e-5: the masked and the unmasked
scans order their sums differently), rows past their end are black, ``observe="audio"`` blanks the vision observations.  Noise is
screened on the CPU under the codes of the 2 N-row run it feeds (margin 1e-4), so that no draw sits at a CDF edge.
"""

from __future__ import annotations

import functools
import itertools

import pytest
import torch

from multimodal_mtrssm_amd import EpisodePanel, EpisodeVideo, StateCarry
from oracle.cases import CASES, build_batch, build_model, build_noise, min_margin, with_sizes
from tests.conftest import product_from_case
from tests.test_episode_panel_host import AUDIO, VISION, fixture_frames, hard_frames
from tests.test_modality_mask_oracle import oracle_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("prior", "observation", "posterior", "error")


def _gpu(xs):  # noqa: ANN001, ANN202
    return [None if x is None else x.to(DEV) for x in xs]


def _differences(got: torch.Tensor, want: torch.Tensor) -> int:
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape), (got.dtype, got.shape, want.shape)
    return int((got.cpu() != want).sum())


# 1. the kernel is the rule ------------------------------------------------------------------------------------------------------------
def test_kernel_gives_the_callbacks_bytes_on_the_fixture() -> None:
    frames, want = fixture_frames()
    panel = EpisodePanel(1, scale=1, gap=0, bar=0, label=0)
    got = panel.render(*_gpu(frames))
    torch.cuda.synchronize()
    assert got.is_cuda and int((got.cpu().numpy() != want).sum()) == 0
    assert _differences(got, panel.reference(*frames)) == 0
    dressed = EpisodePanel(2)  # the defaults: scale 2, gap 1, bar 2, label 1
    assert _differences(dressed.render(*_gpu(frames), frame0=9), dressed.reference(*frames, frame0=9)) == 0


@functools.lru_cache(maxsize=None)
def _hard() -> dict:
    frames = hard_frames()
    return {"frames": frames, "gpu": _gpu(frames),
            "codes": torch.tensor([[3, 1, 2], [0, 3, 3]], dtype=torch.int32), "valid": torch.tensor([3, 1], dtype=torch.int32),
            "context": torch.tensor([1, 2], dtype=torch.int32)}


@pytest.mark.parametrize("scale", [1, 3])
def test_kernel_equals_the_rule_on_the_hard_case(scale: int) -> None:
    h = _hard()
    codes, valid, context = (h[k].to(DEV) for k in ("codes", "valid", "context"))
    row_bytes, tails = set(), set()
    for gap, bar, label, frame0, blank in itertools.product((0, 1), (0, 2), (0, 1), (0, 8, 98), (True, False)):
        panel = EpisodePanel(2, columns=ALL, scale=scale, gap=gap, bar=bar, label=label, blank_unseen=blank)
        hc, wc = panel.shape(AUDIO, VISION)
        row_bytes.add((wc * 3) % 4)
        tails.add((2 * 3 * hc * wc) % 4)
        what = f"scale {scale} gap {gap} bar {bar} label {label} frame0 {frame0} blank {blank}"
        want = panel.reference(*h["frames"], codes=h["codes"], valid=h["valid"], context=h["context"], frame0=frame0)
        got = panel.render(*h["gpu"], codes=codes, valid=valid, context=context, frame0=frame0)
        assert _differences(got, want) == 0, what
        if frame0 == 98 and gap == 1:  # noqa: PLR2004  (without the optional planes; two runs agree bitwise; a given buffer is filled)
            bare = panel.render(*h["gpu"], frame0=frame0)
            assert _differences(bare, panel.reference(*h["frames"], frame0=frame0)) == 0, what
            out = torch.full_like(got, 77)
            assert panel.render(*h["gpu"], codes=codes, valid=valid, context=context, frame0=frame0, out=out) is out
            assert torch.equal(out, got), what
    assert row_bytes == {0, 1}, row_bytes  # Wc * 3 a multiple of 4 (gap 0), and not (gap 1)
    assert tails - {0}, tails  # some of the flat videos end inside a dword
    torch.cuda.synchronize()


def test_kernel_column_subsets_and_grey_vision() -> None:
    h = _hard()
    obs_a, post_a, prior_a, obs_v, post_v, prior_v = h["frames"]
    grey = [obs_a, post_a, prior_a, obs_v[:, :, :1].contiguous(), post_v[:, :, :1].contiguous(), prior_v[:, :, :1].contiguous()]
    for columns, keep in ((("observation",), (1, 0, 0)), (("posterior", "prior"), (0, 1, 1)), (("error",), (1, 0, 1)),
                          (("error", "posterior", "observation"), (1, 1, 1))):
        for frames in (h["frames"], grey):
            given = [f if keep[i % 3] else None for i, f in enumerate(frames)]
            panel = EpisodePanel(1, columns=columns, scale=2, gap=3, bar=1, label=2)
            want = panel.reference(*given, codes=h["codes"], frame0=123456)
            got = panel.render(*_gpu(given), codes=h["codes"].to(DEV), frame0=123456)
            assert _differences(got, want) == 0, (columns, frames[3].shape)
    with pytest.raises(ValueError, match="need the prior"):
        EpisodePanel(1).render(*_gpu([obs_a, post_a, None, obs_v, post_v, prior_v]))


def test_kernel_at_the_bench_frame_sizes() -> None:
    """64 x 64 vision over 128 x 32 audio at scale 2, 32 frames: 4.8 M pixels, more 4-pixel units than the capped grid has lanes."""
    g = torch.Generator().manual_seed(11)
    frames = [torch.rand(2, 16, *chw, generator=g) * 2.1 - 1.05 for chw in ((1, 128, 32),) * 3 + ((1, 64, 64),) * 3]
    valid, context = torch.tensor([16, 5], dtype=torch.int32), torch.tensor([3, 3], dtype=torch.int32)
    panel = EpisodePanel(3)
    want = panel.reference(*frames, valid=valid, context=context, frame0=95)
    got = panel.render(*_gpu(frames), valid=valid.to(DEV), context=context.to(DEV), frame0=95)
    assert tuple(got.shape) == (2, 16, 387, 386, 3) and got.numel() // 3 > 4096 * 256 * 4 and _differences(got, want) == 0


# 2. the model level -------------------------------------------------------------------------------------------------------------------
B, T, Q = 2, 16, 5
MODELS = ["mrssm_default", "mmtrssm_default"]


@functools.lru_cache(maxsize=None)
def _setup(name: str) -> dict:
    """Computed once per model: the oracle, a batch and noise screened on the CPU under the codes of the 2 B-row run it feeds (rows
    ``[0, B)`` see everything, rows ``[B, 2 B)`` the first ``Q`` frames; both halves read the same draws)."""
    case = with_sizes(CASES[name], B, T)
    oracle = build_model(case)
    batch = build_batch(case)
    twice = tuple(torch.cat([x, x]) for x in batch)
    codes = torch.cat([torch.full((B, T), 3), (torch.arange(T) < Q).long().mul(3).expand(B, T)]).contiguous()
    best = None
    for seed in range(500, 540):
        noise = build_noise(case, seed, batch=2 * B, steps=T)
        for u in noise.values():
            u[B:] = u[:B]
        with torch.no_grad():
            out = oracle_step(case, oracle, twice, noise, codes)
        margin = min_margin(case, out, noise)
        if best is None or margin > best[1]:
            best = (noise, margin)
        if margin >= 1e-4:  # noqa: PLR2004
            break
    noise, margin = best
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    return {"case": case, "oracle": oracle, "batch": batch, "noise": {k: u[:B].contiguous() for k, u in noise.items() if not k.startswith("u_prior")}}


@functools.lru_cache(maxsize=None)
def _rendered(name: str) -> dict:
    ref = _setup(name)
    model = product_from_case(ref["case"], ref["oracle"], DEV)
    batch = tuple(x.to(DEV) for x in ref["batch"])
    noise = {k: v.to(DEV) for k, v in ref["noise"].items()}
    panel = EpisodePanel(Q, label=0)  # (no frame number: it would cover a corner of the prior's vision cell)
    video = model.render_episodes(batch, panel, noise, keep_states=True)
    torch.cuda.synchronize()
    return {"model": model, "batch": batch, "noise": noise, "panel": panel, "video": video, "kind": ref["case"].kind,
            "audio": tuple(batch[4].shape[2:]), "vision": tuple(batch[5].shape[2:])}


def _cell(r: dict, video: EpisodeVideo, modality: str, column: str) -> torch.Tensor:
    rows, cols = r["panel"].cell(modality, column, r["audio"], r["vision"])
    return video.frames[:, :, rows, cols]


@pytest.mark.parametrize("name", MODELS)
def test_prior_is_the_posterior_on_the_context_and_the_video_is_the_rule(name: str) -> None:
    r = _rendered(name)
    video, panel = r["video"], r["panel"]
    hc, wc = panel.shape(r["audio"], r["vision"])
    assert isinstance(video, EpisodeVideo) and tuple(video.frames.shape) == (B, T, hc, wc, 3) and video.frames.dtype == torch.uint8
    assert video.valid is None and video.context.tolist() == [Q] * B and tuple(video.chw().shape) == (B, T, 3, hc, wc)
    for modality in ("audio", "vision"):
        prior, post = _cell(r, video, modality, "prior"), _cell(r, video, modality, "posterior")
        assert torch.equal(prior[:, :Q], post[:, :Q]), modality
        assert not torch.equal(prior[:, Q:], post[:, Q:]), modality
    d = {k: v.cpu() for k, v in video.decoded.items()}
    args = (d["observation/audio"], d["posterior/audio"], d["prior/audio"], d["observation/vision"], d["posterior/vision"], d["prior/vision"])
    assert torch.equal(d["observation/audio"], r["batch"][4].cpu()) and torch.equal(d["observation/vision"], r["batch"][5].cpu())
    assert _differences(video.frames, panel.reference(*args)) == 0
    only = EpisodePanel(Q, columns=("observation",), label=0)  # the observation column alone: the rule applied to the targets
    want = only.reference(r["batch"][4].cpu(), None, None, r["batch"][5].cpu(), None, None)
    for modality in ("audio", "vision"):
        rows, cols = only.cell(modality, 0, r["audio"], r["vision"])
        assert torch.equal(_cell(r, video, modality, "observation").cpu(), want[:, :, rows, cols]), modality
    # without keep_states the video carries no batch data beside its frames.  Two calls are NOT compared byte for byte: the
    # encoders' Linear layers meet their split reductions in fp32 atomics, so their embeddings move by an ulp from call to call (3e-8
    # seen), the decoded frames by 6e-7, and about ten of the 2.4 M bytes sit near enough to a quantisation step to flip.  What one
    # call states about itself (above) is exact; across calls the part that reads no model output is.
    again = r["model"].render_episodes(r["batch"], panel, r["noise"])
    assert again.states is None and again.decoded is None and tuple(again.frames.shape) == tuple(video.frames.shape)
    for modality in ("audio", "vision"):
        assert torch.equal(_cell(r, again, modality, "observation"), _cell(r, video, modality, "observation")), modality
    assert torch.equal(again.frames[:, :, : panel.bar], video.frames[:, :, : panel.bar])
    flipped = int((again.frames != video.frames).sum())
    print(name, "bytes that differ between two calls:", flipped, "of", video.frames.numel())


@pytest.mark.parametrize("name", MODELS)
def test_states_are_the_public_rollouts(name: str) -> None:
    r = _rendered(name)
    model, batch, noise, states = r["model"], r["batch"], r["noise"], r["video"].states
    deters, stochs = (("deter",), ("stoch",)) if r["kind"] == "mrssm" else (("deter_l", "deter_h"), ("stoch_l", "stoch_h"))
    obs = (batch[1], batch[2])
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        closed, _ = model.rollout_representation(actions=batch[0], observations=obs, prev_state=s0, noise=noise)
        opened = model.forecast_rollout(actions=batch[0], observations=obs, context=Q, prev_state=s0, noise=noise)
    for half, want in ((slice(0, B), closed), (slice(B, 2 * B), opened)):
        for k in stochs:
            assert torch.equal(getattr(states, k)[half], getattr(want, k)), k
        for k in deters:
            got, ref = getattr(states, k)[half], getattr(want, k)
            err = float((got - ref).abs().max())
            print(name, k, "max |deter difference|", err)
            assert err <= 1e-5, (k, err)  # noqa: PLR2004
    for k in (*deters, *stochs):  # the two halves share their context trajectory bit for bit
        assert torch.equal(getattr(states, k)[:B, :Q], getattr(states, k)[B:, :Q]), k


@pytest.mark.parametrize("name", MODELS)
def test_lengths_rows_and_observe(name: str) -> None:
    r = _rendered(name)
    model, batch, noise, panel = r["model"], r["batch"], r["noise"], r["panel"]
    lengths = torch.tensor([16, 9], dtype=torch.int32, device=DEV)
    ragged = model.render_episodes(batch, panel, noise, lengths=lengths, frame0=3)
    assert ragged.valid.tolist() == [16, 9]
    assert not bool(ragged.frames[1, 9:].any()) and bool(ragged.frames[1, :9].any(dim=-1).any(dim=-1).any(dim=-1).all())
    for modality in ("audio", "vision"):  # the live frames' observation cells read the targets alone: the full video's bytes
        assert torch.equal(_cell(r, ragged, modality, "observation")[0], _cell(r, r["video"], modality, "observation")[0]), modality
        assert torch.equal(_cell(r, ragged, modality, "observation")[1, :9], _cell(r, r["video"], modality, "observation")[1, :9]), modality
    # rows picks the episodes before anything runs: the same as the batch, its noise and its lengths cut by hand.  (Across calls the
    # sampled classes are compared, which the screened noise makes robust, and what reads no model output -- see above.)
    stochs = ("stoch",) if r["kind"] == "mrssm" else ("stoch_l", "stoch_h")
    for rows in ([1], torch.tensor([1, 0], device=DEV)):
        idx = torch.as_tensor(rows, device=DEV)
        picked = model.render_episodes(batch, panel, noise, lengths=lengths, rows=rows, keep_states=True)
        by_hand = model.render_episodes(tuple(x[idx] for x in batch), panel, {k: u[idx] for k, u in noise.items()}, lengths=lengths[idx],
                                        keep_states=True)
        assert tuple(picked.frames.shape[:2]) == (len(idx), T) and picked.valid.tolist() == lengths[idx].tolist()
        assert torch.equal(picked.decoded["observation/audio"], batch[4][idx]) and torch.equal(picked.decoded["observation/vision"], batch[5][idx])
        for k in stochs:
            assert torch.equal(getattr(picked.states, k), getattr(by_hand.states, k)), k
        for modality in ("audio", "vision"):
            assert torch.equal(_cell(r, picked, modality, "observation"), _cell(r, by_hand, modality, "observation")), modality
    with pytest.raises(ValueError, match="picks no episode"):
        model.render_episodes(batch, panel, noise, rows=[])
    heard = EpisodePanel(Q, observe="audio")
    video = model.render_episodes(batch, heard, noise)
    rows, cols = heard.cell("vision", "observation", r["audio"], r["vision"])
    assert not bool(video.frames[:, :, rows, cols].any())
    rows, cols = heard.cell("audio", "observation", r["audio"], r["vision"])
    assert torch.equal(video.frames[:, :, rows, cols], r["video"].frames[:, :, rows, cols])
    shown = model.render_episodes(batch, EpisodePanel(Q, observe="audio", blank_unseen=False), noise)
    rows, cols = heard.cell("vision", "observation", r["audio"], r["vision"])
    assert torch.equal(shown.frames[:, :, rows, cols], r["video"].frames[:, :, rows, cols])


def test_masked_batches_and_carries_are_refused() -> None:
    r = _rendered("mrssm_default")
    model, batch, panel = r["model"], r["batch"], r["panel"]
    mask = torch.ones(B, T, 2, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="7-tuple"):
        model.render_episodes((*batch, mask), panel)
    with pytest.raises(ValueError, match="EpisodePanel"):
        model.render_episodes(batch, Q)
    model.state_carry = StateCarry.for_model(model, B)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.render_episodes(batch, panel)
    finally:
        model.state_carry = None
