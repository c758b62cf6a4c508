"""CPU: the seeded feed augmentation -- the host restatement of the shift and the band masks in exact integers,
the key that keeps their words apart from the noise words, what ``FeedAugment`` and ``DeviceEpisodeLoader`` accept, and which library
call each stream of a batch makes, with which words.  No kernel runs here: the library calls are recorded, not made."""

from __future__ import annotations

import dataclasses

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr

N, T_FULL = 5, 12
KEY = ds.augment_key(7, 1)


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(t: int = 4, events: tuple = ((4,), (1, 8, 8), (2, 4, 12)), std: tuple = (None, 0.1, None)) -> tuple:
    """Action without noise, audio with, vision without: an augmented stream takes the new entry either way."""
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(N, T_FULL, *e, generator=g), _chain(t, s), _chain(t, None)) for e, s in zip(events, std, strict=True))  # noqa: SLF001


def _frames(b: int, t: int, start: int = 0) -> torch.Tensor:
    return (start + torch.arange(t)).repeat(b, 1)


def test_package_exports_the_surface() -> None:
    assert mt.FeedAugment is ds.FeedAugment and mt.augment_key is ds.augment_key
    assert mt.feed_augment_parameters is ds.feed_augment_parameters and mt.feed_augment_reference is ds.feed_augment_reference
    assert "mtrssm_episode_gather_augmented" in _lib.SYMBOLS and hasattr(_lib.load(), "mtrssm_episode_gather_augmented")
    assert [n for n, _ in _lib.FeedAugment._fields_] == ["sy", "sx", "bands", "max_rows", "max_cols", "per_frame", "fill"]  # noqa: SLF001


def test_feed_augment_validates_itself() -> None:
    a = ds.FeedAugment()
    assert (a.shift, a.bands, a.max_rows, a.max_cols, a.per_frame, a.fill) == ((0, 0), 0, 0, 0, False, -1.0)
    assert ds.FeedAugment(shift=[2, 3]).shift == (2, 3)  # (a config file's list)
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.bands = 1  # type: ignore[misc]
    for bad in ({"shift": (-1, 0)}, {"shift": (1,)}, {"shift": (1.5, 0)}, {"shift": 3}, {"bands": 5}, {"bands": -1}, {"bands": 1.0},
                {"max_rows": -1}, {"max_cols": 2.5}, {"per_frame": 1}, {"fill": float("inf")}, {"fill": float("nan")}, {"fill": "0"}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ds.FeedAugment(**bad)
    ds.FeedAugment(shift=(1000, 1000), max_rows=10 ** 6)  # no stream in sight: only the loader knows H and W
    c = ds.FeedAugment(shift=(2, 3), bands=4, max_rows=5, max_cols=6, per_frame=True, fill=0.5).c_struct()
    assert (c.sy, c.sx, c.bands, c.max_rows, c.max_cols, c.per_frame, c.fill) == (2, 3, 4, 5, 6, 1, 0.5)


def test_key_separation() -> None:
    for seed in (0, 7, 2 ** 40 + 5, 2 ** 64 - 1):
        noise_keys = {ds.stream_key(seed, k) for k in range(3)}
        for k in range(3):
            assert ds.augment_key(seed, k) == ds.stream_key(seed, k + 3)
            assert ds.augment_key(seed, k) not in noise_keys
        assert len({ds.augment_key(seed, k) for k in range(3)} | noise_keys) == 6


def test_parameter_ranges_and_extremes() -> None:
    h_, w_ = 16, 12
    aug = ds.FeedAugment(shift=(2, 3), bands=4, max_rows=5, max_cols=3, per_frame=True)
    episodes = torch.arange(60)
    seen = {k: set() for k in ("dy", "dx", "h", "w")}
    triples = 0
    for epoch in range(4):
        p = ds.feed_augment_parameters(KEY, epoch, episodes, _frames(60, 12), aug, h_, w_)
        assert p["dy"].shape == p["dx"].shape == (60,)
        assert all(p[k].shape == (60, 12, 4) for k in ("h", "r0", "w", "c0"))
        assert np.abs(p["dy"]).max() <= 2 and np.abs(p["dx"]).max() <= 3
        assert p["h"].min() >= 0 and p["h"].max() <= 5 and p["r0"].min() >= 0 and (p["r0"] + p["h"]).max() <= h_
        assert p["w"].min() >= 0 and p["w"].max() <= 3 and p["c0"].min() >= 0 and (p["c0"] + p["w"]).max() <= w_
        for k, s in seen.items():
            s.update(p[k].ravel().tolist())
        triples += 60 * 12
    assert triples >= 2000
    assert seen["dy"] == set(range(-2, 3)) and seen["dx"] == set(range(-3, 4))  # both extremes and everything between
    assert seen["h"] == set(range(6)) and seen["w"] == set(range(4))
    # a full-height band can only sit at row 0; a zero-width one masks nothing wherever it sits
    full = ds.feed_augment_parameters(KEY, 0, episodes, _frames(60, 3), ds.FeedAugment(bands=1, max_rows=h_, max_cols=0), h_, w_)
    assert bool(((full["h"] < h_) | (full["r0"] == 0)).all()) and int(full["w"].max()) == 0
    # the draws are umulhi(word, n) of the stated Philox words
    q = [int(x) for x in ds.philox4x32_10((1 + 2, 9 + 1, 4, 3), KEY)]
    one = ds.feed_augment_parameters(KEY, 3, torch.tensor([4]), torch.tensor([[9]]), aug, h_, w_)
    h = (q[0] * 6) >> 32
    w = (q[2] * 4) >> 32
    assert [int(one[k][0, 0, 2]) for k in ("h", "r0", "w", "c0")] == [h, (q[1] * (h_ - h + 1)) >> 32, w, (q[3] * (w_ - w + 1)) >> 32]
    p0 = [int(x) for x in ds.philox4x32_10((0, 0, 4, 3), KEY)]
    assert (int(one["dy"][0]), int(one["dx"][0])) == (((p0[0] * 5) >> 32) - 2, ((p0[1] * 7) >> 32) - 3)


def test_no_bands_mask_nothing_and_no_shift_moves_nothing() -> None:
    g = torch.Generator().manual_seed(5)
    store = torch.randn(N, T_FULL, 2, 4, 12, generator=g)
    idx = torch.tensor([3, 0, 4])
    frames = _frames(3, 5, start=2)
    base, target = ds.feed_augment_reference(store, idx, frames, KEY, 0, ds.FeedAugment())
    assert torch.equal(base, target) and torch.equal(target, store[idx[:, None], frames])
    base, target = ds.feed_augment_reference(store, idx, frames, KEY, 0, ds.FeedAugment(shift=(3, 11)))
    assert torch.equal(base, target)  # bands = 0: the input is the shifted target
    p = ds.feed_augment_parameters(KEY, 0, idx, frames, ds.FeedAugment(shift=(3, 11)), 4, 12)
    assert all(p[k].shape == (3, 5, 0) for k in ("h", "r0", "w", "c0"))


def test_shift_is_constant_over_an_episode_and_depends_on_seed_stream_epoch_episode() -> None:
    aug = ds.FeedAugment(shift=(7, 7), bands=2, max_rows=8, max_cols=8)
    ep = torch.arange(40)

    def shifts(key: tuple, epoch: int, episodes: torch.Tensor, start: int = 0) -> np.ndarray:
        p = ds.feed_augment_parameters(key, epoch, episodes, _frames(40, 6, start), aug, 16, 16)
        return np.stack([p["dy"], p["dx"]])

    base = shifts(KEY, 0, ep)
    assert base.shape == (2, 40)  # ONE (dy, dx) per episode: no frame axis ...
    assert np.array_equal(shifts(KEY, 0, ep, start=5), base)  # ... and other frames of the episode do not move it
    for what, other in {"seed": shifts(ds.augment_key(8, 1), 0, ep), "seed_high": shifts(ds.augment_key(7 + 2 ** 32, 1), 0, ep),
                        "stream": shifts(ds.augment_key(7, 2), 0, ep), "epoch": shifts(KEY, 1, ep), "episode": shifts(KEY, 0, ep + 40)}.items():
        assert float((other == base).all(axis=0).mean()) < 0.2, what  # (225 shifts: two draws agree once in 225)
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(1))
    assert np.array_equal(shifts(KEY, 0, ep[perm]), base[:, perm.numpy()])  # the row does not enter


@pytest.mark.parametrize("per_frame", [False, True])
def test_masks_change_with_the_frame_iff_per_frame(per_frame: bool) -> None:  # noqa: FBT001
    aug = ds.FeedAugment(bands=3, max_rows=8, max_cols=8, per_frame=per_frame)
    ep = torch.arange(20)
    p = ds.feed_augment_parameters(KEY, 0, ep, _frames(20, 6), aug, 16, 16)
    bands = np.stack([p[k] for k in ("h", "r0", "w", "c0")])  # [4, B, T, bands]
    same = (bands == bands[:, :, :1]).all()
    assert bool(same) != per_frame
    later = ds.feed_augment_parameters(KEY, 0, ep, _frames(20, 6, start=3), aug, 16, 16)
    later = np.stack([later[k] for k in ("h", "r0", "w", "c0")])
    assert np.array_equal(later[:, :, :3], bands[:, :, 3:])  # keyed by the ABSOLUTE frame: the window start does not enter
    for what, other in {"epoch": ds.feed_augment_parameters(KEY, 1, ep, _frames(20, 6), aug, 16, 16),
                        "episode": ds.feed_augment_parameters(KEY, 0, ep + 20, _frames(20, 6), aug, 16, 16),
                        "stream": ds.feed_augment_parameters(ds.augment_key(7, 2), 0, ep, _frames(20, 6), aug, 16, 16)}.items():
        assert not np.array_equal(np.stack([other[k] for k in ("h", "r0", "w", "c0")]), bands), what


def test_reference_on_a_store_that_encodes_its_coordinates() -> None:
    """Every value of the store is its own (episode, frame, channel, row, column): a target pixel that is not fill must hold exactly
    (ep, f, c, y - dy, x - dx) -- never another row's, channel's or frame's value -- and a vacated one holds fill."""
    c_, h_, w_ = 2, 6, 8
    e, f, c, y, x = np.meshgrid(np.arange(N), np.arange(T_FULL), np.arange(c_), np.arange(h_), np.arange(w_), indexing="ij")
    code = (((e * T_FULL + f) * c_ + c) * h_ + y) * w_ + x  # < 2^24: exact in fp32, never -1
    store = torch.from_numpy(code.astype(np.float32))
    aug = ds.FeedAugment(shift=(5, 7), bands=2, max_rows=3, max_cols=3, per_frame=True)
    idx = torch.tensor([3, 0, 4, 1, 2, 2])
    frames = _frames(6, 5, start=4)
    shifts = set()
    for epoch in range(6):
        base, target = ds.feed_augment_reference(store, idx, frames, KEY, epoch, aug)
        p = ds.feed_augment_parameters(KEY, epoch, idx, frames, aug, h_, w_)
        assert base.dtype == target.dtype == torch.float32 and base.shape == target.shape == (6, 5, c_, h_, w_)
        for b in range(6):
            dy, dx = int(p["dy"][b]), int(p["dx"][b])
            shifts.add((dy, dx))
            for t in range(5):
                for ch in range(c_):
                    for yy in range(h_):
                        for xx in range(w_):
                            inside = 0 <= yy - dy < h_ and 0 <= xx - dx < w_
                            want = float(code[idx[b], frames[b, t], ch, yy - dy, xx - dx]) if inside else -1.0
                            assert float(target[b, t, ch, yy, xx]) == want
                            hit = any(p["r0"][b, t, j] <= yy < p["r0"][b, t, j] + p["h"][b, t, j]
                                      or p["c0"][b, t, j] <= xx < p["c0"][b, t, j] + p["w"][b, t, j] for j in range(2))
                            assert float(base[b, t, ch, yy, xx]) == (-1.0 if hit else want)
    assert len(shifts) > 10 and any(dy > 0 for dy, _ in shifts) and any(dy < 0 for dy, _ in shifts)
    assert any(dx % 4 for _, dx in shifts) and any(dx > 0 for _, dx in shifts) and any(dx < 0 for _, dx in shifts)
    # dead frames are zero in both and their frame numbers are never read (here they lie past the store)
    live = torch.tensor([[True] * 5, [True, True, False, False, False]] + [[False] * 5] * 4)
    far = torch.where(live, frames, torch.full_like(frames, 10 ** 6))
    base, target = ds.feed_augment_reference(store, idx, far, KEY, 0, aug, live=live)
    assert bool((base[~live] == 0).all()) and bool((target[~live] == 0).all()) and bool((target[live] != 0).any())


def test_loader_rejects_what_it_cannot_augment() -> None:
    aug = ds.FeedAugment(shift=(2, 3), bands=1, max_rows=2, max_cols=2)
    ok = {"shuffle": False, "noise_seed": 7}
    loader = ds.DeviceEpisodeLoader(_streams(), 2, augment={"audio": aug, "vision": aug}, **ok)
    assert loader.augment == (None, aug, aug)
    assert ds.DeviceEpisodeLoader(_streams(), 2, augment={"vision": {"shift": [1, 2]}}, **ok).augment == (None, None, ds.FeedAugment(shift=(1, 2)))
    assert ds.DeviceEpisodeLoader(_streams(), 2, **ok).augment == (None, None, None)
    assert ds.DeviceEpisodeLoader(_streams(), 2, shuffle=False, augment={}).augment == (None, None, None)
    with pytest.raises(ValueError, match=r"audio.*noise_seed"):
        ds.DeviceEpisodeLoader(_streams(), 2, shuffle=False, augment={"audio": aug})
    with pytest.raises(ValueError, match="action"):
        ds.DeviceEpisodeLoader(_streams(), 2, augment={"action": aug}, **ok)
    with pytest.raises(ValueError, match="touch"):
        ds.DeviceEpisodeLoader(_streams(), 2, augment={"touch": aug}, **ok)
    with pytest.raises(ValueError, match="vision.*FeedAugment"):
        ds.DeviceEpisodeLoader(_streams(), 2, augment={"vision": 3}, **ok)
    # a stream that does not run in the gather kernel
    g = torch.Generator().manual_seed(3)
    user = tr.Compose([tr.TakeFirstN(4), tr.NormalizeVisionImage()])
    custom = (*_streams()[:2], ds._Stream(torch.randn(N, T_FULL, 1, 4, 4, generator=g), user, _chain(4, None)))  # noqa: SLF001
    with pytest.raises(ValueError, match="vision.*gather kernel"):
        ds.DeviceEpisodeLoader(custom, 2, augment={"vision": aug}, **ok)
    ds.DeviceEpisodeLoader(custom, 2, augment={"audio": aug}, **ok)  # (the other stream is nobody's problem)
    # frames that are not [C, H, W] with W % 4 == 0
    for events, name in ((((4,), (64,), (1, 8, 8)), "audio"), (((4,), (1, 8, 8), (8, 8)), "vision"), (((4,), (1, 8, 8), (2, 8, 6)), "vision")):
        with pytest.raises(ValueError, match=name + r".*\[C, H, W\]"):
            ds.DeviceEpisodeLoader(_streams(events=events), 2, augment={name: ds.FeedAugment()}, **ok)
    # parameters out of range for the stream's H, W (audio 8 x 8, vision 4 x 12)
    for name, bad in (("audio", {"shift": (8, 0)}), ("audio", {"shift": (0, 8)}), ("vision", {"shift": (4, 0)}), ("vision", {"max_rows": 5}),
                      ("vision", {"max_cols": 13}), ("audio", {"max_cols": 9})):
        with pytest.raises(ValueError, match=name):
            ds.DeviceEpisodeLoader(_streams(), 2, augment={name: ds.FeedAugment(**bad)}, **ok)
    ds.DeviceEpisodeLoader(_streams(), 2, augment={"vision": ds.FeedAugment(shift=(3, 11), bands=4, max_rows=4, max_cols=12)}, **ok)


class _FakeLibrary:
    def __getattr__(self, name: str):  # noqa: ANN204
        return name


def _record(monkeypatch: pytest.MonkeyPatch) -> list[tuple]:
    """Record every library call a batch makes as ``(entry name, arguments)`` and launch nothing: the loader runs on host stores,
    pointers are the host tensors' addresses."""
    calls: list[tuple] = []

    def call(name, fn, *args, **kw):  # noqa: ANN001, ANN002, ANN003, ANN202, ARG001
        assert fn == name
        calls.append((name, args))
        return 0

    monkeypatch.setattr(_lib, "load", lambda: _FakeLibrary())
    monkeypatch.setattr(_lib.TIMERS, "call", call)
    for fn in ("ptr", "raw_ptr", "index_ptr"):
        monkeypatch.setattr(_lib, fn, lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(_lib, "stream_ptr", lambda device: None)  # noqa: ARG005
    return calls


def _augmented_words(args: tuple) -> tuple:
    """``(struct fields, key0, key1, akey0, akey1, epoch, C, H, W, noisy, std)`` of a recorded call of the augmented entry."""
    a = args[0]
    return ((a.sy, a.sx, a.bands, a.max_rows, a.max_cols, a.per_frame, a.fill), *args[6:11], *args[15:20])


@pytest.mark.parametrize("window", ["first", "random", "sequential"])
def test_augmented_streams_make_the_new_call_with_the_permutations_epoch(monkeypatch: pytest.MonkeyPatch, window: str) -> None:
    calls = _record(monkeypatch)
    a_aug = ds.FeedAugment(shift=(2, 3), bands=2, max_rows=3, max_cols=4, per_frame=True, fill=0.0)
    v_aug = ds.FeedAugment(shift=(1, 0))
    streams = _streams()
    loader = ds.DeviceEpisodeLoader(streams, 2, shuffle=True, seed=3, window=window, noise_seed=7, augment={"audio": a_aug, "vision": v_aug})
    plain = ds.DeviceEpisodeLoader(streams, 2, shuffle=True, seed=3, window=window, noise_seed=7)
    old = "mtrssm_episode_gather" if window == "first" else "mtrssm_episode_gather_window"

    def epoch_calls(which: ds.DeviceEpisodeLoader) -> list[tuple]:
        calls.clear()
        assert len(list(which)) == len(which)
        assert len(calls) == 3 * len(which)
        return list(calls)

    for epoch in (0, 1, 2):
        assert loader.epoch == plain.epoch == epoch
        got, was = epoch_calls(loader), epoch_calls(plain)
        for k, ((name, args), (name0, args0)) in enumerate(zip(got, was, strict=True)):
            stream = k % 3
            if stream == 0:  # the action stream: the old call, its arguments unchanged (idx, start and the outputs are fresh buffers)
                assert name == name0 == old
                assert args[0] == args0[0] and args[_B_AT[old] - 2: -3] == args0[_B_AT[old] - 2: -3]  # store; noise, n, B, T, T_full, E, std
                continue
            assert name == "mtrssm_episode_gather_augmented"
            assert name0 == ("mtrssm_episode_gather_seeded" if stream == 1 else old)
            want = (2, 3, 2, 3, 4, 1, 0.0) if stream == 1 else (1, 0, 0, 0, 0, 0, -1.0)
            event = streams[stream].event_shape
            assert _augmented_words(args) == (want, *ds.stream_key(7, stream), *ds.augment_key(7, stream), epoch, *event,
                                              int(stream == 1), 0.1 if stream == 1 else 0.0)
            assert args[1] == streams[stream].store.data_ptr() and args[11:15] == (N, args0[_B_AT[name0]], 4, T_FULL)
    loader.set_epoch(1)
    assert {_augmented_words(a)[5] for n, a in epoch_calls(loader) if n.endswith("augmented")} == {1}  # set_epoch replays
    assert loader.epoch == 2
    fixed = ds.DeviceEpisodeLoader(streams, 2, shuffle=True, seed=3, window=window, noise_seed=7, noise_epoch="fixed",
                                   augment={"audio": a_aug, "vision": v_aug})
    for _ in range(2):  # the same epoch word feeds noise and augmentation: a fixed loader fixes both
        assert {_augmented_words(a)[5] for n, a in epoch_calls(fixed) if n.endswith("augmented")} == {0}


_B_AT = {"mtrssm_episode_gather": 4, "mtrssm_episode_gather_window": 5, "mtrssm_episode_gather_seeded": 9}  # where B stands in each call


def test_ragged_loader_passes_lengths_and_valid_to_the_new_call(monkeypatch: pytest.MonkeyPatch) -> None:
    calls = _record(monkeypatch)
    aug = ds.FeedAugment(shift=(1, 1))
    streams = (*_streams()[:1], *_streams(std=(None, 0.1, 0.1))[1:])
    lengths = torch.tensor([12, 3, 7, 1, 9])
    loader = ds.DeviceEpisodeLoader(streams, 2, shuffle=False, window="random", noise_seed=7, lengths=lengths, augment={"audio": aug})
    batch = next(iter(loader))
    assert [n for n, _ in calls[:3]] == ["mtrssm_episode_gather_ragged", "mtrssm_episode_gather_augmented", "mtrssm_episode_gather_seeded"]
    args = calls[1][1]
    assert args[3] is not None and args[4] == loader.lengths.data_ptr() and args[5] is None  # start, lengths; valid: the first stream writes it
    assert batch.valid is not None


def test_injected_noise_on_an_augmented_stream_raises(monkeypatch: pytest.MonkeyPatch) -> None:
    _record(monkeypatch)
    loader = ds.DeviceEpisodeLoader(_streams(), 2, shuffle=False, noise_seed=7, augment={"audio": ds.FeedAugment(shift=(1, 1))})
    idx = torch.tensor([0, 1])
    loader.batch(idx)
    loader.batch(idx, noise=(None, None, torch.zeros(2, 4, 2, 4, 12)))  # (the vision stream is not augmented)
    with pytest.raises(ValueError, match="audio.*noise="):
        loader.batch(idx, noise=(None, torch.zeros(2, 4, 1, 8, 8), None))


def test_data_module_augments_the_train_loader_only(tmp_path) -> None:  # noqa: ANN001
    d = tmp_path / "processed_toy"
    d.mkdir(parents=True)
    g = torch.Generator().manual_seed(31)
    for i in range(2 * N):
        torch.save(torch.randn(T_FULL, 4, generator=g), d / f"act_{i:03d}.pt")
        torch.save(torch.rand(T_FULL, 1, 8, 8, generator=g), d / f"audio_obs_{i:03d}.pt")
        torch.save(torch.rand(T_FULL, 1, 8, 8, generator=g), d / f"vision_obs_{i:03d}.pt")
    ident = torch.nn.Identity()
    aug = {"audio": ds.FeedAugment(bands=2, max_rows=2, max_cols=2, per_frame=True), "vision": {"shift": [2, 2]}}
    config = ds.EpisodeDataModuleConfig(
        data_name="toy", batch_size=2, num_workers=0, gdrive_url="", action_preprocess=ident,
        action_input_transform=_chain(4, None), action_target_transform=_chain(4, None),
        audio_observation_file_name="audio.npy", vision_observation_file_name="vision.npy",
        audio_observation_preprocess=ident, vision_observation_preprocess=ident,
        audio_observation_input_transform=_chain(4, 0.1), audio_observation_target_transform=_chain(4, None),
        vision_observation_input_transform=_chain(4, 0.1), vision_observation_target_transform=_chain(4, None),
        data_root=tmp_path, window="random", noise_seed=7, augment=aug)
    assert {f.name: f for f in dataclasses.fields(ds.EpisodeDataModuleConfig)}["augment"].default is None
    dm = ds.EpisodeDataModule(config, device="cpu")
    dm.setup()
    train, val = dm.train_dataloader(), dm.val_dataloader()
    assert train.augment == (None, aug["audio"], ds.FeedAugment(shift=(2, 2))) and train.noise_epoch == "advance"
    assert val.augment == (None, None, None) and val.noise_epoch == "fixed"
