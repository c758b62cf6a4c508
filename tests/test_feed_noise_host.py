"""CPU: the seeded input noise of the episode feed -- known answers of the generator's host restatement, the
properties of the normals it defines, what ``DeviceEpisodeLoader`` accepts as ``noise_seed``, and which epoch word each epoch's
batches are made with.  No batch is assembled here (that needs the GPU)."""

from __future__ import annotations

import pytest
import torch

from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr

N, T_FULL = 5, 12


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(t: int = 4, events: tuple = ((4,), (1, 4, 4), (1, 4, 4))) -> tuple:
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(N, T_FULL, *e, generator=g), _chain(t, 0.1), _chain(t, None)) for e in events)  # noqa: SLF001


# Random123's known-answer vectors for philox4x32_10 (kat_vectors: counter words, key words, output words)
@pytest.mark.parametrize(("counter", "key", "want"), [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter: tuple, key: tuple, want: str) -> None:
    assert " ".join(f"{int(w):08x}" for w in ds.philox4x32_10(counter, key)) == want


def test_philox_is_elementwise_over_arrays() -> None:
    import numpy as np

    c0 = np.array([0, 0xFFFFFFFF, 0x243F6A88])
    got = ds.philox4x32_10((c0, np.array([0, 0xFFFFFFFF, 0x85A308D3]), np.array([0, 0xFFFFFFFF, 0x13198A2E]), np.array([0, 0xFFFFFFFF, 0x03707344])),
                           (np.array([0, 0xFFFFFFFF, 0xA4093822]), np.array([0, 0xFFFFFFFF, 0x299F31D0])))
    assert [int(w[2]) for w in got] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    assert [int(w[0]) for w in got] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_stream_key_layout() -> None:
    seed = 0x0123456789ABCDEF
    assert ds.stream_key(seed, 0) == (0x89ABCDEF, 0x01234567 ^ 0x9E3779B9)
    assert ds.stream_key(seed, 2) == (0x89ABCDEF, 0x01234567 ^ ((3 * 0x9E3779B9) & 0xFFFFFFFF))
    assert ds.stream_key(7, 1) == (7, (2 * 0x9E3779B9) & 0xFFFFFFFF)
    assert len({ds.stream_key(7, k) for k in range(3)}) == 3


def _frames(b: int, t: int, start: int = 0) -> torch.Tensor:
    return (start + torch.arange(t)).repeat(b, 1)


def test_reference_normals_are_finite_bounded_and_standard() -> None:
    episodes = torch.arange(50)
    z = ds.feed_noise_reference(ds.stream_key(7, 1), 0, episodes, _frames(50, 12), 512)  # 307 200 values
    assert z.shape == (50, 12, 512) and z.dtype == torch.float64
    assert z.numel() >= 200_000
    assert bool(torch.isfinite(z).all())
    assert float(z.abs().max()) <= 5.77  # sqrt(2 * 24 * ln 2): u1 = 2^-24
    assert abs(float(z.mean())) <= 0.01  # standard error 1 / sqrt(n) = 0.0018
    assert abs(float(z.std()) - 1.0) <= 0.01  # standard error 1 / sqrt(2 n) = 0.0013


def test_reference_layout_two_pairs_per_counter() -> None:
    """Elements 4 e4 .. 4 e4 + 3 of (episode, frame) come from ONE Philox call with counter (e4, frame, episode, epoch)."""
    import math

    key = ds.stream_key(11, 2)
    z = ds.feed_noise_reference(key, 3, torch.tensor([4]), torch.tensor([[9]]), 8)[0, 0]
    for e4 in range(2):
        x = [int(w) for w in ds.philox4x32_10((e4, 9, 4, 3), key)]
        for pair in range(2):
            u1, u2 = ((x[2 * pair] >> 8) + 1) / 2 ** 24, (x[2 * pair + 1] >> 8) / 2 ** 24
            r = math.sqrt(-2.0 * math.log(u1))
            assert float(z[4 * e4 + 2 * pair]) == pytest.approx(r * math.cos(2 * math.pi * u2), abs=1e-14)
            assert float(z[4 * e4 + 2 * pair + 1]) == pytest.approx(r * math.sin(2 * math.pi * u2), abs=1e-14)


def test_reference_depends_on_seed_stream_epoch_episode_and_frame() -> None:
    ep = torch.arange(N)
    base = ds.feed_noise_reference(ds.stream_key(7, 1), 0, ep, _frames(N, 5), 16)
    others = {
        "seed": ds.feed_noise_reference(ds.stream_key(8, 1), 0, ep, _frames(N, 5), 16),
        "seed_high": ds.feed_noise_reference(ds.stream_key(7 + 2 ** 32, 1), 0, ep, _frames(N, 5), 16),
        "stream": ds.feed_noise_reference(ds.stream_key(7, 2), 0, ep, _frames(N, 5), 16),
        "epoch": ds.feed_noise_reference(ds.stream_key(7, 1), 1, ep, _frames(N, 5), 16),
        "episode": ds.feed_noise_reference(ds.stream_key(7, 1), 0, ep + N, _frames(N, 5), 16),
        "frame": ds.feed_noise_reference(ds.stream_key(7, 1), 0, ep, _frames(N, 5, start=5), 16),
    }
    for what, z in others.items():
        assert float((z == base).double().mean()) < 0.01, what
    # ... and on nothing else: the row a frame sits in, the batch size and the window start do not enter
    perm = torch.tensor([3, 0, 4, 1, 2])
    assert torch.equal(ds.feed_noise_reference(ds.stream_key(7, 1), 0, ep[perm], _frames(N, 5), 16), base[perm])
    shifted = ds.feed_noise_reference(ds.stream_key(7, 1), 0, ep, _frames(N, 5, start=3), 16)
    assert torch.equal(shifted[:, :2], base[:, 3:])


def test_loader_rejects_bad_seeds_and_streams_it_cannot_seed() -> None:
    streams = _streams()
    for bad in (1.5, "7", -1, 2 ** 64, True):
        with pytest.raises(ValueError, match="noise_seed"):
            ds.DeviceEpisodeLoader(streams, 2, shuffle=False, noise_seed=bad)
    with pytest.raises(ValueError, match="noise_epoch"):
        ds.DeviceEpisodeLoader(streams, 2, shuffle=False, noise_seed=7, noise_epoch="never")
    for ok in (0, 7, 2 ** 64 - 1):
        assert ds.DeviceEpisodeLoader(streams, 2, shuffle=False, noise_seed=ok).noise_seed == ok
    # a noisy stream whose event size is no multiple of 4 does not run in the gather kernel
    odd = _streams(events=((4,), (1, 3, 2), (1, 4, 4)))
    with pytest.raises(ValueError, match="audio"):
        ds.DeviceEpisodeLoader(odd, 2, shuffle=False, noise_seed=7)
    ds.DeviceEpisodeLoader(odd, 2, shuffle=False)  # (fine without a seed: the per-episode path draws its own noise)
    # arbitrary user transforms around a GaussianNoise
    g = torch.Generator().manual_seed(3)
    user = tr.Compose([tr.TakeFirstN(4), tr.GaussianNoise(0.1), tr.NormalizeVisionImage()])
    custom = (*_streams()[:2], ds._Stream(torch.randn(N, T_FULL, 1, 4, 4, generator=g), user, _chain(4, None)))  # noqa: SLF001
    with pytest.raises(ValueError, match="vision"):
        ds.DeviceEpisodeLoader(custom, 2, shuffle=False, noise_seed=7)
    # an unfused stream WITHOUT noise is nobody's problem
    plain = (*_streams()[:2], ds._Stream(torch.randn(N, T_FULL, 1, 4, 4, generator=g),  # noqa: SLF001
                                         tr.Compose([tr.TakeFirstN(4), tr.NormalizeVisionImage()]), _chain(4, None)))
    ds.DeviceEpisodeLoader(plain, 2, shuffle=False, noise_seed=7)


def _record(monkeypatch: pytest.MonkeyPatch) -> list[tuple[int, tuple | None]]:
    """Replace ``_Stream.batch`` by a recorder of ``(event size, seeded)``: the loader runs on host stores, nothing is launched."""
    calls: list[tuple[int, tuple | None]] = []

    def batch(self, idx, noise, *args, seeded=None, **kwargs):  # noqa: ANN001, ANN002, ANN003, ANN202, ARG001
        calls.append((self.event, seeded))
        return torch.zeros(idx.numel(), 1), torch.zeros(idx.numel(), 1)

    monkeypatch.setattr(ds._Stream, "batch", batch)  # noqa: SLF001
    return calls


@pytest.mark.parametrize("window", ["first", "random", "sequential"])
def test_advancing_epoch_word_is_the_permutations_epoch(monkeypatch: pytest.MonkeyPatch, window: str) -> None:
    calls = _record(monkeypatch)
    # only audio and vision carry noise here: the action stream must never be seeded
    g = torch.Generator().manual_seed(2)
    streams = (ds._Stream(torch.randn(N, T_FULL, 4, generator=g), _chain(4, None), _chain(4, None)), *_streams()[1:])  # noqa: SLF001
    loader = ds.DeviceEpisodeLoader(streams, 2, shuffle=True, seed=3, window=window, noise_seed=7)
    per_epoch = 3 * len(loader)

    def words() -> set:
        got = {(k % 3, s) for k, (_, s) in enumerate(calls)}
        calls.clear()
        return got

    for epoch in (0, 1, 2):
        assert loader.epoch == epoch
        assert len(list(loader)) == len(loader) and len(calls) == per_epoch
        assert words() == {(0, None), (1, (*ds.stream_key(7, 1), epoch)), (2, (*ds.stream_key(7, 2), epoch))}
    loader.set_epoch(1)
    list(loader)
    assert words() == {(0, None), (1, (*ds.stream_key(7, 1), 1)), (2, (*ds.stream_key(7, 2), 1))}
    assert loader.epoch == 2
    # an iteration that is abandoned half way has advanced the counter once: the next epoch's word follows the permutation's
    next(iter(loader))
    calls.clear()
    list(loader)
    assert {s[2] for _, s in calls if s is not None} == {3}


def test_fixed_epoch_word_is_zero_in_every_epoch(monkeypatch: pytest.MonkeyPatch) -> None:
    calls = _record(monkeypatch)
    loader = ds.DeviceEpisodeLoader(_streams(), 2, shuffle=False, window="random", noise_seed=2 ** 40 + 5, noise_epoch="fixed")
    for _ in range(3):
        list(loader)
    loader.set_epoch(9)
    list(loader)
    assert loader.epoch == 10  # (the permutation's epoch still advances)
    assert len(calls) == 4 * 3 * len(loader)
    assert {s for _, s in calls} == {(*ds.stream_key(2 ** 40 + 5, k), 0) for k in range(3)}


def test_fixed_loader_repeats_epoch_zeros_order_and_windows() -> None:
    def triples(loader: ds.DeviceEpisodeLoader) -> list:
        return [(rows.tolist(), start.tolist()) for rows, start, _ in loader.schedule()]

    kw = {"shuffle": True, "seed": 3, "window": "random", "noise_seed": 7}
    fixed = ds.DeviceEpisodeLoader(_streams(), 2, noise_epoch="fixed", **kw)
    moving = ds.DeviceEpisodeLoader(_streams(), 2, **kw)
    zero = triples(moving)
    assert triples(fixed) == zero and triples(fixed) == zero and fixed.epoch == 2
    assert triples(moving) != zero


def test_no_seed_means_no_seeded_call(monkeypatch: pytest.MonkeyPatch) -> None:
    calls = _record(monkeypatch)
    list(ds.DeviceEpisodeLoader(_streams(), 2, shuffle=True, window="random"))
    assert calls and all(s is None for _, s in calls)


def test_data_module_config_carries_the_seed() -> None:
    import dataclasses

    fields = {f.name: f for f in dataclasses.fields(ds.EpisodeDataModuleConfig)}
    assert fields["noise_seed"].default is None
