"""CPU: the window schedule of ``DeviceEpisodeLoader`` -- which frames of which episode a batch holds in the
modes ``"first"`` / ``"random"`` / ``"sequential"``, on any number of ranks -- the torch restatement of the windowed gather, and
the argument checks of ``mtrssm_episode_gather_window``.  No batch is assembled here (that needs the GPU)."""

from __future__ import annotations

import ctypes as C
import dataclasses

import pytest
import torch

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(n: int, t_full: int, t: int) -> tuple:
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(n, t_full, w, generator=g), _chain(t, 0.1), _chain(t, None)) for w in (4, 8, 8))  # noqa: SLF001


def _triples(loader: ds.DeviceEpisodeLoader) -> list[list[tuple[int, int, bool]]]:
    """Per step of one epoch the ``(episode, start, reset)`` of this rank's rows."""
    return [list(zip(rows.tolist(), start.tolist(), reset.tolist(), strict=True)) for rows, start, reset in loader.schedule()]


def test_sequential_visits_every_frame_once_and_resets_on_chunk_zero() -> None:
    n, t_full, t, bs = 10, 26, 8, 4  # 26 = 3 x 8 + 2: the last two frames are not visited
    loader = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=5, window="sequential")
    assert loader.n_chunks == 3 and loader.steps == t
    assert len(loader) == 3 * 3  # ceil(10 / 4) groups x 3 chunks
    for _ in range(2):
        steps = _triples(loader)
        assert len(steps) == len(loader)
        visits = torch.zeros(n, t_full, dtype=torch.int64)
        for i, step in enumerate(steps):
            chunk = i % 3
            for ep, start, reset in step:
                assert start == chunk * t and reset == (chunk == 0)
                visits[ep, start: start + t] += 1
            assert [e for e, _, _ in step] == [e for e, _, _ in steps[i - chunk]]  # the same rows in all chunks of a group
        assert (visits[:, : 3 * t] == 1).all() and (visits[:, 3 * t:] == 0).all()


def test_random_starts_are_in_range_seeded_and_differ_between_epochs() -> None:
    n, t_full, t, bs = 12, 40, 8, 5
    loader = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=9, window="random")
    assert len(loader) == 3
    epochs = [_triples(loader) for _ in range(3)]
    for steps in epochs:
        assert sorted(e for step in steps for e, _, _ in step) == list(range(n))
        assert all(0 <= s <= t_full - t and r for step in steps for _, s, r in step)
    starts = [[s for step in steps for _, s, _ in step] for steps in epochs]
    assert starts[0] != starts[1] and starts[1] != starts[2]
    assert len({s for row in starts for s in row}) > 8  # spread over the range, not a constant
    loader.set_epoch(1)  # the same seed + epoch: the same episodes and windows
    assert _triples(loader) == epochs[1]
    other = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=10, window="random")
    assert _triples(other) != epochs[0]


@pytest.mark.parametrize("window", ["random", "sequential"])
def test_global_rows_are_rank_invariant(window: str) -> None:
    n, t_full, t, bs = 10, 24, 8, 4  # 10 = 4 + 4 + 2: the last global batch is padded for 4 ranks
    streams = _streams(n, t_full, t)
    one = _triples(ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=3, window=window))
    for world in (2, 4):
        ranks = [_triples(ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=3, rank=r, world=world, window=window)) for r in range(world)]
        assert {len(r) for r in ranks} == {len(one)}
        for i, whole in enumerate(one):
            sizes = {len(r[i]) for r in ranks}
            assert len(sizes) == 1 and sizes.pop() > 0  # equal, non-empty shards
            joined = [x for r in ranks for x in r[i]]
            assert joined[: len(whole)] == whole  # global row g: the same (episode, start, reset) as on one rank
            assert len(joined) - len(whole) == (-len(whole)) % world  # the rest is the wrap-around padding
            if len(joined) == len(whole):
                assert len({e for e, _, _ in joined}) == len(joined)  # disjoint shards
        if window == "sequential":  # a rank keeps its rows through the chunks of a group
            for r in ranks:
                for i in range(0, len(r), 3):
                    assert [e for e, _, _ in r[i]] == [e for e, _, _ in r[i + 1]] == [e for e, _, _ in r[i + 2]]


def test_first_mode_is_the_loader_of_before() -> None:
    streams = _streams(11, 20, 6)
    for world, rank in ((1, 0), (3, 1)):
        old = ds.DeviceEpisodeLoader(streams, 4, shuffle=True, seed=7, rank=rank, world=world)
        new = ds.DeviceEpisodeLoader(streams, 4, shuffle=True, seed=7, rank=rank, world=world, window="first")
        assert old.window == "first" and len(old) == len(new) == 3
        for _ in range(2):
            a, b = list(old.index_batches()), list(new.index_batches())
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b, strict=True))
        assert all(start is None and reset is None for _, start, reset in new.schedule())  # plain 6-tuples: no window rides along
    # the pre-existing order, restated: permutation of seed + epoch, cut into batches
    ld = ds.DeviceEpisodeLoader(streams, 4, shuffle=True, seed=7)
    want = torch.randperm(11, generator=torch.Generator().manual_seed(7))
    assert torch.equal(torch.cat(list(ld.index_batches())), want)


def test_config_field_and_argument_checks() -> None:
    fields = [f.name for f in dataclasses.fields(ds.EpisodeDataModuleConfig)]
    assert fields[-1] == "window" and ds.EpisodeDataModuleConfig.__dataclass_fields__["window"].default == "first"
    streams = _streams(6, 20, 6)
    with pytest.raises(ValueError, match="window"):
        ds.DeviceEpisodeLoader(streams, 2, shuffle=False, window="strided")
    ident = tr.Compose([])
    bare = tuple(ds._Stream(torch.zeros(4, 9, w), ident, ident) for w in (4, 8, 8))  # noqa: SLF001
    assert ds.DeviceEpisodeLoader(bare, 2, shuffle=False, window="sequential").n_chunks == 1  # no TakeFirstN: T = T_full
    mixed = (streams[0], ds._Stream(torch.zeros(6, 20, 8), _chain(5, 0.1), _chain(5, None)), streams[2])  # noqa: SLF001
    with pytest.raises(ValueError, match="TakeFirstN"):
        ds.DeviceEpisodeLoader(mixed, 2, shuffle=False, window="random")
    loader = ds.DeviceEpisodeLoader(streams, 2, shuffle=False, window="random")
    for bad in ([0, 15], [-1, 3]):  # T_full - T = 14
        with pytest.raises(ValueError, match="start must lie"):
            loader.batch(torch.tensor([0, 1]), start=torch.tensor(bad))
    # a chain the fused kernel does not implement still says its T
    odd = ds._Stream(torch.zeros(4, 20, 7), tr.Compose([tr.TakeFirstN(6), tr.RemoveDim(1, [0])]), _chain(6, None))  # noqa: SLF001
    assert not odd.fused and odd.steps == 6


def test_gather_window_reference_and_episode_batch() -> None:
    g = torch.Generator().manual_seed(4)
    store = torch.randn(5, 12, 2, 4, generator=g)
    idx, start = torch.tensor([3, 0, 3]), torch.tensor([0, 8, 5], dtype=torch.int32)
    noise = torch.randn(3, 4, 2, 4, generator=g)
    inp, tgt = ds.gather_window_reference(store, idx, start, 4, noise, 0.1)
    for b in range(3):
        assert torch.equal(tgt[b], store[idx[b], start[b]: start[b] + 4])
    assert torch.equal(inp, tgt + noise * 0.1)
    same, _ = ds.gather_window_reference(store, idx, start, 4, None, None)
    assert torch.equal(same, tgt)
    clamped = ds.gather_window_reference(store, idx, torch.tensor([-3, 11, 8], dtype=torch.int32), 4, None, None)[1]
    assert torch.equal(clamped[0], store[3, :4]) and torch.equal(clamped[1], store[0, 8:]) and torch.equal(clamped[2], store[3, 8:])
    # non-fused chains get the episode from its window's first frame on (CPU tensors: this path is plain torch)
    odd = ds._Stream(store[..., :3].reshape(5, 12, 6), tr.Compose([tr.TakeFirstN(4), tr.RemoveDim(1, [0])]), tr.Compose([tr.TakeFirstN(4)]))  # noqa: SLF001
    i2, t2 = odd.batch(idx, None, start, start.tolist())
    assert torch.equal(t2, ds.gather_window_reference(odd.store, idx, start, 4, None, None)[1]) and i2.shape == (3, 4, 5)
    batch = ds.EpisodeBatch(tuple(torch.zeros(1) for _ in range(6)), start, torch.ones(3, dtype=torch.bool), start, torch.ones(3, dtype=torch.bool))
    assert isinstance(batch, tuple) and len(batch) == 6 and batch[5].shape == (1,) and batch.start is start
    a, *_rest = batch
    assert a is batch[0]


def test_window_entry_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    one = C.c_void_p(16)  # a non-null, aligned address: validation returns before anything would read it
    assert lib.mtrssm_episode_gather_window(one, one, None, None, 4, 2, 3, 8, 4, 0.0, one, one, None) == -1
    assert b"start is null" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_gather_window(one, one, one, None, 4, 2, 9, 8, 4, 0.0, one, one, None) == -1  # T > Tfull
    assert lib.mtrssm_episode_gather_window(one, one, one, None, 4, 2, 3, 8, 6, 0.0, one, one, None) == -1  # E % 4
    assert b"multiple of 4" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_gather_window(None, one, one, None, 4, 2, 3, 8, 4, 0.0, one, one, None) == -1
