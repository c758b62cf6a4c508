"""CPU: episodes of different lengths -- the loader's schedule with lengths on any number of ranks, the host
validation, the torch restatements of the ragged mask and the ragged gather, and the argument checks of the new C-ABI entries.  No
batch is assembled here (that needs the GPU)."""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import _lib, carry, dropout
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr
from multimodal_mtrssm_amd.core import MoPoE_MRSSM, check_ragged_rows


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(n: int, t_full: int, t: int) -> tuple:
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(n, t_full, w, generator=g), _chain(t, 0.1), _chain(t, None)) for w in (4, 8, 8))  # noqa: SLF001


def _lengths(n: int, t_full: int, seed: int = 1) -> torch.Tensor:
    lens = torch.randint(1, t_full + 1, (n,), generator=torch.Generator().manual_seed(seed))
    lens[0], lens[1] = t_full, 1  # the longest and the shortest possible episode
    return lens


def _steps(loader: ds.DeviceEpisodeLoader) -> list[dict]:
    """Per step of one epoch: this rank's ``(episode, start, reset, valid)`` rows and the global batch's ``valid``."""
    out = []
    for rows, start, reset, valid_global, row0 in loader.schedule_ragged():
        mine = valid_global[row0: row0 + rows.numel()]
        out.append({"rows": list(zip(rows.tolist(), start.tolist(), reset.tolist(), mine.tolist(), strict=True)),
                    "global": valid_global.tolist(), "row0": row0})
    return out


def test_sequential_with_lengths_walks_to_the_longest_episode() -> None:
    n, t_full, t, bs = 10, 26, 8, 4
    lens = _lengths(n, t_full)
    lens[0] = 26  # 26 = 3 x 8 + 2: a fourth chunk with two live frames, which the loader without lengths drops
    loader = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=5, window="sequential", lengths=lens)
    assert loader.n_chunks == 4 and len(loader) == 3 * 4
    assert ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=5, window="sequential").n_chunks == 3  # unchanged
    short = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=5, window="sequential", lengths=lens.clamp(max=9))
    assert short.n_chunks == 2 and len(short) == 3 * 2  # ceil(9 / 8)
    steps = _steps(loader)
    assert len(steps) == len(loader)
    seen = torch.zeros(n, dtype=torch.int64)
    for i, step in enumerate(steps):
        chunk = i % 4
        for ep, start, reset, valid in step["rows"]:
            assert start == chunk * t and reset == (chunk == 0)
            assert valid == min(max(int(lens[ep]) - start, 0), t)
            seen[ep] += valid
        assert step["global"] == [v for _, _, _, v in step["rows"]] and step["row0"] == 0  # one rank: its own rows
        assert [e for e, *_ in step["rows"]] == [e for e, *_ in steps[i - chunk]["rows"]]
    assert torch.equal(seen, lens.to(torch.int64))  # every valid frame once, none past an episode's end
    assert any(v == 0 for step in steps for *_, v in step["rows"])  # some episode is over before the last chunk
    # the schedule() of before is the same steps without the lengths
    loader.set_epoch(0)
    assert [(r.tolist(), s.tolist(), z.tolist()) for r, s, z in loader.schedule()] == \
           [([e for e, *_ in st["rows"]], [s for _, s, _, _ in st["rows"]], [z for _, _, z, _ in st["rows"]]) for st in steps]


def test_random_with_lengths_keeps_the_window_inside_the_episode() -> None:
    n, t_full, t, bs = 12, 40, 8, 5
    lens = _lengths(n, t_full)
    loader = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=9, window="random", lengths=lens)
    assert loader.n_chunks == 1 and len(loader) == 3
    starts = set()
    for _ in range(3):
        for step in _steps(loader):
            for ep, start, reset, valid in step["rows"]:
                n_ep = int(lens[ep])
                assert reset and 0 <= start <= max(n_ep - t, 0)
                assert valid == min(n_ep, t) == min(max(n_ep - start, 0), t)
                starts.add(start)
    assert len(starts) > 8
    # with all lengths T_full the starts are the draw of the loader without lengths
    full = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=9, window="random", lengths=torch.full((n,), t_full))
    plain = ds.DeviceEpisodeLoader(_streams(n, t_full, t), bs, shuffle=True, seed=9, window="random")
    for _ in range(2):
        a = [(r.tolist(), s.tolist()) for r, s, _ in full.schedule()]
        b = [(r.tolist(), s.tolist()) for r, s, _ in plain.schedule()]
        assert a == b
    assert all(v == t for step in _steps(full) for v in step["global"])


@pytest.mark.parametrize("window", ["random", "sequential"])
def test_global_rows_with_lengths_are_rank_invariant(window: str) -> None:
    n, t_full, t, bs = 10, 24, 8, 4  # 10 = 4 + 4 + 2: the last global batch is padded for 4 ranks
    streams, lens = _streams(n, t_full, t), _lengths(n, 24)
    one = _steps(ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=3, window=window, lengths=lens))
    for world in (2, 4):
        ranks = [_steps(ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=3, rank=r, world=world, window=window, lengths=lens))
                 for r in range(world)]
        assert {len(r) for r in ranks} == {len(one)}
        for i, whole in enumerate(one):
            joined = [x for r in ranks for x in r[i]["rows"]]
            assert joined[: len(whole["rows"])] == whole["rows"]  # global row g: the same (episode, start, reset, valid) as on one rank
            assert len(joined) - len(whole["rows"]) == (-len(whole["rows"])) % world  # the wrap-around padding rows
            for k, r in enumerate(ranks):  # every rank sees ALL the global rows' valid, padding rows included
                assert r[i]["global"] == [v for *_, v in joined]
                assert r[i]["row0"] == k * len(r[i]["rows"])


def test_validation_errors() -> None:
    streams = _streams(6, 20, 5)
    good = torch.tensor([20, 1, 7, 5, 9, 20])
    for bad, match in ((torch.tensor([20, 0, 7, 5, 9, 20]), "1, 20"), (torch.tensor([21, 1, 7, 5, 9, 20]), "1, 20"), (good[:5], "shape"),
                       (good.reshape(2, 3), "shape"), (good.float(), "integer"), (good.tolist(), "integer")):
        with pytest.raises(ValueError, match=match):
            ds.DeviceEpisodeLoader(streams, 2, shuffle=False, window="sequential", lengths=bad)
    with pytest.raises(ValueError, match="random"):
        ds.DeviceEpisodeLoader(streams, 2, shuffle=False, lengths=good)  # window="first" reads no window
    loader = ds.DeviceEpisodeLoader(streams, 2, shuffle=False, window="sequential", lengths=good)
    assert loader.lengths_host.dtype == torch.int32 and torch.equal(loader.lengths_host, good.to(torch.int32))
    with pytest.raises(ValueError, match=r"\[0, 20\]"):  # a chunk may hang over the store's end, not start past it
        loader.batch(torch.tensor([0, 1]), start=torch.tensor([0, 21]))
    # the t = 0 rule: a row that resets needs a valid frame; a continuing row may be empty
    check_ragged_rows(torch.tensor([3, 0, 1]), torch.tensor([True, False, True]))
    with pytest.raises(ValueError, match=r"rows \[1\]"):
        check_ragged_rows(torch.tensor([3, 0, 1]), torch.tensor([True, True, False]))
    with pytest.raises(ValueError, match=r"rows \[1\]"):
        check_ragged_rows(torch.tensor([3, 0, 1]), None)  # no reset given: every row starts an episode
    # lengths together with a modality mask (checked before anything touches a device)
    batch = tuple(torch.zeros(2, 4, 3) for _ in range(6))
    model = object.__new__(MoPoE_MRSSM)  # (the checks read no parameter)
    with pytest.raises(ValueError, match="not both"):
        model._step_mask(batch, None, torch.ones(2, 4, 2, dtype=torch.bool), None, torch.tensor([4, 2], dtype=torch.int32))  # noqa: SLF001
    with pytest.raises(ValueError, match="int32"):
        model._step_mask(batch, None, None, None, torch.tensor([4, 2]))  # noqa: SLF001


def test_ragged_reference_rule() -> None:
    b, t = 5, 7
    full = dropout.ragged_reference(torch.full((b,), t, dtype=torch.int32), None, t)
    assert bool((full.codes == 3).all()) and full.counts.tolist() == [b * t] * 3 and bool(full.live.all())
    assert full.last.tolist() == [t - 1] * b and full.last.dtype == torch.int32
    valid = torch.tensor([7, 4, 0, 1, 9], dtype=torch.int32)  # (9 is clamped to the 7 steps)
    got = dropout.ragged_reference(valid, None, t)
    assert got.last.tolist() == [6, 3, -1, 0, 6]
    assert got.live.sum(dim=1).tolist() == [7, 4, 0, 1, 7] and got.counts.tolist() == [19.0] * 3
    assert bool((got.codes[2] == 0).all()) and got.codes[1].tolist() == [3, 3, 3, 3, 0, 0, 0]
    # with dropout: the t = 0 fix-up first, then the AND with live
    md = dropout.ModalityDropout(0.5, 0.5, span=3)
    u = torch.rand(md.noise_shape(b, t), generator=torch.Generator().manual_seed(0))
    u[0, 0], u[2, 0] = torch.tensor([0.2, 0.1]), torch.tensor([0.1, 0.2])  # both below p: the fix-up gives row 0 audio; row 2 is dead
    both = dropout.ragged_reference(valid, u, t, md)
    plain = md.reference(u, t)
    assert torch.equal(both.mask, plain & got.live.unsqueeze(-1))
    assert both.mask[0, 0].tolist() == [True, False] and not bool(both.mask[2].any())
    assert both.counts.tolist() == [float(both.mask[..., 0].sum()), float(both.mask[..., 1].sum()), 19.0]
    with pytest.raises(ValueError, match="int32"):
        dropout.ragged_reference(valid.long(), None, t)
    with pytest.raises(ValueError, match="ModalityDropout"):
        dropout.ragged_reference(valid, u, t)
    sm = dropout.StepMask.from_mask(torch.ones(2, 3, 2, dtype=torch.bool))
    assert sm.live is None and sm.count_live is None and sm.last is None  # the records of before carry no lengths


def test_gather_ragged_reference_equals_the_window_gather_when_every_frame_is_live() -> None:
    g = torch.Generator().manual_seed(4)
    store = torch.randn(5, 7, 2, 4, generator=g)
    idx, start = torch.tensor([4, 0, 2, 2]), torch.tensor([0, 3, 1, 2])
    noise = torch.randn(4, 4, 2, 4, generator=g)
    for nz, std in ((noise, 0.1), (None, None)):
        inp, tgt, valid = ds.gather_ragged_reference(store, idx, start, torch.full((5,), 7), 4, nz, std)
        want_inp, want_tgt = ds.gather_window_reference(store, idx, start, 4, nz, std)
        assert torch.equal(inp, want_inp) and torch.equal(tgt, want_tgt) and valid.tolist() == [4, 4, 4, 4]
    # short episodes, a start past the end and a negative one: dead frames are exactly zero in both outputs
    lens = torch.tensor([7, 5, 1, 4, 2])
    idx, start = torch.tensor([0, 1, 2, 3, 4]), torch.tensor([3, 4, 0, 7, -2])
    noise = torch.randn(5, 4, 2, 4, generator=g)
    inp, tgt, valid = ds.gather_ragged_reference(store, idx, start, lens, 4, noise, 0.1)
    assert valid.tolist() == [4, 1, 1, 0, 2] and valid.dtype == torch.int32
    for b, n in enumerate(valid.tolist()):
        s = max(int(start[b]), 0)
        assert torch.equal(tgt[b, :n], store[b, s: s + n]) and torch.equal(inp[b, :n], store[b, s: s + n] + noise[b, :n] * 0.1)
        assert not bool(tgt[b, n:].any()) and not bool(inp[b, n:].any())


def test_save_at_reference() -> None:
    out = torch.arange(4 * 5 * 3, dtype=torch.float32).reshape(4, 5, 3)
    held = -torch.ones(4, 3)
    got = carry.save_at_reference(out, torch.tensor([4, 0, -1, 2], dtype=torch.int32), held)
    assert torch.equal(got[0], out[0, 4]) and torch.equal(got[1], out[1, 0]) and torch.equal(got[3], out[3, 2])
    assert torch.equal(got[2], held[2])  # an empty row keeps its carry
    assert torch.equal(carry.save_at_reference(out, torch.full((4,), 4, dtype=torch.int32), held), carry.save_reference(out))


def test_new_entries_reject_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    p = C.c_void_p(64)  # never dereferenced: every call below returns before a launch
    assert lib.mtrssm_episode_gather_ragged(None, p, p, p, None, 5, 2, 4, 7, 8, 0.0, p, p, None, None) == -1
    assert lib.mtrssm_episode_gather_ragged(p, p, p, None, None, 5, 2, 4, 7, 8, 0.0, p, p, None, None) == -1 and b"lengths" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_gather_ragged(p, p, None, p, None, 5, 2, 4, 7, 8, 0.0, p, p, None, None) == -1
    assert lib.mtrssm_episode_gather_ragged(p, p, p, p, None, 5, 2, 8, 7, 8, 0.0, p, p, None, None) == -1  # T > T_full
    assert lib.mtrssm_episode_gather_ragged(p, p, p, p, None, 5, 2, 4, 7, 6, 0.0, p, p, None, None) == -1 and b"multiple of 4" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_gather_ragged(p, p, p, p, None, 5, 2, 4, 7, 8, 0.0, p, p, C.c_void_p(66), None) == -1 and b"aligned" in lib.mtrssm_last_error()
    args = (p, p, p, p, p, p, p)
    assert lib.mtrssm_step_mask_ragged(None, None, 5, 7, 3, 0.0, 0.0, 0, 5, *args, None) == -1 and b"null" in lib.mtrssm_last_error()
    assert lib.mtrssm_step_mask_ragged(p, None, 5, 7, 3, 0.0, 0.0, 0, 5, p, p, p, None, p, p, p, None) == -1  # no live plane
    assert lib.mtrssm_step_mask_ragged(p, None, 5, 7, 3, 0.0, 0.0, 4, 2, *args, None) == -1  # the slice leaves the batch
    assert lib.mtrssm_step_mask_ragged(p, None, 5, 0, 3, 0.0, 0.0, 0, 5, *args, None) == -1
    assert lib.mtrssm_step_mask_ragged(p, p, 5, 7, 3, 1.0, 0.0, 0, 5, *args, None) == -1 and b"probabilities" in lib.mtrssm_last_error()
    assert lib.mtrssm_step_mask_ragged(p, None, 1 << 20, 16, 3, 0.0, 0.0, 0, 5, *args, None) == -1 and b"2^24" in lib.mtrssm_last_error()
    assert lib.mtrssm_elbo_combine_counted_fwd(p, p, p, None, None, p, 10, 1.0, 0.0, p, p, None, p, None) == -1  # no live plane
    assert lib.mtrssm_elbo_combine_counted_fwd(p, p, p, None, p, None, 10, 1.0, 0.0, p, p, None, p, None) == -1  # no count
    assert lib.mtrssm_elbo_combine_counted_fwd(p, p, p, None, p, p, 0, 1.0, 0.0, p, p, None, p, None) == -1
    assert lib.mtrssm_elbo_combine_counted_bwd(None, None, None, p, p, None, 10, 1.0, 0.0, p, p, p, None, None) == -1
    assert lib.mtrssm_elbo_combine_counted_bwd(None, None, None, p, p, p, 10, 1.0, 0.0, p, p, None, None, None) == -1
    table = _lib.StateTable()
    table.count = 1
    table.width[0], table.src[0], table.dst[0] = 4, 64, 128
    assert lib.mtrssm_state_save_at(C.byref(table), None, 4, 5, None) == -1 and b"last" in lib.mtrssm_last_error()
    assert lib.mtrssm_state_save_at(C.byref(table), C.c_void_p(66), 4, 5, None) == -1
    assert lib.mtrssm_state_save_at(C.byref(table), p, 4, 0, None) == -1 and b"steps" in lib.mtrssm_last_error()
    assert lib.mtrssm_state_save_at(None, p, 4, 5, None) == -1
    table.count = 7
    assert lib.mtrssm_state_save_at(C.byref(table), p, 4, 5, None) == -1 and b"count" in lib.mtrssm_last_error()


def test_random_starts_with_lengths_are_uniform_per_row() -> None:
    """One short episode among full-length ones, many epochs: its starts cover [0, len - T] evenly (a modulo of the full-range draw would
    favour the low starts: 33 draw values onto 20 starts make 0..12 twice as likely as 13..19), the others keep the plain draw."""
    n, t_full, t = 4, 40, 8  # the draw has 33 values; episode 2 has room for 20 starts
    lens = torch.tensor([40, 40, 27, 40])
    streams = _streams(n, t_full, t)
    loader = ds.DeviceEpisodeLoader(streams, 4, shuffle=False, seed=0, window="random", lengths=lens)
    plain = ds.DeviceEpisodeLoader(streams, 4, shuffle=False, seed=0, window="random")
    counts = torch.zeros(20, dtype=torch.int64)
    epochs = 4000
    for _ in range(epochs):
        (_, start, _), (_, want, _) = next(iter(loader.schedule())), next(iter(plain.schedule()))
        assert start[[0, 1, 3]].tolist() == want[[0, 1, 3]].tolist()  # full-length rows: the draw of a loader without lengths
        counts[int(start[2])] += 1
    # 20 equally likely starts, 4000 draws: mean 200, standard deviation 13.8 per bin; five sigma either way.  The modulo's bins
    # would sit at 242 (starts 0..12) and 121 (13..19), 5.7 sigma below the mean.
    assert int(counts.min()) > 200 - 69 and int(counts.max()) < 200 + 69, counts.tolist()
    assert abs(int(counts[:13].sum()) - 2600) < 5 * 30.2  # sd of a Binomial(4000, 0.65); the modulo gives 3152


def _write_episodes(root: Path, frames: list[int]) -> None:
    d = root / "processed_toy"
    d.mkdir(parents=True)
    g = torch.Generator().manual_seed(31)
    for i, n in enumerate(frames):
        torch.save(torch.randn(n, 4, generator=g), d / f"act_{i:03d}.pt")
        torch.save(torch.rand(n, 1, 4, 2, generator=g) + 1.0, d / f"audio_obs_{i:03d}.pt")
        torch.save(torch.rand(n, 1, 2, 2, generator=g) + 1.0, d / f"vision_obs_{i:03d}.pt")


def _config(root: Path, lengths: torch.Tensor | None) -> ds.EpisodeDataModuleConfig:
    ident = torch.nn.Identity()
    return ds.EpisodeDataModuleConfig(
        data_name="toy", batch_size=2, num_workers=0, gdrive_url="", action_preprocess=ident,
        action_input_transform=_chain(3, 0.1), action_target_transform=_chain(3, None),
        audio_observation_file_name="audio.npy", vision_observation_file_name="vision.npy",
        audio_observation_preprocess=ident, vision_observation_preprocess=ident,
        audio_observation_input_transform=_chain(3, 0.1), audio_observation_target_transform=_chain(3, None),
        vision_observation_input_transform=_chain(3, 0.1), vision_observation_target_transform=_chain(3, None),
        data_root=root, window="sequential", lengths=lengths)


def test_datamodule_pads_the_store_and_splits_the_lengths(tmp_path: Path) -> None:
    frames = [7, 4, 9, 5, 6, 3, 8, 4, 5, 2]  # 8 train episodes, 2 validation ones
    _write_episodes(tmp_path, frames)
    lens = torch.tensor(frames)
    lens[2] = 6  # an episode may be cut short of its file
    dm = ds.EpisodeDataModule(_config(tmp_path, lens), device="cpu")
    dm.setup("fit")
    assert {tuple(s.store.shape[:2]) for s in dm.train_streams} == {(8, 9)}  # all three streams padded to the longest train file
    assert {tuple(s.store.shape[:2]) for s in dm.val_streams} == {(2, 5)}
    for s in dm.train_streams:
        for i, n in enumerate(frames[:8]):
            assert not bool(s.store[i, n:].any())  # zeros behind the file's end
            assert bool(s.store[i, :n].flatten(1).any(dim=1).all()) or s is dm.train_streams[0]
    train, val = dm.train_dataloader(), dm.val_dataloader()
    assert train.lengths_host.tolist() == lens[:8].tolist() and val.lengths_host.tolist() == lens[8:].tolist()
    assert train.n_chunks == 3 and val.n_chunks == 2 and train.window == "sequential"  # ceil(8 / 3), ceil(5 / 3)
    # without lengths the store is the common prefix, as before
    plain = ds.EpisodeDataModule(_config(tmp_path, None), device="cpu")
    plain.setup("fit")
    assert {tuple(s.store.shape[:2]) for s in plain.train_streams} == {(8, 3)} and plain.train_dataloader().lengths is None
    # a length beyond its file, a wrong number of lengths
    too_long = torch.tensor(frames)
    too_long[1] = 5
    with pytest.raises(ValueError, match="file holds 4"):
        ds.EpisodeDataModule(_config(tmp_path, too_long), device="cpu").setup("fit")
    with pytest.raises(ValueError, match="one entry per episode"):
        ds.EpisodeDataModule(_config(tmp_path, lens[:9]), device="cpu").setup("fit")
    # the streams of an episode must agree on its frames
    torch.save(torch.randn(6, 4), tmp_path / "processed_toy" / "act_000.pt")
    with pytest.raises(ValueError, match="not the same number"):
        ds.EpisodeDataModule(_config(tmp_path, lens), device="cpu").setup("fit")


def test_unfused_stream_takes_the_per_episode_path() -> None:
    """A stream the gather kernel does not take (event size 6) restates the rule per episode: zeros on dead frames, also after a noise
    transform, and ``valid`` on request."""
    g = torch.Generator().manual_seed(8)
    store = torch.randn(3, 6, 6, generator=g)
    stream = ds._Stream(store, _chain(3, 0.1), _chain(3, None))  # noqa: SLF001
    assert not stream.fused
    lens, idx, start = torch.tensor([6, 4, 2], dtype=torch.int32), torch.tensor([0, 1, 2]), torch.tensor([3, 3, 3], dtype=torch.int32)
    valid = torch.zeros(3, dtype=torch.int32)
    inp, tgt = stream.batch(idx, None, start, [3, 3, 3], lens, valid, lens)
    _, want, want_valid = ds.gather_ragged_reference(store, idx, start, lens, 3, None, None)
    assert torch.equal(tgt, want) and torch.equal(valid, want_valid) and valid.tolist() == [3, 1, 0]
    assert not bool(inp[1, 1:].any()) and not bool(inp[2].any()) and bool((inp[0] != tgt[0]).any())  # noise on live frames only
