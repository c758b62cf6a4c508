"""GPU (MI355X): ``mtrssm_episode_gather_seeded`` against its host restatement
``dataset.feed_noise_reference`` and, bit for bit, against the three unseeded gathers; the invariances the seeded noise exists for
(row, batch size, window start, rank count, replayed epochs); the loader and the data module on top of it.

Tolerance of the normals: ``r <= 5.77`` and the accurate ``logf`` / ``sqrtf`` / ``sincospif`` are within a few ulp, which bounds the
error near 3e-6; an fp32 evaluation of the same formulas on the host gave 1.4e-6 over 4e5 samples.  The bound is 1e-5."""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T_FULL = 5, 12
EVENTS = ((1, 4, 4), (4,))
KEY = ds.stream_key(7, 1)
TOL = 1e-5
FORMS = ("first", "window", "ragged")
LENGTHS = (12, 3, 7, 1, 9)


def _store(event: tuple, zero: bool = False) -> torch.Tensor:  # noqa: FBT001, FBT002
    if zero:
        return torch.zeros(N, T_FULL, *event, device=DEV)
    g = torch.Generator().manual_seed(41)
    return (torch.rand(N, T_FULL, *event, generator=g) * 2 - 1).to(DEV)  # |x| < 1: |x + 0.1 z| < 2


def _i32(values) -> torch.Tensor:  # noqa: ANN001
    return torch.as_tensor(values, dtype=torch.int32).to(DEV)


def _seeded(store: torch.Tensor, idx: torch.Tensor, t: int, *, start=None, lengths=None, key=KEY, epoch: int = 0, std: float = 1.0):  # noqa: ANN001, ANN202, PLR0913
    """One call of the C entry: ``(input, target, valid)``; ``valid`` None unless ragged."""
    b, event = idx.numel(), store.shape[2:]
    e = int(torch.Size(event).numel())
    inp = torch.full((b, t, *event), float("nan"), device=DEV)
    tgt = torch.full_like(inp, float("nan"))
    valid = None if lengths is None else torch.full((b,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mtrssm_episode_gather_seeded(
        _lib.ptr(store), _lib.raw_ptr(idx), _lib.index_ptr(start), _lib.index_ptr(lengths), _lib.index_ptr(valid), key[0], key[1], epoch,
        store.shape[0], b, t, store.shape[1], e, std, _lib.ptr(inp), _lib.ptr(tgt), _lib.stream_ptr(store.device)), "mtrssm_episode_gather_seeded")
    torch.cuda.synchronize()
    return inp, tgt, valid


def _unseeded(form: str, store: torch.Tensor, idx: torch.Tensor, t: int, start, lengths):  # noqa: ANN001, ANN202, PLR0913
    """``(target, valid)`` of the unseeded kernel of the same form (no noise: input is not asked for)."""
    lib = _lib.load()
    b, e = idx.numel(), int(torch.Size(store.shape[2:]).numel())
    tgt = torch.full((b, t, *store.shape[2:]), float("nan"), device=DEV)
    valid = None
    common = (store.shape[0], b, t, store.shape[1], e, 0.0, None, _lib.ptr(tgt))
    if form == "first":
        _lib.check(lib.mtrssm_episode_gather(_lib.ptr(store), _lib.raw_ptr(idx), None, *common, None), "gather")
    elif form == "window":
        _lib.check(lib.mtrssm_episode_gather_window(_lib.ptr(store), _lib.raw_ptr(idx), _lib.index_ptr(start), None, *common, None), "window")
    else:
        valid = torch.full((b,), -1, dtype=torch.int32, device=DEV)
        _lib.check(lib.mtrssm_episode_gather_ragged(_lib.ptr(store), _lib.raw_ptr(idx), _lib.index_ptr(start), _lib.index_ptr(lengths), None,
                                                    *common, _lib.index_ptr(valid), None), "ragged")
    torch.cuda.synchronize()
    return tgt, valid


def _case(form: str, t: int):  # noqa: ANN202
    """``idx``, ``start``, ``lengths`` (device) of a form plus the absolute frames ``[B, T]`` and the live mask of its rows (host).
    The starts include one below 0 and one past the last window: the kernel clamps them as the unseeded kernel of the form does."""
    idx = torch.tensor([3, 0, 4, 1, 2, 2])
    raw = torch.tensor([0, 2, 5, -3, 40, 3])
    if form == "first":
        s = torch.zeros(6, dtype=torch.long)
        start = lengths = None
    elif form == "window":
        s, start, lengths = raw.clamp(0, T_FULL - t), _i32(raw), None
    else:
        s, start, lengths = raw.clamp(0, T_FULL), _i32(raw), _i32(LENGTHS)
    frames = s[:, None] + torch.arange(t)
    live = torch.ones(6, t, dtype=torch.bool) if form != "ragged" else frames < torch.tensor(LENGTHS)[idx][:, None]
    return idx.to(DEV), start, lengths, frames, live


def _expand(live: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return live.reshape(*live.shape, *([1] * (like.dim() - 2))).expand_as(like)


@pytest.mark.parametrize("t", [4, 5])
@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("form", FORMS)
def test_kernel_equals_the_restatement(form: str, event: tuple, t: int) -> None:
    idx, start, lengths, frames, live = _case(form, t)
    e = int(torch.Size(event).numel())
    z = ds.feed_noise_reference(KEY, 2, idx, frames, e).reshape(6, t, *event)
    # a zero store and std = 1: both roundings are exact, the input is z itself
    inp, tgt, _ = _seeded(_store(event, zero=True), idx, t, start=start, lengths=lengths, epoch=2, std=1.0)
    mask = _expand(live, z)
    err = float((inp.cpu().double() - z)[mask].abs().max())
    print(f"{form} {event} T={t}: max |input - z_ref| = {err:.3e}")
    assert err <= TOL
    assert bool((tgt == 0).all()) and bool((inp.cpu()[~mask] == 0).all())
    # a random store and std = 0.1: target bitwise the unseeded kernel's, input = target + 0.1 z to the same bound
    store = _store(event)
    inp, tgt, valid = _seeded(store, idx, t, start=start, lengths=lengths, epoch=2, std=0.1)
    want_tgt, want_valid = _unseeded(form, store, idx, t, start, lengths)
    assert torch.equal(tgt, want_tgt)
    if form == "ragged":
        assert torch.equal(valid, want_valid)
    want = tgt.cpu().double() + 0.1 * z
    err = float((inp.cpu().double() - want)[mask].abs().max())
    print(f"{form} {event} T={t}: max |input - (target + 0.1 z_ref)| = {err:.3e}")
    assert err <= 0.1 * TOL + 2.4e-7  # + one ulp at magnitude 2 for the two roundings
    assert bool((inp.cpu()[~mask] == 0).all())


@pytest.mark.parametrize("t", [4, 5])
@pytest.mark.parametrize("event", EVENTS)
def test_ragged_dead_frames_are_zero_and_live_ones_the_windowed_forms(event: tuple, t: int) -> None:
    store = _store(event) + 3.0  # no stored zero: a zero in the output is a dead frame
    idx = torch.tensor([3, 0, 4, 1, 2, 2]).to(DEV)
    raw = torch.tensor([0, 2, 5, 1, 7, 3])  # all inside [0, T_full - T]: both forms see the same windows
    start, lengths = _i32(raw), _i32(LENGTHS)
    inp, tgt, valid = _seeded(store, idx, t, start=start, lengths=lengths, std=0.1)
    win_inp, win_tgt, _ = _seeded(store, idx, t, start=start, std=0.1)
    want_tgt, want_valid = _unseeded("ragged", store, idx, t, start, lengths)
    live = _expand((raw[:, None] + torch.arange(t)) < torch.tensor(LENGTHS)[idx.cpu()][:, None], inp).to(DEV)
    assert 0 < int(live.sum()) < live.numel()
    assert bool((inp[~live] == 0).all()) and bool((tgt[~live] == 0).all())
    assert torch.equal(valid, want_valid) and torch.equal(tgt, want_tgt)
    assert valid.tolist() == [min(max(LENGTHS[i] - s, 0), t) for i, s in zip(idx.tolist(), raw.tolist(), strict=True)]
    assert torch.equal(inp[live], win_inp[live]) and torch.equal(tgt[live], win_tgt[live])
    assert bool((inp[live] != tgt[live]).any())


@pytest.mark.parametrize("event", EVENTS)
def test_noise_is_invariant_to_row_batch_size_and_window_start(event: tuple) -> None:
    t = 4
    store = _store(event)
    idx = torch.tensor([3, 0, 4, 1, 2, 2]).to(DEV)
    start = _i32([0, 2, 5, 1, 8, 3])
    lengths = _i32(LENGTHS)
    for kw in ({}, {"start": start}, {"start": start, "lengths": lengths}):
        a = _seeded(store, idx, t, std=0.1, **kw)
        again = _seeded(store, idx, t, std=0.1, **kw)
        assert torch.equal(a[0], again[0]) and torch.equal(a[1], again[1])  # the same arguments twice
        perm = torch.tensor([4, 2, 0, 5, 1, 3]).to(DEV)  # permuted rows: rows permuted and nothing else
        pkw = {k: (v[perm].contiguous() if k == "start" else v) for k, v in kw.items()}
        p = _seeded(store, idx[perm].contiguous(), t, std=0.1, **pkw)
        assert torch.equal(p[0], a[0][perm]) and torch.equal(p[1], a[1][perm])
        halves = [_seeded(store, idx[lo: lo + 3].contiguous(), t, std=0.1,  # B = 6 against two calls with B = 3
                          **{k: (v[lo: lo + 3].contiguous() if k == "start" else v) for k, v in kw.items()}) for lo in (0, 3)]
        assert torch.equal(torch.cat([h[0] for h in halves]), a[0]) and torch.equal(torch.cat([h[1] for h in halves]), a[1])
    # the same episode at start 0 and at start 3: the absolute frames both windows hold carry the same input
    ep = torch.tensor([2, 2]).to(DEV)
    t5 = 5
    inp, _, _ = _seeded(store, ep, t5, start=_i32([0, 3]), std=0.1)
    assert torch.equal(inp[0, 3:], inp[1, : t5 - 3])
    assert not torch.equal(inp[0, : t5 - 3], inp[1, : t5 - 3])
    # a start past T_full - T gives the clamped window's frames and noise
    far = _seeded(store, ep, t5, start=_i32([40, -7]), std=0.1)
    edge = _seeded(store, ep, t5, start=_i32([T_FULL - t5, 0]), std=0.1)
    assert torch.equal(far[0], edge[0]) and torch.equal(far[1], edge[1])
    # the first-T form is the windowed form at start 0
    first = _seeded(store, idx, t, std=0.1)
    zero = _seeded(store, idx, t, start=_i32([0] * 6), std=0.1)
    assert torch.equal(first[0], zero[0]) and torch.equal(first[1], zero[1])
    assert bool((first[0] != first[1]).any())


@pytest.mark.parametrize("form", FORMS)
def test_epoch_seed_and_stream_change_the_inputs_only(form: str) -> None:
    t, event = 5, (1, 4, 4)
    idx, start, lengths, _, live = _case(form, t)
    store = _store(event)
    base = _seeded(store, idx, t, start=start, lengths=lengths, std=0.1)
    mask = _expand(live, base[0]).to(DEV)
    for what, kw in {"epoch": {"epoch": 1}, "seed": {"key": ds.stream_key(8, 1)}, "seed_high": {"key": ds.stream_key(7 + 2 ** 32, 1)},
                     "stream": {"key": ds.stream_key(7, 2)}}.items():
        other = _seeded(store, idx, t, start=start, lengths=lengths, std=0.1, **kw)
        assert torch.equal(other[1], base[1]), what
        assert float((other[0][mask] == base[0][mask]).float().mean()) < 0.01, what


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(t: int) -> tuple:
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(N, T_FULL, *e, generator=g).to(DEV), _chain(t, 0.1), _chain(t, None))  # noqa: SLF001
                 for e in ((4,), (1, 4, 4), (1, 4, 4)))


def _same(a: tuple, b: tuple) -> bool:
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b, strict=True))


@pytest.mark.parametrize("lengths", [None, torch.tensor(LENGTHS)])
def test_loader_noise_is_the_same_on_one_and_two_ranks_and_replays(lengths: torch.Tensor | None) -> None:
    t = 4
    streams = _streams(t)
    kw = {"shuffle": True, "seed": 3, "window": "random", "noise_seed": 7, "lengths": lengths}
    one = ds.DeviceEpisodeLoader(streams, 4, **kw)
    ranks = [ds.DeviceEpisodeLoader(streams, 4, rank=r, world=2, **kw) for r in (0, 1)]
    epochs = []
    for _ in range(2):
        whole = list(one)
        halves = [list(r) for r in ranks]
        assert len(whole) == len(halves[0]) == len(halves[1]) == 2  # 4 rows, then 1 (two ranks: padded to 2 by wrapping)
        for k, batch in enumerate(whole):
            both = tuple(torch.cat([halves[0][k][j], halves[1][k][j]]) for j in range(6))
            rows = batch[0].shape[0]
            assert rows == (4, 1)[k] and both[0].shape[0] == (4, 2)[k]
            assert _same(tuple(batch), tuple(x[:rows] for x in both))
        # the padding row is the epoch's first row again: same episode, same window, hence the same noise
        assert all(torch.equal(halves[1][1][j][0], whole[0][j][0]) for j in range(6))
        assert all(bool((whole[0][j] != whole[0][3 + j]).any()) for j in range(3))  # all three streams carry noise
        epochs.append(whole)
    assert not any(torch.equal(epochs[0][0][j], epochs[1][0][j]) for j in range(3))  # epoch 1: other rows, other noise
    one.set_epoch(0)
    assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(one), epochs[0], strict=True))  # epoch 0 again, bit for bit
    assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(one), epochs[1], strict=True))
    # a fixed loader yields epoch 0's batches every epoch
    fixed = ds.DeviceEpisodeLoader(streams, 4, noise_epoch="fixed", **kw)
    for _ in range(2):
        assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(fixed), epochs[0], strict=True))


def test_loader_batch_matches_the_restatement_and_injected_noise_wins() -> None:
    t = 5
    streams = _streams(t)
    loader = ds.DeviceEpisodeLoader(streams, 6, shuffle=False, window="random", noise_seed=2 ** 63 + 11)
    loader.set_epoch(4)
    idx = torch.tensor([1, 4, 0]).to(DEV)
    start = torch.tensor([2, 7, 0], dtype=torch.int32)
    batch = loader.batch(idx, start=start)
    frames = start.long()[:, None] + torch.arange(t)
    for k, s in enumerate(streams):
        z = ds.feed_noise_reference(ds.stream_key(2 ** 63 + 11, k), 4, idx, frames, s.event).reshape(3, t, *s.event_shape)
        assert torch.equal(batch[3 + k], s.store[idx.cpu()[:, None], frames])
        # (a randn store: |input| < 8, where the add rounds by at most half an ulp = 2.4e-7 and the product by 3e-8 more)
        assert float((batch[k].cpu().double() - (batch[3 + k].cpu().double() + 0.1 * z)).abs().max()) <= 0.1 * TOL + 4.8e-7
    mine = tuple(torch.full((3, t, *s.event_shape), 2.0, device=DEV) for s in streams)
    injected = loader.batch(idx, noise=mine, start=start)
    for k in range(3):
        assert torch.equal(injected[k], injected[3 + k] + mine[k] * 0.1)


def test_default_loader_still_draws_unseeded_noise() -> None:
    loader = ds.DeviceEpisodeLoader(_streams(4), 4, shuffle=True, seed=3, window="random")
    loader.set_epoch(0)
    a = list(loader)
    loader.set_epoch(0)
    b = list(loader)
    assert all(torch.equal(x[3 + j], y[3 + j]) for x, y in zip(a, b, strict=True) for j in range(3))  # the same rows and windows
    assert not any(torch.equal(x[j], y[j]) for x, y in zip(a, b, strict=True) for j in range(3))  # fresh normals


def _config(root: Path, t: int, **kw) -> ds.EpisodeDataModuleConfig:  # noqa: ANN003
    ident = torch.nn.Identity()
    return ds.EpisodeDataModuleConfig(
        data_name="toy", batch_size=2, num_workers=0, gdrive_url="", action_preprocess=ident,
        action_input_transform=_chain(t, 0.1), action_target_transform=_chain(t, None),
        audio_observation_file_name="audio.npy", vision_observation_file_name="vision.npy",
        audio_observation_preprocess=ident, vision_observation_preprocess=ident,
        audio_observation_input_transform=_chain(t, 0.1), audio_observation_target_transform=_chain(t, None),
        vision_observation_input_transform=_chain(t, 0.1), vision_observation_target_transform=_chain(t, None),
        data_root=root, window="random", **kw)


def test_data_module_validation_inputs_are_the_same_every_epoch(tmp_path: Path) -> None:
    d = tmp_path / "processed_toy"
    d.mkdir(parents=True)
    g = torch.Generator().manual_seed(31)
    for i in range(2 * N):  # 8 train episodes, 2 validation ones
        torch.save(torch.randn(T_FULL, 4, generator=g), d / f"act_{i:03d}.pt")
        torch.save(torch.rand(T_FULL, 1, 4, 4, generator=g), d / f"audio_obs_{i:03d}.pt")
        torch.save(torch.rand(T_FULL, 1, 4, 4, generator=g), d / f"vision_obs_{i:03d}.pt")
    dm = ds.EpisodeDataModule(_config(tmp_path, 4, noise_seed=7), device=DEV)
    dm.setup()
    val = dm.val_dataloader()
    assert val.noise_seed == 7 and val.noise_epoch == "fixed"
    first, second = list(val), list(val)
    assert len(first) == 1 and _same(tuple(first[0]), tuple(second[0]))
    assert all(bool((first[0][j] != first[0][3 + j]).any()) for j in range(3))
    train = dm.train_dataloader()
    assert train.noise_seed == 7 and train.noise_epoch == "advance"
    a, b = list(train), list(train)
    assert not any(torch.equal(x[j], y[j]) for x, y in zip(a, b, strict=True) for j in range(3))
    train.set_epoch(0)
    assert all(_same(tuple(x), tuple(y)) for x, y in zip(list(train), a, strict=True))
    # without a seed the validation loader draws fresh noise each epoch, as before
    plain = ds.EpisodeDataModule(_config(tmp_path, 4), device=DEV)
    plain.setup()
    val = plain.val_dataloader()
    assert val.noise_seed is None and val.noise_epoch == "advance"
    first, second = list(val), list(val)
    assert not torch.equal(first[0][0], second[0][0])


def test_c_entry_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    store = _store((1, 4, 4))
    idx = torch.tensor([0, 1]).to(DEV)
    out = torch.empty(2, 4, 16, device=DEV)
    start, lengths = _i32([0, 1]), _i32(LENGTHS)
    p, q = _lib.ptr(store), _lib.ptr(out)

    def call(*, e: int = 16, src: int = p, dst: int = q, st=_lib.index_ptr(start), ln=None, valid=None, t: int = 4):  # noqa: ANN001, ANN202, PLR0913
        return lib.mtrssm_episode_gather_seeded(src, _lib.raw_ptr(idx), st, ln, valid, 1, 2, 3, N, 2, t, T_FULL, e, 0.1, dst, None, None)

    assert call(e=6) == -1 and b"multiple of 4" in lib.mtrssm_last_error()
    assert call(dst=q + 4) == -1 and b"16-byte aligned" in lib.mtrssm_last_error()
    assert call(src=p + 8) == -1 and b"16-byte aligned" in lib.mtrssm_last_error()
    assert call(st=None, ln=_lib.index_ptr(lengths)) == -1 and b"lengths without start" in lib.mtrssm_last_error()
    assert call(valid=C.c_void_p(_lib.index_ptr(start))) == -1 and b"valid_out without lengths" in lib.mtrssm_last_error()
    assert call(st=C.c_void_p(_lib.index_ptr(start) + 2)) == -1 and b"4-byte aligned" in lib.mtrssm_last_error()
    assert call(t=T_FULL + 1) == -1 and b"bad argument" in lib.mtrssm_last_error()
    assert call(src=None) == -1 and b"bad argument" in lib.mtrssm_last_error()
    assert call() == 0  # the same arguments, all in order
    torch.cuda.synchronize()
