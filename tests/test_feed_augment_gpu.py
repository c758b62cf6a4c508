"""GPU (MI355X): ``mtrssm_episode_gather_augmented`` through the C-ABI against its host restatement
``dataset.feed_augment_reference`` -- bit for bit: the shift and the masks are integers, the pixels are copied or replaced, nothing is
rounded -- and against ``mtrssm_episode_gather_seeded`` for the noise; the invariances the seeded feed exists for; the loader on top.

Shapes: frames of 8 x 8, 2 x 4 x 12 and 16 x 4 (one, three and one aligned quad per row: a shift by ``W - 1`` leaves one pixel of a row,
``dx % 4`` takes every value, 2 channels and more than one row per quad column make a read of the neighbouring row or channel show),
B = 3 rows, T = 4 or 5 of 9 stored frames, starts on both sides of the allowed range.

Tolerance of the noisy input: §6e's, 1e-5 on the normals at std = 1 (see ``test_feed_noise_gpu.py``)."""

from __future__ import annotations

import ctypes as C
import functools
import itertools

import pytest
import torch

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, T_FULL, B = 5, 9, 3
EVENTS = ((1, 8, 8), (2, 4, 12), (1, 16, 4))
FORMS = ("first", "window", "ragged")
LENGTHS = (9, 3, 7, 1, 5)
SEED, STREAM = 7, 1
KEY, AKEY = ds.stream_key(SEED, STREAM), ds.augment_key(SEED, STREAM)
TOL = 1e-5
IDX = (2, 0, 4)
RAW_START = (5, -3, 40)  # inside, below 0, past the end: ragged rows with two live frames, all live, none


def _shifts(event: tuple) -> tuple:
    h, w = event[1:]
    return ((2, 3), (0, 1), (3, 0), (h - 1, w - 1))  # (every event here has H >= 4 and W >= 4)


def _augments(event: tuple) -> list[ds.FeedAugment]:
    """Every shift x (no bands | 1 or 4 bands x max_rows in {0, H} x max_cols in {0, 3} x per_frame)."""
    h = event[1]
    bands = [{}] + [{"bands": n, "max_rows": r, "max_cols": c, "per_frame": p}
                    for n, r, c, p in itertools.product((1, 4), (0, h), (0, 3), (False, True))]
    return [ds.FeedAugment(shift=s, **kw) for s in _shifts(event) for kw in bands]


@functools.cache
def _stores(event: tuple) -> tuple[torch.Tensor, torch.Tensor]:
    """``(device, host)`` copies of one seeded store per event, values in (-1, 1) and never the fill."""
    g = torch.Generator().manual_seed(41)
    host = torch.rand(N, T_FULL, *event, generator=g) * 1.8 - 0.9
    return host.to(DEV), host


def _i32(values) -> torch.Tensor:  # noqa: ANN001
    return torch.as_tensor(values, dtype=torch.int32).to(DEV)


def _case(form: str, t: int, idx: tuple = IDX, raw: tuple = RAW_START):  # noqa: ANN202
    """``idx``, ``start``, ``lengths`` (device) of a form plus the absolute frames ``[B, T]`` and the live mask (host), the clamps
    being those of the form."""
    ep, raw_t = torch.tensor(idx), torch.tensor(raw)
    if form == "first":
        s, start, lengths = torch.zeros(len(idx), dtype=torch.long), None, None
    elif form == "window":
        s, start, lengths = raw_t.clamp(0, T_FULL - t), _i32(raw), None
    else:
        s, start, lengths = raw_t.clamp(0, T_FULL), _i32(raw), _i32(LENGTHS)
    frames = s[:, None] + torch.arange(t)
    live = torch.ones(len(idx), t, dtype=torch.bool) if form != "ragged" else frames < torch.tensor(LENGTHS)[ep][:, None]
    return ep.to(DEV), start, lengths, frames, live


def _augmented(store: torch.Tensor, idx: torch.Tensor, t: int, aug: ds.FeedAugment, *, start=None, lengths=None, key=KEY, akey=AKEY,  # noqa: ANN001, ANN202, PLR0913
               epoch: int = 0, noisy: int = 0, std: float = 1.0):
    """One call of the C entry: ``(input, target, valid)``; ``valid`` None unless ragged.  The outputs start as NaN."""
    b, event = idx.numel(), tuple(store.shape[2:])
    inp = torch.full((b, t, *event), float("nan"), device=DEV)
    tgt = torch.full_like(inp, float("nan"))
    valid = None if lengths is None else torch.full((b,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mtrssm_episode_gather_augmented(
        C.byref(aug.c_struct()), _lib.ptr(store), _lib.raw_ptr(idx), _lib.index_ptr(start), _lib.index_ptr(lengths), _lib.index_ptr(valid),
        key[0], key[1], akey[0], akey[1], epoch, store.shape[0], b, t, store.shape[1], *event, noisy, std, _lib.ptr(inp), _lib.ptr(tgt),
        _lib.stream_ptr(store.device)), "mtrssm_episode_gather_augmented")
    torch.cuda.synchronize()
    return inp, tgt, valid


def _seeded(store: torch.Tensor, idx: torch.Tensor, t: int, *, start=None, lengths=None, key=KEY, epoch: int = 0, std: float = 1.0):  # noqa: ANN001, ANN202, PLR0913
    b, event = idx.numel(), tuple(store.shape[2:])
    inp = torch.full((b, t, *event), float("nan"), device=DEV)
    tgt = torch.full_like(inp, float("nan"))
    valid = None if lengths is None else torch.full((b,), -1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().mtrssm_episode_gather_seeded(
        _lib.ptr(store), _lib.raw_ptr(idx), _lib.index_ptr(start), _lib.index_ptr(lengths), _lib.index_ptr(valid), key[0], key[1], epoch,
        store.shape[0], b, t, store.shape[1], int(torch.Size(event).numel()), std, _lib.ptr(inp), _lib.ptr(tgt), _lib.stream_ptr(store.device)),
        "mtrssm_episode_gather_seeded")
    torch.cuda.synchronize()
    return inp, tgt, valid


def _valid(form: str, t: int, idx: tuple = IDX, raw: tuple = RAW_START) -> list[int]:
    return [min(max(LENGTHS[i] - min(max(s, 0), T_FULL), 0), t) for i, s in zip(idx, raw, strict=True)]


@pytest.mark.parametrize("t", [4, 5])
@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("form", FORMS)
def test_target_and_base_are_bitwise_the_restatement(form: str, event: tuple, t: int) -> None:
    store, host = _stores(event)
    idx, start, lengths, frames, live = _case(form, t)
    moved = masked = 0
    for k, aug in enumerate(_augments(event)):
        epoch = k % 3
        inp, tgt, valid = _augmented(store, idx, t, aug, start=start, lengths=lengths, epoch=epoch)
        base, target = ds.feed_augment_reference(host, idx, frames, AKEY, epoch, aug, live=live)
        assert torch.equal(tgt.cpu(), target), aug
        assert torch.equal(inp.cpu(), base), aug
        moved += int(not torch.equal(target, host[idx.cpu()[:, None], frames.clamp(max=T_FULL - 1)] * live[:, :, None, None, None]))
        masked += int(not torch.equal(base, target))
        if form == "ragged":
            assert valid.tolist() == _valid(form, t)
            dead = ~live
            assert 0 < int(dead.sum()) < dead.numel()
            assert bool((inp.cpu()[dead] == 0).all()) and bool((tgt.cpu()[dead] == 0).all())  # exactly zero, not fill
    assert moved > 10 and masked > 10  # the cases did shift and did mask
    # the noise is the seeded entry's, keyed by the OUTPUT element: zero store, fill 0 -> base 0 whatever the shift and the masks
    zero = torch.zeros_like(store)
    want = _seeded(zero, idx, t, start=start, lengths=lengths, epoch=2)[0]
    assert bool((want != 0).any())
    for shift in _shifts(event):
        aug = ds.FeedAugment(shift=shift, bands=4, max_rows=event[1], max_cols=3, per_frame=True, fill=0.0)
        inp, tgt, _ = _augmented(zero, idx, t, aug, start=start, lengths=lengths, epoch=2, noisy=1)
        assert torch.equal(inp, want) and bool((tgt == 0).all())


@pytest.mark.parametrize("event", [(3, 10, 40), (1, 128, 32), (1, 64, 64), (5, 1, 1040)])
@pytest.mark.parametrize("form", FORMS)
def test_frames_of_more_than_256_quads(form: str, event: tuple) -> None:
    """A lane walks quads q, q + 256, ... by additions: 3 x 10 x 40 (300 quads of 10 per row: the step carries from the column into
    the row and from the row into the channel), the bench frames (1024 quads, no carry), and rows longer than 256 quads."""
    t = 4
    store, host = _stores(event)
    idx, start, lengths, frames, live = _case(form, t)
    h, w = event[1:]
    for k, shift in enumerate(((min(2, h - 1), 3), (0, 1), (h - 1, w - 1))):
        aug = ds.FeedAugment(shift=shift, bands=4, max_rows=h // 2, max_cols=3, per_frame=True)
        inp, tgt, _ = _augmented(store, idx, t, aug, start=start, lengths=lengths, epoch=k)
        base, target = ds.feed_augment_reference(host, idx, frames, AKEY, k, aug, live=live)
        assert torch.equal(tgt.cpu(), target) and torch.equal(inp.cpu(), base), aug
    # the noise follows the output element through the walk too
    zero = torch.zeros_like(store)
    want = _seeded(zero, idx, t, start=start, lengths=lengths, epoch=2)[0]
    aug = ds.FeedAugment(shift=(h - 1, 3), bands=2, max_rows=h, max_cols=3, fill=0.0)
    assert torch.equal(_augmented(zero, idx, t, aug, start=start, lengths=lengths, epoch=2, noisy=1)[0], want)


@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("form", FORMS)
def test_noise_is_added_to_the_base(form: str, event: tuple) -> None:
    t = 5
    store, host = _stores(event)
    idx, start, lengths, frames, live = _case(form, t)
    e = int(torch.Size(event).numel())
    z = ds.feed_noise_reference(KEY, 1, idx, frames.clamp(max=T_FULL - 1), e).reshape(B, t, *event)
    mask = live[:, :, None, None, None].expand_as(z)
    for shift in _shifts(event):
        aug = ds.FeedAugment(shift=shift, bands=4, max_rows=event[1], max_cols=3, per_frame=True)
        inp, tgt, _ = _augmented(store, idx, t, aug, start=start, lengths=lengths, epoch=1, noisy=1, std=1.0)
        base, target = ds.feed_augment_reference(host, idx, frames, AKEY, 1, aug, live=live)
        assert torch.equal(tgt.cpu(), target)
        err = float((inp.cpu().double() - (base.double() + z))[mask].abs().max())
        print(f"{form} {event} shift {shift}: max |input - (base + z_ref)| = {err:.3e}")
        assert err <= TOL
        assert bool((inp.cpu()[~mask] == 0).all())
        assert bool((inp.cpu()[mask] != base[mask]).any())


@pytest.mark.parametrize("event", EVENTS)
@pytest.mark.parametrize("form", FORMS)
def test_no_augmentation_is_the_seeded_entry(form: str, event: tuple) -> None:
    store, _ = _stores(event)
    for t in (4, 5):
        idx, start, lengths, _, _ = _case(form, t)
        got = _augmented(store, idx, t, ds.FeedAugment(), start=start, lengths=lengths, epoch=3, noisy=1, std=0.1)
        want = _seeded(store, idx, t, start=start, lengths=lengths, epoch=3, std=0.1)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert bool((got[0] != got[1]).any())
        if form == "ragged":
            assert torch.equal(got[2], want[2])
        # max_rows / max_cols without bands, and bands of width 0, mask nothing either
        for aug in (ds.FeedAugment(max_rows=event[1], max_cols=3, per_frame=True), ds.FeedAugment(bands=4, per_frame=True)):
            same = _augmented(store, idx, t, aug, start=start, lengths=lengths, epoch=3, noisy=1, std=0.1)
            assert torch.equal(same[0], want[0]) and torch.equal(same[1], want[1])


@pytest.mark.parametrize("per_frame", [False, True])
@pytest.mark.parametrize("event", EVENTS)
def test_output_is_invariant_to_row_batch_size_window_start_and_form(event: tuple, per_frame: bool) -> None:  # noqa: FBT001
    t = 4
    store, _ = _stores(event)
    h = event[1]
    aug = ds.FeedAugment(shift=(2, 3), bands=4, max_rows=h, max_cols=3, per_frame=per_frame)
    kw = {"noisy": 1, "std": 0.1, "epoch": 2}
    idx = torch.tensor([3, 0, 4, 1, 2, 2]).to(DEV)
    start = _i32([0, 2, 5, 1, 4, 3])  # all inside [0, T_full - T]
    lengths = _i32(LENGTHS)
    for form_kw in ({}, {"start": start}, {"start": start, "lengths": lengths}):
        a = _augmented(store, idx, t, aug, **form_kw, **kw)
        again = _augmented(store, idx, t, aug, **form_kw, **kw)
        assert torch.equal(a[0], again[0]) and torch.equal(a[1], again[1])
        perm = torch.tensor([4, 2, 0, 5, 1, 3]).to(DEV)  # another batch row
        pkw = {k: (v[perm].contiguous() if k == "start" else v) for k, v in form_kw.items()}
        p = _augmented(store, idx[perm].contiguous(), t, aug, **pkw, **kw)
        assert torch.equal(p[0], a[0][perm]) and torch.equal(p[1], a[1][perm])
        halves = [_augmented(store, idx[lo: lo + 3].contiguous(), t, aug, **kw,  # another batch size
                             **{k: (v[lo: lo + 3].contiguous() if k == "start" else v) for k, v in form_kw.items()}) for lo in (0, 3)]
        assert torch.equal(torch.cat([x[0] for x in halves]), a[0]) and torch.equal(torch.cat([x[1] for x in halves]), a[1])
    # another window start: the absolute frames both windows hold are the same, masks included
    ep = torch.tensor([2, 2]).to(DEV)
    inp, tgt, _ = _augmented(store, ep, 5, aug, start=_i32([0, 3]), **kw)
    assert torch.equal(inp[0, 3:], inp[1, :2]) and torch.equal(tgt[0, 3:], tgt[1, :2])
    assert not torch.equal(inp[0, :2], inp[1, :2])
    far = _augmented(store, ep, 5, aug, start=_i32([40, -7]), **kw)  # clamped as the windowed form clamps
    edge = _augmented(store, ep, 5, aug, start=_i32([T_FULL - 5, 0]), **kw)
    assert torch.equal(far[0], edge[0]) and torch.equal(far[1], edge[1])
    # first == window at start 0 == the live frames of ragged; dead frames exactly zero, valid_out right
    first = _augmented(store, idx, t, aug, **kw)
    zero = _augmented(store, idx, t, aug, start=_i32([0] * 6), **kw)
    assert torch.equal(first[0], zero[0]) and torch.equal(first[1], zero[1])
    win = _augmented(store, idx, t, aug, start=start, **kw)
    rag = _augmented(store, idx, t, aug, start=start, lengths=lengths, **kw)
    live = (start.cpu()[:, None] + torch.arange(t)) < torch.tensor(LENGTHS)[idx.cpu()][:, None]
    assert 0 < int(live.sum()) < live.numel()
    live = live.to(DEV)
    assert torch.equal(rag[0][live], win[0][live]) and torch.equal(rag[1][live], win[1][live])
    assert bool((rag[0][~live] == 0).all()) and bool((rag[1][~live] == 0).all())
    assert rag[2].tolist() == [min(max(LENGTHS[i] - s, 0), t) for i, s in zip(idx.tolist(), start.tolist(), strict=True)]


@pytest.mark.parametrize("form", FORMS)
def test_epoch_seed_and_stream_change_the_shift_and_masks_change_the_input_only(form: str) -> None:
    t, event = 5, (1, 8, 8)
    store, host = _stores(event)
    idx, start, lengths, frames, live = _case(form, t, idx=(2, 0, 4, 1, 3), raw=(1, -3, 2, 0, 0))
    aug = ds.FeedAugment(shift=(3, 3))
    base = _augmented(store, idx, t, aug, start=start, lengths=lengths)
    others = {"epoch": {"epoch": 1}, "seed": {"akey": ds.augment_key(8, STREAM)}, "seed_high": {"akey": ds.augment_key(SEED + 2 ** 32, STREAM)},
              "stream": {"akey": ds.augment_key(SEED, 2)}}
    for what, kw in others.items():
        other = _augmented(store, idx, t, aug, start=start, lengths=lengths, **kw)
        want = ds.feed_augment_reference(host, idx, frames, kw.get("akey", AKEY), kw.get("epoch", 0), aug, live=live)
        assert torch.equal(other[0].cpu(), want[0]) and torch.equal(other[1].cpu(), want[1]), what
        assert not torch.equal(other[1], base[1]) and not torch.equal(other[0], base[0]), what  # another shift: target AND input move
    # the noise key does not enter the shift; the augmentation key does not enter the noise
    noisy = _augmented(store, idx, t, aug, start=start, lengths=lengths, noisy=1, std=0.1)
    rekeyed = _augmented(store, idx, t, aug, start=start, lengths=lengths, noisy=1, std=0.1, key=ds.stream_key(8, STREAM))
    assert torch.equal(rekeyed[1], noisy[1]) and not torch.equal(rekeyed[0], noisy[0])
    # masks change the input only
    banded = _augmented(store, idx, t, ds.FeedAugment(shift=(3, 3), bands=4, max_rows=8, max_cols=3, per_frame=True), start=start, lengths=lengths)
    assert torch.equal(banded[1], base[1]) and not torch.equal(banded[0], base[0])
    assert torch.equal(base[0], base[1])  # no bands, no noise: the input is the shifted target


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _streams(t: int) -> tuple:
    """Action without noise, audio 1 x 8 x 8 with noise, vision 2 x 4 x 12 without."""
    g = torch.Generator().manual_seed(2)
    return tuple(ds._Stream(torch.randn(N, T_FULL, *e, generator=g).to(DEV), _chain(t, s), _chain(t, None))  # noqa: SLF001
                 for e, s in (((4,), None), ((1, 8, 8), 0.1), ((2, 4, 12), None)))


AUGMENT = {"audio": ds.FeedAugment(shift=(2, 3), bands=2, max_rows=3, max_cols=3, per_frame=True),
           "vision": ds.FeedAugment(shift=(3, 11), bands=1, max_rows=2, max_cols=0, fill=0.0)}


def _same(a: tuple, b: tuple) -> bool:
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b, strict=True))


@pytest.mark.parametrize("lengths", [None, torch.tensor(LENGTHS)])
def test_loader_is_the_same_on_one_and_two_ranks_and_replays(lengths: torch.Tensor | None) -> None:
    t = 4
    streams = _streams(t)
    kw = {"shuffle": True, "seed": 3, "window": "random", "noise_seed": SEED, "lengths": lengths, "augment": AUGMENT}
    one = ds.DeviceEpisodeLoader(streams, 4, **kw)
    ranks = [ds.DeviceEpisodeLoader(streams, 4, rank=r, world=2, **kw) for r in (0, 1)]
    epochs = []
    for epoch in range(2):
        whole = list(one)
        halves = [list(r) for r in ranks]
        assert len(whole) == len(halves[0]) == len(halves[1]) == 2  # 4 rows, then 1 (two ranks: padded to 2 by wrapping)
        for k, batch in enumerate(whole):
            both = tuple(torch.cat([halves[0][k][j], halves[1][k][j]]) for j in range(6))
            rows = batch[0].shape[0]
            assert _same(tuple(batch), tuple(x[:rows] for x in both))
        # the batches are the restatement's: the epoch word is the permutation's epoch
        first = whole[0]
        rows_, start, _, _, _ = next(iter(_schedule(streams, kw, epoch)))
        frames = start.long()[:, None] + torch.arange(t)
        live = None if lengths is None else frames < lengths[rows_.cpu()][:, None]
        for k in (1, 2):
            base, target = ds.feed_augment_reference(streams[k].store.cpu(), rows_, frames.clamp(max=T_FULL - 1), ds.augment_key(SEED, k), epoch,
                                                     AUGMENT[ds.STREAM_NAMES[k]], live=live)
            assert torch.equal(first[3 + k].cpu(), target)
            if k == 2:  # (vision carries no noise: its input is the base itself)
                assert torch.equal(first[k].cpu(), base)
        assert bool((first[1] != first[4]).any()) and torch.equal(first[0], first[3])
        epochs.append(whole)
    assert not any(torch.equal(epochs[0][0][j], epochs[1][0][j]) for j in (1, 2, 4, 5))
    one.set_epoch(0)
    assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(one), epochs[0], strict=True))  # epoch 0 again, bit for bit
    assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(one), epochs[1], strict=True))
    fixed = ds.DeviceEpisodeLoader(streams, 4, noise_epoch="fixed", **kw)  # fixes the augmentation with the noise
    for _ in range(2):
        assert all(_same(tuple(a), tuple(b)) for a, b in zip(list(fixed), epochs[0], strict=True))


def _schedule(streams: tuple, kw: dict, epoch: int):  # noqa: ANN202
    """The schedule of epoch ``epoch`` of a one-rank loader built like the one under test (host side only)."""
    probe = ds.DeviceEpisodeLoader(streams, 4, **kw)
    probe.set_epoch(epoch)
    return probe.schedule_ragged()


@pytest.mark.parametrize("window", ["first", "random"])
def test_loader_without_augment_is_the_seeded_entry_called_directly(window: str) -> None:
    t = 4
    streams = _streams(t)
    loader = ds.DeviceEpisodeLoader(streams, 4, shuffle=True, seed=3, window=window, noise_seed=SEED)
    assert loader.augment == (None, None, None)
    loader.set_epoch(5)
    rows, start, _ = next(iter(loader.schedule()))
    loader.set_epoch(5)
    batch = next(iter(loader))
    dev_start = None if start is None else start.to(DEV)
    inp, tgt, _ = _seeded(streams[1].store, rows, t, start=dev_start, key=ds.stream_key(SEED, 1), epoch=5, std=0.1)
    assert torch.equal(batch[1], inp) and torch.equal(batch[4], tgt)
    frames = (torch.zeros(4, dtype=torch.long) if start is None else start.long())[:, None] + torch.arange(t)
    for k in (0, 2):  # no noise in the chain: input = target = the store's frames
        assert torch.equal(batch[3 + k], streams[k].store[rows[:, None], frames.to(DEV)]) and torch.equal(batch[k], batch[3 + k])


def test_c_entry_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    store, _ = _stores((1, 8, 8))
    idx = torch.tensor([0, 1]).to(DEV)
    out = torch.empty(2, 4, 64, device=DEV)
    start, lengths = _i32([0, 1]), _i32(LENGTHS)
    p, q = _lib.ptr(store), _lib.ptr(out)

    def call(aug=None, *, hw: tuple = (8, 8), src: int = p, dst: int = q, st=_lib.index_ptr(start), ln=None, valid=None, t: int = 4,  # noqa: ANN001, ANN202, PLR0913
             noisy: int = 1, null: bool = False):  # noqa: FBT001, FBT002
        a = None if null else C.byref((aug or ds.FeedAugment(shift=(2, 3), bands=2, max_rows=3, max_cols=3)).c_struct())
        return lib.mtrssm_episode_gather_augmented(a, src, _lib.raw_ptr(idx), st, ln, valid, 1, 2, 3, 4, 5, N, 2, t, T_FULL, 1, *hw, noisy, 0.1,
                                                   dst, None, None)

    def raw(**fields) -> ds.FeedAugment:  # noqa: ANN003
        """A FeedAugment that skipped its own checks: what another caller of the C entry might pass."""
        a = ds.FeedAugment()
        for k, v in fields.items():
            object.__setattr__(a, k, v)
        return a

    for aug, word in ((ds.FeedAugment(shift=(8, 0)), b"shift"), (ds.FeedAugment(shift=(0, 8)), b"shift"), (raw(shift=(-1, 0)), b"shift"),
                      (raw(bands=5), b"bands"), (raw(bands=-1), b"bands"), (ds.FeedAugment(max_rows=9), b"max_rows"),
                      (ds.FeedAugment(max_cols=9), b"max_cols"), (raw(max_rows=-1), b"max_rows"), (raw(fill=float("inf")), b"fill"),
                      (raw(fill=float("nan")), b"fill"), (raw(per_frame=2), b"per_frame")):
        assert call(aug) == -1 and word in lib.mtrssm_last_error(), word
    assert call(hw=(16, 6)) == -1 and b"multiple of 4" in lib.mtrssm_last_error()  # W % 4 != 0
    assert call(hw=(0, 8)) == -1 and b"bad argument" in lib.mtrssm_last_error()
    assert call(null=True) == -1 and b"aug is null" in lib.mtrssm_last_error()
    assert call(noisy=2) == -1 and b"noisy" in lib.mtrssm_last_error()
    assert call(st=None, ln=_lib.index_ptr(lengths)) == -1 and b"lengths without start" in lib.mtrssm_last_error()
    assert call(valid=C.c_void_p(_lib.index_ptr(start))) == -1 and b"valid_out without lengths" in lib.mtrssm_last_error()
    assert call(dst=q + 4) == -1 and b"16-byte aligned" in lib.mtrssm_last_error()
    assert call(src=p + 8) == -1 and b"16-byte aligned" in lib.mtrssm_last_error()
    assert call(st=C.c_void_p(_lib.index_ptr(start) + 2)) == -1 and b"4-byte aligned" in lib.mtrssm_last_error()
    assert call(t=T_FULL + 1) == -1 and b"bad argument" in lib.mtrssm_last_error()
    assert call(src=None) == -1 and b"bad argument" in lib.mtrssm_last_error()
    out.fill_(float("nan"))
    torch.cuda.synchronize()
    assert call(raw(bands=5)) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # nothing was launched
    assert call() == 0  # the same arguments, all in order
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
