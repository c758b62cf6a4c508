"""GPU (MI355X): ``mtrssm_episode_gather_window`` against its torch restatement and against ``mtrssm_episode_gather``, bit for
bit, and the windowed loader end to end."""

from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(Path(__file__).parent / "golden" / "data_feed.npz")


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _golden_stores() -> list[torch.Tensor]:
    return [torch.from_numpy(GOLDEN[f"ep/{k}"]) for k in ("act", "audio_obs", "vision_obs")]


def _bench_stores() -> list[torch.Tensor]:
    g = torch.Generator().manual_seed(6)
    n, t_full = 24, 30
    return [torch.randn(n, t_full, 4, generator=g), torch.randn(n, t_full, 1, 128, 32, generator=g), torch.randn(n, t_full, 1, 64, 64, generator=g)]


@pytest.mark.parametrize(("which", "t", "batch"), [("golden", 6, 5), ("golden", 9, 3), ("golden", 1, 7), ("bench", 10, 16), ("bench", 30, 4)])
def test_window_gather_equals_its_restatement_bit_for_bit(which: str, t: int, batch: int) -> None:
    stores = _golden_stores() if which == "golden" else _bench_stores()
    n, t_full = stores[0].shape[:2]
    g = torch.Generator().manual_seed(17)
    idx = torch.randint(0, n, (batch,), generator=g)
    start = torch.randint(0, t_full - t + 1, (batch,), generator=g).to(torch.int32)
    start[0] = 0
    start[-1] = t_full - t  # both ends of the range are among the starts
    for store in stores:
        noise = torch.randn(batch, t, *store.shape[2:], generator=g)
        for std in (0.1, None):
            stream = ds._Stream(store.to(DEV), _chain(t, std), _chain(t, None))  # noqa: SLF001
            assert stream.fused
            inp, tgt = stream.batch(idx.to(DEV), noise.to(DEV) if std is not None else None, start.to(DEV))
            want_i, want_t = ds.gather_window_reference(store, idx, start, t, noise if std is not None else None, std)
            assert torch.equal(tgt.cpu(), want_t) and torch.equal(inp.cpu(), want_i), (which, tuple(store.shape), std)
            # every start 0: the first-T kernel's result, bit for bit
            zero = torch.zeros(batch, dtype=torch.int32, device=DEV)
            a = stream.batch(idx.to(DEV), noise.to(DEV) if std is not None else None, zero)
            b = stream.batch(idx.to(DEV), noise.to(DEV) if std is not None else None)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        # starts nobody validated (made on the device) are clamped into [0, T_full - T] by the kernel, as the restatement says
        wild = torch.tensor([-7, t_full, 2 ** 30][:batch] + [0] * max(0, batch - 3), dtype=torch.int32)
        stream = ds._Stream(store.to(DEV), _chain(t, None), _chain(t, None))  # noqa: SLF001
        _, tgt = stream.batch(idx.to(DEV), None, wild.to(DEV))
        assert torch.equal(tgt.cpu(), ds.gather_window_reference(store, idx, wild, t, None, None)[1])


def test_windowed_loader_yields_episode_batches() -> None:
    stores = _bench_stores()
    n, t_full, t, bs = stores[0].shape[0], stores[0].shape[1], 10, 8
    streams = tuple(ds._Stream(s.to(DEV), _chain(t, 0.1), _chain(t, None)) for s in stores)  # noqa: SLF001
    first = next(iter(ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=1)))
    assert type(first) is tuple and len(first) == 6
    seq = ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=1, window="sequential")
    sched = list(seq.schedule())
    seq.set_epoch(0)
    batches = list(seq)
    assert len(batches) == len(seq) == (n // bs) * (t_full // t)
    for (rows, start, reset), b in zip(sched, batches, strict=True):
        assert isinstance(b, ds.EpisodeBatch) and len(b) == 6
        assert b.start.dtype == torch.int32 and b.start.is_cuda and torch.equal(b.start.cpu(), start)
        assert b.reset.dtype == torch.bool and b.reset.is_cuda and torch.equal(b.reset.cpu(), reset) and torch.equal(b.reset_host, reset)
        for k in range(3):
            want = ds.gather_window_reference(stores[k], rows.cpu(), start, t, None, None)[1]
            assert torch.equal(b[3 + k].cpu(), want)
            assert 0.05 < float((b[k] - b[3 + k]).std()) < 0.2  # device-drawn noise of std 0.1
    rnd = ds.DeviceEpisodeLoader(streams, bs, shuffle=True, seed=1, window="random")
    sched = list(rnd.schedule())
    rnd.set_epoch(0)
    for (rows, start, _), b in zip(sched, rnd, strict=True):
        assert bool(b.reset.all()) and torch.equal(b.start_host, start)
        assert torch.equal(b[5].cpu(), ds.gather_window_reference(stores[2], rows.cpu(), start, t, None, None)[1])
    # a chain the fused kernel does not implement gets the episode from its window's first frame on
    odd_store = torch.randn(6, 12, 7, generator=torch.Generator().manual_seed(3))
    odd = ds._Stream(odd_store.to(DEV), _chain(5, None), _chain(5, None))  # noqa: SLF001
    assert not odd.fused
    idx, start = torch.tensor([4, 0]), torch.tensor([7, 2], dtype=torch.int32)
    i, tgt = odd.batch(idx.to(DEV), None, start.to(DEV), start.tolist())
    assert torch.equal(tgt.cpu(), ds.gather_window_reference(odd_store, idx, start, 5, None, None)[1]) and torch.equal(i, tgt)
