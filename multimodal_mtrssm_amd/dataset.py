"""Episode feed with the reference DataModule's surface (``multimodal_rssm/models/dataset.py``,
``models/mrssm/dataset.py``): same config fields, same processed-file layout (``act_*.pt``, ``audio_obs_*.pt``,
``vision_obs_*.pt``), same 80/20 split of the SORTED path lists, same 6-tuple batches
``(action_input, audio_input, vision_input, action_target, audio_target, vision_target)`` of shape ``[B, T, ...]``.

MI355X-first: the reference re-reads and re-transforms every episode file in DataLoader workers each epoch
(``EpisodeDataset.__getitem__``: ``torch.load`` + transform; ``prefetch_factor=1``).  Here ``setup()`` loads the processed
episodes ONCE into HBM (288 GB: a whole dataset is a few GB) as three ``[N, T, E]`` stores, and a batch is one
``mtrssm_episode_gather`` launch per stream (index gather + ``TakeFirstN`` + ``GaussianNoise`` fused, input and target
written in the same pass).  Nothing touches the host per step.  Differences: files are read with
``torch.load(weights_only=True)`` (the reference unpickles); no Google-Drive download (``gdown``): missing data raises
with the reference's hint; the noise comes from the device generator, so the random stream differs (not a parity goal:
``GaussianNoise`` is unseeded in the reference's workers too).

Beyond the reference: the store keeps every episode at full length, and ``window="random"`` /
``"sequential"`` train on windows ``[start, start + T)`` anywhere in it (``mtrssm_episode_gather_window``) -- the latter walks
an episode chunk by chunk for truncated BPTT with a carried state (``carry.StateCarry``).  ``lengths``: the
episodes end at different frames; the store keeps them padded to ``T_full``, a batch row carries ``valid`` live steps and its frames
past them are exactly zero (``mtrssm_episode_gather_ragged``).  ``noise_seed``: the input noise is generated
inside the gather (``mtrssm_episode_gather_seeded``) as a pure function of ``(seed, stream, epoch, episode, absolute frame, element)``,
the same on any number of ranks and replayed by ``set_epoch``; without it the normals come from ``torch.randn`` as before.
``augment``: a seeded integer shift per episode and band masks per frame or episode, made in the same launch
(``mtrssm_episode_gather_augmented``) under the same contract; ``FeedAugment`` holds a stream's parameters.
"""

from __future__ import annotations

import math
from collections.abc import Iterator, Mapping
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.transform import GaussianNoise, TakeFirstN, Transform, fused_chain

WINDOWS = ("first", "random", "sequential")
NOISE_EPOCHS = ("advance", "fixed")
STREAM_NAMES = ("action", "audio", "vision")
_M32 = 0xFFFFFFFF

try:  # Lightning is optional (absent here): the module only needs prepare_data / setup / *_dataloader
    from lightning import LightningDataModule as _Base
except ImportError:  # pragma: no cover - depends on the environment
    class _Base:  # noqa: D101
        def __init__(self) -> None:
            pass


def load_tensor(path: Path) -> Tensor:
    """``.npy`` or ``.pt`` tensor file (``dataset.py:44-64``), read without unpickling arbitrary objects."""
    path = Path(path)
    if path.suffix == ".npy":
        return torch.Tensor(np.load(path))
    if path.suffix == ".pt":
        tensor = torch.load(path, weights_only=True)
        if isinstance(tensor, Tensor):
            return tensor
    msg = f"Unknown file extension: {path.suffix}"
    raise ValueError(msg)


def split_path_list(path_list: list[Path], train_ratio: float) -> tuple[list[Path], list[Path]]:
    """``dataset.py:67-81``."""
    split_point = int(len(path_list) * train_ratio)
    return path_list[:split_point], path_list[split_point:]


def normalize_observation_shape(observations: Tensor) -> Tensor:
    """(N,T,H,W,C) -> (N,T,C,H,W); (N,T,H,W) -> (N,T,1,H,W) (``dataset.py:239-256``)."""
    if observations.dim() == 5:  # noqa: PLR2004
        return observations.permute(0, 1, 4, 2, 3)
    if observations.dim() == 4:  # noqa: PLR2004
        return observations.unsqueeze(2)
    return observations


def _is_int(v: object) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


@dataclass(frozen=True)
class FeedAugment:
    """Seeded augmentation of one stream's frames ``[C, H, W]`` inside the gather: ``shift = (sy, sx)``, the
    largest shift in rows / columns (one draw per episode, uniform on ``[-sy, sy] x [-sx, sx]``); ``bands`` pairs of a row band of
    ``0 .. max_rows`` rows and a column band of ``0 .. max_cols`` columns, redrawn per frame (``per_frame``) or once per episode;
    ``fill``, the value of vacated and masked pixels (-1: the background of data normalised to [-1, 1]).  The target is shifted and
    never masked.  Checked here against nothing but itself; the loader checks it against the stream's ``H`` and ``W``."""

    shift: tuple[int, int] = (0, 0)
    bands: int = 0
    max_rows: int = 0
    max_cols: int = 0
    per_frame: bool = False
    fill: float = -1.0

    def __post_init__(self) -> None:
        shift = tuple(self.shift) if isinstance(self.shift, (tuple, list)) else self.shift
        if not isinstance(shift, tuple) or len(shift) != 2 or not all(_is_int(v) and v >= 0 for v in shift):  # noqa: PLR2004
            msg = f"shift must be two integers (sy, sx) >= 0, got {self.shift!r}"
            raise ValueError(msg)
        object.__setattr__(self, "shift", (int(shift[0]), int(shift[1])))
        if not _is_int(self.bands) or not 0 <= self.bands <= _lib.AUGMENT_MAX_BANDS:
            msg = f"bands must be an integer in [0, {_lib.AUGMENT_MAX_BANDS}], got {self.bands!r}"
            raise ValueError(msg)
        for name in ("max_rows", "max_cols"):
            if not _is_int(getattr(self, name)) or getattr(self, name) < 0:
                msg = f"{name} must be an integer >= 0, got {getattr(self, name)!r}"
                raise ValueError(msg)
        if not isinstance(self.per_frame, bool):
            msg = f"per_frame must be a bool, got {self.per_frame!r}"
            raise ValueError(msg)
        if isinstance(self.fill, bool) or not isinstance(self.fill, (int, float)) or not math.isfinite(self.fill):
            msg = f"fill must be a finite number, got {self.fill!r}"
            raise ValueError(msg)
        object.__setattr__(self, "fill", float(self.fill))

    def check_frame(self, H: int, W: int) -> None:  # noqa: N803
        """Raises ``ValueError`` unless the parameters fit a frame of ``H`` rows and ``W`` columns."""
        sy, sx = self.shift
        if sy >= H or sx >= W:
            msg = f"shift {self.shift} must stay below the frame: sy < H = {H}, sx < W = {W}"
            raise ValueError(msg)
        if self.max_rows > H or self.max_cols > W:
            msg = f"max_rows = {self.max_rows}, max_cols = {self.max_cols} exceed the frame (H = {H}, W = {W})"
            raise ValueError(msg)

    def c_struct(self) -> _lib.FeedAugment:
        return _lib.FeedAugment(*self.shift, self.bands, self.max_rows, self.max_cols, int(self.per_frame), self.fill)


@dataclass
class EpisodeDataModuleConfig:
    """Fields of ``BaseEpisodeDataModuleConfig`` + the multimodal ``EpisodeDataModuleConfig`` (``dataset.py:115-128``,
    ``mrssm/dataset.py:22-34``), plus ``data_root`` (the reference hard-codes ``Path("data")``)."""

    data_name: str
    batch_size: int
    num_workers: int
    gdrive_url: str
    action_preprocess: Transform
    action_input_transform: Transform
    action_target_transform: Transform
    audio_observation_file_name: str
    vision_observation_file_name: str
    audio_observation_preprocess: Transform
    vision_observation_preprocess: Transform
    audio_observation_input_transform: Transform
    audio_observation_target_transform: Transform
    vision_observation_input_transform: Transform
    vision_observation_target_transform: Transform
    data_root: Path = Path("data")
    lengths: Tensor | None = None  # host int tensor [N]: valid frames of each episode of the SORTED file list, 1 .. T_full (None: all)
    noise_seed: int | None = None  # in [0, 2**64): seeded input noise made inside the gather; None: torch.randn
    # {"audio": FeedAugment(...), "vision": FeedAugment(...)} (or the FeedAugment fields as dicts): seeded shift and band masks of the
    # TRAIN loader's frames (needs noise_seed); None: none.  Validation is never augmented.
    augment: Mapping | None = None
    window: str = "first"  # "first" | "random" | "sequential": which T frames of an episode a batch holds (DeviceEpisodeLoader)

    @property
    def data_dir(self) -> Path:
        return Path(self.data_root) / self.data_name

    @property
    def processed_data_dir(self) -> Path:
        return Path(self.data_root) / f"processed_{self.data_name}"

    def get_observation_file_names(self) -> list[str]:
        return [self.audio_observation_file_name, self.vision_observation_file_name]

    @staticmethod
    def get_observation_glob_patterns() -> list[str]:
        return ["audio_obs*", "vision_obs*"]

    def get_effective_processed_data_dir(self, observation_patterns: list[str]) -> Path:
        """``data/processed_data`` when it holds actions and every observation kind, else ``processed_<name>``
        (``dataset.py:140-163``)."""
        common = Path(self.data_root) / "processed_data"
        if common.exists() and list(common.glob("act*")) and all(list(common.glob(p)) for p in observation_patterns):
            return common
        return self.processed_data_dir


class _Stream:
    """One HBM-resident stream ``[N, T, *event]`` + how its input / target are derived."""

    def __init__(self, store: Tensor, input_transform: Transform, target_transform: Transform) -> None:
        self.store = store.contiguous()
        self.event_shape = tuple(store.shape[2:])
        self.event = int(np.prod(self.event_shape)) if self.event_shape else 1
        self.chains = (fused_chain(input_transform), fused_chain(target_transform))
        self.transforms = (input_transform, target_transform)

    @property
    def fused(self) -> bool:
        cin, ctg = self.chains
        return cin is not None and ctg is not None and cin[0] == ctg[0] and ctg[1] is None and self.event % 4 == 0

    @property
    def noisy(self) -> bool:
        """The input chain carries a ``GaussianNoise`` (anywhere in it: an unfused chain too)."""
        chain = getattr(self.transforms[0], "transforms", [self.transforms[0]])
        return any(isinstance(t, GaussianNoise) for t in chain)

    @property
    def steps(self) -> int | None:
        """T of a batch: what the input chain's leading ``TakeFirstN`` says (None: the chain has none)."""
        t_full = int(self.store.shape[1])
        if self.chains[0] is not None:
            n = self.chains[0][0]
            return t_full if n is None else min(int(n), t_full)
        chain = getattr(self.transforms[0], "transforms", [self.transforms[0]])
        n = next((int(t.n) for t in chain if isinstance(t, TakeFirstN)), None)
        return None if n is None else min(n, t_full)

    def batch(self, idx: Tensor, noise: Tensor | None, start: Tensor | None = None, start_host: list[int] | None = None,  # noqa: PLR0913
              lengths: Tensor | None = None, valid_out: Tensor | None = None, lengths_host: Tensor | None = None,
              seeded: tuple[int, int, int] | None = None, augment: tuple | None = None) -> tuple[Tensor, Tensor]:
        """``(input, target)`` for the episodes ``idx``; fused when both chains are the YAML's and E % 4 == 0.  ``start`` (int32
        ``[B]`` on the device, ``start_host`` its host copy): the window ``[start, start + T)`` instead of the first T frames.
        ``lengths`` (int32 ``[N]`` on the device): frames at or past an episode's length are exactly zero, ``valid_out`` (int32
        ``[B]``) receives each row's live steps; ``lengths_host`` is the host copy the unfused path reads.  ``seeded`` = ``(key0, key1,
        epoch)``: a fused stream with noise and no injected ``noise`` generates its normals in the kernel (``feed_noise_reference``).
        ``augment`` = ``(FeedAugment, key0, key1, akey0, akey1, epoch)``: the fused stream's frames are shifted and masked in the
        gather (``feed_augment_reference``), its noise, if its chain has one, is the seeded one; ``noise`` cannot be injected."""
        cin, ctg = self.chains
        n_ep, t_full = self.store.shape[:2]
        if augment is not None and (noise is not None or not self.fused):
            msg = "an augmented stream runs in the gather kernel and makes its own noise: noise= cannot be injected"
            raise ValueError(msg)
        if lengths is not None and start is None:
            msg = "episode lengths need window starts"
            raise ValueError(msg)
        if not self.fused and lengths is not None:
            return self._unfused_ragged(idx, start, start_host, lengths if lengths_host is None else lengths_host, valid_out)
        if not self.fused:  # arbitrary user transforms: applied per episode on the device tensors, then stacked
            if start is None:
                eps = [self.store[i] for i in idx.tolist()]
            else:  # the transforms see the episode from its window's first frame on
                starts = start.tolist() if start_host is None else start_host
                eps = [self.store[i, s:] for i, s in zip(idx.tolist(), starts, strict=True)]
            return (torch.stack([self.transforms[0](e) for e in eps]), torch.stack([self.transforms[1](e) for e in eps]))
        t = t_full if cin[0] is None else min(int(cin[0]), t_full)
        b = idx.numel()
        std = cin[1]
        inp = torch.empty(b, t, *self.event_shape, device=self.store.device, dtype=torch.float32)
        tgt = torch.empty_like(inp)
        if augment is not None:
            if start is not None and tuple(start.shape) != (b,):
                msg = f"start must have shape ({b},), got {tuple(start.shape)}"
                raise ValueError(msg)
            aug, *words = augment
            _lib.check(_lib.TIMERS.call(
                "mtrssm_episode_gather_augmented", _lib.load().mtrssm_episode_gather_augmented, aug.c_struct(), _lib.ptr(self.store),
                _lib.raw_ptr(idx), _lib.index_ptr(start), _lib.index_ptr(lengths), _lib.index_ptr(valid_out), *(int(w) & _M32 for w in words), n_ep,
                b, t, t_full, *self.event_shape, int(std is not None), float(std or 0.0), _lib.ptr(inp), _lib.ptr(tgt),
                _lib.stream_ptr(self.store.device), nbytes=4.0 * b * t * self.event * 3), "mtrssm_episode_gather_augmented")
            return inp, tgt
        if std is not None and noise is None and seeded is not None:
            if start is not None and tuple(start.shape) != (b,):
                msg = f"start must have shape ({b},), got {tuple(start.shape)}"
                raise ValueError(msg)
            _lib.check(_lib.TIMERS.call(
                "mtrssm_episode_gather_seeded", _lib.load().mtrssm_episode_gather_seeded, _lib.ptr(self.store), _lib.raw_ptr(idx),
                _lib.index_ptr(start), _lib.index_ptr(lengths), _lib.index_ptr(valid_out), *(int(w) & _M32 for w in seeded), n_ep, b, t, t_full,
                self.event, float(std), _lib.ptr(inp), _lib.ptr(tgt), _lib.stream_ptr(self.store.device), nbytes=4.0 * b * t * self.event * 3),
                "mtrssm_episode_gather_seeded")
            return inp, tgt
        if std is not None and noise is None:
            noise = torch.randn(b, t, *self.event_shape, device=self.store.device, dtype=torch.float32)
        lib = _lib.load()
        nbytes = 4.0 * b * t * self.event * (4 if std is not None else 3)
        if start is None:
            _lib.check(_lib.TIMERS.call(
                "mtrssm_episode_gather", lib.mtrssm_episode_gather, _lib.ptr(self.store), _lib.raw_ptr(idx), _lib.ptr(noise if std is not None else None),
                n_ep, b, t, t_full, self.event, float(std or 0.0), _lib.ptr(inp), _lib.ptr(tgt), _lib.stream_ptr(self.store.device),
                nbytes=nbytes), "mtrssm_episode_gather")
            return inp, tgt
        if tuple(start.shape) != (b,):
            msg = f"start must have shape ({b},), got {tuple(start.shape)}"
            raise ValueError(msg)
        if lengths is not None:
            _lib.check(_lib.TIMERS.call(
                "mtrssm_episode_gather_ragged", lib.mtrssm_episode_gather_ragged, _lib.ptr(self.store), _lib.raw_ptr(idx), _lib.index_ptr(start),
                _lib.index_ptr(lengths), _lib.ptr(noise if std is not None else None), n_ep, b, t, t_full, self.event, float(std or 0.0),
                _lib.ptr(inp), _lib.ptr(tgt), _lib.index_ptr(valid_out), _lib.stream_ptr(self.store.device), nbytes=nbytes),
                "mtrssm_episode_gather_ragged")
            return inp, tgt
        _lib.check(_lib.TIMERS.call(
            "mtrssm_episode_gather_window", lib.mtrssm_episode_gather_window, _lib.ptr(self.store), _lib.raw_ptr(idx), _lib.index_ptr(start),
            _lib.ptr(noise if std is not None else None), n_ep, b, t, t_full, self.event, float(std or 0.0), _lib.ptr(inp), _lib.ptr(tgt),
            _lib.stream_ptr(self.store.device), nbytes=nbytes), "mtrssm_episode_gather_window")
        return inp, tgt

    def _unfused_ragged(self, idx: Tensor, start: Tensor, start_host: list[int] | None, lengths: Tensor,
                        valid_out: Tensor | None) -> tuple[Tensor, Tensor]:
        """The ragged batch of a stream with arbitrary transforms (or an event size that is no multiple of 4): per episode, as the
        unfused path always works -- the transforms see the window's frames, zero-padded to T, and the dead frames are zeroed again
        after them (a noise transform must not reach them)."""
        t_full = int(self.store.shape[1])
        steps = self.steps or t_full
        starts = start.tolist() if start_host is None else start_host
        lens = lengths.tolist()
        pairs, valid = [], []
        for i, s in zip(idx.tolist(), starts, strict=True):
            s = min(max(int(s), 0), t_full)
            n = min(max(min(max(int(lens[i]), 0), t_full) - s, 0), steps)
            window = self.store[i, s: s + n]
            window = torch.cat([window, window.new_zeros(steps - n, *window.shape[1:])])
            out = [tf(window)[:steps].clone() for tf in self.transforms]
            for o in out:
                o[n:] = 0.0
            pairs.append(out)
            valid.append(n)
        if valid_out is not None:
            valid_out.copy_(torch.tensor(valid, dtype=torch.int32))
        return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def gather_window_reference(store: Tensor, idx: Tensor, start: Tensor, T: int, noise: Tensor | None, std: float | None) -> tuple[Tensor, Tensor]:  # noqa: N803, PLR0913
    """``mtrssm_episode_gather_window`` in torch: ``target[b, t] = store[idx[b], clamp(start[b]) + t]``, ``input = target + noise * std``
    (mul, then add; ``input = target`` without noise).  ``store`` ``[N, T_full, *event]``; returns ``(input, target)``."""
    t_full = store.shape[1]
    s = start.to(torch.long).clamp(0, t_full - T)
    frames = s.unsqueeze(1) + torch.arange(T, device=store.device)
    target = store[idx.to(torch.long).unsqueeze(1), frames]
    if noise is None or std is None:
        return target.clone(), target
    return target + noise * std, target


def gather_ragged_reference(store: Tensor, idx: Tensor, start: Tensor, lengths: Tensor, T: int, noise: Tensor | None,  # noqa: N803, PLR0913
                            std: float | None) -> tuple[Tensor, Tensor, Tensor]:
    """``mtrssm_episode_gather_ragged`` in torch: ``target[b, t] = store[idx[b], start[b] + t]`` where ``start[b] + t < lengths[idx[b]]``,
    else 0; ``input = target + noise * std`` on live frames (mul, then add), 0 on dead ones.  ``start`` is clamped into ``[0, T_full]``,
    ``lengths`` into ``[0, T_full]``.  Returns ``(input, target, valid)``, ``valid`` int32 ``[B]`` = ``clamp(length - start, 0, T)``."""
    t_full = store.shape[1]
    s = start.to(torch.long).clamp(0, t_full)
    ep = idx.to(torch.long)
    n = lengths.to(torch.long).clamp(0, t_full)[ep]
    frames = s.unsqueeze(1) + torch.arange(T, device=store.device)
    live = frames < n.unsqueeze(1)
    picked = store[ep.unsqueeze(1), frames.clamp(max=t_full - 1)]
    shape = (*live.shape, *([1] * (store.dim() - 2)))
    target = torch.where(live.reshape(shape), picked, torch.zeros_like(picked))
    valid = (n - s).clamp(0, T).to(torch.int32)
    if noise is None or std is None:
        return target.clone(), target, valid
    return torch.where(live.reshape(shape), target + noise * std, torch.zeros_like(picked)), target, valid


def philox4x32_10(counter: tuple, key: tuple) -> tuple:
    """Philox4x32 with ten rounds (Salmon et al., SC'11; Random123's ``philox4x32_R(10, ...)``) in exact integers: ``counter`` four and
    ``key`` two 32-bit words, each an int or a numpy integer array (broadcast against each other); returns the four output words as
    ``uint64`` arrays holding 32-bit values.  What ``mtrssm_episode_gather_seeded`` computes per float4."""
    c = [np.asarray(w, dtype=np.uint64) & np.uint64(_M32) for w in counter]
    k = [np.asarray(w, dtype=np.uint64) & np.uint64(_M32) for w in key]
    if len(c) != 4 or len(k) != 2:  # noqa: PLR2004
        msg = f"philox4x32_10 takes a 4-word counter and a 2-word key, got {len(c)} and {len(k)}"
        raise ValueError(msg)
    m0, m1, w0, w1, mask, sh = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, _M32, 32))
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ k[0], p1 & mask, (p0 >> sh) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + w0) & mask, (k[1] + w1) & mask]
    return tuple(c)


def stream_key(seed: int, stream: int) -> tuple[int, int]:
    """The generator key of stream ``stream`` (0, 1, 2 = action, audio, vision) under ``seed`` in ``[0, 2**64)``."""
    return (seed & _M32, ((seed >> 32) & _M32) ^ ((0x9E3779B9 * (stream + 1)) & _M32))


def feed_noise_reference(key: tuple[int, int], epoch: int, episodes: Tensor, frames: Tensor, event: int) -> Tensor:
    """The standard normals of ``mtrssm_episode_gather_seeded`` in float64 from exact integers: ``episodes`` ``[B]`` (the batch's
    ``idx``), ``frames`` ``[B, T]`` (ABSOLUTE frame numbers: clamped start + t), ``event`` = E (a multiple of 4); returns ``[B, T, E]``
    on the host.  Elements ``4 e4 .. 4 e4 + 3`` of a frame come from ``Philox4x32-10((e4, frame, episode & 0xffffffff, epoch), key)``:
    words (0, 1) and (2, 3) each give ``u1 = ((xa >> 8) + 1) 2^-24``, ``u2 = (xb >> 8) 2^-24``, ``r = sqrt(-2 ln u1)``,
    ``r cos(2 pi u2)``, ``r sin(2 pi u2)``."""
    if event % 4:
        msg = f"the event size {event} must be a multiple of 4"
        raise ValueError(msg)
    ep = np.asarray(torch.as_tensor(episodes).cpu(), dtype=np.int64)
    fr = np.asarray(torch.as_tensor(frames).cpu(), dtype=np.int64)
    if fr.shape[:1] != ep.shape or fr.ndim != 2:  # noqa: PLR2004
        msg = f"episodes must be [B] and frames [B, T], got {ep.shape} and {fr.shape}"
        raise ValueError(msg)
    e4 = np.arange(event // 4, dtype=np.int64)[None, None, :]
    x = philox4x32_10((e4, fr[:, :, None] & _M32, ep[:, None, None] & _M32, int(epoch) & _M32), key)
    out = np.empty((*fr.shape, event // 4, 4), dtype=np.float64)
    for pair in (0, 1):
        u1 = ((x[2 * pair] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
        u2 = (x[2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        out[..., 2 * pair] = r * np.cos(2.0 * np.pi * u2)
        out[..., 2 * pair + 1] = r * np.sin(2.0 * np.pi * u2)
    return torch.from_numpy(out.reshape(*fr.shape, event))


def augment_key(seed: int, stream: int) -> tuple[int, int]:
    """The key of stream ``stream``'s augmentation words under ``seed``: ``stream_key(seed, stream + 3)``, apart from the noise keys of
    streams 0, 1, 2."""
    return stream_key(seed, stream + 3)


def _umulhi(a: np.ndarray, n: int | np.ndarray) -> np.ndarray:
    """``(a * n) >> 32`` for 32-bit ``a`` (a ``uint64`` array) and ``n <= 2**32``: the uniform draw on ``[0, n)``, as int64."""
    return ((a * np.asarray(n, dtype=np.uint64)) >> np.uint64(32)).astype(np.int64)


def feed_augment_parameters(key: tuple[int, int], epoch: int, episodes: Tensor, frames: Tensor, aug: FeedAugment, H: int,  # noqa: N803, PLR0913
                            W: int) -> dict[str, np.ndarray]:  # noqa: N803
    """The shift and bands of ``mtrssm_episode_gather_augmented`` in exact integers: ``key`` =
    ``augment_key(seed, stream)``, ``episodes`` ``[B]``, ``frames`` ``[B, T]`` (ABSOLUTE frame numbers), ``H`` x ``W`` the frame.
    Returns int64 arrays: ``dy``, ``dx`` ``[B]`` (one draw per episode: ``Philox((0, 0, episode, epoch))``, ``umulhi(P0, 2 sy + 1) - sy``,
    ``umulhi(P1, 2 sx + 1) - sx``) and ``h``, ``r0``, ``w``, ``c0`` ``[B, T, bands]`` (band j: ``Philox((1 + j, per_frame ? frame + 1 : 0,
    episode, epoch))``, ``umulhi(Q0, max_rows + 1)``, ``umulhi(Q1, H - h + 1)``, ``umulhi(Q2, max_cols + 1)``, ``umulhi(Q3, W - w + 1)``)."""
    aug.check_frame(H, W)
    ep = np.asarray(torch.as_tensor(episodes).cpu(), dtype=np.int64)
    fr = np.asarray(torch.as_tensor(frames).cpu(), dtype=np.int64)
    if fr.shape[:1] != ep.shape or fr.ndim != 2:  # noqa: PLR2004
        msg = f"episodes must be [B] and frames [B, T], got {ep.shape} and {fr.shape}"
        raise ValueError(msg)
    sy, sx = aug.shift
    p = philox4x32_10((0, 0, ep & _M32, int(epoch) & _M32), key)
    out = {"dy": _umulhi(p[0], 2 * sy + 1) - sy, "dx": _umulhi(p[1], 2 * sx + 1) - sx}
    j = np.arange(aug.bands, dtype=np.int64)[None, None, :]
    word1 = ((fr[:, :, None] + 1) & _M32) if aug.per_frame else np.zeros_like(fr[:, :, None])
    q = [np.broadcast_to(x, (*fr.shape, aug.bands)) for x in philox4x32_10((1 + j, word1, ep[:, None, None] & _M32, int(epoch) & _M32), key)]
    out["h"] = _umulhi(q[0], aug.max_rows + 1)
    out["r0"] = _umulhi(q[1], (H - out["h"] + 1).astype(np.uint64))
    out["w"] = _umulhi(q[2], aug.max_cols + 1)
    out["c0"] = _umulhi(q[3], (W - out["w"] + 1).astype(np.uint64))
    return out


def feed_augment_reference(store: Tensor, episodes: Tensor, frames: Tensor, key: tuple[int, int], epoch: int, aug: FeedAugment,  # noqa: PLR0913
                           live: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """``(input_base, target)`` of ``mtrssm_episode_gather_augmented`` on the host, bit for bit: ``store`` ``[N, T_full, C, H, W]``,
    ``episodes`` ``[B]``, ``frames`` ``[B, T]`` absolute frame numbers, ``key`` = ``augment_key(seed, stream)``, ``live`` ``[B, T]``
    bool (None: all; a dead frame is zero in both and its frame number is not read).  ``target[b, t, c, y, x] = store[ep, f, c, y - dy,
    x - dx]`` inside the frame, ``fill`` outside; ``input_base`` = ``fill`` on the masked pixels, ``target`` elsewhere.  The whole input
    of a noisy stream is ``input_base + feed_noise_reference(stream_key(seed, stream), ...) * std`` on the live frames."""
    st = np.asarray(torch.as_tensor(store).cpu(), dtype=np.float32)
    if st.ndim != 5:  # noqa: PLR2004
        msg = f"store must be [N, T_full, C, H, W], got {st.shape}"
        raise ValueError(msg)
    H, W = st.shape[3:]  # noqa: N806
    prm = feed_augment_parameters(key, epoch, episodes, frames, aug, H, W)
    ep = np.asarray(torch.as_tensor(episodes).cpu(), dtype=np.int64)
    fr = np.asarray(torch.as_tensor(frames).cpu(), dtype=np.int64)
    on = np.ones(fr.shape, dtype=bool) if live is None else np.asarray(torch.as_tensor(live).cpu(), dtype=bool)
    fill = np.float32(aug.fill)
    target = np.full((*fr.shape, *st.shape[2:]), fill, dtype=np.float32)
    for b in range(fr.shape[0]):
        dy, dx = int(prm["dy"][b]), int(prm["dx"][b])
        y0, y1, x0, x1 = max(dy, 0), min(H, H + dy), max(dx, 0), min(W, W + dx)  # the output pixels whose source lies inside the frame
        src = st[ep[b], np.where(on[b], fr[b], 0)]
        target[b, :, :, y0:y1, x0:x1] = src[:, :, y0 - dy: y1 - dy, x0 - dx: x1 - dx]
    y, x = np.arange(H)[None, None, None, :], np.arange(W)[None, None, None, :]
    rows = ((prm["r0"][..., None] <= y) & (y < (prm["r0"] + prm["h"])[..., None])).any(axis=2)  # [B, T, H]
    cols = ((prm["c0"][..., None] <= x) & (x < (prm["c0"] + prm["w"])[..., None])).any(axis=2)  # [B, T, W]
    masked = rows[:, :, None, :, None] | cols[:, :, None, None, :]
    base = np.where(masked, fill, target)
    dead = ~on[:, :, None, None, None]
    return torch.from_numpy(np.where(dead, np.float32(0), base)), torch.from_numpy(np.where(dead, np.float32(0), target))


class EpisodeBatch(tuple):
    """The 6-tuple of a windowed batch (``len == 6``, indexing as ever) plus where its windows lie: ``start`` (int32 ``[B]``) and
    ``reset`` (bool ``[B]``, True = the row starts an episode) on the device, ``start_host`` / ``reset_host`` their host copies (the
    loader makes them on the host; ``StateCarry`` checks its rules on ``reset_host`` with no device read-back).

    A loader with episode lengths adds ``valid`` (int32 ``[B]`` on the device: the live steps of each row),
    ``valid_host`` its host copy, ``valid_global`` (int32 ``[B_global]`` on the device: every rank's rows, what the loss is
    normalised by; ``valid`` itself on one rank) and ``row0``, the rank's first row in the global batch."""

    start: Tensor
    reset: Tensor
    start_host: Tensor | None  # (None when the caller handed `DeviceEpisodeLoader.batch` starts that live on the device)
    reset_host: Tensor
    valid: Tensor | None
    valid_host: Tensor | None
    valid_global: Tensor | None
    row0: int

    def __new__(cls, items: tuple[Tensor, ...], start: Tensor, reset: Tensor, start_host: Tensor | None, reset_host: Tensor, *,  # noqa: PYI034, PLR0913
                valid: Tensor | None = None, valid_host: Tensor | None = None, valid_global: Tensor | None = None, row0: int = 0) -> EpisodeBatch:
        self = super().__new__(cls, items)
        self.start, self.reset, self.start_host, self.reset_host = start, reset, start_host, reset_host
        self.valid, self.valid_host, self.row0 = valid, valid_host, int(row0)
        self.valid_global = valid if valid_global is None else valid_global
        return self


class DeviceEpisodeLoader:
    """Iterable of 6-tuple batches over device-resident episodes (what ``train_dataloader`` / ``val_dataloader`` return).

    ``shuffle`` draws a fresh permutation per epoch from a CPU generator seeded ``seed + epoch`` -- the SAME order on every
    data-parallel rank -- and ``rank`` / ``world`` give each rank the contiguous block ``[rank * B / world, (rank + 1) * B / world)``
    of every global batch: exactly the rows ``FlatDataParallel.shard`` cuts and ``GlobalRowNoise.draw`` keys its uniforms by, so
    global row g meets the same noise whatever the number of ranks.  All ranks yield the same number of equally sized batches: a batch whose size
    is not a multiple of ``world`` is padded by wrapping to the head of the epoch's order (``DistributedSampler``'s rule),
    so the per-step all-reduce never waits for a rank that ran out of rows.  With one rank the last batch may be short
    (the reference's DataLoader keeps it too).

    ``noise_seed`` (an int in ``[0, 2**64)``): every stream whose input chain carries a ``GaussianNoise`` takes its
    normals from the generator inside ``mtrssm_episode_gather_seeded``, keyed by ``stream_key(noise_seed, stream)`` and the epoch word --
    a frame's noise depends on ``(seed, stream, epoch, episode, absolute frame, element)`` only, so it is the same on any number of
    ranks, at any batch size and window start, and ``set_epoch(e)`` replays epoch e bitwise.  The epoch word is the value the epoch
    counter had when the epoch's iteration began (the one that seeds the permutation); ``noise_epoch="fixed"`` keeps it 0 and draws
    epoch 0's order and window starts every epoch, so the loader yields the same batches each epoch (validation: losses of two epochs
    are computed on the same inputs).  None (the default): ``torch.randn`` from the device generator, as before.

    ``augment`` (``{"audio": FeedAugment(...), "vision": FeedAugment(...)}``, either key optional; needs
    ``noise_seed``): the named stream's frames are shifted by one seeded draw per episode and masked by seeded row / column bands inside
    the gather (``mtrssm_episode_gather_augmented``), keyed by ``augment_key(noise_seed, stream)`` and the same epoch word as the noise --
    the same invariances, the same replay, fixed by ``noise_epoch="fixed"`` too.  The stream must run in the gather kernel and hold
    ``[C, H, W]`` frames with ``W % 4 == 0``.  A stream that is not named makes exactly the call it made before."""

    def __init__(self, streams: tuple[_Stream, _Stream, _Stream], batch_size: int, *, shuffle: bool, rank: int = 0, world: int = 1,  # noqa: PLR0913
                 seed: int = 0, window: str = "first", lengths: Tensor | None = None, noise_seed: int | None = None,
                 noise_epoch: str = "advance", augment: Mapping | None = None) -> None:
        if window not in WINDOWS:
            msg = f"window must be one of {WINDOWS}, got {window!r}"
            raise ValueError(msg)
        if noise_epoch not in NOISE_EPOCHS:
            msg = f"noise_epoch must be one of {NOISE_EPOCHS}, got {noise_epoch!r}"
            raise ValueError(msg)
        if noise_seed is not None:
            if isinstance(noise_seed, bool) or not isinstance(noise_seed, int) or not 0 <= noise_seed < 2 ** 64:
                msg = f"noise_seed must be an int in [0, 2**64), got {noise_seed!r}"
                raise ValueError(msg)
            for name, s in zip(STREAM_NAMES, streams, strict=True):
                if s.noisy and not s.fused:
                    msg = (f"noise_seed: the {name} stream needs noise but does not run in the gather kernel (its transforms must be "
                           f"[TakeFirstN, GaussianNoise] / [TakeFirstN] and its event size a multiple of 4, got {s.event})")
                    raise ValueError(msg)
        self.noise_seed, self.noise_epoch = noise_seed, noise_epoch
        self.augment = self._checked_augment(augment, streams, noise_seed)  # per stream: a FeedAugment or None
        self.noise_word = 0  # the epoch word of the seeded noise: set where an epoch's iteration begins, and by set_epoch
        self.streams = streams
        self.batch_size = int(batch_size)
        self.shuffle = shuffle
        self.rank, self.world = int(rank), int(world)
        self.seed, self.epoch = int(seed), 0
        self.n = int(streams[0].store.shape[0])
        self.window = window
        self.t_full = int(streams[0].store.shape[1])
        self.steps = self.t_full
        if window != "first":
            steps = {s.steps for s in streams}
            if len(steps) != 1 or None in steps:
                msg = f"window={window!r} needs the same TakeFirstN(n) at the head of every input transform chain (found T = {sorted(map(str, steps))})"
                raise ValueError(msg)
            self.steps = int(steps.pop())
        self.n_chunks = self.t_full // self.steps if window == "sequential" else 1
        self.lengths_host: Tensor | None = None  # int32 [N] on the host; `lengths` the same on the device
        self.lengths: Tensor | None = None
        if lengths is not None:
            if window == "first":
                msg = 'episode lengths need window="random" or "sequential"'
                raise ValueError(msg)
            self.lengths_host = self._checked_lengths(lengths, self.n, self.t_full)
            self.lengths = self.lengths_host.to(streams[0].store.device)
            if window == "sequential":  # every chunk that holds a frame of the longest episode; shorter episodes end earlier
                self.n_chunks = -(-int(self.lengths_host.max()) // self.steps)

    @staticmethod
    def _checked_augment(augment: Mapping | None, streams: tuple[_Stream, ...], noise_seed: int | None) -> tuple[FeedAugment | None, ...]:
        """The loader's ``augment`` mapping as one entry per stream (None: not augmented), checked against the streams."""
        if not augment:
            return (None,) * len(streams)
        if not isinstance(augment, Mapping):
            msg = f"augment must map stream names to FeedAugment, got {type(augment).__name__}"
            raise ValueError(msg)  # noqa: TRY004
        for name in augment:
            if name == "action" or name not in STREAM_NAMES:
                msg = f"augment: {name!r} cannot be augmented (only the image streams {STREAM_NAMES[1:]} hold frames)"
                raise ValueError(msg)
        if noise_seed is None:
            msg = f"augment: the augmentation of {sorted(augment)} is seeded: it needs noise_seed"
            raise ValueError(msg)
        out: list[FeedAugment | None] = []
        for name, s in zip(STREAM_NAMES, streams, strict=True):
            aug = augment.get(name)
            if isinstance(aug, Mapping):  # (a config file's plain keys)
                aug = FeedAugment(**aug)
            if aug is not None and not isinstance(aug, FeedAugment):
                msg = f"augment: the {name} entry must be a FeedAugment, got {type(aug).__name__}"
                raise ValueError(msg)  # noqa: TRY004
            if aug is not None:
                if not s.fused:
                    msg = (f"augment: the {name} stream does not run in the gather kernel (its transforms must be [TakeFirstN, GaussianNoise] "
                           f"/ [TakeFirstN] and its event size a multiple of 4, got {s.event})")
                    raise ValueError(msg)
                if len(s.event_shape) != 3 or s.event_shape[2] % 4:  # noqa: PLR2004
                    msg = f"augment: the {name} stream's frames must be [C, H, W] with W % 4 == 0, got {list(s.event_shape)}"
                    raise ValueError(msg)
                try:
                    aug.check_frame(*s.event_shape[1:])
                except ValueError as err:
                    msg = f"augment: the {name} stream: {err}"
                    raise ValueError(msg) from None
            out.append(aug)
        return tuple(out)

    @staticmethod
    def _checked_lengths(lengths: Tensor, n: int, t_full: int) -> Tensor:
        if not isinstance(lengths, Tensor) or lengths.is_cuda or lengths.is_floating_point() or lengths.dtype == torch.bool:
            msg = f"lengths must be a host integer tensor, got {getattr(lengths, 'dtype', type(lengths))}"
            raise ValueError(msg)
        if tuple(lengths.shape) != (n,):
            msg = f"lengths must have shape ({n},), one entry per episode, got {tuple(lengths.shape)}"
            raise ValueError(msg)
        if n and (int(lengths.min()) < 1 or int(lengths.max()) > t_full):
            msg = f"lengths must lie in [1, {t_full}] (T_full), got min {int(lengths.min())}, max {int(lengths.max())}"
            raise ValueError(msg)
        return lengths.to(torch.int32).contiguous()

    def __len__(self) -> int:
        return (self.n + self.batch_size - 1) // self.batch_size * self.n_chunks

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)
        self.noise_word = self.epoch if self.noise_epoch == "advance" else 0

    def _seeded(self) -> list[tuple[int, int, int] | None]:
        """Per stream: ``(key0, key1, epoch word)`` of its seeded noise, None for a stream without noise or a loader without seed."""
        if self.noise_seed is None:
            return [None] * len(self.streams)
        return [(*stream_key(self.noise_seed, k), self.noise_word & _M32) if s.noisy else None for k, s in enumerate(self.streams)]

    def _batch_keywords(self, noise: tuple) -> list[dict]:
        """Per stream: the ``seeded`` / ``augment`` keywords of ``_Stream.batch``.  An augmented stream gets ``augment`` = ``(FeedAugment,
        noise key, augmentation key, epoch word)``; every other stream exactly what it got before there was augmentation."""
        out = []
        for k, (name, sd, aug, n) in enumerate(zip(STREAM_NAMES, self._seeded(), self.augment, noise, strict=True)):
            if aug is None:
                out.append({"seeded": sd})
                continue
            if n is not None:
                msg = f"the {name} stream is augmented in the gather kernel, which makes its noise: noise= cannot be injected for it"
                raise ValueError(msg)
            out.append({"augment": (aug, *stream_key(self.noise_seed, k), *augment_key(self.noise_seed, k), self.noise_word & _M32)})
        return out

    def batch(self, idx: Tensor, noise: tuple[Tensor | None, Tensor | None, Tensor | None] = (None, None, None),  # noqa: PLR0913
              start: Tensor | None = None, reset: Tensor | None = None, *, valid_host: Tensor | None = None,
              valid_global: Tensor | None = None, row0: int = 0) -> tuple[Tensor, ...]:
        """The 6-tuple for episode indices ``idx`` (int64, on the device); ``noise`` injects the standard normals (and takes precedence
        over a ``noise_seed``, whose epoch word is that of the epoch being iterated, or of the last ``set_epoch``).  ``start``: the
        windows' first frames, one per row -- a HOST integer tensor (validated here: ``0 <= start <= T_full - T``) or an int32
        device tensor (not read back: the kernel clamps it into that range); the result is then an ``EpisodeBatch``, ``reset``
        (a host bool tensor, default all True) riding along.

        A loader with lengths: a host ``start`` may reach ``T_full`` (a chunk may hang over the end of the store), the batch's
        ``valid`` comes from the gather kernel, and ``valid_host`` / ``valid_global`` (host int32 ``[B]`` / ``[B_global]``, made by
        ``schedule_ragged``) and ``row0`` ride along."""
        if start is None and self.lengths is not None:
            msg = "a loader with lengths needs start= (the windows' first frames)"
            raise ValueError(msg)
        keywords = self._batch_keywords(noise)
        if start is None:
            pairs = [s.batch(idx, n, **kw) for s, n, kw in zip(self.streams, noise, keywords, strict=True)]
            return (pairs[0][0], pairs[1][0], pairs[2][0], pairs[0][1], pairs[1][1], pairs[2][1])
        dev = self.streams[0].store.device
        start_host = None
        if not start.is_cuda:
            start_host = start.to(torch.int32)
            top = self.t_full - self.steps if self.lengths is None else self.t_full
            if start_host.numel() and (int(start_host.min()) < 0 or int(start_host.max()) > top):
                msg = f"start must lie in [0, {top}] (T_full = {self.t_full}, T = {self.steps}), got {start_host.tolist()}"
                raise ValueError(msg)
            start = start_host.to(dev)
        reset_host = torch.ones(idx.numel(), dtype=torch.bool) if reset is None else reset.to("cpu", torch.bool)
        hosts = None if start_host is None else start_host.tolist()
        if self.lengths is None:
            pairs = [s.batch(idx, n, start.contiguous(), hosts, **kw) for s, n, kw in zip(self.streams, noise, keywords, strict=True)]
            items = (pairs[0][0], pairs[1][0], pairs[2][0], pairs[0][1], pairs[1][1], pairs[2][1])
            return EpisodeBatch(items, start, reset_host.to(dev), start_host, reset_host)
        valid = torch.empty(idx.numel(), dtype=torch.int32, device=dev)
        # written by ONE launch: the first stream the gather kernel takes (a batch of unfused streams only: by the per-episode path)
        writer = next((k for k, s in enumerate(self.streams) if s.fused), 0)
        pairs = [s.batch(idx, n, start.contiguous(), hosts, self.lengths, valid if k == writer else None, self.lengths_host, **kw)
                 for k, (s, n, kw) in enumerate(zip(self.streams, noise, keywords, strict=True))]
        items = (pairs[0][0], pairs[1][0], pairs[2][0], pairs[0][1], pairs[1][1], pairs[2][1])
        vg = None if valid_global is None else valid_global.to(dev, torch.int32)
        return EpisodeBatch(items, start, reset_host.to(dev), start_host, reset_host, valid=valid,
                            valid_host=None if valid_host is None else valid_host.to("cpu", torch.int32), valid_global=vg, row0=row0)

    def _global_batches(self) -> Iterator[tuple[Tensor, Tensor | None, Tensor | None, int]]:
        """Per global batch of the current epoch: this rank's episode indices (on the device), for ``window="random"`` this rank's
        window starts (host int32), with lengths the episode lengths of ALL the global batch's rows (host int32, padding rows
        included), and the rank's first global row -- all cut from per-GLOBAL-row quantities, so global row g is the same episode and
        window on any number of ranks.  Advances the epoch counter."""
        dev = self.streams[0].store.device
        # (a fixed loader draws epoch 0's order and windows every epoch: with its epoch word 0 it yields the same batches each time)
        g = torch.Generator().manual_seed(self.seed + (self.epoch if self.noise_epoch == "advance" else 0))
        order = torch.randperm(self.n, generator=g) if self.shuffle else torch.arange(self.n)
        lens = None if self.lengths_host is None else self.lengths_host[order]  # per position of the epoch's order
        starts = None
        if self.window == "random":  # one start per position of the epoch's order, drawn after the permutation
            starts = torch.randint(0, self.t_full - self.steps + 1, (self.n,), generator=g).to(torch.int32)
            if lens is not None:
                # uniform on [0, max(len - T, 0)] per row: a full-length episode keeps the draw above (all lengths T_full give the
                # starts of a loader without lengths); a shorter one scales a second uniform, drawn AFTER it from the same generator
                # (a modulo of the first draw would favour the low starts wherever the ranges do not divide)
                room = (lens - self.steps).clamp(min=0).to(torch.int64) + 1
                second = (torch.rand(self.n, generator=g, dtype=torch.float64) * room).to(torch.int64).clamp(max=room - 1)
                starts = torch.where(room == self.t_full - self.steps + 1, starts.to(torch.int64), second).to(torch.int32)
        order = order.to(dev)
        self.noise_word = self.epoch if self.noise_epoch == "advance" else 0  # the epoch that seeded the permutation above
        self.epoch += 1
        for lo in range(0, self.n, self.batch_size):
            rows = order[lo: lo + self.batch_size]
            st = None if starts is None else starts[lo: lo + self.batch_size]
            ln = None if lens is None else lens[lo: lo + self.batch_size]
            row0 = 0
            if self.world > 1:
                pad = (-rows.numel()) % self.world
                if pad:
                    wrap = torch.arange(pad) % self.n
                    rows = torch.cat([rows, order[wrap.to(dev)]])
                    st = None if st is None else torch.cat([st, starts[wrap]])
                    ln = None if ln is None else torch.cat([ln, lens[wrap]])
                per = rows.numel() // self.world  # the CONTIGUOUS block FlatDataParallel.shard / GlobalRowNoise.draw give this rank
                row0 = self.rank * per
                rows = rows[row0: row0 + per]
                st = None if st is None else st[row0: row0 + per]
            yield rows.contiguous(), st, ln, row0

    def schedule(self) -> Iterator[tuple[Tensor, Tensor | None, Tensor | None]]:
        """``(episode indices, start, reset)`` of this rank, batch by batch, for the current epoch; ``start`` (int32) and ``reset``
        (bool) are HOST tensors, None in ``"first"`` mode.  ``"sequential"``: a group of episodes comes ``n_chunks`` times in a row,
        chunk c at ``start = c * T``, ``reset`` on chunk 0."""
        for rows, start, reset, _, _ in self.schedule_ragged():
            yield rows, start, reset

    def schedule_ragged(self) -> Iterator[tuple[Tensor, Tensor | None, Tensor | None, Tensor | None, int]]:
        """``schedule`` plus, for a loader with lengths, ``valid_global`` (host int32 ``[B_global]``: the live steps
        ``clamp(len - start, 0, T)`` of every rank's rows, None without lengths) and ``row0``, this rank's first global row: its own
        ``valid`` is ``valid_global[row0 : row0 + B]``.  ``"sequential"``: ``n_chunks = ceil(max(len) / T)``, a row whose episode is
        over has ``valid = 0``."""
        for rows, st, ln, row0 in self._global_batches():
            b = rows.numel()
            if self.window == "first":
                yield rows, None, None, None, row0
            elif self.window == "random":
                valid = None
                if ln is not None:  # (st is this rank's cut; the global rows' starts are recomputed from the same per-row rule)
                    valid = ln.clamp(max=self.steps).to(torch.int32)  # start <= len - T when len >= T, else 0: min(len, T) live steps
                yield rows, st, torch.ones(b, dtype=torch.bool), valid, row0
            else:
                for c in range(self.n_chunks):
                    valid = None if ln is None else (ln - c * self.steps).clamp(0, self.steps).to(torch.int32)
                    yield rows, torch.full((b,), c * self.steps, dtype=torch.int32), torch.full((b,), c == 0, dtype=torch.bool), valid, row0

    def index_batches(self) -> Iterator[Tensor]:
        """This rank's episode indices, batch by batch, for the current epoch (then the epoch counter advances)."""
        for rows, _, _ in self.schedule():
            yield rows

    def __iter__(self) -> Iterator[tuple[Tensor, ...]]:
        return self.batches(0)

    def batches(self, skip: int = 0) -> Iterator[tuple[Tensor, ...]]:
        """The current epoch's batches from entry ``skip`` of its schedule on: the first ``skip`` entries are walked on the host and
        nothing of them is gathered (a run resumed mid-epoch, ``fit.Trainer``).  ``batches(0)`` is ``__iter__``."""
        if isinstance(skip, bool) or not isinstance(skip, int) or skip < 0:
            msg = f"skip must be an integer >= 0, got {skip!r}"
            raise ValueError(msg)
        for k, (rows, start, reset, valid_global, row0) in enumerate(self.schedule_ragged()):
            if k < skip:
                continue
            if start is None:
                yield self.batch(rows)
            elif valid_global is None:
                yield self.batch(rows, start=start, reset=reset)
            else:
                # (one rank: the gather's `valid` IS the global batch's, no copy of the host's to the device)
                yield self.batch(rows, start=start, reset=reset, valid_host=valid_global[row0: row0 + rows.numel()],
                                 valid_global=valid_global if self.world > 1 else None, row0=row0)


class EpisodeDataModule(_Base):
    """``multimodal_rssm.models.mrssm.dataset.EpisodeDataModule`` over an HBM-resident episode store."""

    def __init__(self, config: EpisodeDataModuleConfig, device: str | torch.device = "cuda", rank: int = 0, world: int = 1) -> None:
        super().__init__()
        self.config = config
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        self.train_streams: tuple[_Stream, _Stream, _Stream] | None = None
        self.val_streams: tuple[_Stream, _Stream, _Stream] | None = None

    # ---- prepare_data: raw arrays -> processed per-episode files (mrssm/dataset.py:62-153)
    def _find_data_paths(self) -> tuple[Path, Path, Path, bool]:
        c = self.config
        root = Path(c.data_root)
        cand = [(root / c.audio_observation_file_name, root / c.vision_observation_file_name, root / "joint_states.npy"),
                (c.data_dir / c.audio_observation_file_name, c.data_dir / c.vision_observation_file_name, c.data_dir / "joint_states.npy")]
        for a, v, j in cand:
            if a.is_file() and v.is_file() and j.is_file():
                return a, v, j, True
        return (*cand[1], False)

    def _is_processed_data_ready(self) -> bool:
        d = self.config.get_effective_processed_data_dir(self.config.get_observation_glob_patterns())
        return d.exists() and all(bool(list(d.glob(p))) for p in ("act*", "audio_obs*", "vision_obs*"))

    def prepare_data(self) -> None:
        """Writes the processed per-episode files unless they exist (``dataset.py:281-341``).  No download."""
        if self._is_processed_data_ready():
            return
        c = self.config
        audio_path, vision_path, act_path, has_local = self._find_data_paths()
        if not has_local and not c.data_dir.exists():
            msg = (f"no data for {c.data_name!r}: place {', '.join(c.get_observation_file_names())} and joint_states.npy in "
                   f"{c.data_dir}, or processed act_* / audio_obs_* / vision_obs_* files in {c.processed_data_dir} "
                   "(this build does not download from Google Drive)")
            raise FileNotFoundError(msg)
        c.processed_data_dir.mkdir(parents=True, exist_ok=True)
        if has_local:
            audio = normalize_observation_shape(load_tensor(audio_path))
            vision = normalize_observation_shape(load_tensor(vision_path))
            actions = load_tensor(act_path)
            for i in range(audio.shape[0]):
                torch.save(c.action_preprocess(actions[i]).detach().clone(), c.processed_data_dir / f"act_{i:03d}.pt")
                torch.save(c.audio_observation_preprocess(audio[i]).detach().clone(), c.processed_data_dir / f"audio_obs_{i:03d}.pt")
                torch.save(c.vision_observation_preprocess(vision[i]).detach().clone(), c.processed_data_dir / f"vision_obs_{i:03d}.pt")
            return
        for pattern, pre in (("act*", c.action_preprocess), ("audio_obs*", c.audio_observation_preprocess),
                             ("vision_obs*", c.vision_observation_preprocess)):
            for path in sorted(c.data_dir.glob(pattern)):
                torch.save(pre(load_tensor(path)).detach().clone(), c.processed_data_dir / f"{path.stem}.pt")

    # ---- setup: processed files -> HBM stores, 80/20 split of the sorted lists (mrssm/dataset.py:155-183)
    def _stack(self, paths: list[Path]) -> Tensor:
        eps = [load_tensor(p).to(torch.float32) for p in paths]
        t = min(e.shape[0] for e in eps)  # ragged episode lengths: the common prefix (TakeFirstN cuts further)
        return torch.stack([e[:t] for e in eps]).to(self.device)

    def _stack_padded(self, lists: list[list[Path]], lengths: Tensor) -> list[Tensor]:
        """With ``config.lengths``: the three stores of one side of the split, every episode zero-padded to the side's longest file
        (each file is read once).  Checked file by file: the three streams of an episode hold the same number of frames, and its
        length does not claim more of them (a larger length would turn padding zeros into live frames)."""
        eps = [[load_tensor(p).to(torch.float32) for p in paths] for paths in lists]
        for i, trio in enumerate(zip(*eps, strict=True)):
            frames = sorted({int(e.shape[0]) for e in trio})
            if len(frames) != 1:
                msg = f"{lists[0][i].name}: the action, audio and vision files of this episode hold {frames} frames, not the same number"
                raise ValueError(msg)
            if not 1 <= int(lengths[i]) <= frames[0]:
                msg = f"config.lengths gives {lists[0][i].name} {int(lengths[i])} frames, but the file holds {frames[0]} (need 1 .. {frames[0]})"
                raise ValueError(msg)
        t = max(int(e.shape[0]) for e in eps[0])
        return [torch.stack([torch.cat([e, e.new_zeros(t - e.shape[0], *e.shape[1:])]) for e in stream]).to(self.device) for stream in eps]

    def _lengths(self, train: bool) -> Tensor | None:  # noqa: FBT001
        """The configured lengths of one side of the split: cut by the function that cuts the sorted path lists (None: none configured)."""
        if self.config.lengths is None:
            return None
        return split_path_list(self.config.lengths, 0.8)[0 if train else 1]

    def setup(self, stage: str = "fit") -> None:
        c = self.config
        d = c.get_effective_processed_data_dir(c.get_observation_glob_patterns())
        lists = [sorted(d.glob(p)) for p in ("act*", "audio_obs*", "vision_obs*")]
        if not all(lists) or len({len(x) for x in lists}) != 1:
            msg = f"{d}: need the same number (> 0) of act*, audio_obs* and vision_obs* files, found {[len(x) for x in lists]}"
            raise FileNotFoundError(msg)
        lens = c.lengths
        if lens is not None and (not isinstance(lens, Tensor) or lens.is_floating_point() or tuple(lens.shape) != (len(lists[0]),)):
            msg = (f"config.lengths must be a host integer tensor of shape ({len(lists[0])},), one entry per episode file, "
                   f"got {getattr(lens, 'shape', type(lens))}")
            raise ValueError(msg)
        splits = [split_path_list(x, 0.8) for x in lists]
        tr = ((c.action_input_transform, c.action_target_transform), (c.audio_observation_input_transform, c.audio_observation_target_transform),
              (c.vision_observation_input_transform, c.vision_observation_target_transform))

        def streams(side: int) -> tuple[_Stream, _Stream, _Stream]:
            paths = [s[side] for s in splits]
            stores = [self._stack(p) for p in paths] if lens is None else self._stack_padded(paths, self._lengths(side == 0))
            return tuple(_Stream(store, *t) for store, t in zip(stores, tr, strict=True))

        if stage == "fit" and splits[0][0]:
            self.train_streams = streams(0)
        if splits[0][1]:
            self.val_streams = streams(1)

    def train_dataloader(self) -> DeviceEpisodeLoader:
        if self.train_streams is None:
            msg = "train_dataset is not set. Call setup() first."
            raise RuntimeError(msg)
        return DeviceEpisodeLoader(self.train_streams, self.config.batch_size, shuffle=True, rank=self.rank, world=self.world,
                                   window=self.config.window, lengths=self._lengths(True), noise_seed=self.config.noise_seed,
                                   augment=self.config.augment)  # (the train loader only: validation inputs stay fixed and whole)

    def val_dataloader(self) -> DeviceEpisodeLoader:
        if self.val_streams is None:
            msg = "val_dataset is not set. Call setup() first."
            raise RuntimeError(msg)
        return DeviceEpisodeLoader(self.val_streams, self.config.batch_size, shuffle=False, rank=self.rank, world=self.world,
                                   window=self.config.window, lengths=self._lengths(False), noise_seed=self.config.noise_seed,
                                   noise_epoch="advance" if self.config.noise_seed is None else "fixed")
