"""Modality dropout: a seeded, device-side sampler of modality masks for training.

The rule (``ModalityDropout.reference`` is its restatement in torch, ``mtrssm_modality_dropout`` the kernel): with uniforms
``u`` of shape ``[B_global, S, 2]``, ``S = ceil(T / span)``, modality ``m`` (0 audio, 1 vision) is present at ``(b, t)`` iff
``u[b, t // span, m] >= p_m``.  At ``t = 0`` only, a row with neither present gets the one with the larger ``u`` (tie: audio),
so the initial state always has an embedding; later steps may have none (the scans then take posterior = prior).  Every
comparison is an fp32 compare, so kernel and restatement give identical masks.

One launch writes what a masked ``shared_step`` reads -- the scans' codes, the masked NLL's ``present`` planes, the t = 0
mask -- for a rank's rows, and the present-frame counts of the GLOBAL batch as device scalars.  Nothing is read back to the
host, so the sampler can sit inside a captured hipGraph (``graph.CapturedTrainStep(modality_dropout=...)``).
"""

from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import NamedTuple

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib


@dataclass
class StepMask:
    """What one masked train step reads, all on the device: ``codes`` int32 ``[B, T]`` (bit 0 audio, bit 1 vision),
    ``present_audio`` / ``present_vision`` float32 ``[B * T]`` in {0, 1}, ``mask0`` bool ``[B, 2]`` (the t = 0 frame),
    ``count_audio`` / ``count_vision`` float32 scalars: what each reconstruction sum is divided by.  A ragged batch's record
    (``ragged_step_mask``) also carries ``live`` float32 ``[B * T]`` in {0, 1}, ``count_live`` (what the KL sums
    are divided by) and ``last`` int32 ``[B]`` (the last live step, -1 for an empty row: where the carry is saved from)."""

    codes: Tensor
    present_audio: Tensor
    present_vision: Tensor
    mask0: Tensor
    count_audio: Tensor
    count_vision: Tensor
    live: Tensor | None = None
    count_live: Tensor | None = None
    last: Tensor | None = None

    @classmethod
    def from_mask(cls, mask: Tensor) -> StepMask:
        """The record of a caller-supplied bool ``[B, T, 2]`` mask: each count is the number of present frames in ``mask``
        itself (a data-parallel rank's own rows)."""
        pa = mask[..., 0].reshape(-1).to(torch.float32)
        pv = mask[..., 1].reshape(-1).to(torch.float32)
        codes = (mask[..., 0].to(torch.int32) + 2 * mask[..., 1].to(torch.int32)).contiguous()
        return cls(codes, pa, pv, mask[:, 0], pa.sum(), pv.sum())


@dataclass
class DropoutSample:
    """``ModalityDropout.sample``'s result for one rank: the masks of its rows and ``counts`` (float32 ``[2]``: present audio
    and vision frames of the GLOBAL batch)."""

    codes: Tensor
    present_audio: Tensor
    present_vision: Tensor
    mask0: Tensor
    counts: Tensor
    world: int = 1

    @property
    def mask(self) -> Tensor:
        """The bool ``[B, T, 2]`` mask these codes stand for."""
        return torch.stack([(self.codes & 1) != 0, (self.codes & 2) != 0], dim=-1)

    def step_mask(self) -> StepMask:
        """Data-parallel exact normalisation: each rank divides its local sums by ``global count / world``, so the mean over
        ranks is the global masked mean and the all-reduced gradient scaled by ``1 / world`` is the global batch's."""
        norm = self.counts if self.world == 1 else self.counts / float(self.world)
        return StepMask(self.codes, self.present_audio, self.present_vision, self.mask0, norm[0], norm[1])


class ModalityDropout:
    """Drops audio with probability ``p_audio`` and vision with ``p_vision``, independently per batch row and per block of
    ``span`` consecutive steps.  ``world`` / ``rank`` (``for_rank``) say which rows of the global batch a rank trains on."""

    def __init__(self, p_audio: float, p_vision: float, span: int = 1) -> None:
        for name, p in (("p_audio", p_audio), ("p_vision", p_vision)):
            if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= float(p) < 1.0:
                msg = f"{name} must be a probability in [0, 1), got {p!r}"
                raise ValueError(msg)
        if isinstance(span, bool) or not isinstance(span, int) or span < 1:
            msg = f"span must be an integer >= 1, got {span!r}"
            raise ValueError(msg)
        self.p_audio, self.p_vision, self.span = float(p_audio), float(p_vision), span
        self.world, self.rank = 1, 0

    def __repr__(self) -> str:
        return f"ModalityDropout(p_audio={self.p_audio}, p_vision={self.p_vision}, span={self.span})"

    def for_rank(self, world: int, rank: int) -> ModalityDropout:
        """A copy bound to rank ``rank`` of ``world`` (``FlatDataParallel.modality_dropout`` calls this)."""
        if world < 1 or not 0 <= rank < world:
            msg = f"need 0 <= rank < world, got rank {rank}, world {world}"
            raise ValueError(msg)
        bound = copy.copy(self)
        bound.world, bound.rank = int(world), int(rank)
        return bound

    def noise_shape(self, batch: int, steps: int) -> tuple[int, int, int]:
        """Shape of the ``u_mask`` uniforms for ``batch`` rows: ``(batch, ceil(steps / span), 2)``."""
        return (batch, -(-steps // self.span), 2)

    def _checked(self, u: Tensor, steps: int, world: int | None, rank: int | None) -> tuple[int, int, int]:
        world = self.world if world is None else int(world)
        rank = self.rank if rank is None else int(rank)
        if steps < 1 or world < 1 or not 0 <= rank < world:
            msg = f"need steps >= 1 and 0 <= rank < world, got steps {steps}, rank {rank}, world {world}"
            raise ValueError(msg)
        if u.dim() != 3 or u.dtype != torch.float32 or tuple(u.shape[1:]) != self.noise_shape(1, steps)[1:]:  # noqa: PLR2004
            msg = f"u must be float32 [B_global, {self.noise_shape(1, steps)[1]}, 2] for {steps} steps, got {u.dtype} {tuple(u.shape)}"
            raise ValueError(msg)
        if u.shape[0] == 0 or u.shape[0] % world:
            msg = f"the global batch {u.shape[0]} is not a positive multiple of the world size {world}"
            raise ValueError(msg)
        return world, rank, u.shape[0] // world

    def reference(self, u: Tensor, steps: int) -> Tensor:
        """The rule in torch: uniforms ``[B, S, 2]`` -> bool mask ``[B, steps, 2]`` (audio, vision) of all rows."""
        self._checked(u, steps, 1, 0)
        block = torch.arange(steps, device=u.device) // self.span
        ub = u[:, block]  # [B, steps, 2]
        p = torch.tensor([self.p_audio, self.p_vision], dtype=torch.float32, device=u.device)
        mask = ub >= p
        none0 = ~mask[:, 0].any(dim=-1)
        audio_wins = ub[:, 0, 0] >= ub[:, 0, 1]
        mask[:, 0, 0] |= none0 & audio_wins
        mask[:, 0, 1] |= none0 & ~audio_wins
        return mask

    def sample(self, u: Tensor, steps: int, *, world: int | None = None, rank: int | None = None) -> DropoutSample:
        """One kernel launch on torch's current stream: the masks of rank ``rank``'s rows of the global batch ``u`` describes,
        and the global present-frame counts."""
        world, rank, local = self._checked(u, steps, world, rank)
        u = u.contiguous()
        dev = u.device
        codes = torch.empty(local, steps, dtype=torch.int32, device=dev)
        pa = torch.empty(local * steps, dtype=torch.float32, device=dev)
        pv = torch.empty(local * steps, dtype=torch.float32, device=dev)
        mask0 = torch.empty(local, 2, dtype=torch.bool, device=dev)
        counts = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().mtrssm_modality_dropout(_lib.ptr(u), u.shape[0], steps, self.span, self.p_audio, self.p_vision, rank * local, local,
                                                       _lib.index_ptr(codes), _lib.ptr(pa), _lib.ptr(pv), _lib.raw_ptr(mask0), _lib.ptr(counts),
                                                       _lib.stream_ptr(dev)), "mtrssm_modality_dropout")
        return DropoutSample(codes, pa, pv, mask0, counts, world)


class RaggedMask(NamedTuple):
    """``ragged_reference``'s result over all rows: ``mask`` bool ``[B, T, 2]``, ``live`` bool ``[B, T]``, ``last`` int32 ``[B]``,
    ``counts`` float32 ``[3]`` (present audio frames, present vision frames, live steps)."""

    mask: Tensor
    live: Tensor
    last: Tensor
    counts: Tensor

    @property
    def codes(self) -> Tensor:
        return (self.mask[..., 0].to(torch.int32) + 2 * self.mask[..., 1].to(torch.int32)).contiguous()


def _checked_valid(valid: Tensor, steps: int) -> None:
    if not isinstance(valid, Tensor) or valid.dtype != torch.int32 or valid.dim() != 1 or valid.numel() == 0:
        msg = f"valid must be an int32 [B_global] tensor, got {getattr(valid, 'dtype', type(valid))} {tuple(getattr(valid, 'shape', ()))}"
        raise ValueError(msg)
    if steps < 1:
        msg = f"need steps >= 1, got {steps}"
        raise ValueError(msg)


def ragged_reference(valid: Tensor, u: Tensor | None, steps: int, md: ModalityDropout | None = None) -> RaggedMask:
    """The rule of a ragged batch in torch (``mtrssm_step_mask_ragged`` is the kernel): step ``(b, t)`` is live iff
    ``t < clamp(valid[b], 0, steps)``; a modality is present iff the step is live AND (``u`` None: no dropout, or ``md.reference``
    says present -- its t = 0 fix-up is applied before the AND).  A dead step has code 0."""
    _checked_valid(valid, steps)
    n = valid.to(torch.long).clamp(0, steps)
    live = torch.arange(steps, device=valid.device) < n.unsqueeze(1)
    if u is None:
        mask = live.unsqueeze(-1).expand(-1, -1, 2).clone()
    else:
        if md is None:
            msg = "uniforms need the ModalityDropout whose rule they feed"
            raise ValueError(msg)
        if u.shape[0] != valid.numel():
            msg = f"u has {u.shape[0]} rows, valid {valid.numel()}"
            raise ValueError(msg)
        mask = md.reference(u, steps) & live.unsqueeze(-1)
    counts = torch.stack([mask[..., 0].sum(), mask[..., 1].sum(), live.sum()]).to(torch.float32)
    return RaggedMask(mask, live, (n - 1).to(torch.int32), counts)


def ragged_step_mask(valid: Tensor, u: Tensor | None, steps: int, md: ModalityDropout | None = None, *, world: int = 1,
                     rank: int = 0) -> StepMask:
    """One ``mtrssm_step_mask_ragged`` launch on torch's current stream: the ``StepMask`` of rank ``rank``'s rows of the global batch
    ``valid`` (int32 ``[B_global]``, on the device) describes.  The three counts are the GLOBAL batch's, divided by ``world`` as
    ``DropoutSample.step_mask`` does: the mean over ranks is the global batch's loss."""
    _checked_valid(valid, steps)
    if world < 1 or not 0 <= rank < world or valid.numel() % world:
        msg = f"need 0 <= rank < world and a global batch that is a multiple of world, got rank {rank}, world {world}, {valid.numel()} rows"
        raise ValueError(msg)
    span, pa, pv = 1, 0.0, 0.0
    if u is not None:
        if md is None:
            msg = "uniforms need the ModalityDropout whose rule they feed"
            raise ValueError(msg)
        md._checked(u, steps, world, rank)  # noqa: SLF001
        if u.shape[0] != valid.numel():
            msg = f"u has {u.shape[0]} rows, valid {valid.numel()}"
            raise ValueError(msg)
        u = u.contiguous()
        span, pa, pv = md.span, md.p_audio, md.p_vision
    valid = valid.contiguous()
    dev = valid.device
    local = valid.numel() // world
    codes = torch.empty(local, steps, dtype=torch.int32, device=dev)
    planes = [torch.empty(local * steps, dtype=torch.float32, device=dev) for _ in range(3)]
    mask0 = torch.empty(local, 2, dtype=torch.bool, device=dev)
    last = torch.empty(local, dtype=torch.int32, device=dev)
    counts = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().mtrssm_step_mask_ragged(_lib.index_ptr(valid), _lib.ptr(u), valid.numel(), steps, span, pa, pv, rank * local, local,
                                                   _lib.index_ptr(codes), _lib.ptr(planes[0]), _lib.ptr(planes[1]), _lib.ptr(planes[2]),
                                                   _lib.raw_ptr(mask0), _lib.index_ptr(last), _lib.ptr(counts), _lib.stream_ptr(dev)),
               "mtrssm_step_mask_ragged")
    norm = counts if world == 1 else counts / float(world)
    return StepMask(codes, planes[0], planes[1], mask0, norm[0], norm[1], planes[2], norm[2], last)


__all__ = ["DropoutSample", "ModalityDropout", "RaggedMask", "StepMask", "ragged_reference", "ragged_step_mask"]
