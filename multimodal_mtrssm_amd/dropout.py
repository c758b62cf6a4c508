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

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib


@dataclass
class StepMask:
    """What one masked train step reads, all on the device: ``codes`` int32 ``[B, T]`` (bit 0 audio, bit 1 vision),
    ``present_audio`` / ``present_vision`` float32 ``[B * T]`` in {0, 1}, ``mask0`` bool ``[B, 2]`` (the t = 0 frame),
    ``count_audio`` / ``count_vision`` float32 scalars: what each reconstruction sum is divided by."""

    codes: Tensor
    present_audio: Tensor
    present_vision: Tensor
    mask0: Tensor
    count_audio: Tensor
    count_vision: Tensor

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


__all__ = ["DropoutSample", "ModalityDropout", "StepMask"]
