"""Forecast objective: observe a sampled context, run the rest of the row open loop, reconstruct every live frame.

The rule (``Forecast.reference`` is its restatement in torch, ``mtrssm_step_mask_forecast`` the kernel): with ``n = hi - lo + 1`` and
uniforms ``u_context`` of shape ``[B_global]``, row ``b`` observes a context of ``c_b = lo + min(int(u_context[b] * float(n)), n - 1)``
frames -- one fp32 multiply, truncated.  ``live(b, t) = t < clamp(valid[b], 0, T)``, ``observed = live and t < c_b``; modality m is
SEEN at ``(b, t)`` iff the step is observed and the dropout rule (when there is one, its t = 0 fix-up applied first) says present.
The scans read the seen bits: on the tail they run posterior = prior, so the gradient of a tail frame's reconstruction travels
back through the prior steps to the last observed frame.  Both NLL planes are ``live``: every live frame of both modalities is a
target, seen or not.  The KL's plane is ``observed`` (it is exactly 0 elsewhere), divided by the observed steps.

One launch writes all of it for a rank's rows, with the two counts of the GLOBAL batch as device scalars; nothing is read back,
so the sampler can sit inside a captured hipGraph (``graph.CapturedTrainStep(forecast=...)``).
"""

from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import NamedTuple

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.dropout import ModalityDropout, StepMask, _checked_valid

_INT31 = 1 << 31


class ForecastMask(NamedTuple):
    """``Forecast.reference``'s result over all rows: ``codes`` int32 ``[B, T]`` (the seen bits), ``target`` and ``observed`` bool
    ``[B, T]``, ``last`` int32 ``[B]``, ``counts`` float32 ``[2]`` (live steps, observed steps), ``context`` int32 ``[B]`` (``c_b``)."""

    codes: Tensor
    target: Tensor
    observed: Tensor
    last: Tensor
    counts: Tensor
    context: Tensor

    @property
    def mask(self) -> Tensor:
        """The bool ``[B, T, 2]`` mask of what is seen."""
        return torch.stack([(self.codes & 1) != 0, (self.codes & 2) != 0], dim=-1)


@dataclass
class ForecastStepMask(StepMask):
    """The ``StepMask`` of a forecast step (``Forecast.sample``): ``codes`` / ``mask0`` say what the scans see, ``present_audio`` and
    ``present_vision`` are both the ``live`` plane (what the NLLs reconstruct), ``live`` / ``count_live`` the ``observed`` plane and its
    count (the KL).  Beside it the kernel's own outputs: ``seen_audio`` / ``seen_vision`` float32 ``[B * T]`` in {0, 1} and ``counts``
    float32 ``[2]`` (live, observed steps of the GLOBAL batch, not divided by the world size)."""

    seen_audio: Tensor | None = None
    seen_vision: Tensor | None = None
    counts: Tensor | None = None

    @property
    def mask(self) -> Tensor:
        """The bool ``[B, T, 2]`` mask of what is seen."""
        return torch.stack([self.seen_audio != 0, self.seen_vision != 0], dim=-1).reshape(*self.codes.shape, 2)


class Forecast:
    """``Forecast(q)``: every row observes ``q`` frames; ``Forecast((lo, hi))``: a context length drawn per row, uniform on
    ``lo .. hi``.  ``1 <= lo <= hi``; ``hi`` may exceed T -- a row whose context reaches its end is a plain closed-loop row.
    ``world`` / ``rank`` (``for_rank``) say which rows of the global batch a rank trains on."""

    def __init__(self, context: int | tuple[int, int]) -> None:
        bounds = (context, context) if not isinstance(context, (tuple, list)) else tuple(context)
        if len(bounds) != 2 or any(isinstance(c, bool) or not isinstance(c, int) for c in bounds):  # noqa: PLR2004
            msg = f"context must be an integer q or a pair of integers (lo, hi), got {context!r}"
            raise ValueError(msg)
        lo, hi = bounds
        if not 1 <= lo <= hi < _INT31:
            msg = f"context needs 1 <= lo <= hi < 2^31 (frame 0 is always observed), got lo {lo}, hi {hi}"
            raise ValueError(msg)
        self.lo, self.hi = lo, hi
        self.world, self.rank = 1, 0

    def __repr__(self) -> str:
        return f"Forecast({self.lo})" if self.fixed else f"Forecast(({self.lo}, {self.hi}))"

    @property
    def fixed(self) -> bool:
        """One context length for every row: the uniforms do not matter."""
        return self.lo == self.hi

    def for_rank(self, world: int, rank: int) -> Forecast:
        """A copy bound to rank ``rank`` of ``world`` (``FlatDataParallel.forecast`` calls this)."""
        if world < 1 or not 0 <= rank < world:
            msg = f"need 0 <= rank < world, got rank {rank}, world {world}"
            raise ValueError(msg)
        bound = copy.copy(self)
        bound.world, bound.rank = int(world), int(rank)
        return bound

    @staticmethod
    def noise_shape(batch: int) -> tuple[int]:
        """Shape of the ``u_context`` uniforms for ``batch`` rows: ``(batch,)``."""
        return (batch,)

    def _checked(self, u_context: Tensor, steps: int, valid: Tensor | None, u_mask: Tensor | None, md: ModalityDropout | None) -> None:
        if not isinstance(u_context, Tensor) or u_context.dtype != torch.float32 or u_context.dim() != 1 or u_context.numel() == 0:
            msg = (f"u_context must be a float32 [B_global] tensor, got {getattr(u_context, 'dtype', type(u_context))} "
                   f"{tuple(getattr(u_context, 'shape', ()))}")
            raise ValueError(msg)
        if steps < 1:
            msg = f"need steps >= 1, got {steps}"
            raise ValueError(msg)
        rows = u_context.numel()
        if valid is not None:
            _checked_valid(valid, steps)
            if valid.numel() != rows:
                msg = f"valid has {valid.numel()} rows, u_context {rows}"
                raise ValueError(msg)
        if (u_mask is None) != (md is None):
            msg = "the dropout uniforms and the ModalityDropout whose rule they feed come together"
            raise ValueError(msg)
        if md is not None:
            md._checked(u_mask, steps, 1, 0)  # noqa: SLF001
            if u_mask.shape[0] != rows:
                msg = f"u_mask has {u_mask.shape[0]} rows, u_context {rows}"
                raise ValueError(msg)

    def reference(self, u_context: Tensor, steps: int, valid: Tensor | None = None, u_mask: Tensor | None = None,
                  md: ModalityDropout | None = None) -> ForecastMask:
        """The rule in torch, on any device, over all rows."""
        self._checked(u_context, steps, valid, u_mask, md)
        dev = u_context.device
        n = self.hi - self.lo + 1
        bins = (u_context * torch.tensor(float(n), dtype=torch.float32, device=dev)).to(torch.int64).clamp(max=n - 1)
        context = bins + self.lo
        length = torch.full_like(context, steps) if valid is None else valid.to(torch.int64).clamp(0, steps)
        t = torch.arange(steps, device=dev)
        live = t < length.unsqueeze(1)
        observed = live & (t < context.unsqueeze(1))
        seen = observed.unsqueeze(-1).expand(-1, -1, 2)
        if md is not None:
            seen = md.reference(u_mask, steps) & seen
        codes = (seen[..., 0].to(torch.int32) + 2 * seen[..., 1].to(torch.int32)).contiguous()
        counts = torch.stack([live.sum(), observed.sum()]).to(torch.float32)
        return ForecastMask(codes, live, observed, (length - 1).to(torch.int32), counts, context.to(torch.int32))

    def sample(self, u_context: Tensor, steps: int, valid: Tensor | None = None, u_mask: Tensor | None = None,  # noqa: PLR0913
               md: ModalityDropout | None = None, *, world: int | None = None, rank: int | None = None) -> ForecastStepMask:
        """One ``mtrssm_step_mask_forecast`` launch on torch's current stream, nothing read back: the ``StepMask`` of rank ``rank``'s
        rows of the global batch ``u_context`` (and ``valid``, ``u_mask``) describes.  Both counts are the GLOBAL batch's, divided by
        ``world``: the mean over ranks is the global batch's loss."""
        world = self.world if world is None else int(world)
        rank = self.rank if rank is None else int(rank)
        self._checked(u_context, steps, valid, u_mask, md)
        rows = u_context.numel()
        if world < 1 or not 0 <= rank < world or rows % world:
            msg = f"need 0 <= rank < world and a global batch that is a multiple of world, got rank {rank}, world {world}, {rows} rows"
            raise ValueError(msg)
        span, pa, pv = (1, 0.0, 0.0) if md is None else (md.span, md.p_audio, md.p_vision)
        u_context = u_context.contiguous()
        valid = None if valid is None else valid.contiguous()
        u_mask = None if u_mask is None else u_mask.contiguous()
        dev = u_context.device
        local = rows // world
        codes = torch.empty(local, steps, dtype=torch.int32, device=dev)
        seen_a, seen_v, target, observed = (torch.empty(local * steps, dtype=torch.float32, device=dev) for _ in range(4))
        mask0 = torch.empty(local, 2, dtype=torch.bool, device=dev)
        last = torch.empty(local, dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().mtrssm_step_mask_forecast(
            _lib.index_ptr(valid), _lib.ptr(u_mask), _lib.ptr(u_context), rows, steps, span, pa, pv, self.lo, self.hi, rank * local, local,
            _lib.index_ptr(codes), _lib.ptr(seen_a), _lib.ptr(seen_v), _lib.ptr(target), _lib.ptr(observed), _lib.raw_ptr(mask0),
            _lib.index_ptr(last), _lib.ptr(counts), _lib.stream_ptr(dev)), "mtrssm_step_mask_forecast")
        norm = counts if world == 1 else counts / float(world)
        return ForecastStepMask(codes, target, target, mask0, norm[0], norm[0], observed, norm[1], last, seen_a, seen_v, counts)


__all__ = ["Forecast", "ForecastMask", "ForecastStepMask"]
