"""Free helpers the train step (``core.py``) and the evaluation steps (``evaluation.py``) both use."""

from __future__ import annotations

import torch
from torch import Tensor, nn

from multimodal_mtrssm_amd import conv


def _pairable(a: nn.Module, b: nn.Module, kind: type) -> bool:
    """Paired launches (``conv.paired``): the audio and the vision stack's equal layers share one grid (this package's own
    stacks only).  Everything runs on ONE stream: a two-stream variant of the step was removed in round 2 (it bought nothing
    once the layers were paired and stalled the GPU in about one run in fifteen, profiles/round1_notes.md)."""
    return conv.PAIR_LAUNCH and isinstance(a, kind) and isinstance(b, kind)


def _rand(like: Tensor, *shape: int) -> Tensor:
    return torch.rand(shape, device=like.device, dtype=torch.float32)


def _check_lengths(valid: Tensor, rows: int, device: torch.device) -> None:
    """A ragged batch's live-step counts: int32 ``[rows]`` on ``device`` (not read back)."""
    if not isinstance(valid, Tensor) or valid.dtype != torch.int32 or tuple(valid.shape) != (rows,):
        msg = f"lengths must be an int32 tensor of shape ({rows},), got {getattr(valid, 'dtype', type(valid))} {tuple(getattr(valid, 'shape', ()))}"
        raise ValueError(msg)
    if valid.device != torch.device(device):
        msg = f"lengths is on {valid.device}, the model's tensors on {device}"
        raise ValueError(msg)


def _masked_mean_embed(ea: Tensor | None, ev: Tensor | None, mask0: Tensor | None) -> Tensor:
    """t = 0 embedding: the mean over the present modalities of each row; both present is exactly ``(ea + ev) / 2``."""
    if ea is None or ev is None:
        return ea if ev is None else ev
    both = (ea + ev) / 2.0
    if mask0 is None:
        return both
    a, v = mask0[:, 0:1], mask0[:, 1:2]
    return torch.where(a & v, both, torch.where(a, ea, ev))
