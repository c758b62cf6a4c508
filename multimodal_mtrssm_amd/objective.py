"""Gaussian negative log-likelihood with unit scale, as one fused HIP reduction.

Replaces ``models/objective.py:7-23`` (``-Independent(Normal(pred, scale), k).log_prob(target).mean()``).
For ``scale == 1`` the value is ``mean_frames sum_event [0.5 (t - p)^2 + 0.5 log 2pi]``; the kernel reads
prediction and target once (HBM-bound, 16 B / lane) and the backward writes ``(p - t) / frames``.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib


def _aligned(t: Tensor) -> Tensor:
    """``t`` contiguous at a 16-byte aligned address, as the kernels' 16 B / lane accesses need it: ``t`` itself when it already
    is (no launch), else a copy -- a contiguous slice such as ``x[1:]`` of an odd event size starts anywhere."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _fresh_like(pred: Tensor) -> Tensor:
    """The gradient buffer: a new allocation, which the caching allocator hands out on far more than 16 bytes.  Nothing is ever
    copied here (there is nothing to copy yet); should an allocator break that, the launch below would refuse the pointer."""
    g_pred = torch.empty_like(pred)
    assert g_pred.data_ptr() % 16 == 0, "a fresh allocation is 16-byte aligned"  # noqa: S101
    return g_pred


class _GaussianNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction: Tensor, target: Tensor, event_ndims: int, act: int = 0) -> Tensor:  # noqa: ANN001
        lib = _lib.load()
        pred, tgt = _aligned(prediction), _aligned(target)
        event = math.prod(pred.shape[-event_ndims:])
        frames = pred.numel() // event
        out = torch.empty((), device=pred.device, dtype=torch.float32)
        _lib.check(_lib.TIMERS.call("mtrssm_gaussian_nll_fwd", lib.mtrssm_gaussian_nll_fwd, _lib.ptr(pred), _lib.ptr(tgt), frames, event,
                                    int(act), _lib.ptr(out), _lib.stream_ptr(pred.device), nbytes=8.0 * pred.numel()),
                   "mtrssm_gaussian_nll_fwd")
        ctx.save_for_backward(pred, tgt)
        ctx.frames, ctx.event, ctx.act = frames, event, int(act)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):  # noqa: ANN001, ANN205
        lib = _lib.load()
        pred, tgt = ctx.saved_tensors
        g_pred = _fresh_like(pred)
        g = g_out.contiguous()
        _lib.check(_lib.TIMERS.call("mtrssm_gaussian_nll_bwd", lib.mtrssm_gaussian_nll_bwd, _lib.ptr(pred), _lib.ptr(tgt), _lib.ptr(g), ctx.frames,
                                    ctx.event, ctx.act, _lib.ptr(g_pred), _lib.stream_ptr(pred.device), nbytes=12.0 * pred.numel()),
                   "mtrssm_gaussian_nll_bwd")
        return g_pred, None, None, None


class _GaussianNLLMasked(torch.autograd.Function):
    """The NLL averaged over the frames whose ``present`` entry is 1 (``mtrssm_gaussian_nll_masked_fwd / _bwd``); ``count`` is
    the device scalar sum(present): nothing is read back to the host."""

    @staticmethod
    def forward(ctx, prediction: Tensor, target: Tensor, present: Tensor, count: Tensor, event_ndims: int, act: int = 0) -> Tensor:  # noqa: ANN001, PLR0913
        lib = _lib.load()
        pred, tgt = _aligned(prediction), _aligned(target)
        event = math.prod(pred.shape[-event_ndims:])
        frames = pred.numel() // event
        out = torch.empty((), device=pred.device, dtype=torch.float32)
        _lib.check(_lib.TIMERS.call("mtrssm_gaussian_nll_masked_fwd", lib.mtrssm_gaussian_nll_masked_fwd, _lib.ptr(pred), _lib.ptr(tgt),
                                    _lib.ptr(present), _lib.ptr(count), frames, event, int(act), _lib.ptr(out), _lib.stream_ptr(pred.device),
                                    nbytes=8.0 * pred.numel()), "mtrssm_gaussian_nll_masked_fwd")
        ctx.save_for_backward(pred, tgt, present, count)
        ctx.frames, ctx.event, ctx.act = frames, event, int(act)
        return out

    @staticmethod
    def backward(ctx, g_out: Tensor):  # noqa: ANN001, ANN205
        lib = _lib.load()
        pred, tgt, present, count = ctx.saved_tensors
        g_pred = _fresh_like(pred)
        g = g_out.contiguous()
        _lib.check(_lib.TIMERS.call("mtrssm_gaussian_nll_masked_bwd", lib.mtrssm_gaussian_nll_masked_bwd, _lib.ptr(pred), _lib.ptr(tgt),
                                    _lib.ptr(present), _lib.ptr(count), _lib.ptr(g), ctx.frames, ctx.event, ctx.act, _lib.ptr(g_pred),
                                    _lib.stream_ptr(pred.device), nbytes=12.0 * pred.numel()), "mtrssm_gaussian_nll_masked_bwd")
        return g_pred, None, None, None, None, None


def likelihood(prediction: Tensor, target: Tensor, event_ndims: int, scale: float = 1.0, *, out_act: int = 0,  # noqa: PLR0913
               frame_mask: Tensor | None = None, frame_present: tuple[Tensor, Tensor] | None = None) -> Tensor:
    """Negative mean log-likelihood of ``target`` under ``Normal(act(prediction), scale)`` (``objective.py:7``).  ``out_act``
    (0 = Identity as in the reference's signature, 3 = Tanh) lets the decoder hand in its raw last-layer output: the
    out_activation is applied while the kernel reads it and its derivative in the backward.

    ``frame_mask``: optional bool tensor over the frame dims (``prediction.shape[:-event_ndims]``).  The mean then runs over the
    frames where it is True only; a mask with no True entry gives 0 and a zero gradient.

    ``frame_present``: the same mask already in the kernels' form, ``(present, count)``: float32 {0, 1} per frame (flat) and the
    device scalar the masked sum is divided by.  ``count`` need not be ``present.sum()``: a data-parallel rank passes
    ``global count / world`` (``dropout.DropoutSample.step_mask``)."""
    if prediction.shape != target.shape:
        msg = f"prediction {tuple(prediction.shape)} and target {tuple(target.shape)} must have the same shape"
        raise ValueError(msg)
    if frame_mask is not None and frame_present is not None:
        msg = "give frame_mask or frame_present, not both"
        raise ValueError(msg)
    if frame_mask is not None or frame_present is not None:
        frame_shape = tuple(prediction.shape[: prediction.dim() - event_ndims])
        if frame_present is not None:
            present, count = frame_present
            if present.dtype != torch.float32 or present.numel() != math.prod(frame_shape) or count.numel() != 1:
                msg = f"frame_present must be (float32 [{math.prod(frame_shape)}], scalar), got {present.dtype} {tuple(present.shape)}"
                raise ValueError(msg)
            present = present.reshape(-1)
        else:
            if frame_mask.dtype != torch.bool or tuple(frame_mask.shape) != frame_shape:
                msg = f"frame_mask must be a bool tensor of shape {frame_shape}, got {frame_mask.dtype} {tuple(frame_mask.shape)}"
                raise ValueError(msg)
            present = frame_mask.reshape(-1).to(torch.float32)
            count = present.sum()
        if scale != 1.0:
            if out_act:
                prediction = torch.tanh(prediction) if out_act == 3 else prediction  # noqa: PLR2004
            unit = _GaussianNLLMasked.apply(prediction / scale, target / scale, present, count, event_ndims, 0)
            # log(scale) is a term of every present frame, divided by count like the rest (count may be a rank's share)
            share = torch.where(count > 0, (present != 0).sum() / count, torch.zeros_like(count)).reshape(())  # counted as the kernel does
            return unit + share * (math.prod(prediction.shape[-event_ndims:]) * math.log(scale))
        return _GaussianNLLMasked.apply(prediction, target, present, count, event_ndims, int(out_act))
    if scale != 1.0:
        # Normal(pred, s): 0.5 ((t-p)/s)^2 + log s + 0.5 log 2pi, by rescaling the unit-scale kernel
        event = math.prod(prediction.shape[-event_ndims:])
        if out_act:
            prediction = torch.tanh(prediction) if out_act == 3 else prediction  # noqa: PLR2004
        unit = _GaussianNLL.apply(prediction / scale, target / scale, event_ndims, 0)
        return unit + event * math.log(scale)
    return _GaussianNLL.apply(prediction, target, event_ndims, int(out_act))
