"""The digit reader: the small CNN that reads a digit off a predicted vision frame (inference; ``digit_train.py`` fits it).

The network is the evaluation's classifier, layer for layer and name for name (a checkpoint of it loads with ``strict=True``):

    x      = clamp((act(pred) + 1) / 2, 0, 1)                       the decoder's raw output, denormalised to [0, 1]; [N, 1, 32, 32]
    f      = pool2(relu(conv2(pool2(relu(conv1(x))))))              3x3 / pad 1 convolutions 1 -> 32 -> 64, 2x2 max pools; [N, 64, 8, 8]
    logits = fc2(relu(fc1(f.view(-1, 4096))))                       4096 -> 128 -> 10; dropout is the identity (``eval()``)
    digit  = the lowest index among the largest logits              ``torch.max``'s first occurrence

``reference_logits`` states this in torch for any float dtype: it is the checker, and what runs for non-GPU tensors.  On the GPU the
trunk is ONE ``mtrssm_digit_features`` launch (neither intermediate is written to memory; conv2 multiplies two bf16 pieces per
operand), fc1 one ``mtrssm_gemm`` with its bias + ReLU epilogue, the head one ``mtrssm_digit_head`` launch.  ``select`` (int32
``[N]``) picks the frames to read out of a larger decode without a copy.  ``DigitClassifier()`` is frozen and in ``eval()``; ``digit_train.DigitTrainer``
trains it on labelled frames and hands it back frozen.
"""

from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F  # noqa: N812
from torch import Tensor, nn

from multimodal_mtrssm_amd import _lib, linear

PIXELS = 32 * 32
FEATURES = 64 * 8 * 8
HIDDEN = 128
CLASSES = 10
_TILE_ROWS = 128           # row multiple of the bf16-piece tile GEMM
_ACT_RELU = _lib.ACT_IDS["ReLU"]


def _check_act(act: int) -> int:
    if act not in (0, 3):
        msg = f"act must be 0 (Identity) or 3 (Tanh), got {act}"
        raise ValueError(msg)
    return int(act)


class DigitClassifier(nn.Module):
    """``conv1 [32,1,3,3]``, ``conv2 [64,32,3,3]``, ``fc1 [128,4096]``, ``fc2 [10,128]`` with their biases: the evaluation's
    ``SimpleMNISTClassifier`` (its pool / relu / dropout members carry no state)."""

    def __init__(self) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3, padding=1)
        self.fc1 = nn.Linear(FEATURES, HIDDEN)
        self.fc2 = nn.Linear(HIDDEN, CLASSES)
        self.requires_grad_(False)
        self.eval()

    # -- the rule in torch -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _frames(pred_raw: Tensor, select: Tensor | None) -> Tensor:
        if pred_raw.numel() == 0 or pred_raw.numel() % PIXELS:
            msg = f"pred_raw must hold whole 32 x 32 frames, got shape {tuple(pred_raw.shape)}"
            raise ValueError(msg)
        frames = pred_raw.reshape(-1, PIXELS)
        if select is not None and (select.dim() != 1 or select.dtype != torch.int32 or select.numel() == 0):
            msg = f"select must be a non-empty int32 vector of frame indices, got {select.dtype} {tuple(select.shape)}"
            raise ValueError(msg)
        return frames

    @staticmethod
    def images(pred_raw: Tensor, act: int = 0, select: Tensor | None = None) -> Tensor:
        """``[N, 1, 32, 32]`` in [0, 1]: the frames the classifier sees."""
        act = _check_act(act)
        x = DigitClassifier._frames(pred_raw, select)
        if select is not None:
            x = x[select.long()]
        y = torch.tanh(x) if act == 3 else x  # noqa: PLR2004
        return ((y + 1.0) / 2.0).clamp(0.0, 1.0).reshape(-1, 1, 32, 32)

    def reference_features(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None) -> Tensor:
        """The trunk in torch, in ``pred_raw``'s dtype: ``[N, 4096]``."""
        x = self.images(pred_raw, act, select)
        dt = x.dtype
        x = F.max_pool2d(F.relu(F.conv2d(x, self.conv1.weight.to(dt), self.conv1.bias.to(dt), padding=1)), 2, 2)
        x = F.max_pool2d(F.relu(F.conv2d(x, self.conv2.weight.to(dt), self.conv2.bias.to(dt), padding=1)), 2, 2)
        return x.reshape(-1, FEATURES)

    def reference_logits(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None) -> Tensor:
        """The rule in torch, in ``pred_raw``'s dtype (any float dtype, any device): ``[N, 10]``."""
        f = self.reference_features(pred_raw, act, select)
        dt = f.dtype
        h = F.relu(F.linear(f, self.fc1.weight.to(dt), self.fc1.bias.to(dt)))
        return F.linear(h, self.fc2.weight.to(dt), self.fc2.bias.to(dt))

    @staticmethod
    def first_max(logits: Tensor) -> Tensor:
        """int32 ``[N]``: the lowest index among the maxima of each row."""
        top = logits.max(dim=1, keepdim=True).values
        idx = torch.arange(logits.shape[1], device=logits.device).expand_as(logits)
        return torch.where(logits == top, idx, torch.full_like(idx, logits.shape[1])).min(dim=1).values.to(torch.int32)

    # -- kernels on the GPU, the rule elsewhere ------------------------------------------------------------------------------------------
    def features(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None, *, out: Tensor | None = None) -> Tensor:
        """One ``mtrssm_digit_features`` launch on torch's current stream: fp32 ``[N, 4096]`` (non-GPU tensors: the torch rule).  ``out``:
        a contiguous fp32 buffer of at least ``N`` rows to write into."""
        act = _check_act(act)
        frames = self._frames(pred_raw, select)
        if not pred_raw.is_cuda:
            return self.reference_features(pred_raw, act, select)
        frames = frames.contiguous()
        n = frames.shape[0] if select is None else select.numel()
        if out is None:
            out = torch.empty(n, FEATURES, device=frames.device, dtype=torch.float32)
        if out.dim() != 2 or out.shape[0] < n or out.shape[1] != FEATURES or not out.is_contiguous():  # noqa: PLR2004
            msg = f"out must be a contiguous [>= {n}, {FEATURES}] buffer, got {tuple(out.shape)}"
            raise ValueError(msg)
        w1, b1, w2, b2 = (p.contiguous() for p in (self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias))
        sel = None if select is None else select.contiguous()
        _lib.check(_lib.TIMERS.call("mtrssm_digit_features", _lib.load().mtrssm_digit_features, _lib.ptr(frames), frames.shape[0],
                                    _lib.index_ptr(sel), n, act, _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(out),
                                    _lib.stream_ptr(frames.device), flops=2.0 * n * (1024 * 9 * 32 + 256 * 288 * 64),
                                    nbytes=4.0 * n * (PIXELS + FEATURES)), "mtrssm_digit_features")
        return out[:n]

    def hidden(self, features: Tensor) -> Tensor:
        """``relu(fc1(features))`` on ``mtrssm_gemm`` (bias and ReLU in its epilogue; one reduction slice: ordered sums).  A row count
        that is a multiple of 128 runs the bf16-piece tile kernel when the problem is large, anything else the fp32 MFMA kernels."""
        h = torch.empty(features.shape[0], HIDDEN, device=features.device, dtype=torch.float32)
        g, flops, nbytes = linear._problem(features, self.fc1.weight.contiguous(), h, a_rmajor=False, b_rmajor=False,  # noqa: SLF001
                                           bias=self.fc1.bias.contiguous())
        g.act_out = _ACT_RELU
        _lib.check(_lib.TIMERS.call("mtrssm_gemm", _lib.load().mtrssm_gemm, C.byref(g), _lib.stream_ptr(features.device), flops=flops,
                                    nbytes=nbytes), "mtrssm_gemm")
        return h

    def read(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None, *, want_logits: bool = True) -> tuple[Tensor, Tensor | None]:
        """``(digit int32 [N], logits fp32 [N, 10] or None)``."""
        if not pred_raw.is_cuda:
            logits = self.reference_logits(pred_raw, act, select)
            return self.first_max(logits), (logits if want_logits else None)
        frames = self._frames(pred_raw, select)
        n = frames.shape[0] if select is None else select.numel()
        rows = n
        if 2.0 * n * HIDDEN * FEATURES >= linear.SPLIT_MIN_FLOPS:  # large enough for the tile GEMM: whole 128-row tiles
            rows = -(-n // _TILE_ROWS) * _TILE_ROWS
        buf = torch.empty(rows, FEATURES, device=frames.device, dtype=torch.float32)
        if rows > n:
            buf[n:].zero_()
        self.features(pred_raw, act, select, out=buf)
        h = self.hidden(buf)  # (the pad rows are zeros: rows do not mix)
        digit = torch.empty(n, device=frames.device, dtype=torch.int32)
        logits = torch.empty(n, CLASSES, device=frames.device, dtype=torch.float32) if want_logits else None
        w, b = self.fc2.weight.contiguous(), self.fc2.bias.contiguous()
        sel = None if select is None else select.contiguous()
        _lib.check(_lib.load().mtrssm_digit_head(_lib.ptr(h), _lib.ptr(w), _lib.ptr(b), n, _lib.index_ptr(sel), frames.shape[0], _lib.index_ptr(digit),
                                                 _lib.ptr(logits),
                                                 _lib.stream_ptr(frames.device)), "mtrssm_digit_head")
        return digit, logits

    def logits(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None) -> Tensor:
        """``[N, 10]`` from the decoder's raw output ``pred_raw`` (any shape of whole 32 x 32 frames)."""
        return self.read(pred_raw, act, select)[1]

    def digits(self, pred_raw: Tensor, act: int = 0, select: Tensor | None = None) -> Tensor:
        """int32 ``[N]``: the digit read off each frame."""
        return self.read(pred_raw, act, select, want_logits=False)[0]

    def forward(self, images: Tensor) -> Tensor:
        """Logits of already denormalised images ``[N, 1, 32, 32]`` in [0, 1].  On the GPU the images go through the same launch as
        ``2 x - 1`` (exact at 0 and 1, within 2^-25 of x elsewhere)."""
        if images.dim() != 4 or tuple(images.shape[1:]) != (1, 32, 32):  # noqa: PLR2004
            msg = f"images must be [N, 1, 32, 32], got {tuple(images.shape)}"
            raise ValueError(msg)
        return self.logits(images * 2.0 - 1.0, 0)


def word_counts(word: Tensor, digit: Tensor, counts: Tensor) -> None:
    """``counts[word[n], digit[n]] += 1`` into the fp32 ``[10, 11]`` table (column 10: the failure bin); ``word < 0`` (silence) is skipped.
    One ``mtrssm_word_counts`` launch for GPU tensors, ``bincount`` elsewhere; whole numbers either way."""
    if word.dtype != torch.int32 or digit.dtype != torch.int32 or word.dim() != 1 or tuple(digit.shape) != tuple(word.shape):
        msg = f"word and digit must be int32 vectors of one length, got {word.dtype} {tuple(word.shape)} and {digit.dtype} {tuple(digit.shape)}"
        raise ValueError(msg)
    if tuple(counts.shape) != (CLASSES, CLASSES + 1) or counts.dtype != torch.float32 or not counts.is_contiguous():
        msg = f"counts must be a contiguous fp32 [{CLASSES}, {CLASSES + 1}] table, got {counts.dtype} {tuple(counts.shape)}"
        raise ValueError(msg)
    n = word.numel()
    if not 0 < n < 1 << 24:
        msg = f"{n} frames: need 0 < N < 2^24 (the fp32 counts are exact below 2^24)"
        raise ValueError(msg)
    if not word.is_cuda:
        w, d = word.long(), digit.long()
        keep = (w >= 0) & (w < CLASSES) & (d >= 0) & (d <= CLASSES)
        counts += torch.bincount(w[keep] * (CLASSES + 1) + d[keep], minlength=CLASSES * (CLASSES + 1)).reshape(CLASSES, CLASSES + 1).to(counts.dtype)
        return
    _lib.check(_lib.load().mtrssm_word_counts(_lib.index_ptr(word.contiguous()), _lib.index_ptr(digit.contiguous()), n, _lib.ptr(counts),
                                              _lib.stream_ptr(word.device)), "mtrssm_word_counts")


__all__ = ["DigitClassifier", "word_counts"]
