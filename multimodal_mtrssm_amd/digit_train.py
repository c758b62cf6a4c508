"""Training the digit reader: the classifier of ``digits.py`` fitted on labelled frames.

The evaluation's own episodes carry ``image (T, 1, 32, 32)`` next to ``label (T,)`` (-1 = silence): the labelled frames of exactly the
digits the reader must read.  ``DigitTrainer`` fits a ``DigitClassifier`` on them with the reference's recipe (Adam at 1e-3, batch 64,
``Dropout(0.5)`` behind fc1, cross-entropy), so the matching rate needs no second code base and no download.

The rule of one step, for rows ``n`` with ``labels[n]`` in 0 .. 9 (any other label: a dead row, not read, adds nothing):

    x   = clamp((act(frame) + 1) / 2, 0, 1)
    p1  = pool2(relu(conv1(x)))      f = pool2(relu(conv2(p1))).view(4096)      h = relu(fc1(f))
    z   = fc2(h * keep / (1 - p))    nll = logsumexp(z) - z[label]              loss = sum nll / max(live count, 1)

``keep`` is a pure function of (seed, optimizer step, global row, unit): unit ``j`` of row ``r`` at step ``s`` is kept iff
``(w >> 8) 2^-24 >= p`` with ``w`` = word ``j & 3`` of ``Philox4x32-10((j >> 2, r, s, 0), dataset.stream_key(seed, 3))``
(``dropout_mask_reference``; ``p = 0`` keeps everything).  Nothing is stored, and rows sharded over ranks draw the masks of the unsharded fit.

The TAPE makes the trunk's backward well defined: one byte per pooled unit -- conv1's ``[32][16][16]``, then conv2's ``[64][8][8]`` in
the ``view(-1, 4096)`` order -- naming the member ``2 dy + dx`` of the 2 x 2 window that holds the maximum (the first in row-major order
among equal maxima: torch's ``max_pool2d`` backward), 4 when ``max + bias <= 0`` (``relu' = 0``).  Near a pool tie or a ReLU zero the
float64 choice and the kernel's may differ, and one re-routed unit moves a weight gradient by a whole term; with the kernel's own tape
imposed, ``DigitTrainer.rule`` is a linear function of ``g_features`` and states what the kernel must compute exactly.

On the GPU one step is: ``mtrssm_digit_features_train`` (the fused trunk, bit-identical features, plus the tape), fc1 on ``mtrssm_gemm``,
``mtrssm_digit_head_train`` (dropout, loss, ``g_hidden``, fc2's gradients), fc1's gradients and ``g_features`` on ``mtrssm_gemm``
(one reduction slice: ordered sums), ``mtrssm_digit_trunk_bwd``, and the two ``FlatAdamW`` launches.  Elsewhere the rule runs, with
``torch.optim.Adam``.
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F  # noqa: N812
from torch import Tensor

from multimodal_mtrssm_amd import _lib, linear
from multimodal_mtrssm_amd.dataset import philox4x32_10, stream_key
from multimodal_mtrssm_amd.digits import CLASSES, FEATURES, HIDDEN, DigitClassifier

TAPE_CONV1 = 32 * 16 * 16
TAPE = TAPE_CONV1 + FEATURES
DEAD = 4                 # the tape's code of a unit with max + bias <= 0
DROPOUT_STREAM = 3       # dataset.stream_key's stream of the dropout masks (0, 1, 2 are the feed's noise)
PARAMETERS = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
_TILE_ROWS = 128
_M32 = 0xFFFFFFFF


class DigitStats(NamedTuple):
    """Sums over the live rows of a step: the loss terms, the correct first-maximum predictions, the number of rows."""

    nll_sum: Tensor
    hits: Tensor
    count: Tensor


class TapeReference(NamedTuple):
    """The float64 choices: ``tape`` uint8 ``[N, 12288]``; per unit ``margin`` (largest minus second largest member of its window) and
    ``value`` (``max + bias``); ``scales``: the largest ``|value|`` of conv1's and of conv2's units."""

    tape: Tensor
    margin: Tensor
    value: Tensor
    scales: tuple[float, float]

    def uncertain(self, bound: float) -> Tensor:
        """Bool ``[N, 12288]``: units whose entry arithmetic within ``bound x scale`` per member may change -- ``|max + bias| < bound
        scale`` (dead or not), or a live unit whose top-2 margin is below ``2 bound scale`` (which member; a unit that is dead beyond
        the bound is code 4 whichever member is largest)."""
        scale = torch.cat([torch.full((TAPE_CONV1,), self.scales[0], dtype=torch.float64), torch.full((FEATURES,), self.scales[1], dtype=torch.float64)])
        return (self.value.abs() < bound * scale) | ((self.value > 0) & (self.margin < 2.0 * bound * scale))


def dropout_mask_reference(seed: int, step: int, rows: int | Tensor, units: int = HIDDEN, p: float = 0.5) -> Tensor:
    """Bool ``[rows, units]`` on the host: the keep-mask of optimizer step ``step`` in exact integers.  ``rows``: a count (rows
    0 .. rows - 1) or a vector of global row numbers."""
    r = np.arange(int(rows), dtype=np.int64) if isinstance(rows, int) else np.asarray(torch.as_tensor(rows).cpu(), dtype=np.int64)
    if not 0.0 <= p < 1.0:
        msg = f"the dropout rate lies in [0, 1), got {p}"
        raise ValueError(msg)
    if p == 0.0:
        return torch.ones(r.shape[0], units, dtype=torch.bool)
    j = np.arange(units, dtype=np.int64)
    words = philox4x32_10(((j >> 2)[None, :], (r & _M32)[:, None], int(step) & _M32, 0), stream_key(seed, DROPOUT_STREAM))
    w = np.choose((j & 3)[None, :], [np.broadcast_to(x, (r.shape[0], units)) for x in words])
    u = (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return torch.from_numpy(u >= float(np.float32(p)))


def _windows(c: Tensor) -> Tensor:
    """``[N, C, H, W] -> [N, C, H/2, W/2, 4]``: the members ``2 dy + dx`` of every 2 x 2 pool window."""
    n, ch, h, w = c.shape
    return c.reshape(n, ch, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, ch, h // 2, w // 2, 4)


def _choices(c: Tensor) -> tuple[Tensor, Tensor, Tensor]:
    """Of a biased conv output: ``(code uint8, top-2 margin, max)`` per pooled unit."""
    win = _windows(c)
    top = win.max(dim=-1, keepdim=True).values
    first = (win == top).to(torch.int8).argmax(-1)  # (the first maximum)
    top2 = win.topk(2, dim=-1).values
    value = top.squeeze(-1)
    code = torch.where(value <= 0, torch.full_like(first, DEAD), first).to(torch.uint8)
    return code, top2[..., 0] - top2[..., 1], value


def _pool_by_tape(c: Tensor, codes: Tensor) -> Tensor:
    """``pool2(relu(c))`` with the choices imposed: the named member of each window, 0 for a dead unit."""
    win = _windows(c)
    idx = codes.to(torch.int64).clamp(max=3).unsqueeze(-1)
    return torch.where(codes < DEAD, win.gather(-1, idx).squeeze(-1), torch.zeros((), dtype=c.dtype, device=c.device))


@torch.no_grad()
def tape_reference(classifier: DigitClassifier, frames_raw: Tensor, act: int = 0, select: Tensor | None = None) -> TapeReference:
    """The tape in float64, with the margins that tell which of its entries a kernel within a given error bound must reproduce."""
    x = DigitClassifier.images(frames_raw.double(), act, select)
    c1 = F.conv2d(x, classifier.conv1.weight.double(), classifier.conv1.bias.double(), padding=1)
    code1, margin1, value1 = _choices(c1)
    c2 = F.conv2d(F.max_pool2d(F.relu(c1), 2, 2), classifier.conv2.weight.double(), classifier.conv2.bias.double(), padding=1)
    code2, margin2, value2 = _choices(c2)
    n = x.shape[0]
    cat = lambda a, b: torch.cat([a.reshape(n, TAPE_CONV1), b.reshape(n, FEATURES)], dim=1)  # noqa: E731
    return TapeReference(cat(code1, code2).contiguous(), cat(margin1, margin2), cat(value1, value2),
                         (float(value1.abs().max()), float(value2.abs().max())))


def _check_labels(labels: Tensor, n: int, device: torch.device) -> None:
    if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or labels.device != device:
        msg = f"labels must be an int32 tensor of shape ({n},) on {device}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}"
        raise ValueError(msg)


def _workspace(need: int, device: torch.device, given: Tensor | None) -> Tensor:
    if given is not None and given.numel() * given.element_size() >= need and given.device == device:
        return given
    return torch.empty((need + 7) // 8, dtype=torch.float64, device=device)


@torch.no_grad()
def features_train(classifier: DigitClassifier, frames_raw: Tensor, act: int = 0, select: Tensor | None = None, *, out: Tensor | None = None,
                   tape: Tensor | None = None) -> tuple[Tensor, Tensor]:
    """One ``mtrssm_digit_features_train`` launch: ``(features fp32 [N, 4096], tape uint8 [N, 12288])``; the features are bit-identical
    to ``classifier.features``.  ``out`` / ``tape``: contiguous buffers of at least ``N`` rows to write into."""
    frames = DigitClassifier._frames(frames_raw, select).contiguous()  # noqa: SLF001
    n = frames.shape[0] if select is None else select.numel()
    if out is None:
        out = torch.empty(n, FEATURES, device=frames.device, dtype=torch.float32)
    if tape is None:
        tape = torch.empty(n, TAPE, device=frames.device, dtype=torch.uint8)
    if out.shape[0] < n or out.shape[1:] != (FEATURES,) or not out.is_contiguous() or tape.shape[0] < n or tape.shape[1:] != (TAPE,) or \
            not tape.is_contiguous() or tape.dtype != torch.uint8 or not tape.is_cuda:
        msg = f"out must be a contiguous fp32 [>= {n}, {FEATURES}] and tape a contiguous uint8 [>= {n}, {TAPE}] GPU buffer"
        raise ValueError(msg)
    w1, b1, w2, b2 = (q.detach().contiguous() for q in (classifier.conv1.weight, classifier.conv1.bias, classifier.conv2.weight, classifier.conv2.bias))
    sel = None if select is None else select.contiguous()
    _lib.check(_lib.TIMERS.call("mtrssm_digit_features_train", _lib.load().mtrssm_digit_features_train, _lib.ptr(frames), frames.shape[0],
                                _lib.index_ptr(sel), n, int(act), _lib.ptr(w1), _lib.ptr(b1), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(out), tape.data_ptr(),
                                _lib.stream_ptr(frames.device), flops=2.0 * n * (1024 * 9 * 32 + 256 * 288 * 64),
                                nbytes=n * (4.0 * (1024 + FEATURES) + TAPE)), "mtrssm_digit_features_train")
    return out[:n], tape[:n]


@torch.no_grad()
def trunk_backward(classifier: DigitClassifier, frames_raw: Tensor, tape: Tensor, g_features: Tensor, labels: Tensor, act: int = 0,  # noqa: PLR0913
                   select: Tensor | None = None, *, grads: tuple[Tensor, Tensor, Tensor, Tensor] | None = None, accumulate: bool = False,
                   workspace: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``mtrssm_digit_trunk_bwd``: the gradients of ``conv1.weight``, ``conv1.bias``, ``conv2.weight``, ``conv2.bias`` from ``g_features
    [N, 4096]`` with the tape's choices; rows whose label is not in 0 .. 9 are skipped.  ``grads``: the four buffers to overwrite (or,
    ``accumulate``, to add to); fresh ones otherwise."""
    frames = DigitClassifier._frames(frames_raw, select).contiguous()  # noqa: SLF001
    n = frames.shape[0] if select is None else select.numel()
    _check_labels(labels, n, frames.device)
    if tape.dtype != torch.uint8 or tuple(tape.shape) != (n, TAPE) or not tape.is_contiguous() or not tape.is_cuda or tuple(g_features.shape) != (n, FEATURES):
        msg = f"tape must be a contiguous uint8 [{n}, {TAPE}] GPU tensor and g_features [{n}, {FEATURES}], got {tuple(tape.shape)} and {tuple(g_features.shape)}"
        raise ValueError(msg)
    w1, b1, w2 = (q.detach().contiguous() for q in (classifier.conv1.weight, classifier.conv1.bias, classifier.conv2.weight))
    if grads is None:
        if accumulate:
            msg = "accumulate needs the gradients to add to"
            raise ValueError(msg)
        grads = tuple(torch.empty_like(q, dtype=torch.float32) for q in (w1, b1, w2, classifier.conv2.bias.detach()))
    lib = _lib.load()
    ws = _workspace(int(lib.mtrssm_digit_trunk_bwd_workspace_bytes(n)), frames.device, workspace)
    sel = None if select is None else select.contiguous()
    _lib.check(_lib.TIMERS.call("mtrssm_digit_trunk_bwd", lib.mtrssm_digit_trunk_bwd, _lib.ptr(frames), frames.shape[0], _lib.index_ptr(sel), n, int(act),
                                tape.data_ptr(), _lib.ptr(g_features.contiguous()), _lib.index_ptr(labels.contiguous()), _lib.ptr(w1), _lib.ptr(b1),
                                _lib.ptr(w2), _lib.ptr(grads[0]), _lib.ptr(grads[1]), _lib.ptr(grads[2]), _lib.ptr(grads[3]), int(bool(accumulate)),
                                ws.data_ptr(), ws.numel() * ws.element_size(), _lib.stream_ptr(frames.device), flops=2.0 * n * 2 * 4096 * 288,
                                nbytes=n * (4.0 * (1024 + FEATURES) + TAPE)), "mtrssm_digit_trunk_bwd")
    return grads


class HeadStep(NamedTuple):
    """``stats`` fp32 ``[3]`` (sum nll, sum hit, live count), ``g_hidden [N, 128]``, fc2's gradients, and the per-row ``nll`` / ``pred``
    planes (None unless asked for)."""

    stats: Tensor
    g_hidden: Tensor
    g_weight: Tensor
    g_bias: Tensor
    nll: Tensor | None
    pred: Tensor | None


@torch.no_grad()
def head_train(hidden: Tensor, weight: Tensor, bias: Tensor, labels: Tensor, *, rows: Tensor | None = None, step: int = 0,  # noqa: PLR0913
               key: tuple[int, int] = (0, 0), p: float = 0.0, normalize: bool = True, g_hidden: Tensor | None = None, g_weight: Tensor | None = None,
               g_bias: Tensor | None = None, accumulate: bool = False, planes: bool = False, workspace: Tensor | None = None) -> HeadStep:
    """``mtrssm_digit_head_train`` on ``hidden [>= N, 128]`` (fc1's activated output), N = ``labels.numel()``."""
    n = labels.numel()
    _check_labels(labels, n, hidden.device)
    if hidden.dim() != 2 or hidden.shape[0] < n or hidden.shape[1] != HIDDEN or not hidden.is_contiguous():  # noqa: PLR2004
        msg = f"hidden must be a contiguous [>= {n}, {HIDDEN}] tensor, got {tuple(hidden.shape)}"
        raise ValueError(msg)
    dev = hidden.device
    g_hidden = torch.empty(n, HIDDEN, device=dev, dtype=torch.float32) if g_hidden is None else g_hidden
    if g_weight is None or g_bias is None:
        if accumulate:
            msg = "accumulate needs the gradients to add to"
            raise ValueError(msg)
        g_weight, g_bias = torch.empty(CLASSES, HIDDEN, device=dev, dtype=torch.float32), torch.empty(CLASSES, device=dev, dtype=torch.float32)
    stats = torch.empty(3, device=dev, dtype=torch.float32)
    nll = torch.empty(n, device=dev, dtype=torch.float32) if planes else None
    pred = torch.empty(n, device=dev, dtype=torch.int32) if planes else None
    lib = _lib.load()
    ws = _workspace(int(lib.mtrssm_digit_head_train_workspace_bytes(n)), dev, workspace)
    _lib.check(_lib.TIMERS.call("mtrssm_digit_head_train", lib.mtrssm_digit_head_train, _lib.ptr(hidden), _lib.ptr(weight.detach().contiguous()),
                                _lib.ptr(bias.detach().contiguous()), _lib.index_ptr(labels.contiguous()), _lib.index_ptr(None if rows is None else rows.contiguous()),
                                n, 0, int(step), int(key[0]), int(key[1]), float(p), int(bool(normalize)), _lib.ptr(nll), _lib.index_ptr(pred), _lib.ptr(stats),
                                _lib.ptr(g_hidden), _lib.ptr(g_weight), _lib.ptr(g_bias), int(bool(accumulate)), ws.data_ptr(), ws.numel() * ws.element_size(),
                                _lib.stream_ptr(dev), flops=6.0 * n * HIDDEN * CLASSES, nbytes=8.0 * n * HIDDEN), "mtrssm_digit_head_train")
    return HeadStep(stats, g_hidden, g_weight, g_bias, nll, pred)


def _trunk(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, tape: Tensor | None) -> Tensor:
    """``[N, 4096]`` features of images ``x``; ``tape`` imposes the pool and ReLU choices (None: torch's own)."""
    n = x.shape[0]
    c1 = F.conv2d(x, w1, b1, padding=1)
    if tape is None:
        p1 = F.max_pool2d(F.relu(c1), 2, 2)
        return F.max_pool2d(F.relu(F.conv2d(p1, w2, b2, padding=1)), 2, 2).reshape(n, FEATURES)
    if tape.dtype != torch.uint8 or tuple(tape.shape) != (n, TAPE):
        msg = f"tape must be uint8 [{n}, {TAPE}], got {tape.dtype} {tuple(tape.shape)}"
        raise ValueError(msg)
    tape = tape.to(x.device)
    p1 = _pool_by_tape(c1, tape[:, :TAPE_CONV1].reshape(n, 32, 16, 16))
    return _pool_by_tape(F.conv2d(p1, w2, b2, padding=1), tape[:, TAPE_CONV1:].reshape(n, 64, 8, 8)).reshape(n, FEATURES)


def trunk_rule(classifier: DigitClassifier, frames_raw: Tensor, labels: Tensor, g_features: Tensor, act: int = 0, select: Tensor | None = None,  # noqa: PLR0913
               tape: Tensor | None = None) -> list[Tensor]:
    """What ``mtrssm_digit_trunk_bwd`` computes, in float64: the gradients of ``sum(g_features * features)`` over the live rows with
    respect to ``conv1.weight``, ``conv1.bias``, ``conv2.weight``, ``conv2.bias``."""
    x = DigitClassifier.images(frames_raw.double(), act, select)
    live = (labels >= 0) & (labels < CLASSES)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    x = torch.where(live[:, None, None, None], x, zero)
    params = [dict(classifier.named_parameters())[k].detach().to(torch.float64).requires_grad_(True) for k in PARAMETERS[:4]]
    with torch.enable_grad():
        f = _trunk(x, *params, tape)
        total = (torch.where(live[:, None], g_features.to(torch.float64), zero) * f).sum()
        grads = torch.autograd.grad(total, params, allow_unused=True)
    return [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params, strict=True)]


def head_rule(hidden: Tensor, weight: Tensor, bias: Tensor, labels: Tensor, keep: Tensor | None = None, p: float = 0.0,  # noqa: PLR0913
              normalize: bool = True) -> HeadStep:
    """What ``mtrssm_digit_head_train`` computes, in float64 (both planes included)."""
    h = hidden.detach().to(torch.float64)[: labels.numel()]
    live = (labels >= 0) & (labels < CLASSES)
    zero = torch.zeros((), dtype=torch.float64, device=h.device)
    m = torch.ones_like(h) if keep is None else keep.to(h.device).to(torch.float64) / (1.0 - float(np.float32(p)))
    w, b = weight.detach().to(torch.float64), bias.detach().to(torch.float64)
    hd = h * m
    z = hd @ w.T + b
    lab = labels.clamp(0, CLASSES - 1).to(torch.int64)
    nll = torch.where(live, torch.logsumexp(z, dim=1) - z.gather(1, lab[:, None]).squeeze(1), zero)
    first = DigitClassifier.first_max(z)
    pred = torch.where(live, first, torch.full_like(first, -1))
    count = live.sum().to(torch.float64)
    d = torch.where(live[:, None], torch.softmax(z, dim=1) - F.one_hot(lab, CLASSES).to(torch.float64), zero)
    if normalize:
        d = d / count.clamp_min(1.0)
    g_hidden = (d @ w) * m * (h > 0)
    stats = torch.stack([nll.sum(), (live & (first.to(torch.int64) == lab)).sum().to(torch.float64), count])
    return HeadStep(stats, g_hidden, d.T @ hd, d.sum(0), nll, pred)


class DigitTrainer:
    """``DigitTrainer(classifier, lr=1e-3, dropout=0.5, seed=0, weight_decay=0.0)``: turns the classifier's eight parameters trainable,
    re-homes them in one flat buffer and steps them with Adam (``FlatAdamW`` without clipping on the GPU, ``torch.optim.Adam``
    elsewhere).  ``close()``, or leaving the ``with`` block, freezes the classifier again and returns it to ``eval()``."""

    def __init__(self, classifier: DigitClassifier, lr: float = 1e-3, dropout: float = 0.5, seed: int = 0, weight_decay: float = 0.0) -> None:
        if not isinstance(classifier, DigitClassifier):
            msg = f"DigitTrainer trains a DigitClassifier, got {type(classifier).__name__}"
            raise TypeError(msg)
        if not 0.0 <= dropout < 1.0:
            msg = f"the dropout rate lies in [0, 1), got {dropout}"
            raise ValueError(msg)
        from multimodal_mtrssm_amd.optim import FlatAdamW, FlatParameters  # noqa: PLC0415  (optim imports the scan stack)

        self.classifier = classifier
        self.dropout, self.seed = float(dropout), int(seed)
        self.key = stream_key(self.seed, DROPOUT_STREAM)
        self.steps = 0          # optimizer steps taken: the dropout masks' step word
        self.epochs = 0         # epochs begun by fit: the permutations' seed word
        classifier.requires_grad_(True)
        classifier.train()
        self.device = classifier.conv1.weight.device
        self.flat = FlatParameters(classifier, extra=4)
        if self.device.type == "cuda":
            for i in range(len(self.flat.params)):  # the kernels write the gradient views themselves: no autograd hook ever fires
                self.flat.mark_touched(i)
            self.opt = FlatAdamW(self.flat, lr=lr, weight_decay=weight_decay, clip_norm=0.0)
        else:
            self.opt = torch.optim.Adam(list(classifier.parameters()), lr=lr, weight_decay=weight_decay)
        self._work: dict[str, Tensor] = {}
        self._closed = False

    def __enter__(self) -> DigitTrainer:
        return self

    def __exit__(self, *exc: object) -> None:
        self.close()

    def close(self) -> None:
        """Freeze the classifier (its parameters leave the flat buffer for storage of their own) and return it to ``eval()``."""
        if self._closed:
            return
        self._closed = True
        for h in self.flat._hooks:  # noqa: SLF001
            if h is not None:
                h.remove()
        with torch.no_grad():
            for p in self.classifier.parameters():
                p.data = p.data.clone()
                p.grad = None
        self.classifier.requires_grad_(False)
        self.classifier.eval()
        self._work.clear()

    # -- the rule in torch, in float64 ---------------------------------------------------------------------------------------------------
    @staticmethod
    def rule(classifier, frames_raw: Tensor, labels: Tensor, keep: Tensor | None = None, p: float = 0.0, act: int = 0,  # noqa: ANN001, PLR0913
             select: Tensor | None = None, tape: Tensor | None = None, normalize: bool = True) -> tuple[Tensor, DigitStats, list[Tensor]]:
        """One step's loss, stats and the eight gradients (``PARAMETERS`` order) in float64, on ``frames_raw``'s device.  ``labels`` int32
        ``[N]``: one per row (after ``select``).  ``keep`` bool ``[N, 128]`` is the dropout mask (None: everything is kept), scaled by
        ``1 / (1 - p)``.  ``tape`` uint8 ``[N, 12288]`` imposes the pool and ReLU choices (None: torch's own).  ``normalize``: the mean
        over the live rows, else the sum."""
        x = DigitClassifier.images(frames_raw.double(), act, select)
        n = x.shape[0]
        _check_labels(labels, n, x.device)
        live = (labels >= 0) & (labels < CLASSES)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        x = torch.where(live[:, None, None, None], x, zero)  # a dead row is not read
        params = [dict(classifier.named_parameters())[k].detach().to(torch.float64).requires_grad_(True) for k in PARAMETERS]
        w1, b1, w2, b2, wf1, bf1, wf2, bf2 = params
        with torch.enable_grad():
            f = _trunk(x, w1, b1, w2, b2, tape)
            h = F.relu(F.linear(f.reshape(n, FEATURES), wf1, bf1))
            if keep is not None:
                h = h * (keep.to(x.device).to(torch.float64) / (1.0 - float(np.float32(p)) if p else 1.0))
            z = F.linear(h, wf2, bf2)
            lab = labels.clamp(0, CLASSES - 1).to(torch.int64)
            nll = torch.where(live, torch.logsumexp(z, dim=1) - z.gather(1, lab[:, None]).squeeze(1), zero)
            count = live.sum().to(torch.float64)
            loss = nll.sum() / count.clamp_min(1.0) if normalize else nll.sum()
            grads = torch.autograd.grad(loss, params, allow_unused=True)
        grads = [torch.zeros_like(q) if g is None else g for g, q in zip(grads, params, strict=True)]
        hits = (live & (DigitClassifier.first_max(z.detach()).to(torch.int64) == lab)).sum().to(torch.float64)
        return loss.detach(), DigitStats(nll.detach().sum(), hits, count), grads

    # -- one optimizer step --------------------------------------------------------------------------------------------------------------
    def _buffer(self, name: str, shape: tuple[int, ...], dtype: torch.dtype) -> Tensor:
        t = self._work.get(name)
        if t is None or tuple(t.shape) != shape or t.dtype != dtype:
            t = self._work[name] = torch.empty(shape, device=self.device, dtype=dtype)
        return t

    def _workspace(self, name: str, need: int) -> Tensor:
        t = self._work.get(name)
        if t is None or t.numel() * 8 < need:
            t = self._work[name] = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
        return t

    def _grads_gpu(self, frames_raw: Tensor, labels: Tensor, act: int, select: Tensor | None, rows: Tensor | None, normalize: bool) -> DigitStats:  # noqa: PLR0913
        """The launches of one step's forward and backward: the eight flat gradient views and the stats (device tensors)."""
        clf, flat = self.classifier, self.flat
        n = labels.numel()
        pad = -(-n // _TILE_ROWS) * _TILE_ROWS if 2.0 * n * HIDDEN * FEATURES >= linear.SPLIT_MIN_FLOPS else n  # whole tiles for the tile GEMM
        feats = self._buffer("features", (pad, FEATURES), torch.float32)
        if pad > n:
            feats[n:].zero_()
        par = {k: v.detach() for k, v in clf.named_parameters()}
        grad = {k: v.grad for k, v in clf.named_parameters()}
        flat.zero_grad()  # fc1's gradients are accumulated by the GEMM; the others are overwritten
        _, tape = features_train(clf, frames_raw, act, select, out=feats, tape=self._buffer("tape", (n, TAPE), torch.uint8))
        h = clf.hidden(feats)
        lib = _lib.load()
        head = head_train(h, par["fc2.weight"], par["fc2.bias"], labels, rows=rows, step=self.steps, key=self.key, p=self.dropout, normalize=normalize,
                          g_hidden=self._buffer("g_hidden", (n, HIDDEN), torch.float32), g_weight=grad["fc2.weight"], g_bias=grad["fc2.bias"],
                          workspace=self._workspace("head_ws", int(lib.mtrssm_digit_head_train_workspace_bytes(n))))
        # fc1: dW += g_hidden^T f, db += column sums, in ONE reduction slice (a split reduction meets in fp32 atomics, whose order changes
        # from run to run); g_features = g_hidden W
        linear.gemm(head.g_hidden, feats[:n], grad["fc1.weight"], a_rmajor=True, b_rmajor=True, colsum=grad["fc1.bias"], accumulate=True, split_r=1)
        g_feat = self._buffer("g_features", (n, FEATURES), torch.float32)
        linear.gemm(head.g_hidden, par["fc1.weight"], g_feat, a_rmajor=False, b_rmajor=True)
        trunk_backward(clf, frames_raw, tape, g_feat, labels, act, select,
                       grads=(grad["conv1.weight"], grad["conv1.bias"], grad["conv2.weight"], grad["conv2.bias"]),
                       workspace=self._workspace("trunk_ws", int(lib.mtrssm_digit_trunk_bwd_workspace_bytes(n))))
        return DigitStats(head.stats[0], head.stats[1], head.stats[2])

    def _grads_host(self, frames_raw: Tensor, labels: Tensor, act: int, select: Tensor | None, rows: Tensor | None, normalize: bool) -> DigitStats:  # noqa: PLR0913
        n = labels.numel()
        keep = None
        if self.dropout > 0.0:
            keep = dropout_mask_reference(self.seed, self.steps, n if rows is None else rows, HIDDEN, self.dropout)
        _, stats, grads = DigitTrainer.rule(self.classifier, frames_raw, labels, keep, self.dropout, act, select, None, normalize)
        for p, g in zip((dict(self.classifier.named_parameters())[k] for k in PARAMETERS), grads, strict=True):
            p.grad.copy_(g)
        return DigitStats(*(s.to(torch.float32) for s in stats))

    @torch.no_grad()
    def _step(self, frames_raw: Tensor, labels: Tensor, act: int, select: Tensor | None, rows: Tensor | None, group) -> DigitStats:  # noqa: ANN001, PLR0913
        """``labels`` int32 ``[N]`` per row (after ``select``); ``rows`` int32 ``[N]``: the rows' global numbers (None: 0 .. N - 1)."""
        if self._closed:
            msg = "this DigitTrainer is closed"
            raise RuntimeError(msg)
        if act not in (0, 3):
            msg = f"act must be 0 (Identity) or 3 (Tanh), got {act}"
            raise ValueError(msg)
        frames = DigitClassifier._frames(frames_raw, select)  # noqa: SLF001
        n = frames.shape[0] if select is None else select.numel()
        if frames_raw.device != self.device:
            msg = f"the frames are on {frames_raw.device}, the classifier on {self.device}"
            raise ValueError(msg)
        _check_labels(labels, n, self.device)
        if rows is not None and (rows.dtype != torch.int32 or tuple(rows.shape) != (n,)):
            msg = f"rows must be an int32 vector of {n} global row numbers, got {rows.dtype} {tuple(rows.shape)}"
            raise ValueError(msg)
        shared = group is not None
        grads = self._grads_gpu if self.device.type == "cuda" else self._grads_host
        stats = grads(frames_raw, labels.contiguous(), act, select, None if rows is None else rows.contiguous(), not shared)
        if shared:  # sums, the stats in the flat buffer's tail: ONE all-reduce, then the division by the global live count
            import torch.distributed as dist  # noqa: PLC0415

            self.flat.tail[:3].copy_(torch.stack(list(stats)))
            dist.all_reduce(self.flat.grad_full, op=dist.ReduceOp.SUM, group=group)
            total = self.flat.tail[:3].clone()
            self.flat.grad /= total[2].clamp_min(1.0)
            stats = DigitStats(total[0], total[1], total[2])
        else:
            stats = DigitStats(*(s.clone() for s in stats))
        if self.device.type == "cuda":
            self.opt.step(check=False)
        else:
            self.opt.step()
        self.steps += 1
        return stats

    def step(self, frames_raw: Tensor, labels: Tensor, act: int = 0, select: Tensor | None = None, group=None, row0: int = 0) -> DigitStats:  # noqa: ANN001, PLR0913
        """One optimizer step on the mean loss of the rows ``select`` picks (None: every frame).  ``labels`` int32: one per FRAME of
        ``frames_raw``.  Under ``group`` the rows are sharded: ``row0`` is the global number of this rank's frame 0, the gradients and stats
        are all-reduced as sums and divided by the global live count; the returned stats are the global ones."""
        frames = DigitClassifier._frames(frames_raw, select)  # noqa: SLF001
        _check_labels(labels, frames.shape[0], frames_raw.device)
        rows = None
        if select is not None:
            labels = labels[select.long()]
            rows = select + row0 if row0 else select
        elif row0:
            rows = torch.arange(row0, row0 + frames.shape[0], dtype=torch.int32, device=frames_raw.device)
        return self._step(frames_raw, labels, act, select, rows, group)

    @torch.no_grad()
    def evaluate(self, frames_raw: Tensor, labels: Tensor, act: int = 0) -> DigitStats:
        """Dropout off, through the classifier's own ``read``: the stats of the live frames."""
        frames = DigitClassifier._frames(frames_raw, None)  # noqa: SLF001
        _check_labels(labels, frames.shape[0], frames_raw.device)
        digit, logits = self.classifier.read(frames_raw, act)
        live = (labels >= 0) & (labels < CLASSES)
        lab = labels.clamp(0, CLASSES - 1).to(torch.int64)
        z = logits.to(torch.float32)
        nll = torch.where(live, torch.logsumexp(z, dim=1) - z.gather(1, lab[:, None]).squeeze(1), torch.zeros((), device=z.device))
        return DigitStats(nll.sum(), (live & (digit.to(torch.int64) == lab)).sum().to(torch.float32), live.sum().to(torch.float32))

    @torch.no_grad()
    def fit(self, frames_raw: Tensor, labels: Tensor, epochs: int = 5, batch_size: int = 64, act: int = 0, group=None) -> DigitStats:  # noqa: ANN001, PLR0913
        """``epochs`` passes over the rows in minibatches of ``batch_size``: per epoch one seeded permutation of the GLOBAL row numbers,
        whose slices go to the kernels as ``select`` (nothing is copied).  Under ``group`` every rank holds a contiguous shard of the rows
        (in rank order) and walks the same permutation: of each minibatch it reads its own rows and marks the others dead, so the fit over
        sharded rows is the fit over all rows.  Returns the sums of the last epoch's stats (taken before each update)."""
        for name, value in (("epochs", epochs), ("batch_size", batch_size)):
            if isinstance(value, bool) or not isinstance(value, int) or value < 1:
                msg = f"{name} must be an integer >= 1, got {value!r}"
                raise ValueError(msg)
        frames = DigitClassifier._frames(frames_raw, None)  # noqa: SLF001
        local = frames.shape[0]
        _check_labels(labels, local, frames_raw.device)
        row0, total = 0, local
        if group is not None:
            import torch.distributed as dist  # noqa: PLC0415

            counts = [torch.zeros(1, dtype=torch.int64, device=self.device) for _ in range(dist.get_world_size(group))]
            dist.all_gather(counts, torch.tensor([local], dtype=torch.int64, device=self.device), group=group)
            counts = [int(c) for c in counts]
            row0, total = sum(counts[: dist.get_rank(group)]), sum(counts)
        sums = None
        for _ in range(epochs):
            gen = torch.Generator().manual_seed((self.seed * 1000003 + self.epochs) & 0x7FFFFFFFFFFFFFFF)
            perm = torch.randperm(total, generator=gen).to(torch.int32).to(self.device)
            self.epochs += 1
            sums = torch.zeros(3, device=self.device, dtype=torch.float32)
            for lo in range(0, total, batch_size):
                rows = perm[lo : lo + batch_size]
                if group is None:
                    select, batch_labels = rows, labels[rows.long()]
                else:
                    mine = (rows >= row0) & (rows < row0 + local)
                    select = torch.where(mine, rows - row0, torch.zeros_like(rows))
                    batch_labels = torch.where(mine, labels[select.long()], torch.full_like(rows, -1))
                sums += torch.stack(list(self._step(frames_raw, batch_labels, act, select, rows, group)))
        return DigitStats(sums[0], sums[1], sums[2])


__all__ = ["DigitStats", "DigitTrainer", "HeadStep", "TapeReference", "dropout_mask_reference", "features_train", "head_rule", "head_train",
           "tape_reference", "trunk_backward", "trunk_rule"]
