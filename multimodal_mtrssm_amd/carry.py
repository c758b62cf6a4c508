"""Carried state for training on whole episodes chunk by chunk (truncated BPTT).

``StateCarry`` owns fixed device buffers for the posterior state the previous chunk ended with -- MRSSM ``deter [B, D]``,
``stoch [B, S]``; MMTRSSM ``deter_l, deter_h, stoch_l, stoch_h, hidden_l, hidden_h`` -- one set per step prefix (``"train"``,
``"val"``), and a host flag per set saying whether it holds anything.  A step with a carry runs

    state0 = select(reset, fresh, carry)        ``mtrssm_state_select``: ``state0[b] = reset[b] ? fresh[b] : carry[b]``
    ... rollout, decoders, loss as always ...
    carry  = posterior at t = T - 1, detached   ``mtrssm_state_save``

``reset`` (bool ``[B]``) is read on the device, so the launch sequence is the same whether a row starts an episode or
continues one and ONE captured graph serves every chunk (``graph.CapturedTrainStep(state_carry=...)``).  Gradients stop at the
chunk border: the select's backward hands ``reset[b] ? g[b] : 0`` to the fresh state and nothing to the carry.

``select_reference`` / ``select_backward_reference`` / ``save_reference`` restate the two kernels in torch; ``save_at_reference`` the
save of a ragged batch (``mtrssm_state_save_at``, DESIGN.md section 6d: each row's LAST LIVE step, an empty row keeps its carry).
"""

from __future__ import annotations

import ctypes as C

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.distributions import MultiOneHot
from multimodal_mtrssm_amd.state import MTState, State

PREFIXES = ("train", "val")
MRSSM_FIELDS = ("deter", "stoch")
MMTRSSM_FIELDS = ("deter_l", "deter_h", "stoch_l", "stoch_h", "hidden_l", "hidden_h")


def select_reference(reset: Tensor, fresh: Tensor, carry: Tensor) -> Tensor:
    """``state0[b] = reset[b] ? fresh[b] : carry[b]`` (rows of ``[B, W]`` tensors)."""
    return torch.where(reset.reshape(-1, 1), fresh, carry)


def select_backward_reference(reset: Tensor, grad: Tensor) -> Tensor:
    """Gradient of the fresh state: ``reset[b] ? g[b] : 0``; the carry gets none."""
    return torch.where(reset.reshape(-1, 1), grad, torch.zeros_like(grad))


def save_reference(last: Tensor) -> Tensor:
    """``carry[b] = last[b, T - 1]`` for a scan output ``[B, T, W]``."""
    return last[:, -1].detach().clone()


def save_at_reference(out: Tensor, last: Tensor, carry: Tensor) -> Tensor:
    """``carry[b] = out[b, last[b]]`` for ``0 <= last[b] < T`` (``out``: a scan output ``[B, T, W]``); other rows keep ``carry[b]``."""
    steps = out.shape[1]
    at = last.to(torch.long)
    ok = (at >= 0) & (at < steps)
    rows = out.detach()[torch.arange(out.shape[0], device=out.device), at.clamp(0, steps - 1)]
    return torch.where(ok.reshape(-1, 1), rows, carry)


def _table(entries: list[tuple[Tensor, Tensor | None, Tensor]]) -> C.Structure:
    """``MtrssmStateTable`` of ``(src, alt, dst)`` entries.  ``src`` is ``[B, W]`` with unit column stride and any row stride
    (select) or a contiguous ``[B, T, W]`` (save); ``alt`` and ``dst`` are contiguous ``[B, W]``."""
    if not 0 < len(entries) <= _lib.STATE_MAX:
        msg = f"a state table holds 1 .. {_lib.STATE_MAX} tensors, got {len(entries)}"
        raise ValueError(msg)
    table = _lib.StateTable()
    table.count = len(entries)
    for k, (src, alt, dst) in enumerate(entries):
        table.width[k] = dst.shape[-1]
        table.src_stride[k] = src.stride(0)
        table.src[k] = _lib.raw_ptr(src)
        table.alt[k] = _lib.ptr(alt)
        table.dst[k] = _lib.ptr(dst)
    table._refs = entries  # noqa: SLF001  (keeps temporaries alive until the launch is enqueued, as _lib.fill)
    return table


def _rows(t: Tensor) -> Tensor:
    """A float32 ``[B, W]`` view the select kernel can read: unit column stride, rows a fixed number of floats apart."""
    t = t.float()
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:  # noqa: PLR2004
        t = t.contiguous()
    return t


def select_launch(reset: Tensor, fresh: list[Tensor], carry: list[Tensor | None]) -> list[Tensor]:
    """One ``mtrssm_state_select`` launch on torch's current stream (``carry[k]`` None: zeros, the backward form)."""
    if reset.dtype != torch.bool or reset.dim() != 1 or not reset.is_contiguous():
        msg = f"reset must be a contiguous bool [B] tensor, got {reset.dtype} {tuple(reset.shape)}"
        raise ValueError(msg)
    fresh = [_rows(f) for f in fresh]
    for f, c in zip(fresh, carry, strict=True):  # the kernel trusts these extents
        if f.dim() != 2 or f.shape[0] != reset.numel() or (c is not None and tuple(c.shape) != tuple(f.shape)):  # noqa: PLR2004
            msg = f"state_select: fresh {tuple(f.shape)}, carry {None if c is None else tuple(c.shape)}, reset [{reset.numel()}] do not match"
            raise ValueError(msg)
    out =[torch.empty(f.shape, device=f.device, dtype=torch.float32) for f in fresh]
    table = _table(list(zip(fresh, carry, out, strict=True)))
    dev = fresh[0].device
    _lib.check(_lib.load().mtrssm_state_select(C.byref(table), _lib.raw_ptr(reset), reset.numel(), _lib.stream_ptr(dev)), "mtrssm_state_select")
    return out


def save_launch(last: list[Tensor], carry: list[Tensor], at: Tensor | None = None) -> None:
    """One ``mtrssm_state_save`` launch on torch's current stream: ``carry[k][b] = last[k][b, T - 1]``, read in place.  ``at`` (int32
    ``[B]`` on the device): ``mtrssm_state_save_at`` instead, ``carry[k][b] = last[k][b, at[b]]`` where ``0 <= at[b] < T``."""
    b, steps = last[0].shape[:2]
    if at is not None and (at.dtype != torch.int32 or tuple(at.shape) != (b,)):
        msg = f"state_save_at: last must be int32 [{b}], got {at.dtype} {tuple(at.shape)}"
        raise ValueError(msg)
    srcs = []
    for t, c in zip(last, carry, strict=True):
        if t.dim() != 3 or tuple(t.shape[:2]) != (b, steps) or tuple(c.shape) != (b, t.shape[2]):  # noqa: PLR2004
            msg = f"state_save: scan output {tuple(t.shape)} does not match the carry {tuple(c.shape)} of {b} rows x {steps} steps"
            raise ValueError(msg)
        srcs.append(t.detach())
        _lib.ptr(srcs[-1])  # (contiguous fp32 on the GPU, or MtrssmLibraryError)
    table = _table([(s, None, c) for s, c in zip(srcs, carry, strict=True)])
    if at is None:
        _lib.check(_lib.load().mtrssm_state_save(C.byref(table), b, steps, _lib.stream_ptr(carry[0].device)), "mtrssm_state_save")
    else:
        _lib.check(_lib.load().mtrssm_state_save_at(C.byref(table), _lib.index_ptr(at.contiguous()), b, steps, _lib.stream_ptr(carry[0].device)),
                   "mtrssm_state_save_at")


class _StateSelect(torch.autograd.Function):
    """``state0 = select(reset, fresh, carry)`` for all tensors of a state in one launch each way."""

    @staticmethod
    def forward(ctx, reset: Tensor, n: int, *tensors: Tensor):  # noqa: ANN001, ANN205
        ctx.set_materialize_grads(False)
        fresh, carry = list(tensors[:n]), list(tensors[n:])
        ctx.reset = reset
        return tuple(select_launch(reset, fresh, carry))

    @staticmethod
    def backward(ctx, *grads):  # noqa: ANN001, ANN205
        n = len(grads)
        live = [k for k, g in enumerate(grads) if g is not None and ctx.needs_input_grad[2 + k]]
        res: list[Tensor | None] = [None] * n
        if live:
            got = select_launch(ctx.reset, [grads[k] for k in live], [None] * len(live))
            for k, g in zip(live, got, strict=True):
                res[k] = g
        return (None, None, *res, *([None] * n))


class StateCarry:
    """The carried state of ``batch`` rows on ``device``: ``widths`` maps each state tensor's name to its width (``for_model``
    reads them off a model).  ``categoricals`` (name of a stoch tensor -> ``(K, C)``) shapes the distributions of ``last``."""

    def __init__(self, widths: dict[str, int], batch: int, device: torch.device | str = "cuda",
                 categoricals: dict[str, tuple[int, int]] | None = None) -> None:
        names = tuple(widths)
        if set(names) not in (set(MRSSM_FIELDS), set(MMTRSSM_FIELDS)):
            msg = f"widths must name {MRSSM_FIELDS} (MRSSM) or {MMTRSSM_FIELDS} (MMTRSSM), got {names}"
            raise ValueError(msg)
        if isinstance(batch, bool) or not isinstance(batch, int) or batch < 1:
            msg = f"batch must be an integer >= 1, got {batch!r}"
            raise ValueError(msg)
        self.fields = MRSSM_FIELDS if len(names) == len(MRSSM_FIELDS) else MMTRSSM_FIELDS
        self.widths = {k: int(widths[k]) for k in self.fields}
        self.batch = batch
        self.device = torch.device(device)
        self.categoricals = dict(categoricals or {})
        self.buffers = {p: {k: torch.zeros(batch, w, device=self.device, dtype=torch.float32) for k, w in self.widths.items()}
                        for p in PREFIXES}
        self.filled = dict.fromkeys(PREFIXES, False)

    @classmethod
    def for_model(cls, model: torch.nn.Module, batch: int, device: torch.device | str | None = None) -> StateCarry:
        """The carry of ``model`` (a ``MoPoE_MRSSM`` or ``MoPoE_MMTRSSM``) for ``batch`` rows, on the model's device by default."""
        dev = model.device if device is None else device
        if hasattr(model, "ld_dim"):
            ld, hd = model.l_dist, model.h_dist
            ls, hs = ld.category_size * ld.class_size, hd.category_size * hd.class_size
            widths = {"deter_l": model.ld_dim, "deter_h": model.hd_dim, "stoch_l": ls, "stoch_h": hs, "hidden_l": model.ld_dim,
                      "hidden_h": model.hd_dim}
            cats = {"stoch_l": (ld.category_size, ld.class_size), "stoch_h": (hd.category_size, hd.class_size)}
        else:
            f = model.transition.distribution_factory
            widths = {"deter": model.transition.deterministic_size, "stoch": f.category_size * f.class_size}
            cats = {"stoch": (f.category_size, f.class_size)}
        return cls(widths, batch, dev, cats)

    def __repr__(self) -> str:
        return f"StateCarry({self.widths}, batch={self.batch}, filled={self.filled})"

    # -- host rules -------------------------------------------------------------------------------
    def _set(self, prefix: str) -> dict[str, Tensor]:
        if prefix not in self.buffers:
            msg = f"prefix must be one of {PREFIXES}, got {prefix!r}"
            raise ValueError(msg)
        return self.buffers[prefix]

    def check(self, prefix: str, batch: int, reset_host: Tensor | None) -> None:
        """The host-side rules of a step, from the ``reset`` the loader made on the host (no device read-back): the batch has the
        buffers' rows, and an empty set is only entered with every row resetting.  ``reset_host`` None: the caller vouches for a
        ``reset`` it made on the device; an EMPTY set still refuses it."""
        self._set(prefix)
        if batch != self.batch:
            msg = f"the batch has {batch} rows, the carry was made for {self.batch}"
            raise ValueError(msg)
        if reset_host is not None and tuple(reset_host.shape) != (self.batch,):
            msg = f"reset must have shape ({self.batch},), got {tuple(reset_host.shape)}"
            raise ValueError(msg)
        if not self.filled[prefix] and (reset_host is None or not bool(reset_host.all())):
            msg = (f"the {prefix!r} carry is empty: its first step must reset every row (reset all True, known on the host: "
                   "EpisodeBatch.reset_host or a CPU reset=)")
            raise ValueError(msg)

    def clear(self, prefix: str | None = None) -> None:
        """Mark a set (None: both) empty; its next step must reset every row."""
        for p in PREFIXES if prefix is None else (prefix,):
            self._set(p)
            self.filled[p] = False

    # -- the two launches -------------------------------------------------------------------------
    def select(self, prefix: str, reset: Tensor, fresh: dict[str, Tensor]) -> dict[str, Tensor]:
        """``{name: reset ? fresh : carry}`` for every tensor of the state (autograd: the fresh state gets ``reset ? g : 0``)."""
        carry = self._set(prefix)
        out = _StateSelect.apply(reset, len(self.fields), *[fresh[k] for k in self.fields], *[carry[k] for k in self.fields])
        return dict(zip(self.fields, out, strict=True))

    @torch.no_grad()
    def save(self, prefix: str, tensors: dict[str, Tensor], last: Tensor | None = None) -> None:
        """``carry = tensors[:, T - 1]`` for every tensor of the state (``tensors``: the scan's ``[B, T, .]`` outputs) and mark the set
        filled.  ``last`` (int32 ``[B]`` on the device, ragged batches): ``carry[b] = tensors[b, last[b]]``, a row with ``last[b] = -1``
        keeps its carry."""
        carry = self._set(prefix)
        save_launch([tensors[k] for k in self.fields], [carry[k] for k in self.fields], last)
        self.filled[prefix] = True

    # -- snapshots (the captured step's warm-up leaves the carry as it found it) --------------------
    def snapshot(self) -> tuple[dict[str, dict[str, Tensor]], dict[str, bool]]:
        return {p: {k: v.clone() for k, v in s.items()} for p, s in self.buffers.items()}, dict(self.filled)

    @torch.no_grad()
    def restore(self, snap: tuple[dict[str, dict[str, Tensor]], dict[str, bool]]) -> None:
        for p, s in snap[0].items():
            for k, v in s.items():
                self.buffers[p][k].copy_(v)
        self.filled = dict(snap[1])

    # -- reading the carry ------------------------------------------------------------------------
    def _point_mass(self, name: str, stoch: Tensor) -> MultiOneHot:
        k, c = self.categoricals.get(name, (1, stoch.shape[-1]))
        probs = stoch.reshape(*stoch.shape[:-1], k, c)
        return MultiOneHot(probs.log(), probs)

    def last(self, prefix: str) -> State | MTState:
        """The carried state of ``prefix`` as a ``State`` / ``MTState`` (clones: later steps do not change it).  Its distributions
        are the point masses on the carried samples: the rollouts read ``deter`` / ``hidden`` / ``stoch`` only."""
        carry = self._set(prefix)
        if not self.filled[prefix]:
            msg = f"the {prefix!r} carry is empty"
            raise ValueError(msg)
        c = {k: v.clone() for k, v in carry.items()}
        if self.fields is MRSSM_FIELDS:
            return State(deter=c["deter"], distribution=self._point_mass("stoch", c["stoch"]), stoch=c["stoch"])
        return MTState(deter_h=c["deter_h"], deter_l=c["deter_l"], distribution_h=self._point_mass("stoch_h", c["stoch_h"]),
                       distribution_l=self._point_mass("stoch_l", c["stoch_l"]), hidden_h=c["hidden_h"], hidden_l=c["hidden_l"],
                       stoch_h=c["stoch_h"], stoch_l=c["stoch_l"])


__all__ = ["StateCarry", "save_at_reference", "save_reference", "select_backward_reference", "select_reference"]
