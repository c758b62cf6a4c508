"""Latent overshooting: the KL between the posterior at frame ``t0 + k`` and the prior rolled ``k`` steps open loop from the posterior
at ``t0``.

Every other objective asks the prior for ONE step in latent space; the models are used open loop for many.  ``LatentOvershoot(depth=D,
stride=s, offset=o)`` adds, per latent level (MRSSM one, MMTRSSM ``_l`` and ``_h``), the multi-step terms ``k = 2 .. D`` -- no decoder is
involved -- and reports all of ``k = 1 .. D`` by distance.

For a batch of ``T`` frames (``o <= T - 2``): ``N = (T - 2 - o) // s + 1`` starts ``t0_i = o + i * s``; overshoot row ``r = b * N + i``
starts from the closed-loop posterior state at ``(b, t0_i)`` and runs ``D`` steps with modality code 0 (posterior = prior) and no
embeddings.  Step ``j`` (0-based) is driven by ``actions[b, t0_i + 1 + j]`` (zeros past the last frame), sampled with
``u_overshoot[b, i, j, :]``, and its prior logits are the ``k = j + 1`` step prior for frame ``t = t0_i + k``.  Term ``(r, k)`` is live iff
``t < clamp(valid[b], 0, T)`` (no lengths: iff ``t < T``).  With ``lq`` / ``lp`` the log-softmax per categorical of the closed-loop
``post_logits[b, t]`` / the row's ``prior_logits[r, k - 1]`` and ``q = exp(lq)``:

    kl(r, k) = sum_cat sum_c q_c (lq_c - lp_c)          (a class with q_c = 0 adds 0; exactly 0 on a dead term)
    overshoot = world * sum_{live, k >= 2} kl / max(count, 1)

``count``: the live ``k >= 2`` terms of the GLOBAL batch, so the mean over the ranks is the global batch's term.  The ``k = 1`` terms are
the ELBO's own KL: computed and reported, never added to the loss.  The value is the KL; its gradient is weighted ``(w_prior, w_post) =
(1, 0)`` (the posterior is a fixed target), with ``balanced=True`` ``(KL_BALANCE_ALPHA, 1 - KL_BALANCE_ALPHA)`` for a model that balances
its KL, else ``(1, 1)``:  ``d kl / d prior logits = w_prior (p - q)``,  ``d kl / d posterior logits_c = w_post q_c ((lq_c - lp_c) - kl_cat)``.

``LatentOvershoot.reference`` states the rule in torch, in float64, on any device; ``mtrssm_overshoot_gather`` / ``_scatter`` /
``_kl_fwd`` / ``_kl_bwd`` (csrc/overshoot_ops.hip) are the kernels, used for GPU tensors; elsewhere the torch rules run.
"""

from __future__ import annotations

import copy
import ctypes as C
from typing import NamedTuple

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.distributions import KL_BALANCE_ALPHA
from multimodal_mtrssm_amd.skill import SumTable

_INT24 = 1 << 24


class OvershootTerms(NamedTuple):
    """``term``: the rank's overshoot scalar (differentiable); ``plane`` ``[B * N, D]``: kl per row and distance, 0 on dead terms;
    ``table`` double ``[2, D]``: per ``k = 1 .. D`` the sum and the count of the rank's live terms; ``count``: the live ``k >= 2`` terms
    of the global batch."""

    term: Tensor
    plane: Tensor
    table: Tensor
    count: Tensor


def _is_int(x: object) -> bool:
    return isinstance(x, int) and not isinstance(x, bool)


class LatentOvershoot:
    """``LatentOvershoot(depth=D, stride=s, offset=o, weight=1.0, balanced=False, detach_state=False)``: ``D >= 2`` steps open loop
    from every ``s``-th posterior state from frame ``o`` on; the term enters the loss as ``kl_coeff * weight * overshoot``.
    ``detach_state``: the start states get no gradient.  ``world`` / ``rank`` (``for_rank``) say which rows of the global batch a rank
    trains on."""

    def __init__(self, depth: int, stride: int = 1, offset: int = 0, weight: float = 1.0, balanced: bool = False,  # noqa: FBT001, FBT002, PLR0913
                 detach_state: bool = False) -> None:  # noqa: FBT001, FBT002
        if not _is_int(depth) or not 2 <= depth < _INT24:  # noqa: PLR2004
            msg = f"depth must be an integer 2 <= D < 2^24 (k = 1 is the ELBO's own KL), got {depth!r}"
            raise ValueError(msg)
        if not _is_int(stride) or not 1 <= stride < _INT24:
            msg = f"stride must be an integer 1 <= s < 2^24, got {stride!r}"
            raise ValueError(msg)
        if not _is_int(offset) or not 0 <= offset < _INT24:
            msg = f"offset must be an integer 0 <= o < 2^24, got {offset!r}"
            raise ValueError(msg)
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not float(weight) >= 0.0 or float(weight) == float("inf"):
            msg = f"weight must be a finite number >= 0, got {weight!r}"
            raise ValueError(msg)
        if not isinstance(balanced, bool) or not isinstance(detach_state, bool):
            msg = f"balanced and detach_state are booleans, got {balanced!r} and {detach_state!r}"
            raise ValueError(msg)
        self.depth, self.stride, self.offset, self.weight = depth, stride, offset, float(weight)
        self.balanced, self.detach_state = balanced, detach_state
        self.world, self.rank = 1, 0
        self.group = None  # the process group OvershootTable.all_reduce uses (FlatDataParallel.overshoot binds it)

    def __repr__(self) -> str:
        return (f"LatentOvershoot(depth={self.depth}, stride={self.stride}, offset={self.offset}, weight={self.weight}, "
                f"balanced={self.balanced}, detach_state={self.detach_state})")

    def for_rank(self, world: int, rank: int) -> LatentOvershoot:
        """A copy bound to rank ``rank`` of ``world`` (``FlatDataParallel.overshoot`` calls this)."""
        if world < 1 or not 0 <= rank < world:
            msg = f"need 0 <= rank < world, got rank {rank}, world {world}"
            raise ValueError(msg)
        bound = copy.copy(self)
        bound.world, bound.rank = int(world), int(rank)
        return bound

    # -- geometry ----------------------------------------------------------------------------------------------------------------------
    def rows(self, steps: int) -> int:
        """``N = (T - 2 - o) // s + 1``: the starts of a row of ``steps`` frames (``o <= T - 2`` is required)."""
        if not _is_int(steps) or self.offset > steps - 2:  # noqa: PLR2004
            msg = f"a batch of {steps} frames has no start at offset {self.offset}: need offset <= T - 2"
            raise ValueError(msg)
        return (steps - 2 - self.offset) // self.stride + 1

    def starts(self, steps: int) -> list[int]:
        """``t0_i = o + i * s`` for ``i < N``."""
        return [self.offset + i * self.stride for i in range(self.rows(steps))]

    def noise_shape(self, batch: int, steps: int, cats: int) -> tuple[int, int, int, int]:
        """Shape of the ``u_overshoot`` uniforms of ``batch`` rows: ``(batch, N, D, K)`` -- batch row first, so ``GlobalRowNoise`` slices it."""
        return (batch, self.rows(steps), self.depth, cats)

    def kl_weights(self, balancing: bool) -> tuple[float, float]:  # noqa: FBT001
        """``(w_prior, w_post)`` of the term's gradient for a model that balances its KL (or not)."""
        if not self.balanced:
            return 1.0, 0.0
        return (KL_BALANCE_ALPHA, 1.0 - KL_BALANCE_ALPHA) if balancing else (1.0, 1.0)

    def _checked_kl(self, post_logits: Tensor, os_logits: Tensor, cats: int, valid: Tensor | None, row0: int) -> tuple[int, int, int, int, int]:
        if post_logits.dim() != 3 or os_logits.dim() != 3:  # noqa: PLR2004
            msg = f"post_logits must be [B, T, K * C] and os_logits [B * N, D, K * C], got {tuple(post_logits.shape)} and {tuple(os_logits.shape)}"
            raise ValueError(msg)
        b, t, width = post_logits.shape
        n = self.rows(t)
        if not _is_int(cats) or cats < 1 or width % cats or width < 1:
            msg = f"the logits' width {width} is no multiple of {cats!r} categoricals"
            raise ValueError(msg)
        if tuple(os_logits.shape) != (b * n, self.depth, width) or b < 1:
            msg = f"os_logits must be {(b * n, self.depth, width)} for post_logits {tuple(post_logits.shape)}, got {tuple(os_logits.shape)}"
            raise ValueError(msg)
        if os_logits.device != post_logits.device or os_logits.dtype != post_logits.dtype:
            msg = "post_logits and os_logits must share device and dtype"
            raise ValueError(msg)
        b_global = b * self.world if valid is None else valid.numel()
        if valid is not None and (valid.dtype != torch.int32 or valid.dim() != 1 or valid.device != post_logits.device):
            msg = f"valid must be an int32 [B_global] tensor on {post_logits.device}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}"
            raise ValueError(msg)
        if not _is_int(row0) or row0 < 0 or row0 + b > b_global:
            msg = f"the rank's rows {row0} .. {row0 + b - 1} do not lie inside the {b_global} global rows"
            raise ValueError(msg)
        return b, t, n, width // cats, b_global

    def _live(self, b_global: int, steps: int, valid: Tensor | None, device: torch.device) -> Tensor:
        """bool ``[B_global, N, D]``: term ``(b, i, k = j + 1)`` is live."""
        n = self.rows(steps)
        length = (torch.full((b_global,), steps, device=device, dtype=torch.int64) if valid is None
                  else valid.to(torch.int64).clamp(0, steps))
        t0 = self.offset + self.stride * torch.arange(n, device=device)
        target = t0.unsqueeze(1) + 1 + torch.arange(self.depth, device=device).unsqueeze(0)  # [N, D]
        return target.unsqueeze(0) < length.reshape(-1, 1, 1)

    # -- the rule in torch, in float64 -------------------------------------------------------------------------------------------------
    def reference(self, post_logits: Tensor, os_logits: Tensor, cats: int, valid: Tensor | None = None, row0: int = 0,  # noqa: PLR0913
                  weights: tuple[float, float] = (1.0, 0.0)) -> OvershootTerms:
        """The rule in float64 on any device.  ``post_logits`` ``[B, T, K * C]`` (the rank's rows ``row0 ..`` of the global batch),
        ``os_logits`` ``[B * N, D, K * C]``, ``valid`` int32 of ALL global rows or None, ``weights = (w_prior, w_post)``.  Autograd through
        ``term`` gives the stated gradients."""
        b, t, n, classes, b_global = self._checked_kl(post_logits, os_logits, cats, valid, row0)
        dev, d = post_logits.device, self.depth
        live_all = self._live(b_global, t, valid, dev)
        live = live_all[row0 : row0 + b]
        count = live_all[:, :, 1:].sum().to(torch.float64)
        t0 = self.offset + self.stride * torch.arange(n, device=dev)
        target = (t0.unsqueeze(1) + 1 + torch.arange(d, device=dev).unsqueeze(0)).clamp(max=t - 1)  # [N, D] (clamped where dead)
        q_logits = post_logits.to(torch.float64)[:, target.reshape(-1)].reshape(b, n, d, cats, classes)
        p_logits = os_logits.to(torch.float64).reshape(b, n, d, cats, classes)
        lq, lp = torch.log_softmax(q_logits, dim=-1), torch.log_softmax(p_logits, dim=-1)

        def kl_of(lq_: Tensor, lp_: Tensor) -> Tensor:
            q = lq_.exp()
            each = torch.where(q > 0, q * (lq_ - lp_), torch.zeros_like(q))
            return each.sum(dim=-1).sum(dim=-1)  # [B, N, D]

        value = kl_of(lq, lp)
        w_prior, w_post = float(weights[0]), float(weights[1])
        surrogate = w_prior * kl_of(lq.detach(), lp) + w_post * kl_of(lq, lp.detach())
        kl = surrogate + (value - surrogate).detach()
        kl = torch.where(live, kl, torch.zeros_like(kl))
        plane = kl.detach().reshape(b * n, d)
        table = torch.stack([plane.sum(dim=0), live.reshape(b * n, d).sum(dim=0).to(torch.float64)])
        term = float(self.world) * kl[:, :, 1:].sum() / count.clamp(min=1.0)
        return OvershootTerms(term, plane, table, count)

    def gather_reference(self, states: list[Tensor], actions: Tensor) -> tuple[list[Tensor], Tensor]:
        """``states[k]`` ``[B, T, W_k]`` -> ``[B * N, W_k]`` at the starts, and the action windows ``[B * N, D, A]`` (zeros past ``T``)."""
        b, t, a = actions.shape
        n, d = self.rows(t), self.depth
        t0 = torch.tensor(self.starts(t), device=actions.device, dtype=torch.int64)
        picked = [x.index_select(1, t0).reshape(b * n, x.shape[-1]) for x in states]
        padded = torch.cat([actions, actions.new_zeros(b, d, a)], dim=1)
        frames = (t0.unsqueeze(1) + 1 + torch.arange(d, device=actions.device).unsqueeze(0)).reshape(-1)
        return picked, padded.index_select(1, frames).reshape(b * n, d, a)

    def scatter_reference(self, grads: list[Tensor], batch: int, steps: int) -> list[Tensor]:
        """The gather's backward for the states: ``g[k]`` ``[B * N, W_k]`` -> ``[B, T, W_k]``, zero off the starts."""
        n = self.rows(steps)
        t0 = torch.tensor(self.starts(steps), device=grads[0].device, dtype=torch.int64)
        out = []
        for g in grads:
            full = g.new_zeros(batch, steps, g.shape[-1])
            full.index_copy_(1, t0, g.reshape(batch, n, g.shape[-1]))
            out.append(full)
        return out

    # -- kernels on the GPU, the rules elsewhere ---------------------------------------------------------------------------------------
    def _checked_states(self, states: list[Tensor], actions: Tensor) -> tuple[int, int, int]:
        if actions.dim() != 3 or actions.shape[-1] < 1 or actions.shape[0] < 1:  # noqa: PLR2004
            msg = f"actions must be [B, T, A], got {tuple(actions.shape)}"
            raise ValueError(msg)
        b, t, _ = actions.shape
        n = self.rows(t)
        if not 0 < len(states) <= _lib.STATE_MAX:
            msg = f"a state table holds 1 .. {_lib.STATE_MAX} tensors, got {len(states)}"
            raise ValueError(msg)
        for x in states:
            if x.dim() != 3 or tuple(x.shape[:2]) != (b, t) or x.shape[2] < 1 or x.device != actions.device:  # noqa: PLR2004
                msg = f"overshoot gather: state {tuple(x.shape)} is not [{b}, {t}, W] on {actions.device}"
                raise ValueError(msg)
        return b, t, n

    def gather(self, states: list[Tensor], actions: Tensor) -> tuple[list[Tensor], Tensor]:
        """One ``mtrssm_overshoot_gather`` launch on torch's current stream for all tensors of a state (non-GPU tensors:
        ``gather_reference``): the start states ``[B * N, W_k]`` and the action windows ``[B * N, D, A]``.  Differentiable in the states
        (``mtrssm_overshoot_scatter``) unless ``detach_state`` is set."""
        self._checked_states(states, actions)
        if self.detach_state:
            states = [x.detach() for x in states]
        if not actions.is_cuda:
            return self.gather_reference(states, actions)
        out = _OvershootGather.apply(self, actions.detach(), *states)
        return list(out[1:]), out[0]

    def kl(self, post_logits: Tensor, os_logits: Tensor, cats: int, valid: Tensor | None = None, row0: int = 0,  # noqa: PLR0913
           weights: tuple[float, float] = (1.0, 0.0)) -> OvershootTerms:
        """``mtrssm_overshoot_kl_fwd`` (two launches, nothing read back) with ``mtrssm_overshoot_kl_bwd`` as its backward; non-GPU tensors:
        ``reference``, rounded to fp32.  Arguments as ``reference``; only ``term`` carries a gradient."""
        b, t, n, classes, b_global = self._checked_kl(post_logits, os_logits, cats, valid, row0)
        w_prior, w_post = float(weights[0]), float(weights[1])
        if not w_prior >= 0.0 or not w_post >= 0.0:
            msg = f"the gradient weights must be >= 0, got {weights!r}"
            raise ValueError(msg)
        if not post_logits.is_cuda:
            got = self.reference(post_logits, os_logits, cats, valid, row0, (w_prior, w_post))
            return OvershootTerms(got.term.to(torch.float32), got.plane.to(torch.float32), got.table, got.count.to(torch.float32))
        geom = (b_global, row0, b, t, n, self.stride, self.offset, self.depth, cats, classes)
        term, plane, table, count = _OvershootKL.apply(post_logits, os_logits, valid, geom, w_prior, w_post)
        if self.world != 1:
            term = term * float(self.world)
        return OvershootTerms(term, plane, table, count)


def _state_table(srcs: list[Tensor], dsts: list[Tensor]) -> C.Structure:
    table = _lib.StateTable()
    table.count = len(srcs)
    for k, (src, dst) in enumerate(zip(srcs, dsts, strict=True)):
        table.width[k] = src.shape[-1]
        table.src_stride[k] = 0
        table.src[k] = _lib.ptr(src)  # (contiguous fp32 on the GPU, or MtrssmLibraryError)
        table.alt[k] = None
        table.dst[k] = _lib.ptr(dst)
    return table


class _OvershootGather(torch.autograd.Function):
    """``(windows, *starts) = gather(actions, *states)``; the states' gradients come back through ``mtrssm_overshoot_scatter``."""

    @staticmethod
    def forward(ctx, lo: LatentOvershoot, actions: Tensor, *states: Tensor):  # noqa: ANN001, ANN205
        ctx.set_materialize_grads(False)
        b, t, a = actions.shape
        n, d = lo.rows(t), lo.depth
        srcs = [x.detach().contiguous().float() for x in states]
        acts = actions.contiguous().float()
        dsts = [torch.empty(b * n, x.shape[-1], device=x.device, dtype=torch.float32) for x in srcs]
        windows = torch.empty(b * n, d, a, device=acts.device, dtype=torch.float32)
        table = _state_table(srcs, dsts)
        moved = 8.0 * b * n * (sum(x.shape[-1] for x in srcs) + d * a)
        _lib.check(_lib.TIMERS.call("mtrssm_overshoot_gather", _lib.load().mtrssm_overshoot_gather, C.byref(table), _lib.ptr(acts),
                                    _lib.ptr(windows), b, t, n, lo.stride, lo.offset, d, a, _lib.stream_ptr(acts.device), nbytes=moved),
                   "mtrssm_overshoot_gather")
        ctx.geom = (b, t, n, lo.stride, lo.offset)
        ctx.mark_non_differentiable(windows)
        return (windows, *dsts)

    @staticmethod
    def backward(ctx, _g_windows, *grads):  # noqa: ANN001, ANN205
        b, t, n, stride, offset = ctx.geom
        have = [(k, g.contiguous().float()) for k, g in enumerate(grads) if g is not None and ctx.needs_input_grad[2 + k]]
        out: list[Tensor | None] = [None] * len(grads)
        if have:
            srcs = [g for _, g in have]
            dsts = [torch.empty(b, t, g.shape[-1], device=g.device, dtype=torch.float32) for g in srcs]
            table = _state_table(srcs, dsts)
            moved = 4.0 * b * (t + n) * sum(g.shape[-1] for g in srcs)
            _lib.check(_lib.TIMERS.call("mtrssm_overshoot_scatter", _lib.load().mtrssm_overshoot_scatter, C.byref(table), b, t, n, stride, offset,
                                        _lib.stream_ptr(srcs[0].device), nbytes=moved), "mtrssm_overshoot_scatter")
            for (k, _), full in zip(have, dsts, strict=True):
                out[k] = full
        return (None, None, *out)


class _OvershootKL(torch.autograd.Function):
    """``(term, plane, table, count) = kl(post_logits, os_logits)``; ``term`` alone is differentiable."""

    @staticmethod
    def forward(ctx, post: Tensor, os_logits: Tensor, valid: Tensor | None, geom: tuple[int, ...], w_prior: float, w_post: float):  # noqa: ANN001, ANN205, PLR0913
        lib = _lib.load()
        b_global, _row0, b, t, n, _s, _o, d, cats, classes = geom
        post, os_logits = post.detach().contiguous().float(), os_logits.detach().contiguous().float()
        valid = None if valid is None else valid.contiguous()
        dev = post.device
        plane = torch.empty(b * n, d, device=dev, dtype=torch.float32)
        table = torch.empty(2, d, device=dev, dtype=torch.float64)
        count, term = (torch.empty((), device=dev, dtype=torch.float32) for _ in range(2))
        nbytes = int(lib.mtrssm_overshoot_kl_workspace_bytes(b, n, d))
        if nbytes < 0:
            msg = f"overshoot: {b} x {n} rows of {d} steps are out of range"
            raise ValueError(msg)
        workspace = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        width = cats * classes
        moved = 4.0 * (b * n * d * width + b * t * width + b * n * d)
        _lib.check(_lib.TIMERS.call("mtrssm_overshoot_kl_fwd", lib.mtrssm_overshoot_kl_fwd, _lib.ptr(post), _lib.ptr(os_logits),
                                    _lib.index_ptr(valid), *geom, _lib.ptr(plane), _lib.raw_ptr(table), _lib.ptr(count), _lib.ptr(term),
                                    _lib.raw_ptr(workspace), nbytes, _lib.stream_ptr(dev), nbytes=moved), "mtrssm_overshoot_kl_fwd")
        ctx.geom, ctx.weights, ctx.valid = geom, (w_prior, w_post), valid
        ctx.save_for_backward(post, os_logits, count)
        ctx.mark_non_differentiable(plane, table, count)
        return term, plane, table, count

    @staticmethod
    def backward(ctx, g_term, _g_plane, _g_table, _g_count):  # noqa: ANN001, ANN205
        post, os_logits, count = ctx.saved_tensors
        w_prior, w_post = ctx.weights
        if g_term is None:
            return None, None, None, None, None, None
        g_term = g_term.contiguous().float()
        g_os = torch.empty_like(os_logits)
        g_post = torch.empty_like(post) if w_post > 0.0 else None
        moved = 4.0 * (2 * os_logits.numel() + (1 + ctx.geom[7]) * post.numel())
        _lib.check(_lib.TIMERS.call("mtrssm_overshoot_kl_bwd", _lib.load().mtrssm_overshoot_kl_bwd, _lib.ptr(post), _lib.ptr(os_logits),
                                    _lib.index_ptr(ctx.valid), _lib.ptr(g_term), _lib.ptr(count), *ctx.geom, w_prior, w_post, _lib.ptr(g_os),
                                    _lib.ptr(g_post), _lib.stream_ptr(post.device), nbytes=moved), "mtrssm_overshoot_kl_bwd")
        return g_post, g_os, None, None, None, None


class OvershootTable(SumTable):
    """The accumulated by-distance KL of any number of steps in ONE double buffer ``[levels, 2, D]``: per latent level and distance
    ``k = 1 .. D`` the sum and the count of live terms (MRSSM one level, MMTRSSM ``_l`` then ``_h``)."""

    def __init__(self, levels: int, depth: int, device: torch.device | str = "cpu") -> None:
        if levels < 1 or depth < 2:  # noqa: PLR2004
            msg = f"need levels >= 1 and depth >= 2, got {levels} and {depth}"
            raise ValueError(msg)
        self.buffer = torch.zeros(levels, 2, depth, dtype=torch.float64, device=device)

    @property
    def levels(self) -> int:
        return self.buffer.shape[0]

    def fold(self, tables: list[Tensor]) -> OvershootTable:
        """Adds one step's ``table`` ``[2, D]`` per level (``OvershootTerms.table``); nothing is read back."""
        if len(tables) != self.levels or any(tuple(x.shape) != tuple(self.buffer.shape[1:]) for x in tables):
            msg = f"need {self.levels} tables of shape {tuple(self.buffer.shape[1:])}, got {[tuple(x.shape) for x in tables]}"
            raise ValueError(msg)
        for level, x in enumerate(tables):
            self.buffer[level] += x.to(self.buffer)
        return self

    def curves(self) -> dict[str, Tensor]:
        """``kl`` (and ``kl_h``): ``[D]`` each, the mean KL of the live terms at distance ``k = 1 .. D``; NaN where nothing was counted."""
        names = ("kl", "kl_h", *(f"kl_{i}" for i in range(2, self.levels)))
        return {names[level]: self._mean(self.buffer[level, 0], self.buffer[level, 1]) for level in range(self.levels)}

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix/kl_d{k}`` (and ``prefix/kl_h_d{k}``) for ``k = 1 .. D``, fp32."""
        return {f"{prefix}/{name}_d{k + 1}": curve[k].to(torch.float32) for name, curve in self.curves().items() for k in range(self.steps)}


__all__ = ["LatentOvershoot", "OvershootTable", "OvershootTerms"]
