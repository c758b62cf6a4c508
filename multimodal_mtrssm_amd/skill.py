"""Forecast skill by horizon: sampled ensembles scored in one pass.

A *skill step* observes a fixed context of ``q`` frames of every row, rolls ``S`` sampled futures per row open loop on the masked
scans (the ``S`` copies of a row share their context trajectory bit for bit), decodes them and scores every frame against its target:

    se_s   = sum_e 0.5 (x_e - y_s,e)^2                    y_s = act(pred[b, s, t]), x = target[b, t]
    mean   = (se_0 + ... + se_{S-1}) / S                  the expected error of a sample
    best   = min_s se_s                                   per FRAME, not per trajectory (``se_samples`` allows the latter on the host)
    ybar_e = (y_0,e + ... + y_{S-1},e) / S
    ens    = sum_e 0.5 (x_e - ybar_e)^2                   the error of the ensemble mean
    spread = sum_e 0.5 (sum_s (y_s,e - ybar_e)^2) / S     mean = ens + spread in exact arithmetic

(sums over s are left folds; the data term only -- ``0.5 E log 2 pi`` is added where an NLL is reported; a dead frame scores 0).  The
planes are folded by horizon: with ``c_b = clamp(q, 1, T)`` a live frame has ``h = 0`` when ``t < c_b`` ("observed"; with
``observe="audio"`` bin 0 of vision is the cross-modal reconstruction), else ``h = t - c_b + 1``; ``sums[p][h] += plane[p][b][t]``,
``counts[h] += 1``, the live frames of a bin added in ascending ``b`` onto the value already there.  ``ForecastSkill.reference`` and
``ForecastSkill.reference_table`` state both in torch (any float dtype); ``mtrssm_ensemble_score`` and ``mtrssm_horizon_table`` are the
kernels, used for GPU tensors; elsewhere the torch rule runs.
"""

from __future__ import annotations

import copy
from typing import NamedTuple

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib

MODALITIES = ("audio", "vision")
SCORES = ("mean", "ens", "best", "spread")
OBSERVE_BITS = {"both": 3, "audio": 1, "vision": 2}
MAX_SAMPLES = 16
_EXACT = 1 << 24  # fp32 counts are whole numbers below this


class SkillPlanes(NamedTuple):
    """Per-frame scores ``[B, T]`` of one modality and the per-sample errors ``se_samples`` ``[B, S, T]`` (None when not asked for)."""

    mean: Tensor
    ens: Tensor
    best: Tensor
    spread: Tensor
    se_samples: Tensor | None


class ForecastSkill:
    """``ForecastSkill(q, samples=S, observe=...)``: every row observes ``q >= 1`` frames (``observe``: of both modalities, of audio
    only or of vision only), then ``S`` (1 .. 16) sampled futures per row run open loop.  ``max_frames``: the decoders and the scorer
    run over chunks of whole rows (all ``S`` copies of a row together) of at most this many frames."""

    def __init__(self, context: int, samples: int = 1, observe: str = "both") -> None:
        if isinstance(context, bool) or not isinstance(context, int) or not 1 <= context < 1 << 31:
            msg = f"context must be an integer 1 <= q < 2^31 (frame 0 is always observed), got {context!r}"
            raise ValueError(msg)
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
            msg = f"samples must be an integer in 1 .. {MAX_SAMPLES}, got {samples!r}"
            raise ValueError(msg)
        if observe not in OBSERVE_BITS:
            msg = f"observe must be one of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        self.context, self.samples, self.observe = context, samples, observe
        self.max_frames = 4096
        self.group = None  # the process group SkillTable.all_reduce uses (FlatDataParallel.skill binds it)
        self._observed: dict[torch.device, Tensor] = {}

    def __repr__(self) -> str:
        return f"ForecastSkill({self.context}, samples={self.samples}, observe={self.observe!r})"

    @property
    def bits(self) -> int:
        """The scans' modality code of an observed step: bit 0 audio, bit 1 vision."""
        return OBSERVE_BITS[self.observe]

    def observed(self, device: torch.device) -> Tensor:
        """Bool ``[2]`` (audio, vision) on ``device``: what an observed step sees; made once per device."""
        device = torch.device(device)
        if device not in self._observed:
            self._observed[device] = torch.tensor([bool(self.bits & 1), bool(self.bits & 2)], device=device)
        return self._observed[device]

    def for_group(self, group) -> ForecastSkill:  # noqa: ANN001
        """A copy whose table is all-reduced over ``group`` (``FlatDataParallel.skill`` calls this)."""
        bound = copy.copy(self)
        bound.group = group
        return bound

    def noise_shapes(self, model, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # noqa: ANN001
        """The uniforms of one skill step, batch dimension first (``GlobalRowNoise`` shards them as they are): the initial state's, the
        context's ``u_post (B, T, K)`` shared by a row's copies and the tails' ``u_tail (B, S, T, K)`` (MMTRSSM: the ``_l`` / ``_h`` pairs)."""
        s = self.samples
        if hasattr(model, "l_dist"):
            kl, kh = model.l_dist.category_size, model.h_dist.category_size
            return {"u_init_h": (batch, kh), "u_init_l": (batch, kl), "u_post_l": (batch, steps, kl), "u_post_h": (batch, steps, kh),
                    "u_tail_l": (batch, s, steps, kl), "u_tail_h": (batch, s, steps, kh)}
        k = model.transition.distribution_factory.category_size
        return {"u_init": (batch, k), "u_post": (batch, steps, k), "u_tail": (batch, s, steps, k)}

    def compose_noise(self, u_post: Tensor, u_tail: Tensor) -> Tensor:
        """``[B * S, T, K]``: row ``b * S + s`` reads ``u_post[b, t]`` on ``t < q`` and ``u_tail[b, s, t]`` from ``q`` on."""
        b, t, k = u_post.shape
        s = self.samples
        if tuple(u_tail.shape) != (b, s, t, k):
            msg = f"the tail uniforms must have shape {(b, s, t, k)}, got {tuple(u_tail.shape)}"
            raise ValueError(msg)
        q = min(self.context, t)
        return torch.cat([u_post[:, None, :q].expand(b, s, q, k), u_tail[:, :, q:]], dim=2).reshape(b * s, t, k).contiguous()

    # -- the rule in torch -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked(pred: Tensor, target: Tensor, valid: Tensor | None, act: int) -> tuple[int, int, int, int]:
        if pred.dim() != 4 or target.dim() != 3:  # noqa: PLR2004
            msg = f"pred must be [B, S, T, E] and target [B, T, E], got {tuple(pred.shape)} and {tuple(target.shape)}"
            raise ValueError(msg)
        b, s, t, e = pred.shape
        if tuple(target.shape) != (b, t, e) or not 1 <= s <= MAX_SAMPLES or min(b, t, e) < 1:
            msg = f"pred {tuple(pred.shape)} needs a target of shape {(b, t, e)} and 1 <= S <= {MAX_SAMPLES}, got {tuple(target.shape)}"
            raise ValueError(msg)
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (b,)):
            msg = f"valid must be an int32 tensor of shape ({b},), got {valid.dtype} {tuple(valid.shape)}"
            raise ValueError(msg)
        if act not in (0, 3):
            msg = f"act must be 0 (Identity) or 3 (Tanh), got {act}"
            raise ValueError(msg)
        return b, s, t, e

    @staticmethod
    def reference(pred: Tensor, target: Tensor, valid: Tensor | None = None, act: int = 0) -> SkillPlanes:
        """The scores in torch, in ``pred``'s dtype: ``pred`` ``[B, S, T, E]`` raw, ``target`` ``[B, T, E]``, ``valid`` int32 ``[B]`` (None:
        every frame is live), ``act`` 0 (Identity) or 3 (Tanh)."""
        _, s, t, _ = ForecastSkill._checked(pred, target, valid, act)
        y = torch.tanh(pred) if act == 3 else pred  # noqa: PLR2004
        x = target.to(y.dtype)
        se = (0.5 * (x.unsqueeze(1) - y) ** 2).sum(-1)  # [B, S, T]
        total, ysum = se[:, 0], y[:, 0]
        for i in range(1, s):  # (left folds)
            total, ysum = total + se[:, i], ysum + y[:, i]
        ybar = ysum / s
        ens = (0.5 * (x - ybar) ** 2).sum(-1)
        dev = (y[:, 0] - ybar) ** 2
        for i in range(1, s):
            dev = dev + (y[:, i] - ybar) ** 2
        spread = (0.5 * dev / s).sum(-1)
        mean, best = total / s, se.min(dim=1).values
        if valid is not None:
            live = torch.arange(t, device=pred.device) < valid.unsqueeze(1)
            zero = torch.zeros((), dtype=y.dtype, device=y.device)
            mean, ens, best, spread = (torch.where(live, p, zero) for p in (mean, ens, best, spread))
            se = torch.where(live.unsqueeze(1), se, zero)
        return SkillPlanes(mean, ens, best, spread, se)

    @staticmethod
    def horizon(context: Tensor, valid: Tensor | None, steps: int) -> tuple[Tensor, Tensor]:
        """``(h, live)``, int64 and bool ``[B, T]``: ``h = 0`` when ``t < c_b`` else ``t - c_b + 1``, ``c_b = clamp(context, 1, T)``."""
        c = context.to(torch.int64).clamp(1, steps).unsqueeze(1)
        t = torch.arange(steps, device=context.device)
        length = torch.full_like(c, steps) if valid is None else valid.to(torch.int64).clamp(0, steps).unsqueeze(1)
        return torch.where(t < c, torch.zeros_like(t), t - c + 1), t < length

    @staticmethod
    def reference_table(planes: Tensor, context: Tensor, valid: Tensor | None, sums: Tensor, counts: Tensor) -> None:
        """The fold in torch, in place and in ``sums``' dtype: ``planes`` ``[P, B, T]``, ``context`` int32 ``[B]``, ``sums`` ``[P, T]``,
        ``counts`` ``[T]``.  Each bin's live frames are added one by one in ascending ``(b, t)``; in fp32 this is the kernel bit for bit."""
        p, b, t = planes.shape
        if tuple(sums.shape) != (p, t) or tuple(counts.shape) != (t,) or tuple(context.shape) != (b,):
            msg = f"planes {tuple(planes.shape)} need sums {(p, t)}, counts {(t,)} and context {(b,)}"
            raise ValueError(msg)
        if b * t >= _EXACT:
            msg = f"{b} x {t} frames: the fp32 counts are exact below 2^24"
            raise ValueError(msg)
        h, live = ForecastSkill.horizon(context, valid, t)
        planes = planes.to(sums.dtype)
        for row in range(b):
            idx = live[row].nonzero().flatten()
            head = idx[h[row, idx] == 0]
            for i in head.tolist():  # bin 0 takes several frames of a row: one add each
                sums[:, 0] += planes[:, row, i]
                counts[0] += 1
            tail = idx[h[row, idx] > 0]  # every other bin takes at most one
            sums[:, h[row, tail]] += planes[:, row, tail]
            counts[h[row, tail]] += 1

    # -- kernels on the GPU, the rule elsewhere ------------------------------------------------------------------------------------------
    @staticmethod
    def score(pred: Tensor, target: Tensor, valid: Tensor | None = None, act: int = 0, *, out: Tensor | None = None,
              se_samples: bool = False) -> SkillPlanes:
        """One ``mtrssm_ensemble_score`` launch on torch's current stream (non-GPU tensors: ``reference``).  ``out``: an fp32 ``[4, B, T]``
        buffer the four planes are written to (mean, ens, best, spread)."""
        b, s, t, e = ForecastSkill._checked(pred, target, valid, act)
        if not pred.is_cuda:
            got = ForecastSkill.reference(pred, target, valid, act)
            if out is not None:
                out.copy_(torch.stack(got[:4]))
                got = SkillPlanes(out[0], out[1], out[2], out[3], got.se_samples)
            return got if se_samples else got._replace(se_samples=None)
        pred, target = pred.contiguous(), target.contiguous()
        valid = None if valid is None else valid.contiguous()
        if out is None:
            out = torch.empty(4, b, t, device=pred.device, dtype=torch.float32)
        if tuple(out.shape) != (4, b, t) or not out.is_contiguous():
            msg = f"out must be a contiguous [4, {b}, {t}] buffer, got {tuple(out.shape)}"
            raise ValueError(msg)
        se = torch.empty(b, s, t, device=pred.device, dtype=torch.float32) if se_samples else None
        _lib.check(_lib.TIMERS.call("mtrssm_ensemble_score", _lib.load().mtrssm_ensemble_score, _lib.ptr(pred), _lib.ptr(target),
                                    _lib.index_ptr(valid), b, s, t, e, int(act), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                    _lib.ptr(out[3]), _lib.ptr(se), _lib.stream_ptr(pred.device), nbytes=4.0 * (s + 1) * b * t * e),
                   "mtrssm_ensemble_score")
        return SkillPlanes(out[0], out[1], out[2], out[3], se)

    @staticmethod
    def table_add(planes: Tensor, context: Tensor, valid: Tensor | None, sums: Tensor, counts: Tensor) -> None:
        """``sums`` / ``counts`` += the fold of ``planes``: one ``mtrssm_horizon_table`` launch (non-GPU tensors: ``reference_table``)."""
        if not planes.is_cuda:
            ForecastSkill.reference_table(planes, context, valid, sums, counts)
            return
        p, b, t = planes.shape
        if tuple(sums.shape) != (p, t) or tuple(counts.shape) != (t,) or tuple(context.shape) != (b,):
            msg = f"planes {tuple(planes.shape)} need sums {(p, t)}, counts {(t,)} and context {(b,)}"
            raise ValueError(msg)
        if b * t >= _EXACT:
            msg = f"{b} x {t} frames: the fp32 counts are exact below 2^24"
            raise ValueError(msg)
        _lib.check(_lib.load().mtrssm_horizon_table(_lib.ptr(planes), p, _lib.index_ptr(context), _lib.index_ptr(valid), b, t, _lib.ptr(sums),
                                                    _lib.ptr(counts), _lib.stream_ptr(planes.device)), "mtrssm_horizon_table")


class SkillTable:
    """The accumulated skill of any number of skill steps in ONE fp32 buffer ``[2 * 4 + 1, T]``: audio then vision x (mean, ens, best,
    spread), then the counts.  A step run with ``keep_states`` also leaves its score planes (``planes``, ``[8, B, T]``) and its rollout
    (``states``) here; otherwise both are None and the table holds nothing of a batch."""

    ROWS = len(MODALITIES) * len(SCORES)

    def __init__(self, steps: int, device: torch.device | str = "cpu") -> None:
        if steps < 1:
            msg = f"need steps >= 1, got {steps}"
            raise ValueError(msg)
        self.buffer = torch.zeros(self.ROWS + 1, steps, dtype=torch.float32, device=device)
        self.planes: Tensor | None = None
        self.states = None

    @property
    def steps(self) -> int:
        return self.buffer.shape[1]

    @property
    def sums(self) -> Tensor:
        return self.buffer[: self.ROWS]

    @property
    def counts(self) -> Tensor:
        return self.buffer[self.ROWS]

    def add(self, other: SkillTable) -> SkillTable:
        if tuple(other.buffer.shape) != tuple(self.buffer.shape):
            msg = f"tables of {self.steps} and {other.steps} steps do not add"
            raise ValueError(msg)
        self.buffer += other.buffer.to(self.buffer.device)
        return self

    def all_reduce(self, group=None) -> SkillTable:  # noqa: ANN001
        """One SUM all-reduce of the buffer (counts stay exact below 2^24 frames per bin); a no-op without a process group."""
        import torch.distributed as dist  # noqa: PLC0415

        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.buffer, op=dist.ReduceOp.SUM, group=group)
        return self

    def curves(self) -> dict[str, dict[str, Tensor]]:
        """``sums / counts`` per modality and score, ``[T]`` each; an empty bin gives NaN."""
        counts = self.counts
        nan = torch.full_like(counts, float("nan"))
        rows = iter(self.sums)
        return {m: {k: torch.where(counts > 0, next(rows) / counts, nan) for k in SCORES} for m in MODALITIES}

    def _bin_slices(self, edges: tuple[int, ...]) -> list[tuple[str, slice]]:
        edges = tuple(int(e) for e in edges)
        if not edges or edges[0] < 1 or any(a >= b for a, b in zip(edges, edges[1:])):  # noqa: RUF007
            msg = f"edges must be ascending horizons >= 1, got {edges}"
            raise ValueError(msg)
        t = self.steps
        out = [("obs", slice(0, 1))]
        for lo, hi in zip(edges, (*edges[1:], t)):
            out.append((f"h{lo}", slice(min(lo, t), min(max(hi, lo), t))))
        return out

    def binned(self, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, dict[str, Tensor]]:
        """The curves over horizon bins: ``(1, 2, 4, 8)`` gives bin 0 and ``[1, 2) [2, 4) [4, 8) [8, T)`` -- each the bin's summed scores
        over its summed counts (NaN for a bin without frames)."""
        slices = self._bin_slices(edges)
        counts = torch.stack([self.counts[s].sum() for _, s in slices])
        nan = torch.full_like(counts, float("nan"))
        rows = iter(self.sums)
        out: dict[str, dict[str, Tensor]] = {}
        for m in MODALITIES:
            out[m] = {}
            for k in SCORES:
                row = next(rows)
                out[m][k] = torch.where(counts > 0, torch.stack([row[s].sum() for _, s in slices]) / counts, nan)
        return out

    def scalars(self, prefix: str, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, Tensor]:
        """``prefix/{audio,vision}/{mean,ens,best,spread}/{obs,h1,h2,...}``: the binned curves as a flat dict of scalars."""
        names = [n for n, _ in self._bin_slices(edges)]
        binned = self.binned(edges)
        return {f"{prefix}/{m}/{k}/{n}": binned[m][k][i] for m in MODALITIES for k in SCORES for i, n in enumerate(names)}


__all__ = ["ForecastSkill", "SkillPlanes", "SkillTable"]
