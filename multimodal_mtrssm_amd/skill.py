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
import functools
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


class ObservingConfig:
    """What the evaluation configs that decide what the model observes share (``ForecastSkill``, ``LikelihoodBound``, ``LatentProbe``,
    ``EpisodePanel``): the modality code of ``observe``, its device tensors, the binding to a process group and the uniforms of a step.
    A subclass sets ``observe`` and ``group`` and states the copies of a row in ``plan`` (``evaluation.CopyPlan``)."""

    observe: str | tuple[str, ...]
    group = None  # the process group the config's table is all-reduced over (FlatDataParallel binds it)

    @property
    def bits(self) -> int | tuple[int, ...]:
        """The scans' modality code of an observed step: bit 0 audio, bit 1 vision (a tuple of ``observe``: one code per copy of a row)."""
        return OBSERVE_BITS[self.observe] if isinstance(self.observe, str) else tuple(OBSERVE_BITS[o] for o in self.observe)

    def observed(self, device: torch.device) -> Tensor:
        """Bool ``[2]`` (audio, vision) on ``device``: what an observed step sees (``[G, 2]`` for per-copy ``bits``); made once per device."""
        bits = self.bits
        if isinstance(bits, tuple):
            return observed_bits(bits, torch.device(device))[1]
        return observed_bits((bits,), torch.device(device))[1][0]

    def for_group(self, group):  # noqa: ANN001, ANN201
        """A copy bound to ``group`` (``FlatDataParallel.skill`` / ``.likelihood`` / ``.probe`` call this)."""
        bound = copy.copy(self)
        bound.group = group
        return bound

    def noise_shapes(self, model, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # noqa: ANN001
        """The uniforms of one step, batch dimension first (``GlobalRowNoise`` shards them as they are): what ``plan`` says of the
        copies of a row -- shared ``(B, K)`` / ``(B, T, K)``, own ``(B, S, K)`` / ``(B, S, T, K)``, or shared on the context with own tails
        ``u_tail (B, S, T, K)`` (MMTRSSM: the ``_l`` / ``_h`` pairs); row ``(b, s)`` is scan row ``b * S + s``."""
        return self.plan().noise_shapes(model, batch, steps)


@functools.lru_cache(maxsize=None)
def observed_bits(bits: tuple[int, ...], device: torch.device) -> tuple[Tensor, Tensor]:
    """``(int32 [G], bool [G, 2])`` on ``device`` for the modality codes ``bits``: the codes and what each sees (audio, vision).  Made
    once per device; never written to."""
    return (torch.tensor(bits, dtype=torch.int32, device=device), torch.tensor([[bool(b & 1), bool(b & 2)] for b in bits], device=device))


class SumTable:
    """What the evaluation tables share: ONE fp32 ``buffer`` of sums and counts (so that one all-reduce, one ``add`` and one state entry
    carry a table), ``steps`` in its last dimension, the NaN-on-empty division and the horizon bins."""

    buffer: Tensor

    @staticmethod
    def _checked_steps(steps: int) -> int:
        if steps < 1:
            msg = f"need steps >= 1, got {steps}"
            raise ValueError(msg)
        return steps

    @property
    def steps(self) -> int:
        return self.buffer.shape[-1]

    def _sizes(self, other: SumTable) -> str:
        return f"{self.steps} and {other.steps} steps"

    def add(self, other):  # noqa: ANN001, ANN201
        if tuple(other.buffer.shape) != tuple(self.buffer.shape):
            msg = f"tables of {self._sizes(other)} do not add"
            raise ValueError(msg)
        self.buffer += other.buffer.to(self.buffer.device)
        return self

    def all_reduce(self, group=None):  # noqa: ANN001, ANN201
        """One SUM all-reduce of the buffer (counts stay exact below 2^24 frames per bin); a no-op without a process group."""
        import torch.distributed as dist  # noqa: PLC0415

        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.buffer, op=dist.ReduceOp.SUM, group=group)
        return self

    @staticmethod
    def _mean(sums: Tensor, counts: Tensor) -> Tensor:
        """``sums / counts``, NaN where nothing was counted."""
        return torch.where(counts > 0, sums / counts, float("nan"))

    def _bin_slices(self, edges: tuple[int, ...]) -> list[tuple[str, slice]]:
        """``(1, 2, 4, 8)`` names bin 0 ``obs`` and the horizons ``[1, 2) [2, 4) [4, 8) [8, T)`` ``h1 h2 h4 h8``."""
        edges = tuple(int(e) for e in edges)
        if not edges or edges[0] < 1 or any(a >= b for a, b in zip(edges, edges[1:])):  # noqa: RUF007
            msg = f"edges must be ascending horizons >= 1, got {edges}"
            raise ValueError(msg)
        t = self.steps
        out = [("obs", slice(0, 1))]
        for lo, hi in zip(edges, (*edges[1:], t)):
            out.append((f"h{lo}", slice(min(lo, t), min(max(hi, lo), t))))
        return out


class ForecastSkill(ObservingConfig):
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

    def __repr__(self) -> str:
        return f"ForecastSkill({self.context}, samples={self.samples}, observe={self.observe!r})"

    def plan(self):  # noqa: ANN201
        """``S`` copies of a row observe ``q`` frames of ``observe``; they share the row's initial uniforms and ``u_post`` on the context and
        read their own ``u_tail[b, s]`` after it."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(self.samples, self.bits, self.context, post="tail")

    def compose_noise(self, u_post: Tensor, u_tail: Tensor) -> Tensor:
        """``[B * S, T, K]``: row ``b * S + s`` reads ``u_post[b, t]`` on ``t < q`` and ``u_tail[b, s, t]`` from ``q`` on."""
        return self.plan().tail_uniforms("u_post", u_post, u_tail)

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


class PlaneTable(SumTable):
    """A ``SumTable`` of ``ROWS`` summed planes and, behind them, the counts of the frames they were summed over: ``[ROWS + 1, T]``.  A
    step run with ``keep_states`` also leaves its planes (``planes``, ``[8, B, T]``) and its rollout (``states``) here; otherwise both
    are None and the table holds nothing of a batch."""

    ROWS: int

    def __init__(self, steps: int, device: torch.device | str = "cpu") -> None:
        self.buffer = torch.zeros(self.ROWS + 1, self._checked_steps(steps), dtype=torch.float32, device=device)
        self.planes: Tensor | None = None
        self.states = None

    @property
    def sums(self) -> Tensor:
        return self.buffer[: self.ROWS]

    @property
    def counts(self) -> Tensor:
        return self.buffer[self.ROWS]


class SkillTable(PlaneTable):
    """The accumulated skill of any number of skill steps in ONE fp32 buffer ``[2 * 4 + 1, T]``: audio then vision x (mean, ens, best,
    spread), then the counts."""

    ROWS = len(MODALITIES) * len(SCORES)

    def curves(self) -> dict[str, dict[str, Tensor]]:
        """``sums / counts`` per modality and score, ``[T]`` each; an empty bin gives NaN."""
        rows = iter(self.sums)
        return {m: {k: self._mean(next(rows), self.counts) for k in SCORES} for m in MODALITIES}

    def binned(self, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, dict[str, Tensor]]:
        """The curves over horizon bins: ``(1, 2, 4, 8)`` gives bin 0 and ``[1, 2) [2, 4) [4, 8) [8, T)`` -- each the bin's summed scores
        over its summed counts (NaN for a bin without frames)."""
        slices = self._bin_slices(edges)
        counts = torch.stack([self.counts[s].sum() for _, s in slices])
        rows = iter(self.sums)
        out: dict[str, dict[str, Tensor]] = {}
        for m in MODALITIES:
            out[m] = {}
            for k in SCORES:
                row = next(rows)
                out[m][k] = self._mean(torch.stack([row[s].sum() for _, s in slices]), counts)
        return out

    def scalars(self, prefix: str, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, Tensor]:
        """``prefix/{audio,vision}/{mean,ens,best,spread}/{obs,h1,h2,...}``: the binned curves as a flat dict of scalars."""
        names = [n for n, _ in self._bin_slices(edges)]
        binned = self.binned(edges)
        return {f"{prefix}/{m}/{k}/{n}": binned[m][k][i] for m in MODALITIES for k in SCORES for i, n in enumerate(names)}


__all__ = ["ForecastSkill", "ObservingConfig", "PlaneTable", "SkillPlanes", "SkillTable", "SumTable", "observed_bits"]
