"""Latent census: code usage, entropies, KL and dwell times of the categorical latent in one fold.

A *census step* gives row ``b`` ``G`` copies (``1 <= G <= 4``).  Copy ``g`` observes ``observe[g]`` on every live frame; the copies share
the row's uniforms and copy ``g`` is scan row ``r = b * G + g``, exactly as ``LatentProbe`` arranges it.  Frame ``t`` is live iff
``t < valid[b]``.

Per latent level (MRSSM: one; MMTRSSM: ``_l`` and ``_h``) with ``K`` categoricals of ``C`` classes: ``lq_k`` / ``lp_k`` are the log-softmax
of categorical ``k``'s posterior / prior logits, ``q = exp(lq)``, ``p = exp(lp)``; ``c*_k(t)`` is the first class with ``post_stoch > 0.5``
(class 0 when there is none); ``lq0_k`` is ``lq_k`` of scan row ``b * G`` (the row's first copy).  Per categorical, in double, with max,
log-sum and differences formed as ``mtrssm_latent_log_ratio`` forms them:

    hq_k = -sum_c q_c lq_c          hp_k = -sum_c p_c lp_c               (a class with probability 0 adds 0)
    kl_k = sum_c q_c (lq_c - lp_c)  cross_k = sum_c q0_c (lq0_c - lq_c)  (exactly 0 for g = 0 and whenever the two rows' logits are bitwise equal)
    sw_k(t) = 1 if t >= 1 and c*_k(t) != c*_k(t-1) else 0                (t - 1 is live whenever t is)

**Frame planes** ``[5, R, T]`` fp32 (``PLANES``: post_entropy, prior_entropy, kl, cross, switches): each the sum over ``k`` in ascending
``k`` of the quantity above, rounded to fp32 once, exactly 0 on a dead frame; ``kl`` and ``cross`` are not clamped.

**Accumulators**, per level and group, in double (``[G, GS]``, ``GS = 3 K C + 5 K + 2 + 6 T``; batches add up in the same buffer): per class
``[K, C]`` ``n`` (live frames with ``c*_k = c``), ``qsum`` (the sum of ``q_c``), ``psum`` (the sum of ``p_c``); per categorical ``[K]`` the
sums of ``hq``, ``hp``, ``kl``, ``cross``, ``sw``; ``frames`` (live frames) and ``pairs`` (live frames with ``t >= 1``); by frame position
``[5, T]`` the sum over the group's rows of the fp32 planes read back as doubles; ``[T]`` the count of live rows at each position.

**Fold order**, fixed by the shapes alone: a row's partial of a cell is a left fold from +0 over its live frames in ascending ``t``;
the step's sum is a left fold from +0 over the rows' partials in ascending ``b``; that sum is added, in one add, onto what the buffer
holds.  The position sums likewise take ``plane[p][b * G + g][t]`` in ascending ``b`` from +0 (dead frames, exactly 0, included) and
are added once: a float64 left fold of a step's returned planes reproduces its sums bit for bit, a second call of the same step
doubles the buffer exactly, and two steps into one table are the ``add`` of two tables.  ``LatentCensus.reference`` states all of this in torch, in float64; ``mtrssm_latent_census`` is the kernel, used for
GPU tensors; elsewhere the torch rule runs.  ``CensusTable`` derives usage, perplexity, mutual information, the aggregate
posterior's gap to the aggregate prior, the active categoricals and the dwell times from the accumulators alone.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.skill import OBSERVE_BITS, ObservingConfig, SumTable

PLANES = ("post_entropy", "prior_entropy", "kl", "cross", "switches")
MAX_GROUPS = 4
_EXACT = 1 << 24


def group_cells(cats: int, classes: int, steps: int) -> int:
    """``GS``: the doubles a group's block of one level holds."""
    return 3 * cats * classes + len(PLANES) * cats + 2 + (len(PLANES) + 1) * steps


def table_views(table: Tensor, cats: int, classes: int, steps: int) -> dict[str, Tensor]:
    """Views into one level's ``[G, GS]`` block: ``n``, ``qsum``, ``psum`` ``[G, K, C]``; ``post_entropy``, ``prior_entropy``, ``kl``,
    ``cross``, ``switches`` ``[G, K]``; ``frames``, ``pairs`` ``[G]``; ``positions`` ``[G, 5, T]``; ``counts`` ``[G, T]``."""
    g, kc, p = table.shape[0], cats * classes, len(PLANES)
    out = {name: table[:, i * kc : (i + 1) * kc].reshape(g, cats, classes) for i, name in enumerate(("n", "qsum", "psum"))}
    at = 3 * kc
    for i, name in enumerate(PLANES):
        out[name] = table[:, at + i * cats : at + (i + 1) * cats]
    at += p * cats
    out["frames"], out["pairs"] = table[:, at], table[:, at + 1]
    out["positions"] = table[:, at + 2 : at + 2 + p * steps].reshape(g, p, steps)
    out["counts"] = table[:, at + 2 + p * steps :]
    return out


_WS: dict[tuple[int, int], Tensor] = {}
_WS_CACHED_BYTES = 64 << 20  # a larger call takes a tensor of its own


def _workspace(device: torch.device, nbytes: int) -> Tensor:
    """The census kernel's workspace on the current stream of ``device`` (float64 words, >= nbytes): one cached buffer per (device,
    stream) where it fits, a tensor per call above ``_WS_CACHED_BYTES``.  Calls on one stream run in order, so they can share it."""
    words = (nbytes + 7) // 8
    if nbytes > _WS_CACHED_BYTES:
        return torch.empty(words, dtype=torch.float64, device=device)
    key = (torch.device(device).index or 0, _lib.stream_ptr(device))
    ws = _WS.get(key)
    if ws is None or ws.numel() < words:
        ws = _WS[key] = torch.empty(words, dtype=torch.float64, device=device)
    return ws


def _left_fold(x: Tensor) -> Tensor:
    """The sum over the last dimension, one add per element in ascending order."""
    total = x[..., 0]
    for i in range(1, x.shape[-1]):
        total = total + x[..., i]
    return total


def _log_softmax(x: Tensor) -> Tensor:
    """``(x - max) - log(sum exp(x - max))`` with the sum a left fold, as the kernels form it."""
    m = x.max(-1, keepdim=True).values
    return (x - m) - torch.log(_left_fold(torch.exp(x - m))).unsqueeze(-1)


class LatentCensus(ObservingConfig):
    """``LatentCensus(observe=("both",), active_nats=0.01)``: which posteriors are counted.  Copy ``g`` of every row observes subset
    ``observe[g]`` on every live step (and at frame 0); the copies share the row's uniforms, so the subsets differ only in what they
    observe, and ``cross`` of copy ``g > 0`` is ``KL(q_observe[0] || q_observe[g])``.  A categorical is *active* when its mean KL per
    live frame exceeds ``active_nats``."""

    def __init__(self, observe: tuple[str, ...] = ("both",), active_nats: float = 0.01) -> None:
        if (isinstance(observe, str) or not isinstance(observe, (tuple, list)) or not observe or len(observe) > MAX_GROUPS
                or any(not isinstance(o, str) or o not in OBSERVE_BITS for o in observe) or len(set(observe)) != len(tuple(observe))):
            msg = f"observe must be a non-empty tuple of at most {MAX_GROUPS} distinct keys out of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        if isinstance(active_nats, bool) or not isinstance(active_nats, (int, float)) or not math.isfinite(active_nats) or active_nats < 0:
            msg = f"active_nats must be a finite number >= 0, got {active_nats!r}"
            raise ValueError(msg)
        self.observe, self.active_nats = tuple(observe), float(active_nats)
        self.group = None  # the process group CensusTable.all_reduce uses (FlatDataParallel.census binds it)

    def __repr__(self) -> str:
        return f"LatentCensus(observe={self.observe!r}, active_nats={self.active_nats})"

    @property
    def samples(self) -> int:
        """Copies of a row in the rollout: one per observed subset."""
        return len(self.observe)

    groups = samples

    def plan(self):  # noqa: ANN201
        """Copy ``g`` of a row observes ``observe[g]`` on every live frame; the copies share the row's uniforms (the model's own shapes)."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(self.groups, self.bits, None)

    # -- the rule in torch, in float64 -------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, groups: int, cats: int, classes: int,  # noqa: PLR0913
                 valid: Tensor | None, table: Tensor | None) -> tuple[int, int]:
        if isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= MAX_GROUPS or cats < 1 or classes < 1:
            msg = f"need 1 <= G <= {MAX_GROUPS} and K, C >= 1, got G {groups!r}, K {cats}, C {classes}"
            raise ValueError(msg)
        if post_logits.dim() != 3 or post_logits.shape[-1] != cats * classes or post_logits.numel() == 0 or post_logits.shape[0] % groups:  # noqa: PLR2004
            msg = (f"the logits must be [B * {groups}, T, {cats * classes}] (G = {groups} copies per row, K = {cats} categoricals of "
                   f"C = {classes} classes), got {tuple(post_logits.shape)}")
            raise ValueError(msg)
        if (prior_logits.shape != post_logits.shape or stoch.shape != post_logits.shape
                or any(x.dtype != torch.float32 or x.device != post_logits.device for x in (post_logits, prior_logits, stoch))):
            msg = (f"post_logits, prior_logits and stoch must be float32 tensors of one shape on one device, got {tuple(post_logits.shape)}, "
                   f"{tuple(prior_logits.shape)}, {tuple(stoch.shape)}")
            raise ValueError(msg)
        rows, steps = post_logits.shape[:2]
        if rows * steps >= _EXACT or post_logits.numel() >= 1 << 31:
            msg = f"logits {tuple(post_logits.shape)}: need B * G * T < 2^24 and B * G * T * K * C < 2^31"
            raise ValueError(msg)
        batch = rows // groups
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (batch,) or valid.device != post_logits.device):
            msg = f"valid must be an int32 tensor of shape ({batch},) on {post_logits.device}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}"
            raise ValueError(msg)
        want = (groups, group_cells(cats, classes, steps))
        if table is not None and (tuple(table.shape) != want or table.dtype != torch.float64 or not table.is_contiguous()
                                  or table.device != post_logits.device):
            msg = f"table must be a contiguous float64 {want} buffer on {post_logits.device}, got {table.dtype} {tuple(table.shape)} on {table.device}"
            raise ValueError(msg)
        return batch, steps

    @staticmethod
    def reference(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, groups: int, cats: int, classes: int,  # noqa: PLR0913, PLR0914
                  valid: Tensor | None = None, table: Tensor | None = None) -> tuple[Tensor, Tensor]:
        """The rule in float64 on any device, in the kernel's fold order: ``(planes [5, B * G, T] float64, table [G, GS])``.  The
        inputs are ``[B * G, T, K * C]``, ``valid`` int32 ``[B]`` (None: every frame is live); ``table`` (float64 ``[G, GS]``) is added
        onto in place, a new one is made when it is None.  The position sums are taken of the planes rounded to fp32."""
        b, t = LatentCensus._checked(post_logits, prior_logits, stoch, groups, cats, classes, valid, table)
        dev, g, f64 = post_logits.device, groups, torch.float64
        zero = torch.zeros((), dtype=f64, device=dev)
        length = torch.full((b,), t, device=dev, dtype=torch.int64) if valid is None else valid.to(torch.int64).clamp(0, t)
        live = torch.arange(t, device=dev) < length.unsqueeze(1)  # [B, T]
        lq = _log_softmax(post_logits.to(f64).reshape(b, g, t, cats, classes))
        lp = _log_softmax(prior_logits.to(f64).reshape(b, g, t, cats, classes))
        q, p = lq.exp(), lp.exp()
        lq0, q0 = lq[:, :1], q[:, :1]
        star = (stoch.reshape(b, g, t, cats, classes) > 0.5).to(torch.int8).argmax(-1)  # noqa: PLR2004  (the first maximum)
        switch = torch.zeros(b, g, t, cats, dtype=f64, device=dev)
        switch[:, :, 1:] = (star[:, :, 1:] != star[:, :, :-1]).to(f64)
        per_cat = torch.stack([
            -_left_fold(torch.where(q > 0, q * lq, zero)), -_left_fold(torch.where(p > 0, p * lp, zero)),
            _left_fold(torch.where(q > 0, q * (lq - lp), zero)), _left_fold(torch.where(q0 > 0, q0 * (lq0 - lq), zero)), switch], dim=3)  # [B, G, T, 5, K]
        live5 = live[:, None, :, None]
        planes = torch.where(live5, _left_fold(per_cat), zero).permute(3, 0, 1, 2).reshape(len(PLANES), b * g, t)
        onehot = torch.nn.functional.one_hot(star.to(torch.int64), classes).to(f64)
        cells = torch.cat([x.reshape(b, g, t, -1) for x in (onehot, q, p, per_cat)], dim=3)  # [B, G, T, PS]
        cells = torch.where(live[:, None, :, None], cells, zero)
        partial = torch.zeros(b, g, cells.shape[-1], dtype=f64, device=dev)
        for i in range(t):  # (a row's left fold over its frames; a dead frame adds +0)
            partial = partial + cells[:, :, i]
        if table is None:
            table = torch.zeros(g, group_cells(cats, classes, t), dtype=f64, device=dev)
        ps = partial.shape[-1]
        views = table_views(table, cats, classes, t)
        rounded = planes.to(torch.float32).to(f64).reshape(len(PLANES), b, g, t)
        cells_sum, positions = torch.zeros(g, ps, dtype=f64, device=dev), torch.zeros(g, len(PLANES), t, dtype=f64, device=dev)
        for row in range(b):  # (the step's sums: the rows in ascending b from +0, one add each)
            cells_sum = cells_sum + partial[row]
            positions = positions + rounded[:, row].permute(1, 0, 2)
        table[:, :ps] += cells_sum  # (one add onto what the table holds)
        views["positions"] += positions
        views["frames"] += length.sum().to(f64)
        views["pairs"] += (length - 1).clamp(min=0).sum().to(f64)
        views["counts"] += live.sum(0).to(f64)
        return planes, table

    # -- the kernel on the GPU, the rule elsewhere -----------------------------------------------------------------------------------------
    @staticmethod
    def fold(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, groups: int, cats: int, classes: int, valid: Tensor | None = None, *,  # noqa: PLR0913
             table: Tensor | None = None, planes: bool = True) -> tuple[Tensor | None, Tensor]:
        """One ``mtrssm_latent_census`` call (two launches, nothing read back) on torch's current stream; non-GPU tensors take
        ``reference``.  Returns ``(planes, table)``: the planes fp32 ``[5, B * G, T]`` (None without ``planes``) and the level's
        accumulators ``[G, GS]`` float64 -- ``table`` with this step added in place, or a new one."""
        b, t = LatentCensus._checked(post_logits, prior_logits, stoch, groups, cats, classes, valid, table)
        if not post_logits.is_cuda:
            got, table = LatentCensus.reference(post_logits, prior_logits, stoch, groups, cats, classes, valid, table)
            return (got.to(torch.float32) if planes else None), table
        lib, dev = _lib.load(), post_logits.device
        need = int(lib.mtrssm_latent_census_workspace_bytes(b, groups, t, cats, classes))
        if need < 0:
            msg = f"latent census: B {b}, G {groups}, T {t}, K {cats}, C {classes} are out of range"
            raise ValueError(msg)
        ws = _workspace(dev, need)
        post_logits, prior_logits, stoch = post_logits.contiguous(), prior_logits.contiguous(), stoch.contiguous()
        valid = None if valid is None else valid.contiguous()
        if table is None:
            table = torch.zeros(groups, group_cells(cats, classes, t), dtype=torch.float64, device=dev)
        out = torch.empty(len(PLANES), b * groups, t, device=dev, dtype=torch.float32) if planes else None
        _lib.check(_lib.TIMERS.call("mtrssm_latent_census", lib.mtrssm_latent_census, _lib.ptr(post_logits), _lib.ptr(prior_logits), _lib.ptr(stoch),
                                    _lib.index_ptr(valid), b, groups, t, cats, classes, _lib.ptr(out), _lib.raw_ptr(table), ws.data_ptr(), ws.numel() * 8,
                                    _lib.stream_ptr(dev), nbytes=16.0 * b * groups * t * cats * classes), "mtrssm_latent_census")
        return out, table


def _entropy(x: Tensor) -> Tensor:
    """``-sum x log x`` over the last dimension; a zero adds 0."""
    return -torch.where(x > 0, x * torch.log(x.clamp_min(torch.finfo(x.dtype).tiny)), torch.zeros_like(x)).sum(-1)


class CensusTable(SumTable):
    """The accumulated census of any number of steps in ONE float64 buffer: per level ``(name, K, C)`` of ``levels`` a ``[G, GS]`` block
    (``level_view``), one after the other.  MRSSM: ``(("", K, C),)``; MMTRSSM: ``"l"`` and ``"h"``.  A step run with ``keep_states``
    also leaves its planes (``planes``: per level fp32 ``[5, B * G, T]``), what the fold read (``inputs``: per level the raw
    ``post_logits``, ``prior_logits``, ``post_stoch``; ``valid``) and its rollout (``states``) here; otherwise they are None."""

    def __init__(self, levels: tuple[tuple[str, int, int], ...], groups: int, steps: int, device: torch.device | str = "cpu",
                 observe: tuple[str, ...] | None = None) -> None:
        levels = tuple((str(name), int(k), int(c)) for name, k, c in levels)
        if not levels or any(k < 1 or c < 1 for _, k, c in levels) or not 1 <= groups <= MAX_GROUPS:
            msg = f"need at least one level of K, C >= 1 and 1 <= groups <= {MAX_GROUPS}, got {levels!r} and {groups}"
            raise ValueError(msg)
        if observe is not None and len(observe) != groups:
            msg = f"{groups} groups need {groups} names, got {observe!r}"
            raise ValueError(msg)
        self.levels, self.groups, self._steps = levels, groups, self._checked_steps(steps)
        self.observe = tuple(observe) if observe is not None else (("both", "audio", "vision")[:groups] if groups <= 3 else  # noqa: PLR2004
                                                                   tuple(f"g{i}" for i in range(groups)))
        self.active_nats = 0.01  # (model.latent_census sets its config's)
        sizes = [groups * group_cells(k, c, steps) for _, k, c in levels]
        self._offsets = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
        self.buffer = torch.zeros(self._offsets[-1], dtype=torch.float64, device=device)
        self.planes: list[Tensor] | None = None
        self.inputs: list[tuple[Tensor, Tensor, Tensor]] | None = None
        self.valid: Tensor | None = None
        self.states = None

    @property
    def steps(self) -> int:
        return self._steps

    def _sizes(self, other: SumTable) -> str:
        return f"{self.levels}, {self.groups} groups, {self.steps} steps and {getattr(other, 'levels', '?')}, {getattr(other, 'groups', '?')} groups, {other.steps} steps"

    def add(self, other):  # noqa: ANN001, ANN201
        if (getattr(other, "levels", None), getattr(other, "groups", None), other.steps) != (self.levels, self.groups, self.steps):
            msg = f"tables of {self._sizes(other)} do not add"
            raise ValueError(msg)
        return super().add(other)

    def level_view(self, level: int) -> Tensor:
        """Level ``level``'s accumulators ``[G, GS]``: a contiguous view of the buffer (what ``LatentCensus.fold`` adds onto)."""
        _, k, c = self.levels[level]
        return self.buffer[self._offsets[level] : self._offsets[level + 1]].view(self.groups, group_cells(k, c, self.steps))

    def views(self, level: int) -> dict[str, Tensor]:
        """``table_views`` of level ``level``."""
        _, k, c = self.levels[level]
        return table_views(self.level_view(level), k, c, self.steps)

    def usage(self) -> dict[str, Tensor]:
        """Per level ``n / frames``, ``[G, K, C]``: how often categorical ``k`` sampled class ``c``; NaN for an empty table."""
        out = {}
        for i, (name, _, _) in enumerate(self.levels):
            v = self.views(i)
            out[name] = self._mean(v["n"], v["frames"][:, None, None])
        return out

    def per_categorical(self) -> dict[str, dict[str, Tensor]]:
        """Per level a dict of ``[G, K]`` float64 tensors: ``perplexity`` (``exp`` of the usage's entropy), ``unused`` (classes never
        sampled), ``marginal_entropy`` (of ``qsum / frames``), ``mi`` (``marginal_entropy - post_entropy``: ``>= 0`` and ``<= log C`` up
        to rounding), ``prior_gap`` (``KL(qsum / frames || psum / frames)``), ``kl``, ``post_entropy``, ``prior_entropy``, ``cross``
        (means per live frame), ``active`` (1.0 where ``kl > active_nats``), ``switch_rate`` (``sw / pairs``) and ``dwell``
        (``1 / switch_rate``, ``inf`` when nothing switched).  An empty table gives NaN."""
        out = {}
        nan = float("nan")
        for i, (name, _, _) in enumerate(self.levels):
            v = self.views(i)
            frames, pairs = v["frames"][:, None], v["pairs"][:, None]
            have = frames > 0
            usage = self._mean(v["n"], frames[:, :, None])
            marginal, prior = self._mean(v["qsum"], frames[:, :, None]), self._mean(v["psum"], frames[:, :, None])
            res = {name_: self._mean(v[name_], frames) for name_ in ("post_entropy", "prior_entropy", "kl", "cross")}
            res["perplexity"] = torch.where(have, torch.exp(_entropy(usage)), nan)
            res["unused"] = torch.where(have, (v["n"] == 0).sum(-1).to(torch.float64), nan)
            res["marginal_entropy"] = torch.where(have, _entropy(marginal), nan)
            res["mi"] = res["marginal_entropy"] - res["post_entropy"]
            tiny = torch.finfo(torch.float64).tiny
            gap = torch.where(marginal > 0, marginal * (torch.log(marginal.clamp_min(tiny)) - torch.log(prior)), torch.zeros_like(marginal)).sum(-1)
            res["prior_gap"] = torch.where(have, gap, nan)
            res["active"] = torch.where(have, (res["kl"] > self.active_nats).to(torch.float64), nan)
            res["switch_rate"] = self._mean(v["switches"], pairs)
            res["dwell"] = 1.0 / res["switch_rate"]
            out[name] = res
        return out

    def curves(self) -> dict[str, dict[str, Tensor]]:
        """Per level ``{plane: [G, T]}``: the planes' mean over the rows that are live at frame ``t``; an empty bin gives NaN."""
        out = {}
        for i, (name, _, _) in enumerate(self.levels):
            v = self.views(i)
            out[name] = {plane: self._mean(v["positions"][:, j], v["counts"]) for j, plane in enumerate(PLANES)}
        return out

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix[/level][/observe]/{post_entropy,prior_entropy,kl,cross,perplexity,mi,prior_gap,switch_rate,unused,active}``, fp32:
        means over ``k``, except ``unused`` and ``active``, which are sums over ``k``.  The ``/observe`` part appears only with more than
        one group, ``cross`` only for ``g > 0``."""
        out = {}
        for name, per in self.per_categorical().items():
            for g, subset in enumerate(self.observe):
                base = prefix + (f"/{name}" if name else "") + (f"/{subset}" if self.groups > 1 else "")
                for key in ("post_entropy", "prior_entropy", "kl", "cross", "perplexity", "mi", "prior_gap", "switch_rate"):
                    if key != "cross" or g > 0:
                        out[f"{base}/{key}"] = per[key][g].mean().to(torch.float32)
                for key in ("unused", "active"):
                    out[f"{base}/{key}"] = per[key][g].sum().to(torch.float32)
        return out


__all__ = ["PLANES", "CensusTable", "LatentCensus", "group_cells", "table_views"]
