"""Generation coherence: do the two decodes of a sampled rollout read as the same digit, and as the right one.

A *coherence step* gives row ``b`` ``G * S`` copies (``1 <= G <= 4`` observed subsets, ``1 <= S <= 16`` samples each).  Copy ``g * S + s``
observes ``observe[g]`` on the first ``context`` frames (and at frame 0) and runs open loop after them; the copies of a row share its
initial uniforms and ``u_post`` on the context and read their own ``u_tail[b, g * S + s]`` after it; copy ``c`` of row ``b`` is scan row
``b * G * S + c``.  With ``observe[0] == "both"`` the first ``S`` copies are ``ForecastSkill(context, samples=S)``'s rollout.  Both decodes
of every copy-frame are read by a ``DigitClassifier`` each (``zv`` / ``za``: the 10 fp32 logits of the vision / audio reader).

A frame ``(b, t)`` is live iff ``t < clamp(valid[b], 0, T)`` and ``0 <= labels[b, t] <= 9``; a dead frame adds exactly nothing.  With
``c = min(context, T)`` frame ``t`` has horizon ``h = 0`` for ``t < c`` (phase 0, "observed") and ``h = t - c + 1`` after it (phase 1,
"open"): ``skill.py``'s convention.  Per copy of a live frame, in double:

    dv     = the lowest index among the largest zv, or 10 (the failure bin) when any of the 10 is not finite; da likewise
    vision = [dv == label]      audio = [da == label]      agree = [dv == da and dv < 10]      joint = [dv == da == label]
    pv_k   = exp(zv_k - max) / (left fold over ascending k of exp(zv_k - max)); pa_k likewise
    soft   = left fold over ascending k of pv_k * pa_k, exactly 0 when either reader failed
    pairs[phase][dv][da] += 1

**Frame planes** ``[5, B * G, T]`` fp32 (``PLANES``): for ``(b, g, t)`` the left fold from +0 over ``s = 0 .. S - 1`` of the per-copy value,
divided by ``S`` and rounded to fp32 once; exactly 0 on a dead frame.

**The table**, per group in double (``[G, GS]``, ``GS = 6 T + 2 * 121``; steps add up in the same buffer): ``sums [5][T]`` by horizon (the
per-copy values added up, not the means), ``counts [T]`` (live copy-frames per horizon: ``S`` per live frame) and ``pairs [2][11][11]``.

**Fold order**, fixed by the shapes alone: ``u[p][b][g][t]`` is the left fold over ``s`` of the per-copy doubles (+0 on a dead frame);
cell ``(g, p, h)`` is a left fold from +0 over ``b`` ascending and, within a row, over ``t`` ascending, of the frames with ``h(t) = h``
(a dead frame's +0 changes nothing); the result is added, in one add, onto what the buffer holds.  So a second call of the same step
doubles the table exactly and two steps into one table are the ``add`` of two tables.  Every cell but ``soft`` is a whole number, exact
while a table has seen fewer than 2^24 copy-frames per cell (the bound the census states; a double holds whole numbers up to 2^53).
``GenerationCoherence.reference`` states all of this in torch, in float64; ``mtrssm_coherence_fold`` is the kernel, used for GPU tensors;
elsewhere the torch rule runs.  ``CoherenceTable`` derives rates by horizon, failed reads and Cohen's kappa from the buffer alone.
"""

from __future__ import annotations

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.census import MAX_GROUPS, _left_fold, _workspace
from multimodal_mtrssm_amd.skill import MAX_SAMPLES, OBSERVE_BITS, ObservingConfig, SumTable

PLANES = ("vision", "audio", "agree", "joint", "soft")
PHASES = ("obs", "open")
CLASSES = 10
BINS = CLASSES + 1  # the ten digits and the failure bin
_EXACT = 1 << 24


def group_cells(steps: int) -> int:
    """``GS``: the doubles a group's block holds."""
    return (len(PLANES) + 1) * steps + len(PHASES) * BINS * BINS


def table_views(table: Tensor, steps: int) -> dict[str, Tensor]:
    """Views into a ``[G, GS]`` table: ``sums [G, 5, T]``, ``counts [G, T]``, ``pairs [G, 2, 11, 11]``."""
    g, p = table.shape[0], len(PLANES)
    return {"sums": table[:, : p * steps].reshape(g, p, steps), "counts": table[:, p * steps : (p + 1) * steps],
            "pairs": table[:, (p + 1) * steps :].reshape(g, len(PHASES), BINS, BINS)}


def _first_max(z: Tensor) -> tuple[Tensor, Tensor]:
    """``(digit int64, ok bool)`` over the last dimension: the lowest index among the largest, 10 where a value is not finite."""
    ok = torch.isfinite(z).all(-1)
    safe = torch.where(ok.unsqueeze(-1), z, torch.zeros_like(z))
    first = (safe == safe.max(-1, keepdim=True).values).to(torch.int8).argmax(-1)  # (argmax: the first maximum)
    return torch.where(ok, first, torch.full_like(first, CLASSES)), ok


def _softmax(z: Tensor, ok: Tensor) -> Tensor:
    """``exp(z - max) / sum`` with the sum a left fold, as the kernel forms it; a failed read is softmaxed as zeros (and masked later)."""
    safe = torch.where(ok.unsqueeze(-1), z, torch.zeros_like(z))
    e = torch.exp(safe - safe.max(-1, keepdim=True).values)
    return e / _left_fold(e).unsqueeze(-1)


class GenerationCoherence(ObservingConfig):
    """``GenerationCoherence(context, samples=S, observe=("both", "audio", "vision"))``: every row observes ``context >= 1`` frames of
    ``observe[g]`` in its copies ``g * S .. g * S + S - 1``, which then run open loop as ``S`` sampled futures.  ``max_frames``: the
    decoders and the readers run over chunks of whole rows (all ``G * S`` copies of a row together) of at most this many frames."""

    def __init__(self, context: int, samples: int = 1, observe: tuple[str, ...] = ("both", "audio", "vision")) -> None:
        if isinstance(context, bool) or not isinstance(context, int) or not 1 <= context < 1 << 31:
            msg = f"context must be an integer 1 <= q < 2^31 (frame 0 is always observed), got {context!r}"
            raise ValueError(msg)
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
            msg = f"samples must be an integer in 1 .. {MAX_SAMPLES}, got {samples!r}"
            raise ValueError(msg)
        if (isinstance(observe, str) or not isinstance(observe, (tuple, list)) or not observe or len(observe) > MAX_GROUPS
                or any(not isinstance(o, str) or o not in OBSERVE_BITS for o in observe) or len(set(observe)) != len(tuple(observe))):
            msg = f"observe must be a non-empty tuple of at most {MAX_GROUPS} distinct keys out of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        self.context, self.samples, self.observe = context, samples, tuple(observe)
        self.max_frames = 4096
        self.group = None  # the process group CoherenceTable.all_reduce uses (FlatDataParallel.coherence binds it)

    def __repr__(self) -> str:
        return f"GenerationCoherence({self.context}, samples={self.samples}, observe={self.observe!r})"

    @property
    def groups(self) -> int:
        """The observed subsets: ``S`` copies of a row each."""
        return len(self.observe)

    @property
    def copies(self) -> int:
        """Copies of a row in the rollout: ``G * S``."""
        return self.groups * self.samples

    def plan(self):  # noqa: ANN201
        """Copy ``g * S + s`` of a row observes ``observe[g]`` on the context; the copies share the row's initial uniforms and ``u_post`` on
        the context and read their own ``u_tail[b, g * S + s]`` after it."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        bits = tuple(b for b in self.bits for _ in range(self.samples))
        return CopyPlan(self.copies, bits, self.context, init="row", post="tail")

    # -- the rule in torch, in float64 -------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked(logits_v: Tensor, logits_a: Tensor, labels: Tensor, groups: int, samples: int, context: int,  # noqa: PLR0913
                 valid: Tensor | None, table: Tensor | None) -> tuple[int, int]:
        if (isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= MAX_GROUPS or isinstance(samples, bool)
                or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES or isinstance(context, bool) or not isinstance(context, int)
                or not 1 <= context < 1 << 31):
            msg = f"need 1 <= G <= {MAX_GROUPS}, 1 <= S <= {MAX_SAMPLES} and 1 <= context < 2^31, got G {groups!r}, S {samples!r}, context {context!r}"
            raise ValueError(msg)
        copies = groups * samples
        if logits_v.dim() != 3 or logits_v.shape[-1] != CLASSES or logits_v.numel() == 0 or logits_v.shape[0] % copies:  # noqa: PLR2004
            msg = (f"the logits must be [B * {copies}, T, {CLASSES}] (G = {groups} groups of S = {samples} copies per row), "
                   f"got {tuple(logits_v.shape)}")
            raise ValueError(msg)
        if logits_a.shape != logits_v.shape or any(x.dtype != torch.float32 or x.device != logits_v.device for x in (logits_v, logits_a)):
            msg = (f"both readers' logits must be float32 tensors of one shape on one device, got {tuple(logits_v.shape)} and "
                   f"{tuple(logits_a.shape)}")
            raise ValueError(msg)
        rows, steps = logits_v.shape[:2]
        if rows * steps >= _EXACT:
            msg = f"logits {tuple(logits_v.shape)}: need B * G * S * T < 2^24"
            raise ValueError(msg)
        batch, dev = rows // copies, logits_v.device
        if tuple(labels.shape) != (batch, steps) or labels.dtype != torch.int32 or labels.device != dev:
            msg = f"labels must be an int32 tensor of shape {(batch, steps)} on {dev}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}"
            raise ValueError(msg)
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (batch,) or valid.device != dev):
            msg = f"valid must be an int32 tensor of shape ({batch},) on {dev}, got {valid.dtype} {tuple(valid.shape)} on {valid.device}"
            raise ValueError(msg)
        want = (groups, group_cells(steps))
        if table is not None and (tuple(table.shape) != want or table.dtype != torch.float64 or not table.is_contiguous() or table.device != dev):
            msg = f"table must be a contiguous float64 {want} buffer on {dev}, got {table.dtype} {tuple(table.shape)} on {table.device}"
            raise ValueError(msg)
        return batch, steps

    @staticmethod
    def _rule(logits_v: Tensor, logits_a: Tensor, labels: Tensor, groups: int, samples: int, context: int,  # noqa: PLR0913, PLR0914
              valid: Tensor | None, table: Tensor | None) -> tuple[Tensor, Tensor, Tensor]:
        """``(planes, table, u)``: ``u`` float64 ``[5, B * G, T]`` are the frame sums the table is folded from."""
        b, t = GenerationCoherence._checked(logits_v, logits_a, labels, groups, samples, context, valid, table)
        dev, g, s, f64 = logits_v.device, groups, samples, torch.float64
        zero = torch.zeros((), dtype=f64, device=dev)
        length = torch.full((b,), t, device=dev, dtype=torch.int64) if valid is None else valid.to(torch.int64).clamp(0, t)
        lab = labels.to(torch.int64)
        live = (torch.arange(t, device=dev) < length.unsqueeze(1)) & (lab >= 0) & (lab < CLASSES)  # [B, T]
        zv, za = logits_v.to(f64).reshape(b, g, s, t, CLASSES), logits_a.to(f64).reshape(b, g, s, t, CLASSES)
        (dv, ok_v), (da, ok_a) = _first_max(zv), _first_max(za)
        word = lab[:, None, None, :]
        soft = torch.where(ok_v & ok_a, _left_fold(_softmax(zv, ok_v) * _softmax(za, ok_a)), zero)
        per_copy = torch.stack([(dv == word).to(f64), (da == word).to(f64), ((dv == da) & (dv < CLASSES)).to(f64),
                                ((dv == da) & (dv == word)).to(f64), soft])  # [5, B, G, S, T]
        live5 = live[None, :, None, None, :]
        per_copy = torch.where(live5, per_copy, zero)
        u = _left_fold(per_copy.permute(0, 1, 2, 4, 3))  # [5, B, G, T]: the left fold over s
        planes = (u / float(s)).reshape(len(PLANES), b * g, t)
        c = min(context, t)
        sums = torch.zeros(g, len(PLANES), t, dtype=f64, device=dev)
        head = torch.zeros(len(PLANES), g, dtype=f64, device=dev)
        tail = torch.zeros(len(PLANES), g, t - c, dtype=f64, device=dev)
        for row in range(b):  # (ascending b; within a row ascending t: bin 0 takes the row's context frames one by one)
            for i in range(c):
                head = head + u[:, row, :, i]
            tail = tail + u[:, row, :, c:]
        sums[:, :, 0] = head.permute(1, 0)
        sums[:, :, 1 : t - c + 1] = tail.permute(1, 0, 2)
        frames = torch.zeros(t, dtype=f64, device=dev)
        frames[0] = live[:, :c].sum().to(f64)
        frames[1 : t - c + 1] = live[:, c:].sum(0).to(f64)
        phase = (torch.arange(t, device=dev) >= c).to(torch.int64)
        cell = ((torch.arange(g, device=dev)[None, :, None, None] * len(PHASES) + phase) * BINS + dv) * BINS + da  # [B, G, S, T]
        keep = live[:, None, None, :].expand(b, g, s, t)
        pairs = torch.bincount(cell[keep], minlength=g * len(PHASES) * BINS * BINS).reshape(g, len(PHASES), BINS, BINS).to(f64)
        if table is None:
            table = torch.zeros(g, group_cells(t), dtype=f64, device=dev)
        views = table_views(table, t)
        views["sums"] += sums  # (one add onto what the table holds)
        views["counts"] += frames * float(s)
        views["pairs"] += pairs
        return planes, table, u.reshape(len(PLANES), b * g, t)

    @staticmethod
    def reference(logits_v: Tensor, logits_a: Tensor, labels: Tensor, groups: int, samples: int, context: int,  # noqa: PLR0913
                  valid: Tensor | None = None, table: Tensor | None = None) -> tuple[Tensor, Tensor]:
        """The rule in float64 on any device, in the kernel's fold order: ``(planes [5, B * G, T] float64, table [G, GS])``.  The logits
        are fp32 ``[B * G * S, T, 10]`` in scan-row order, ``labels`` int32 ``[B, T]``, ``valid`` int32 ``[B]`` (None: no row ends early);
        ``table`` (float64 ``[G, GS]``) is added onto in place, a new one is made when it is None."""
        planes, table, _ = GenerationCoherence._rule(logits_v, logits_a, labels, groups, samples, context, valid, table)
        return planes, table

    # -- the kernel on the GPU, the rule elsewhere -----------------------------------------------------------------------------------------
    @staticmethod
    def fold(logits_v: Tensor, logits_a: Tensor, labels: Tensor, groups: int, samples: int, context: int, valid: Tensor | None = None, *,  # noqa: PLR0913
             table: Tensor | None = None, planes: bool = True, frame_sums: bool = False) -> tuple[Tensor | None, ...]:
        """One ``mtrssm_coherence_fold`` call (two launches, nothing read back) on torch's current stream; non-GPU tensors take
        ``reference``.  Returns ``(planes, table)``: the planes fp32 ``[5, B * G, T]`` (None without ``planes``) and the accumulators
        ``[G, GS]`` float64 -- ``table`` with this step added in place, or a new one.  ``frame_sums``: a third entry, the float64 frame
        sums ``u [5, B * G, T]`` the table was folded from (a copy of the head of the kernel's workspace)."""
        b, t = GenerationCoherence._checked(logits_v, logits_a, labels, groups, samples, context, valid, table)
        if not logits_v.is_cuda:
            got, table, u = GenerationCoherence._rule(logits_v, logits_a, labels, groups, samples, context, valid, table)
            out = ((got.to(torch.float32) if planes else None), table)
            return (*out, u) if frame_sums else out
        lib, dev = _lib.load(), logits_v.device
        need = int(lib.mtrssm_coherence_fold_workspace_bytes(b, groups, samples, t))
        if need < 0:
            msg = f"coherence fold: B {b}, G {groups}, S {samples}, T {t} are out of range"
            raise ValueError(msg)
        ws = _workspace(dev, need)
        logits_v, logits_a, labels = logits_v.contiguous(), logits_a.contiguous(), labels.contiguous()
        valid = None if valid is None else valid.contiguous()
        if table is None:
            table = torch.zeros(groups, group_cells(t), dtype=torch.float64, device=dev)
        out = torch.empty(len(PLANES), b * groups, t, device=dev, dtype=torch.float32) if planes else None
        _lib.check(_lib.TIMERS.call("mtrssm_coherence_fold", lib.mtrssm_coherence_fold, _lib.ptr(logits_v), _lib.ptr(logits_a), _lib.index_ptr(labels),
                                    _lib.index_ptr(valid), b, groups, samples, t, context, _lib.ptr(out), _lib.raw_ptr(table), ws.data_ptr(),
                                    ws.numel() * 8, _lib.stream_ptr(dev), nbytes=80.0 * b * groups * samples * t), "mtrssm_coherence_fold")
        if frame_sums:
            return out, table, ws[: len(PLANES) * b * groups * t].clone().reshape(len(PLANES), b * groups, t)
        return out, table


class CoherenceTable(SumTable):
    """The accumulated coherence of any number of steps in ONE float64 buffer ``[G, GS]`` (``views``: ``sums``, ``counts``, ``pairs``).  A
    step run with ``keep_states`` also leaves its planes (``planes``: fp32 ``[5, B * G, T]``), what the fold read (``logits``: the vision and
    the audio reader's ``[B * G * S, T, 10]``) and its rollout (``states``) here; otherwise they are None."""

    def __init__(self, groups: int, steps: int, device: torch.device | str = "cpu", observe: tuple[str, ...] | None = None) -> None:
        if isinstance(groups, bool) or not isinstance(groups, int) or not 1 <= groups <= MAX_GROUPS:
            msg = f"need 1 <= groups <= {MAX_GROUPS}, got {groups!r}"
            raise ValueError(msg)
        if observe is not None and len(observe) != groups:
            msg = f"{groups} groups need {groups} names, got {observe!r}"
            raise ValueError(msg)
        self.groups, self._steps = groups, self._checked_steps(steps)
        self.observe = tuple(observe) if observe is not None else (("both", "audio", "vision")[:groups] if groups <= 3 else  # noqa: PLR2004
                                                                   tuple(f"g{i}" for i in range(groups)))
        self.buffer = torch.zeros(groups, group_cells(steps), dtype=torch.float64, device=device)
        self.planes: Tensor | None = None
        self.logits: tuple[Tensor, Tensor] | None = None
        self.states = None

    @property
    def steps(self) -> int:
        return self._steps

    def _sizes(self, other: SumTable) -> str:
        return f"{self.groups} groups, {self.steps} steps and {getattr(other, 'groups', '?')} groups, {other.steps} steps"

    def add(self, other):  # noqa: ANN001, ANN201
        if (getattr(other, "groups", None), other.steps) != (self.groups, self.steps):
            msg = f"tables of {self._sizes(other)} do not add"
            raise ValueError(msg)
        return super().add(other)

    def views(self) -> dict[str, Tensor]:
        """``table_views`` of the buffer."""
        return table_views(self.buffer, self.steps)

    def rates(self, group: int) -> dict[str, Tensor]:
        """The five planes by horizon ``[T]``: ``sums / counts``, NaN where nothing was counted."""
        v = self.views()
        return {plane: self._mean(v["sums"][group, i], v["counts"][group]) for i, plane in enumerate(PLANES)}

    def binned(self, group: int, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, Tensor]:
        """``rates`` over horizon bins: ``(1, 2, 4, 8)`` gives bin 0 and ``[1, 2) [2, 4) [4, 8) [8, T)``."""
        v, slices = self.views(), self._bin_slices(edges)
        counts = torch.stack([v["counts"][group, s].sum() for _, s in slices])
        return {plane: self._mean(torch.stack([v["sums"][group, i, s].sum() for _, s in slices]), counts) for i, plane in enumerate(PLANES)}

    def failed(self, group: int) -> dict[str, Tensor]:
        """The share of reads in bin 10 per modality, ``[2]`` (phase 0, phase 1) each; NaN for a phase without reads."""
        pairs = self.views()["pairs"][group]
        n = pairs.sum((1, 2))
        return {"vision": self._mean(pairs[:, CLASSES, :].sum(-1), n), "audio": self._mean(pairs[:, :, CLASSES].sum(-1), n)}

    def kappa(self, group: int, phase: int) -> Tensor:
        """Cohen's kappa of the two readers over the reads with ``d < 10``: ``(po - pe) / (1 - pe)`` with ``po = sum_d pairs[d][d] / n`` and
        ``pe = sum_d row_d col_d / n^2`` -- agreement above what two readers with these marginals reach by chance.  NaN for ``n = 0`` or
        ``pe = 1``."""
        m = self.views()["pairs"][group, phase, :CLASSES, :CLASSES]
        n = m.sum()
        po, pe = m.diagonal().sum() / n, (m.sum(1) * m.sum(0)).sum() / (n * n)
        return torch.where((n > 0) & (pe != 1), (po - pe) / (1 - pe), float("nan"))

    def scalars(self, prefix: str, edges: tuple[int, ...] = (1, 2, 4, 8)) -> dict[str, Tensor]:
        """``prefix/{observe[g]}/{plane}/{obs,h1,h2,...}``, ``prefix/{observe[g]}/kappa/{obs,open}``,
        ``prefix/{observe[g]}/failed/{vision,audio}`` (over both phases) and ``prefix/reads`` (the copy-frames counted), fp32."""
        names = [n for n, _ in self._bin_slices(edges)]
        v = self.views()
        out = {}
        for g, subset in enumerate(self.observe):
            binned = self.binned(g, edges)
            for plane in PLANES:
                for i, name in enumerate(names):
                    out[f"{prefix}/{subset}/{plane}/{name}"] = binned[plane][i].to(torch.float32)
            for phase, name in enumerate(PHASES):
                out[f"{prefix}/{subset}/kappa/{name}"] = self.kappa(g, phase).to(torch.float32)
            pairs = v["pairs"][g].sum(0)
            n = pairs.sum()
            out[f"{prefix}/{subset}/failed/vision"] = self._mean(pairs[CLASSES].sum(), n).to(torch.float32)
            out[f"{prefix}/{subset}/failed/audio"] = self._mean(pairs[:, CLASSES].sum(), n).to(torch.float32)
        out[f"{prefix}/reads"] = v["counts"].sum().to(torch.float32)
        return out


__all__ = ["PLANES", "CoherenceTable", "GenerationCoherence", "group_cells", "table_views"]
