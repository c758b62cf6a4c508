"""Latent quality: linear word probes on subset posteriors.

A *probe* reads a label (the digit being said) out of a latent feature with a linear classifier.  ``G`` classifiers run side by side,
one per observed subset (``both``, ``audio``, ``vision``): classifier ``g`` sees the features of the posterior that observes subset ``g``.

The rule.  ``x [G, N, ld]`` fp32, of which columns ``[col0, col0 + F)`` are read; ``labels`` int32 ``[N]`` shared by the groups, frame
``n`` live iff ``0 <= labels[n] < C`` (-1 = silence, or a frame past its row's end); ``weight [G, C, F]``, ``bias [G, C]``;
``2 <= C <= 16``.  Per group ``g`` and live frame ``n``:

    z = W_g x_n + b_g            nll = logsumexp(z) - z[label]         pred = the lowest index among the largest z
    hit = (pred == label)        stats[g] = (sum nll, sum hit, live count)
    g_weight[g] = sum_n (softmax(z) - onehot) x_n^T                    g_bias[g] = sum_n (softmax(z) - onehot)

(``normalize``: both gradients divided by ``max(count, 1)``: the gradient of the mean loss).  A dead frame has ``nll = hit = 0`` and
``pred = -1``, is not read and adds nothing; with no live frame every sum is exactly 0.  ``LinearProbe.rule`` states this in torch, in
float64; ``mtrssm_linear_probe_step`` is the kernel, used for GPU tensors; elsewhere the torch rule runs.
"""

from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor, nn

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.skill import OBSERVE_BITS, ForecastSkill, ObservingConfig, SumTable, observed_bits

MAX_CLASSES = 16
MAX_FEATURES = 2048  # the kernel stages 16 rows of F floats in LDS
PARTS = ("feature", "deter", "stoch", "higher", "lower")
_EXACT = 1 << 24


class ProbeStats(NamedTuple):
    """``nll_sum``, ``hits``, ``count``: ``[G]`` each (sums over the live frames); ``nll``, ``hit`` (fp) and ``pred`` (int32): ``[G, N]``
    per-frame planes, None unless asked for."""

    nll_sum: Tensor
    hits: Tensor
    count: Tensor
    nll: Tensor | None
    hit: Tensor | None
    pred: Tensor | None


class LinearProbe(nn.Module):
    """``LinearProbe(groups, features, classes=10)``: ``G`` linear classifiers ``[C, F]`` side by side, zero-initialised (the uniform
    classifier: ``nll = log C`` per frame)."""

    def __init__(self, groups: int, features: int, classes: int = 10) -> None:
        super().__init__()
        for name, value, lo, hi in (("groups", groups, 1, None), ("features", features, 1, None), ("classes", classes, 2, MAX_CLASSES)):
            if isinstance(value, bool) or not isinstance(value, int) or value < lo or (hi is not None and value > hi):
                msg = f"{name} must be an integer >= {lo}" + (f" and <= {hi}" if hi is not None else "") + f", got {value!r}"
                raise ValueError(msg)
        self.groups, self.features, self.classes = groups, features, classes
        self.weight = nn.Parameter(torch.zeros(groups, classes, features))
        self.bias = nn.Parameter(torch.zeros(groups, classes))
        self._flat = None
        self._workspace: Tensor | None = None

    def extra_repr(self) -> str:
        return f"groups={self.groups}, features={self.features}, classes={self.classes}"

    # -- the rule in torch, in float64 ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked(x: Tensor, labels: Tensor, weight: Tensor, bias: Tensor, col0: int) -> tuple[int, int, int, int, int]:
        if weight.dim() != 3 or bias.dim() != 2 or tuple(bias.shape) != tuple(weight.shape[:2]):  # noqa: PLR2004
            msg = f"weight must be [G, C, F] and bias [G, C], got {tuple(weight.shape)} and {tuple(bias.shape)}"
            raise ValueError(msg)
        g, c, f = weight.shape
        if not 2 <= c <= MAX_CLASSES or f < 1 or g < 1:  # noqa: PLR2004
            msg = f"need G, F >= 1 and 2 <= C <= {MAX_CLASSES}, got G {g}, C {c}, F {f}"
            raise ValueError(msg)
        if x.dim() != 3 or x.shape[0] != g or x.shape[1] < 1 or x.dtype != torch.float32:  # noqa: PLR2004
            msg = f"x must be a float32 [G = {g}, N >= 1, ld] tensor, got {x.dtype} {tuple(x.shape)}"
            raise ValueError(msg)
        n, ld = x.shape[1:]
        if isinstance(col0, bool) or not isinstance(col0, int) or col0 < 0 or col0 + f > ld:
            msg = f"columns [{col0}, {col0} + {f}) do not lie inside rows of {ld} floats"
            raise ValueError(msg)
        if n >= _EXACT or g * n * ld >= 1 << 31:
            msg = f"x {tuple(x.shape)}: need N < 2^24 and G * N * ld < 2^31"
            raise ValueError(msg)
        if labels.dtype != torch.int32 or tuple(labels.shape) != (n,) or labels.device != x.device:
            msg = f"labels must be an int32 tensor of shape ({n},) on {x.device}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}"
            raise ValueError(msg)
        return g, n, ld, c, f

    @staticmethod
    def rule(x: Tensor, labels: Tensor, weight: Tensor, bias: Tensor, *, col0: int = 0, grad: bool = True,  # noqa: PLR0913
             normalize: bool = True) -> tuple[ProbeStats, Tensor | None, Tensor | None]:
        """The rule in float64: ``(ProbeStats with all planes, g_weight, g_bias)`` (the gradients None without ``grad``)."""
        _, _, _, c, f = LinearProbe._checked(x, labels, weight, bias, col0)
        live = (labels >= 0) & (labels < c)
        xs = torch.where(live[None, :, None], x[:, :, col0 : col0 + f].to(torch.float64), torch.zeros((), dtype=torch.float64, device=x.device))
        w, b = weight.detach().to(torch.float64), bias.detach().to(torch.float64)
        z = torch.einsum("gnf,gcf->gnc", xs, w) + b[:, None, :]
        lab = labels.clamp(0, c - 1).to(torch.int64)[None, :, None].expand(z.shape[0], -1, 1)
        lse = torch.logsumexp(z, dim=-1)
        zero = torch.zeros((), dtype=torch.float64, device=x.device)
        nll = torch.where(live[None], lse - z.gather(-1, lab).squeeze(-1), zero)
        first = (z == z.max(dim=-1, keepdim=True).values).to(torch.int8).argmax(-1)  # (the first maximum)
        hit = torch.where(live[None], (first == lab.squeeze(-1)).to(torch.float64), zero)
        pred = torch.where(live[None], first, torch.full_like(first, -1)).to(torch.int32)
        count = live.sum().to(torch.float64).expand(z.shape[0])
        stats = ProbeStats(nll.sum(1), hit.sum(1), count, nll, hit, pred)
        if not grad:
            return stats, None, None
        d = torch.softmax(z, dim=-1) - torch.nn.functional.one_hot(lab.squeeze(-1), c).to(torch.float64)
        d = torch.where(live[None, :, None], d, zero)
        g_weight, g_bias = torch.einsum("gnc,gnf->gcf", d, xs), d.sum(1)
        if normalize:
            scale = count.clamp_min(1.0)
            g_weight, g_bias = g_weight / scale[:, None, None], g_bias / scale[:, None]
        return stats, g_weight, g_bias

    def reference(self, x: Tensor, labels: Tensor, *, col0: int = 0, grad: bool = True,
                  normalize: bool = True) -> tuple[ProbeStats, Tensor | None, Tensor | None]:
        """``rule`` on this module's weights."""
        return LinearProbe.rule(x, labels, self.weight, self.bias, col0=col0, grad=grad, normalize=normalize)

    # -- one launch on the GPU, the rule elsewhere -------------------------------------------------------------------------------------------
    def _grads(self) -> tuple[Tensor, Tensor]:
        for p in (self.weight, self.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        return self.weight.grad, self.bias.grad

    @torch.no_grad()
    def step(self, x: Tensor, labels: Tensor, *, col0: int = 0, grad: bool = True, normalize: bool = True,  # noqa: PLR0913
             planes: bool = False) -> ProbeStats:
        """One fused step: the loss, the hits and -- ``grad`` -- the gradients of the (``normalize``: mean, else summed) loss, which
        OVERWRITE ``weight.grad`` / ``bias.grad``.  ``planes``: the per-frame ``nll`` / ``hit`` / ``pred`` too.  One
        ``mtrssm_linear_probe_step`` call on torch's current stream; non-GPU tensors take the torch rule."""
        g, n, ld, c, f = LinearProbe._checked(x, labels, self.weight, self.bias, col0)
        if x.device != self.weight.device:
            msg = f"x is on {x.device}, the probe on {self.weight.device}"
            raise ValueError(msg)
        if not x.is_cuda:
            stats, g_w, g_b = self.reference(x, labels, col0=col0, grad=grad, normalize=normalize)
            if grad:
                dst_w, dst_b = self._grads()
                dst_w.copy_(g_w)
                dst_b.copy_(g_b)
            f32 = [t.to(torch.float32) for t in stats[:5]]
            return ProbeStats(f32[0], f32[1], f32[2], *((f32[3], f32[4], stats.pred) if planes else (None, None, None)))
        if f > MAX_FEATURES:
            msg = f"the probe kernel stages 16 rows of F floats in LDS: F <= {MAX_FEATURES}, got {f}"
            raise ValueError(msg)
        lib = _lib.load()
        need = int(lib.mtrssm_linear_probe_workspace_bytes(g, n, c, f))
        if self._workspace is None or self._workspace.device != x.device or self._workspace.numel() * 8 < need:
            self._workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=x.device)
        x, labels = x.contiguous(), labels.contiguous()
        g_w, g_b = self._grads() if grad else (None, None)
        stats = torch.empty(g, 3, device=x.device, dtype=torch.float32)
        nll = torch.empty(g, n, device=x.device, dtype=torch.float32) if planes else None
        hit = torch.empty(g, n, device=x.device, dtype=torch.float32) if planes else None
        pred = torch.empty(g, n, device=x.device, dtype=torch.int32) if planes else None
        weight, bias = self.weight.detach(), self.bias.detach()
        _lib.check(_lib.TIMERS.call("mtrssm_linear_probe_step", lib.mtrssm_linear_probe_step, _lib.ptr(x), ld, col0, _lib.index_ptr(labels),
                                    _lib.ptr(weight), _lib.ptr(bias), g, n, c, f, int(bool(normalize)), _lib.ptr(g_w), _lib.ptr(g_b), _lib.ptr(stats),
                                    _lib.ptr(nll), _lib.ptr(hit), _lib.index_ptr(pred), self._workspace.data_ptr(), self._workspace.numel() * 8,
                                    _lib.stream_ptr(x.device), flops=(4.0 if grad else 2.0) * g * n * c * f, nbytes=4.0 * g * n * f),
                   "mtrssm_linear_probe_step")
        return ProbeStats(stats[:, 0], stats[:, 1], stats[:, 2], nll, hit, pred)

    def _flat_parameters(self, extra: int):  # noqa: ANN202
        """This module's own flat buffer (made once per placement of the parameters; ``extra`` tail slots carry the stats)."""
        from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: PLC0415  (optim imports the scan stack)

        flat = self._flat
        if flat is None or flat.param.data_ptr() != self.weight.data_ptr() or flat.extra < extra:
            flat = self._flat = FlatParameters(self, extra=extra)
        return flat

    @torch.no_grad()
    def fit(self, x: Tensor, labels: Tensor, steps: int, lr: float = 1e-2, weight_decay: float = 0.0, col0: int = 0,  # noqa: PLR0913
            group=None) -> ProbeStats:  # noqa: ANN001
        """``steps`` full-batch iterations of AdamW (fresh moments, no clipping) on the mean loss: one ``step`` plus one ``FlatAdamW`` step on
        this module's own flat buffer (non-GPU tensors: ``torch.optim.AdamW``).  ``group``: the rows are sharded over a process group --
        each iteration all-reduces (``g_weight``, ``g_bias``, ``stats``) as sums in ONE call and divides by the global count, so the fit
        is the fit over all rows.  Returns the last iteration's stats (global ones under ``group``), taken BEFORE its update."""
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            msg = f"steps must be an integer >= 1, got {steps!r}"
            raise ValueError(msg)
        import torch.distributed as dist  # noqa: PLC0415

        from multimodal_mtrssm_amd.optim import FlatAdamW  # noqa: PLC0415

        shared = group is not None
        g = self.groups
        flat = self._flat_parameters(3 * g)
        if x.is_cuda:
            for i in range(len(flat.params)):  # the kernel writes the gradient views itself: no autograd hook ever fires
                flat.mark_touched(i)
            opt = FlatAdamW(flat, lr=lr, weight_decay=weight_decay, clip_norm=0.0)
        else:
            opt = torch.optim.AdamW([self.weight, self.bias], lr=lr, weight_decay=weight_decay)
        stats = None
        for _ in range(steps):
            stats = self.step(x, labels, col0=col0, grad=True, normalize=not shared)
            if shared:
                flat.tail[: 3 * g].copy_(torch.stack([stats.nll_sum, stats.hits, stats.count], dim=1).reshape(-1))
                dist.all_reduce(flat.grad_full, op=dist.ReduceOp.SUM, group=group)
                total = flat.tail[: 3 * g].reshape(g, 3).clone()
                scale = total[:, 2].clamp_min(1.0)
                self.weight.grad /= scale[:, None, None]
                self.bias.grad /= scale[:, None]
                stats = ProbeStats(total[:, 0], total[:, 1], total[:, 2], None, None, None)
            if x.is_cuda:
                opt.step(check=False)
            else:
                opt.step()
        return stats


class LatentProbe(ObservingConfig):
    """``LatentProbe(observe=("both", "audio", "vision"), part="feature")``: which posteriors are probed and which part of their feature.
    Copy ``g`` of every row observes subset ``observe[g]`` on every live step (and at frame 0); the copies share the row's uniforms, so
    the subsets differ only in what they observe.  ``part``: ``feature`` (all of it), ``deter`` / ``stoch`` (MRSSM's two halves) or, for
    MMTRSSM, ``higher`` / ``lower`` (a level's ``deter`` and ``stoch``; its ``deter`` / ``stoch`` are not contiguous columns and are
    refused)."""

    def __init__(self, observe: tuple[str, ...] = ("both", "audio", "vision"), part: str = "feature") -> None:
        if isinstance(observe, str) or not observe or any(o not in OBSERVE_BITS for o in observe) or len(set(observe)) != len(tuple(observe)):
            msg = f"observe must be a non-empty tuple of distinct keys out of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        if part not in PARTS:
            msg = f"part must be one of {PARTS}, got {part!r}"
            raise ValueError(msg)
        self.observe, self.part = tuple(observe), part
        self.group = None  # the process group ProbeTable.all_reduce and LinearProbe.fit use (FlatDataParallel.probe binds it)

    def __repr__(self) -> str:
        return f"LatentProbe(observe={self.observe!r}, part={self.part!r})"

    @property
    def samples(self) -> int:
        """Copies of a row in the rollout: one per observed subset."""
        return len(self.observe)

    groups = samples

    def copy_bits(self, device: torch.device) -> Tensor:
        """int32 ``[G]`` on ``device``: the scans' modality code of a live step of copy ``g`` (bit 0 audio, bit 1 vision)."""
        return observed_bits(self.bits, torch.device(device))[0]

    def copy_observed(self, device: torch.device) -> Tensor:
        """Bool ``[G, 2]`` (audio, vision) on ``device``: what a live step of copy ``g`` sees."""
        return self.observed(device)

    def plan(self):  # noqa: ANN201
        """Copy ``g`` of a row observes ``observe[g]`` on every live frame; the copies share the row's uniforms (the model's own shapes)."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(self.groups, self.bits, None)

    @staticmethod
    def layout(model) -> dict[str, tuple[int, int]]:  # noqa: ANN001
        """``part -> (col0, F)`` of ``model``'s feature (MRSSM: ``deter | stoch``; MMTRSSM: ``deter_h | stoch_h | deter_l | stoch_l``)."""
        if hasattr(model, "l_dist"):
            hd, hs, ld, ls = model.hd_dim, model.hs_dim, model.ld_dim, model.ls_dim
            return {"feature": (0, hd + hs + ld + ls), "higher": (0, hd + hs), "lower": (hd + hs, ld + ls)}
        factory = model.transition.distribution_factory
        deter, stoch = model.transition.deterministic_size, factory.category_size * factory.class_size
        return {"feature": (0, deter + stoch), "deter": (0, deter), "stoch": (deter, stoch)}

    def columns(self, model) -> tuple[int, int]:  # noqa: ANN001
        """``(col0, F)`` of ``part`` in ``model``'s feature."""
        layout = LatentProbe.layout(model)
        if self.part not in layout:
            msg = f"part {self.part!r} is not a contiguous part of {type(model).__name__}'s feature: choose one of {tuple(layout)}"
            raise ValueError(msg)
        return layout[self.part]

    def linear(self, model, classes: int = 10) -> LinearProbe:  # noqa: ANN001
        """A zero-initialised ``LinearProbe`` of this probe's shape on the model's device."""
        return LinearProbe(self.groups, self.columns(model)[1], classes).to(next(model.parameters()).device)


class ProbeTable(SumTable):
    """The accumulated evaluation of any number of probe steps in ONE fp32 buffer ``[2 G + 1, T]``: ``hit`` of the ``G`` groups, then
    their ``nll``, summed by frame position over the live (labelled) frames, then the counts of those frames."""

    def __init__(self, groups: int, steps: int, device: torch.device | str = "cpu", observe: tuple[str, ...] | None = None) -> None:
        if groups < 1 or steps < 1:
            msg = f"need groups, steps >= 1, got {groups}, {steps}"
            raise ValueError(msg)
        if observe is not None and len(observe) != groups:
            msg = f"{groups} groups need {groups} names, got {observe!r}"
            raise ValueError(msg)
        self.groups = groups
        self.observe = tuple(observe) if observe is not None else (("both", "audio", "vision")[:groups] if groups <= 3 else  # noqa: PLR2004
                                                                   tuple(f"g{i}" for i in range(groups)))
        self.buffer = torch.zeros(2 * groups + 1, steps, dtype=torch.float32, device=device)
        self.stats: ProbeStats | None = None  # the last step's, kept by probe_evaluate

    @property
    def hit(self) -> Tensor:
        return self.buffer[: self.groups]

    @property
    def nll(self) -> Tensor:
        return self.buffer[self.groups : 2 * self.groups]

    @property
    def counts(self) -> Tensor:
        return self.buffer[2 * self.groups]

    def fold(self, hit: Tensor, nll: Tensor, live: Tensor) -> ProbeTable:
        """Adds a step's planes by frame position: ``hit`` / ``nll`` ``[G, B, T]`` (exactly 0 on dead frames) and ``live`` ``[B, T]`` (1.0
        on a labelled frame).  ``mtrssm_horizon_table`` with ``context = 1``, whose bin ``h`` is then the frame ``t``; the ``live`` plane
        rides along as the last row, the kernel's own count of ALL frames per bin is dropped."""
        g, t = self.groups, self.steps
        if tuple(hit.shape) != tuple(nll.shape) or hit.dim() != 3 or hit.shape[0] != g or hit.shape[2] != t or tuple(live.shape) != tuple(hit.shape[1:]):  # noqa: PLR2004
            msg = f"need hit, nll [{g}, B, {t}] and live [B, {t}], got {tuple(hit.shape)}, {tuple(nll.shape)}, {tuple(live.shape)}"
            raise ValueError(msg)
        planes = torch.cat([hit.to(torch.float32), nll.to(torch.float32), live.to(torch.float32)[None]]).contiguous()
        context = torch.ones(hit.shape[1], dtype=torch.int32, device=hit.device)
        frames = torch.zeros(t, dtype=torch.float32, device=hit.device)
        ForecastSkill.table_add(planes, context, None, self.buffer, frames)
        return self

    def _sizes(self, other: SumTable) -> str:
        return f"{tuple(self.buffer.shape)} and {tuple(other.buffer.shape)}"

    def curves(self) -> dict[str, dict[str, Tensor]]:
        """``{subset: {"acc", "nll"}}``, ``[T]`` each: the mean over the labelled frames at position ``t``; an empty bin gives NaN."""
        return {name: {"acc": self._mean(self.hit[i], self.counts), "nll": self._mean(self.nll[i], self.counts)} for i, name in enumerate(self.observe)}

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix/{both,audio,vision}/{acc,nll}``: summed rows over the summed counts; NaN for an empty table."""
        total = self.counts.sum()
        out = {}
        for i, name in enumerate(self.observe):
            out[f"{prefix}/{name}/acc"] = self._mean(self.hit[i].sum(), total)
            out[f"{prefix}/{name}/nll"] = self._mean(self.nll[i].sum(), total)
        return out


def frame_labels(labels: Tensor, valid: Tensor | None) -> Tensor:
    """int32 ``[B * T]``: ``labels`` ``[B, T]`` with the frames at or past a row's end (``t >= valid[b]``) set to -1."""
    b, t = labels.shape
    labels = labels.to(torch.int32)
    if valid is not None:
        live = torch.arange(t, device=labels.device) < valid.to(labels.device).unsqueeze(1)
        labels = torch.where(live, labels, torch.full_like(labels, -1))
    return labels.reshape(b * t).contiguous()


__all__ = ["LatentProbe", "LinearProbe", "ProbeStats", "ProbeTable", "frame_labels"]
