"""The fit loop: ``Trainer``, per-epoch metrics that never synchronise the host per step, and a checkpoint
from which training resumes with every piece of training state restored bit for bit.

The reference trains through Lightning (``scripts/_train_common.py:9-33``, the ``trainer:`` / ``lr_scheduler:`` / ``callbacks:`` blocks
of ``default.yaml:103-155``).  ``Trainer`` runs what those blocks describe on this project's own step -- ``FlatParameters``,
``FlatAdamW``, ``FlatDataParallel``, ``GlobalRowNoise``, ``DeviceEpisodeLoader`` and the model's ``modality_dropout`` / ``forecast`` /
``elbo_schedule`` / ``state_carry`` attributes -- and keeps the promises only a loop can keep: lr, step count and beta live in device
memory, ``set_epoch`` replays an epoch, the uniforms depend on a seed and a draw count, so a run that stops can continue from exactly
the state it had.

``EpochMetrics`` is the loop's own hot path: ONE call per step (``mtrssm_fit_fold``: two launches over the flat gradient and
parameter buffers and the loss scalars in the gradient buffer's tail) folds the step into a device-resident accumulator; the host
reads it once per epoch (``compute``) and every ``check_every_n_steps`` (the non-finite flags).  ``fold_reference`` is the same rule
in torch float64: it runs for tensors that are not on the GPU and is the kernels' checker.
"""

from __future__ import annotations

import ctypes as C
import json
import math
import time
from collections.abc import Callable, Iterable, Iterator, Sequence
from pathlib import Path

import torch
import torch.distributed as dist
from torch import Tensor, nn

from multimodal_mtrssm_amd import _lib, conv
from multimodal_mtrssm_amd.optim import FlatAdamW, FlatParameters
from multimodal_mtrssm_amd.panel import MAX_EPISODES
from multimodal_mtrssm_amd.parallel import FlatDataParallel

FORMAT = "mtrssm-fit-1"

# include/mtrssm.h: the accumulator's doubles and the flag block's int32 words
MAX_SEGMENTS, MAX_SCALARS = 32, 8
ACC_WEIGHT, ACC_STEPS, ACC_CLIPPED, ACC_GRAD_SUM, ACC_GRAD_MAX, ACC_PARAM, ACC_SCALARS, ACC_SEGMENTS, ACC_DOUBLES = 0, 1, 2, 3, 4, 5, 6, 14, 110
FLAG_BAD_STEPS, FLAG_FIRST_BAD, FLAG_BAD_SEGMENTS, FLAG_BAD_SCALARS, FLAG_STEP, FLAG_INTS = 0, 1, 2, 3, 4, 8
_BANK_BYTES = ACC_DOUBLES * 8 + FLAG_INTS * 4


def _f32(x: float) -> float:
    """``x`` rounded to fp32, as a by-value float argument of the C call arrives."""
    return C.c_float(float(x)).value


def fold_reference(grad: Tensor, param: Tensor, offsets: Sequence[int], group: Sequence[int] | None, scalars: Tensor | Sequence[float],  # noqa: PLR0913
                   scalar_scale: float, grad_scale: float, clip_norm: float, weight: float, acc: Tensor, flags: Tensor) -> Tensor:
    """``mtrssm_fit_fold`` in torch float64.  ``offsets``: ``G + 1`` ascending offsets covering ``[0, numel)``; ``group[s]``: the first
    segment of the name segment ``s`` belongs to (None: itself); ``acc`` (float64 ``[ACC_DOUBLES]``) and ``flags`` (int32 ``[FLAG_INTS]``)
    are updated in place.  Returns the per-segment sums, float64 ``[3, G]``: ``sum(g^2)``, ``sum(p^2)``, non-finite gradient elements.

    A step with a non-finite scalar or gradient element leaves ``acc`` alone, counts in ``flags[FLAG_BAD_STEPS]``, ORs its segments and
    scalars into the two masks and, when it is the first, records its index (``flags[FLAG_STEP]``, which every call advances)."""
    n_seg = len(offsets) - 1
    group = list(range(n_seg)) if group is None else [int(v) for v in group]
    sums = torch.zeros(3, n_seg, dtype=torch.float64)
    for s in range(n_seg):
        g = grad[offsets[s]: offsets[s + 1]].detach().to("cpu", torch.float64)
        p = param[offsets[s]: offsets[s + 1]].detach().to("cpu", torch.float64)
        sums[0, s], sums[1, s], sums[2, s] = (g * g).sum(), (p * p).sum(), float((~torch.isfinite(g)).sum())
    values = torch.as_tensor(scalars, dtype=torch.float32).detach().to("cpu").reshape(-1)
    bad_segments = sum(1 << s for s in range(n_seg) if float(sums[2, s]) > 0)
    bad_segments -= (bad_segments >> 31) << 32  # (bit 31 as the sign of an int32 word)
    bad_scalars = sum(1 << k for k in range(values.numel()) if not math.isfinite(float(values[k])))
    step = int(flags[FLAG_STEP])
    flags[FLAG_STEP] = step + 1
    if bad_segments or bad_scalars:
        if int(flags[FLAG_BAD_STEPS]) == 0:
            flags[FLAG_FIRST_BAD] = step
        flags[FLAG_BAD_STEPS] += 1
        flags[FLAG_BAD_SEGMENTS] |= bad_segments
        flags[FLAG_BAD_SCALARS] |= bad_scalars
        return sums
    w, scale, clip = float(_f32(weight)), _f32(grad_scale), _f32(clip_norm)
    norm = math.sqrt(float(sums[0].sum())) * scale
    acc[ACC_WEIGHT] += w
    acc[ACC_STEPS] += 1.0
    if clip > 0.0 and norm > clip:
        acc[ACC_CLIPPED] += 1.0
    acc[ACC_GRAD_SUM] += norm
    acc[ACC_GRAD_MAX] = max(float(acc[ACC_GRAD_MAX]), norm)
    acc[ACC_PARAM] = math.sqrt(float(sums[1].sum()))
    for k in range(values.numel()):
        acc[ACC_SCALARS + k] += w * (float(values[k]) * _f32(scalar_scale))
    for s in range(n_seg):
        if group[s] != s:
            continue
        runs = [t for t in range(s, n_seg) if group[t] == s]
        gn = math.sqrt(sum(float(sums[0, t]) for t in runs)) * scale
        at = ACC_SEGMENTS + 3 * s
        acc[at] += gn
        acc[at + 1] = max(float(acc[at + 1]), gn)
        acc[at + 2] = math.sqrt(sum(float(sums[1, t]) for t in runs))
    return sums


def parameter_names(model: nn.Module, flat: FlatParameters) -> list[str]:
    """Per entry of ``flat.params``: the name of the model's top-level child that owns it (a shared parameter: the first owner)."""
    owner = {id(p): name.split(".")[0] for name, p in model.named_parameters()}
    return [owner[id(p)] for p in flat.params]


def segment_runs(names: Sequence[str], offsets: Sequence[int], numel: int) -> tuple[list[str], list[int], list[int]]:
    """``(segment names, G + 1 offsets, group)``: the segments are the maximal runs of consecutive parameters that share a name;
    ``group[s]`` is the first segment that carries segment ``s``'s name."""
    if len(names) != len(offsets) or not names:
        msg = f"need one name per parameter, got {len(names)} names for {len(offsets)} parameters"
        raise ValueError(msg)
    seg_names, seg_offsets = [], []
    for name, off in zip(names, offsets, strict=True):
        if not seg_names or seg_names[-1] != name:
            seg_names.append(name)
            seg_offsets.append(int(off))
    if len(seg_names) > MAX_SEGMENTS:
        msg = f"the parameters form {len(seg_names)} runs of top-level names, the fold takes {MAX_SEGMENTS}"
        raise ValueError(msg)
    seg_offsets.append(int(numel))
    return seg_names, seg_offsets, [seg_names.index(n) for n in seg_names]


class EpochMetrics:
    """Epoch sums of a step's scalars, weighted by batch rows (what Lightning's ``on_epoch=True`` logs), and of the gradient and
    parameter norms per top-level child of the model -- in device memory, one ``fold`` per step, one copy per ``compute``.

    ``flat``: the ``FlatParameters`` whose buffers are folded, or None for scalars only (validation).  ``names``: the model, or one
    name per entry of ``flat.params``.  ``keys``: the scalars' names in the order they are folded (train: the order of
    ``FlatDataParallel.sync``'s dict, which is the order of the gradient buffer's tail; at most eight); without a flat buffer more
    than eight keys take further banks of the accumulator, one call each.  ``scalar_scale`` (1 / world) and ``grad_scale`` scale what the buffers hold, ``clip_norm`` is the
    optimizer's; metric names are ``prefix + key``."""

    def __init__(self, flat: FlatParameters | None, names: nn.Module | Sequence[str] | None, keys: Sequence[str], *,  # noqa: PLR0913
                 scalar_scale: float = 1.0, grad_scale: float = 1.0, clip_norm: float = 0.0, prefix: str = "train/",
                 device: torch.device | str | None = None) -> None:
        self.flat, self.keys, self.prefix = flat, [str(k) for k in keys], prefix
        if not self.keys:
            msg = "EpochMetrics needs at least one scalar key"
            raise ValueError(msg)
        self.scalar_scale, self.grad_scale, self.clip_norm = float(scalar_scale), float(grad_scale), float(clip_norm)
        if flat is not None:
            if names is None:
                msg = "names: the model, or one name per parameter of flat"
                raise ValueError(msg)
            per_param = parameter_names(names, flat) if isinstance(names, nn.Module) else list(names)
            self.names, self.offsets, self.group = segment_runs(per_param, flat.offsets, flat.numel)
            self.device = flat.param.device
            self._grad, self._param = flat.grad, flat.param
        else:
            self.names, self.offsets, self.group = [], [0, 4], [0]
            self.device = torch.device("cpu" if device is None else device)
            self._grad = self._param = torch.zeros(4, dtype=torch.float32, device=self.device)  # (the fold's buffers: one empty segment)
        self.banks = -(-len(self.keys) // MAX_SCALARS)
        if flat is not None and self.banks > 1:  # (every bank would reduce both buffers again; the tail of a flat buffer holds eight)
            msg = f"with a flat buffer the fold takes {MAX_SCALARS} scalars, got {len(self.keys)}: {self.keys}"
            raise ValueError(msg)
        self.on_gpu = self.device.type == "cuda"
        # ONE block holds every bank's doubles, then every bank's flags: compute() copies it to the host in one piece
        self.block = torch.zeros(self.banks * _BANK_BYTES, dtype=torch.uint8, device=self.device)
        self.acc = self.block[: self.banks * ACC_DOUBLES * 8].view(torch.float64).view(self.banks, ACC_DOUBLES)
        self.flags = self.block[self.banks * ACC_DOUBLES * 8:].view(torch.int32).view(self.banks, FLAG_INTS)
        self.chunk = 0
        self._weights: dict[float, Tensor] = {}
        self._staged: Tensor | None = None
        if self.on_gpu:
            chunk = C.c_int64(0)
            numel = int(self._grad.numel())
            nbytes = int(_lib.load().mtrssm_fit_fold_workspace_bytes(numel, len(self.offsets) - 1, C.byref(chunk)))
            if nbytes < 0:
                _lib.check(-1, "mtrssm_fit_fold_workspace_bytes")
            self.chunk = int(chunk.value)
            self.workspace = torch.zeros(nbytes // 8, dtype=torch.float64, device=self.device)
            self.offsets_dev = torch.tensor(self.offsets, dtype=torch.int64).to(self.device)
            self.group_dev = torch.tensor(self.group, dtype=torch.int32).to(self.device)
        self.last_sums: Tensor | None = None  # (the CPU path's per-segment sums of the last fold; the GPU's are `sums()`)
        self._next_step = 0
        self.reset(0)

    # -- state ------------------------------------------------------------------------------------
    def reset(self, step: int = 0) -> None:
        """Empty accumulators and flags; the next fold's step index is ``step``."""
        self.block.zero_()
        self.flags[:, FLAG_FIRST_BAD] = -1
        self.flags[:, FLAG_STEP] = int(step)
        self._next_step = int(step)

    def state(self) -> dict[str, object]:
        return {"keys": list(self.keys), "names": list(self.names), "acc": self.acc.detach().to("cpu").clone(),
                "flags": self.flags.detach().to("cpu").clone()}

    def load_state(self, state: dict[str, object]) -> None:
        if list(state["keys"]) != self.keys or list(state["names"]) != self.names:  # type: ignore[arg-type]
            msg = f"the saved metrics hold {state['keys']} over {state['names']}, these {self.keys} over {self.names}"
            raise ValueError(msg)
        self.acc.copy_(state["acc"])  # type: ignore[arg-type]
        self.flags.copy_(state["flags"])  # type: ignore[arg-type]
        self._next_step = int(state["flags"][0, FLAG_STEP])  # type: ignore[index]

    def sums(self) -> Tensor:
        """The last fold's per-segment sums, float64 ``[3, G]`` on the host: ``sum(g^2)``, ``sum(p^2)``, non-finite gradient elements."""
        if not self.on_gpu:
            if self.last_sums is None:
                msg = "nothing was folded yet"
                raise ValueError(msg)
            return self.last_sums
        return self.workspace[: 3 * MAX_SEGMENTS].view(3, MAX_SEGMENTS)[:, : len(self.offsets) - 1].to("cpu")

    # -- the step ---------------------------------------------------------------------------------
    def _weight(self, weight: float) -> Tensor:
        w = float(weight)
        if w not in self._weights:  # (a run sees two values: the full batch's rows and the last, short batch's)
            self._weights[w] = torch.tensor([w], dtype=torch.float32).to(self.device)
        return self._weights[w]

    def _scalars(self, scalars: Tensor | dict[str, Tensor]) -> Tensor:
        """The ``K`` scalars as one contiguous fp32 tensor on the device: a tensor is taken as it is (the gradient buffer's tail, no
        copy), a dict is stacked in the order of ``keys`` (one launch)."""
        if isinstance(scalars, dict):
            if list(scalars) != self.keys and set(scalars) != set(self.keys):
                msg = f"the step's scalars are {list(scalars)}, the metrics were made for {self.keys}"
                raise ValueError(msg)
            scalars = torch.stack([torch.as_tensor(scalars[k]).detach().reshape(()).to(self.device, torch.float32) for k in self.keys])
        if scalars.dtype != torch.float32 or scalars.dim() != 1 or scalars.numel() < len(self.keys) or scalars.device != self.device:
            msg = f"scalars must be a float32 [{len(self.keys)}] tensor on {self.device}, got {scalars.dtype} {tuple(scalars.shape)} on {scalars.device}"
            raise ValueError(msg)
        return scalars[: len(self.keys)]

    @torch.no_grad()
    def fold(self, scalars: Tensor | dict[str, Tensor], weight: float, step: int) -> None:
        """Fold one step: ``scalars`` (a float32 tensor whose first ``K`` entries are the step's scalars in the order of ``keys``, or
        a dict of them), ``weight`` (the step's global batch rows), ``step`` (its index, recorded if it is the first bad one).  Call it
        AFTER the optimizer: the gradient buffer still holds the reduced, unclipped gradient, the parameters are the updated ones."""
        values = self._scalars(scalars)
        if int(step) != self._next_step:  # (an eager fill; a loop that counts its steps one by one never gets here)
            self.flags[:, FLAG_STEP] = int(step)
        self._next_step = int(step) + 1
        for bank in range(self.banks):
            part = values[bank * MAX_SCALARS: (bank + 1) * MAX_SCALARS]
            if not self.on_gpu:
                got = fold_reference(self._grad, self._param, self.offsets, self.group, part, self.scalar_scale, self.grad_scale, self.clip_norm,
                                     weight, self.acc[bank], self.flags[bank])
                self.last_sums = got if bank == 0 else self.last_sums
                continue
            self._staged = part  # (alive until the next fold: the launch reads it)
            _lib.check(_lib.TIMERS.call(
                "mtrssm_fit_fold", _lib.load().mtrssm_fit_fold, _lib.ptr(self._grad), _lib.ptr(self._param), int(self._grad.numel()),
                self.offsets_dev.data_ptr(), self.group_dev.data_ptr(), len(self.offsets) - 1, part.data_ptr(), int(part.numel()),
                self.scalar_scale, self.grad_scale, self.clip_norm, _lib.ptr(self._weight(weight)), self.acc[bank].data_ptr(),
                self.flags[bank].data_ptr(), self.workspace.data_ptr(), self.workspace.numel() * 8, _lib.stream_ptr(self.device),
                nbytes=8.0 * self._grad.numel()), "mtrssm_fit_fold")

    # -- reading ----------------------------------------------------------------------------------
    def _host(self, group: object | None = None) -> tuple[Tensor, Tensor]:
        """``(acc, flags)`` on the host from ONE copy of the block.  ``group`` (a process group, or True for the default one), for
        metrics each rank folded from its own rows (validation): ONE all-reduce sums the accumulators, the counts of bad steps and, bit by
        bit, the scalars' mask; the first bad step and the segments' mask stay this rank's."""
        block = self.block.to("cpu")
        n = self.banks * ACC_DOUBLES * 8
        acc, flags = block[:n].view(torch.float64).view(self.banks, ACC_DOUBLES).clone(), block[n:].view(torch.int32).view(self.banks, FLAG_INTS).clone()
        if group is not None and dist.is_available() and dist.is_initialized():
            bits = (flags[:, FLAG_BAD_SCALARS : FLAG_BAD_SCALARS + 1] >> torch.arange(MAX_SCALARS)) & 1
            packed = torch.cat([acc, flags[:, FLAG_BAD_STEPS : FLAG_BAD_STEPS + 1].double(), bits.double()], dim=1).to(self.device)
            dist.all_reduce(packed, op=dist.ReduceOp.SUM, group=None if group is True else group)
            packed = packed.to("cpu")
            acc = packed[:, :ACC_DOUBLES].clone()
            flags[:, FLAG_BAD_STEPS] = packed[:, ACC_DOUBLES].to(torch.int32)
            flags[:, FLAG_BAD_SCALARS] = ((packed[:, ACC_DOUBLES + 1 :] > 0).to(torch.int32) << torch.arange(MAX_SCALARS, dtype=torch.int32)).sum(1).to(torch.int32)
        return acc, flags

    def bad_steps(self, group: object | None = None) -> dict[str, object] | None:
        """None when every folded step was finite, else ``{"count", "first", "scalars", "modules"}`` (one copy of the block)."""
        return self._bad(self._host(group)[1])

    def _bad(self, flags: Tensor) -> dict[str, object] | None:
        count = int(flags[:, FLAG_BAD_STEPS].max())
        if count == 0:
            return None
        firsts = [int(v) for v in flags[:, FLAG_FIRST_BAD] if int(v) >= 0]
        scalars = [self.prefix + self.keys[b * MAX_SCALARS + k] for b in range(self.banks) for k in range(MAX_SCALARS)
                   if int(flags[b, FLAG_BAD_SCALARS]) >> k & 1 and b * MAX_SCALARS + k < len(self.keys)]
        modules = [name for s, name in enumerate(self.names) if int(flags[0, FLAG_BAD_SEGMENTS]) >> s & 1]
        return {"count": count, "first": min(firsts) if firsts else -1, "scalars": scalars, "modules": sorted(set(modules), key=modules.index)}

    def check(self, group: object | None = None) -> None:
        """Raise ``FloatingPointError`` naming the first bad step, the non-finite scalars and the modules with non-finite gradients."""
        self._raise(self.bad_steps(group))

    @staticmethod
    def _raise(bad: dict[str, object] | None) -> None:
        if bad is not None:
            msg = (f"{bad['count']} step(s) with non-finite values, the first at step {bad['first']}: scalars {bad['scalars']}, "
                   f"gradients of {bad['modules']} (these steps are not in the epoch's metrics; the optimizer was not changed)")
            raise FloatingPointError(msg)

    def compute(self, group: object | None = None, *, check: bool = False) -> dict[str, float]:
        """The epoch's metrics from one device-to-host copy: ``prefix + key`` (the mean weighted by batch rows) and, with a flat
        buffer, ``grad_norm[/<name>]`` (mean over the finite steps), ``grad_norm/max[/<name>]``, ``param_norm[/<name>]`` (after the last
        finite step), ``clipped`` (steps whose global norm exceeded ``clip_norm``) and ``bad_steps``.  ``check``: raise as ``check()``
        does, from the same copy.  A key that was non-finite on some step reports NaN, as its plain mean would: the finite steps' mean
        must not pass for the epoch's (a monitor then stops ``EarlyStopping`` and never counts as an improvement)."""
        acc, flags = self._host(group)
        if check:
            self._raise(self._bad(flags))
        out: dict[str, float] = {}
        for i, key in enumerate(self.keys):
            a = acc[i // MAX_SCALARS]
            w = float(a[ACC_WEIGHT])
            flagged = int(flags[i // MAX_SCALARS, FLAG_BAD_SCALARS]) >> (i % MAX_SCALARS) & 1
            out[self.prefix + key] = float(a[ACC_SCALARS + i % MAX_SCALARS]) / w if w > 0 and not flagged else float("nan")
        if self.flat is not None:
            a = acc[0]
            steps = float(a[ACC_STEPS])
            mean = (lambda v: float(v) / steps) if steps > 0 else (lambda _v: float("nan"))
            out["grad_norm"], out["grad_norm/max"], out["param_norm"] = mean(a[ACC_GRAD_SUM]), float(a[ACC_GRAD_MAX]), float(a[ACC_PARAM])
            for s, name in enumerate(self.names):
                if self.group[s] == s:
                    at = ACC_SEGMENTS + 3 * s
                    out[f"grad_norm/{name}"], out[f"grad_norm/max/{name}"], out[f"param_norm/{name}"] = mean(a[at]), float(a[at + 1]), float(a[at + 2])
            out["clipped"] = float(a[ACC_CLIPPED])
        out["bad_steps"] = float(int(flags[:, FLAG_BAD_STEPS].max()))
        return out


class EarlyStopping:
    """``lightning.pytorch.callbacks.EarlyStopping`` as ``default.yaml:137-142`` configures it (monitor ``val/loss``, patience 100, mode
    ``min``), ``min_delta`` 0: ``step(value)`` once per validation epoch returns True when ``patience`` epochs in a row brought no
    improvement.  A non-finite value stops at once (Lightning's ``check_finite``)."""

    def __init__(self, monitor: str = "val/loss", patience: int = 100, mode: str = "min", min_delta: float = 0.0) -> None:
        if mode not in {"min", "max"}:
            msg = f"mode must be 'min' or 'max', got {mode!r}"
            raise ValueError(msg)
        if isinstance(patience, bool) or not isinstance(patience, int) or patience < 0:
            msg = f"patience must be an integer >= 0, got {patience!r}"
            raise ValueError(msg)
        self.monitor, self.patience, self.mode, self.min_delta = monitor, patience, mode, abs(float(min_delta))
        self.best = float("inf") if mode == "min" else -float("inf")
        self.wait = 0
        self.stopped_epoch: int | None = None

    def step(self, value: float, epoch: int | None = None) -> bool:
        value = float(value)
        if not math.isfinite(value):
            self.stopped_epoch = epoch
            return True
        better = value < self.best - self.min_delta if self.mode == "min" else value > self.best + self.min_delta
        if better:
            self.best, self.wait = value, 0
            return False
        self.wait += 1
        if self.wait >= self.patience:
            self.stopped_epoch = epoch
            return True
        return False

    def state_dict(self) -> dict[str, object]:
        return {"best": self.best, "wait": self.wait, "stopped_epoch": self.stopped_epoch}

    def load_state_dict(self, state: dict[str, object]) -> None:
        self.best, self.wait, self.stopped_epoch = float(state["best"]), int(state["wait"]), state["stopped_epoch"]  # type: ignore[arg-type, assignment]


def _scheduler_state(scheduler: object | None) -> dict[str, object] | None:
    if scheduler is None:
        return None
    return {"best": float(scheduler.best), "num_bad_epochs": int(scheduler.num_bad_epochs)}  # type: ignore[attr-defined]


def _cpu(t: Tensor) -> Tensor:
    return t.detach().to("cpu").clone()


class Trainer:
    """``Trainer(model, flat, opt, dp, seed=..., max_epochs=..., directory=...).fit(train_loader, val_loader)``.

    One train step is ``model._step``'s dispatch on the model's ``modality_dropout`` / ``forecast`` / ``elbo_schedule`` /
    ``state_carry`` / ``overshoot`` attributes with uniforms from ``dp.noise_source(seed)``: ``opt.zero_grad()``, backward, ``dp.sync(scalars)``,
    ``opt.step(grad_scale=dp.grad_scale)``, then ``EpochMetrics.fold``.  ``train_step`` (``batch -> {key: device scalar}``) replaces
    everything from zero_grad to the optimizer: a ``CapturedTrainStep.step`` fits (the Trainer itself captures no graph), and so does a
    stub.  Loaders yield this rank's rows; a loader with ``set_epoch`` is told the epoch, one with ``batches(skip)`` resumes mid-epoch
    without gathering what it skips.

    Validation runs ``model.validation_step`` under ``no_grad`` inside ``torch.random.fork_rng`` seeded ``seed + 1`` -- every pass sees
    the same draws and the training streams are not touched -- into a second, scalars-only ``EpochMetrics`` whose sums are all-reduced
    once per epoch; ``model.on_validation_epoch_end()`` adds ``val/skill/*`` / ``val/loglik/*``; ``panel_logger(model, batch, "val",
    epoch, first_index)`` sees the batches below its 60-episode horizon after the last validation draw, so an epoch with panels
    validates on the same draws as one without.  A validation key that was non-finite on some batch reports NaN (and ``val/bad_steps``
    the count): a non-finite monitor stops ``EarlyStopping`` and is never the best; ``metrics.jsonl`` writes it as null.

    At an epoch's end: ``scheduler.step(monitor)``, early stopping, the best checkpoint (``save_top_k: 1``) and ``last.ckpt``, and one
    JSON line in ``{directory}/metrics.jsonl`` (epoch, global_step, the lr the epoch trained with, every metric, the seconds the epoch's
    steps took and the wall time since ``fit`` began).  Rank 0
    writes; every rank decides alike, because the metrics are those of all ranks.  The non-finite flags are read at an epoch's end
    and every ``check_every_n_steps``: a bad step raises ``FloatingPointError``; the optimizer's own handling is not changed.

    ``max_steps``: stop when ``global_step`` reaches it; mid-epoch that writes ``last.ckpt`` and returns without an epoch end, and
    ``fit(resume=".../last.ckpt")`` continues the epoch at the next batch.  ``save_every_n_steps`` writes ``last.ckpt`` likewise."""

    def __init__(self, model: nn.Module, flat: FlatParameters | None, opt: FlatAdamW | None, dp: FlatDataParallel | None, *, seed: int,  # noqa: PLR0913
                 max_epochs: int, max_steps: int | None = None, scheduler: object | None = None, early_stopping: EarlyStopping | None = None,
                 monitor: str = "val/loss", mode: str = "min", directory: str | Path, save_every_n_steps: int | None = None,
                 check_every_n_steps: int = 50, panel_logger: Callable[..., object] | None = None,
                 train_step: Callable[[tuple[Tensor, ...]], dict[str, Tensor]] | None = None) -> None:
        if mode not in {"min", "max"}:
            msg = f"mode must be 'min' or 'max', got {mode!r}"
            raise ValueError(msg)
        if train_step is None and (flat is None or opt is None or dp is None):
            msg = "without train_step= the Trainer needs flat, opt and dp: its own step runs on them"
            raise ValueError(msg)
        if check_every_n_steps < 1 or (save_every_n_steps is not None and save_every_n_steps < 1):
            msg = "check_every_n_steps and save_every_n_steps must be >= 1"
            raise ValueError(msg)
        self.model, self.flat, self.opt, self.dp = model, flat, opt, dp
        self.seed, self.max_epochs, self.max_steps = int(seed), int(max_epochs), max_steps
        self.scheduler, self.early_stopping, self.monitor, self.mode = scheduler, early_stopping, monitor, mode
        self.directory = Path(directory)
        self.save_every, self.check_every = save_every_n_steps, int(check_every_n_steps)
        self.panel_logger, self.train_step = panel_logger, train_step
        self.world = 1 if dp is None else dp.world
        self.rank = 0 if dp is None else dp.rank
        self.group = None if dp is None else dp.group
        self.device = flat.param.device if flat is not None else torch.device("cpu")
        self.noise = None if dp is None or flat is None else dp.noise_source(self.seed)
        if train_step is None and getattr(model, "elbo_schedule", None) is not None:
            model.elbo_schedule.bind(opt)  # (beta follows the optimizer's device-resident count of steps, which a checkpoint restores)
        self.epoch = self.global_step = self.batch_in_epoch = 0
        self.best: dict[str, object] = {"value": None, "epoch": None, "global_step": None}
        self.train_metrics: EpochMetrics | None = None
        self.val_metrics: EpochMetrics | None = None
        self.should_stop = False
        self.history: list[dict[str, object]] = []
        self._loader_state: dict[str, object] | None = None
        self._pending: dict[str, object] | None = None  # (a checkpoint's metrics, loaded once their keys are known again)

    # -- the step ---------------------------------------------------------------------------------
    def _own_step(self, batch: tuple[Tensor, ...]) -> dict[str, Tensor]:
        model, dp, opt = self.model, self.dp, self.opt
        b, t = batch[0].shape[:2]
        dropout = None if model.modality_dropout is None else model.modality_dropout.for_rank(dp.world, dp.rank)
        forecast = None if model.forecast is None else model.forecast.for_rank(dp.world, dp.rank)
        overshoot = getattr(model, "overshoot", None)
        overshoot = None if overshoot is None else overshoot.for_rank(dp.world, dp.rank)
        shapes = dict(model.noise_shapes(b, t))  # (assembled as CapturedTrainStep does; with model.overshoot its uniforms are in)
        if dropout is not None:
            shapes["u_mask"] = dropout.noise_shape(b, t)
        if forecast is not None:
            shapes["u_context"] = forecast.noise_shape(b)
        noise = self.noise.draw(shapes)
        opt.zero_grad()
        if forecast is not None:  # (with a state_carry set too, shared_step refuses)
            out = model.shared_step(batch, noise, modality_dropout=dropout, state_carry=model.state_carry, forecast=forecast,
                                    elbo_schedule=model.elbo_schedule, overshoot=overshoot)
        elif model.state_carry is None:
            out = model.shared_step(batch, noise, modality_dropout=dropout, elbo_schedule=model.elbo_schedule, overshoot=overshoot)
        else:
            out = model.shared_step(batch, noise, modality_dropout=dropout, state_carry=model.state_carry, carry_prefix="train",
                                    elbo_schedule=model.elbo_schedule, overshoot=overshoot)
        out["loss"].backward()
        logs = dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)
        return logs

    def _make_train_metrics(self, keys: Sequence[str]) -> EpochMetrics:
        if self.flat is not None:
            clip = 0.0 if self.opt is None else float(self.opt.clip_norm)
            grad_scale = 1.0 if self.dp is None else self.dp.grad_scale
            return EpochMetrics(self.flat, self.model, keys, scalar_scale=1.0 / self.world, grad_scale=grad_scale, clip_norm=clip)
        return EpochMetrics(None, None, keys, device=self.device)

    def _fold_train(self, logs: dict[str, Tensor], rows: int) -> None:
        if self.train_metrics is None:
            self.train_metrics = self._make_train_metrics(list(logs))
            self._load_pending("train", self.train_metrics)
        m = self.train_metrics
        # the tail of the gradient buffer holds the all-reduced sums of exactly these scalars, in this order: no copy, no stack
        from_tail = self.flat is not None and self.train_step is None
        if from_tail:
            m.fold(self.flat.tail, float(rows * self.world), self.global_step)
        else:  # (a caller's step hands back the means over ranks)
            scale, m.scalar_scale = m.scalar_scale, 1.0
            m.fold(dict(logs), float(rows * self.world), self.global_step)
            m.scalar_scale = scale

    def _load_pending(self, which: str, metrics: EpochMetrics) -> None:
        if self._pending is not None and self._pending.get(which) is not None:
            metrics.load_state(self._pending[which])  # type: ignore[arg-type]
            self._pending[which] = None

    # -- validation -------------------------------------------------------------------------------
    def _validate(self, val_loader: Iterable[tuple[Tensor, ...]]) -> dict[str, float]:
        model = self.model
        devices = [self.device] if self.device.type == "cuda" else []
        was_training = model.training
        first, shown = 0, []
        with torch.no_grad(), torch.random.fork_rng(devices=devices):
            torch.manual_seed(self.seed + 1)
            for k, batch in enumerate(val_loader):
                logged = model.validation_step(batch, k)
                rows = int(batch[0].shape[0])
                if self.val_metrics is None:
                    self.val_metrics = EpochMetrics(None, None, list(logged), prefix="", device=self.device)
                    self._load_pending("val", self.val_metrics)
                self.val_metrics.fold(logged, float(rows), k)
                if self.panel_logger is not None and first < MAX_EPISODES:
                    shown.append((batch, first))
                first += rows * self.world
            extra = model.on_validation_epoch_end() if hasattr(model, "on_validation_epoch_end") else {}
            for batch, at in shown:  # (after the last validation draw: an epoch with panels validates on the same draws as one without)
                self.panel_logger(model, batch, "val", self.epoch, at)
        model.train(was_training)
        out: dict[str, float] = {}
        if self.val_metrics is not None:
            out = self.val_metrics.compute(group=True if self.group is None else self.group)
            bad = out.pop("bad_steps")
            if bad:
                out["val/bad_steps"] = bad
            self.val_metrics.reset(0)
        out.update({k: float(v) for k, v in (extra or {}).items()})
        return out

    # -- checkpoints ------------------------------------------------------------------------------
    def checkpoint(self) -> dict[str, object]:
        """Everything a run continues from, as tensors and plain Python values (``torch.load(weights_only=True)`` reads it)."""
        model, opt = self.model, self.opt
        carry = getattr(model, "state_carry", None)
        ckpt: dict[str, object] = {
            "format": FORMAT,
            "state_dict": {k: _cpu(v) for k, v in model.state_dict().items()},
            "epoch": self.epoch, "global_step": self.global_step, "batch_in_epoch": self.batch_in_epoch,
            "optimizer": None, "scheduler": _scheduler_state(self.scheduler),
            "early_stopping": None if self.early_stopping is None else self.early_stopping.state_dict(),
            "best": dict(self.best), "seed": self.seed, "world": self.world,
            "noise_generator": None if self.noise is None else self.noise.gen.get_state().clone(),
            "device_rng": (torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else torch.get_rng_state()).clone(),
            "loader": self._loader_state,
            "state_carry": None,
            "metrics": {"train": None if self.train_metrics is None else self.train_metrics.state(),
                        "val": None if self.val_metrics is None else self.val_metrics.state()},
        }
        if carry is not None:
            buffers, filled = carry.snapshot()
            ckpt["state_carry"] = {"buffers": {p: {k: _cpu(v) for k, v in s.items()} for p, s in buffers.items()}, "filled": dict(filled)}
        if opt is not None:
            opt.sync_lr()  # (a rate the scheduler just changed reaches the device word before it is written down)
            ckpt["optimizer"] = {**{k: _cpu(v) if isinstance(v, Tensor) else v for k, v in opt.state_dict().items()},
                                 "state": _cpu(opt.state), "touched": [bool(t) for t in opt.flat.touched]}
        return ckpt

    def save(self, name: str) -> Path | None:
        """Write ``{directory}/{name}`` (rank 0 only; the other ranks return None)."""
        if self.rank != 0:
            return None
        self.directory.mkdir(parents=True, exist_ok=True)
        path = self.directory / name
        tmp = path.with_name(path.name + ".tmp")
        torch.save(self.checkpoint(), tmp)
        tmp.replace(path)
        return path

    def load(self, path: str | Path) -> dict[str, object]:
        """Restore a checkpoint of ``save`` into this Trainer's (freshly built) objects."""
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(ckpt, dict) or ckpt.get("format") != FORMAT:
            msg = f"{path} is not a checkpoint of this Trainer (format {FORMAT!r})"
            raise ValueError(msg)
        if int(ckpt["world"]) != self.world:
            msg = f"{path} was written by {ckpt['world']} rank(s), this run has {self.world}: the accumulators and the carry hold per-rank rows"
            raise ValueError(msg)
        model, opt = self.model, self.opt
        with torch.no_grad():  # (parameters are views of the flat buffer: copied in place)
            model.load_state_dict(ckpt["state_dict"], strict=True)
        conv.invalidate_packs()
        if opt is not None and ckpt["optimizer"] is not None:
            saved = ckpt["optimizer"]
            opt.load_state_dict(saved)
            with torch.no_grad():
                opt.state.copy_(saved["state"])  # (the device-resident lr, step count and bias corrections, bit for bit)
            opt._lr_on_device = float(saved["state"][0])  # noqa: SLF001  (what the device holds NOW: sync_lr uploads param_groups' rate if it differs)
            for i, t in enumerate(saved["touched"]):
                if t:
                    opt.flat.mark_touched(i)
        if self.scheduler is not None and ckpt["scheduler"] is not None:
            self.scheduler.best, self.scheduler.num_bad_epochs = float(ckpt["scheduler"]["best"]), int(ckpt["scheduler"]["num_bad_epochs"])
        if self.early_stopping is not None and ckpt["early_stopping"] is not None:
            self.early_stopping.load_state_dict(ckpt["early_stopping"])
        self.best = dict(ckpt["best"])
        if self.noise is not None and ckpt["noise_generator"] is not None:
            self.noise.gen.set_state(ckpt["noise_generator"])
        if self.device.type == "cuda":
            torch.cuda.set_rng_state(ckpt["device_rng"], self.device)
        else:
            torch.set_rng_state(ckpt["device_rng"])
        carry = getattr(model, "state_carry", None)
        if ckpt["state_carry"] is not None:
            if carry is None:
                msg = f"{path} holds a carried state: set model.state_carry before fit(resume=...)"
                raise ValueError(msg)
            carry.restore((ckpt["state_carry"]["buffers"], ckpt["state_carry"]["filled"]))
        self.epoch, self.global_step, self.batch_in_epoch = int(ckpt["epoch"]), int(ckpt["global_step"]), int(ckpt["batch_in_epoch"])
        self._loader_state = ckpt["loader"]
        self._pending = dict(ckpt["metrics"])
        for which, attr in (("train", "train_metrics"), ("val", "val_metrics")):
            state = self._pending.get(which)
            if state is not None and getattr(self, attr) is None:  # (their keys are in the file: made now, not at the first step)
                made = self._make_train_metrics(state["keys"]) if which == "train" else EpochMetrics(None, None, state["keys"], prefix="", device=self.device)
                setattr(self, attr, made)
                self._load_pending(which, made)
        return ckpt

    # -- the loop ---------------------------------------------------------------------------------
    @staticmethod
    def _epoch_batches(loader: Iterable[tuple[Tensor, ...]], epoch: int, skip: int) -> Iterator[tuple[Tensor, ...]]:
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(epoch)
        if hasattr(loader, "batches"):
            return iter(loader.batches(skip))
        it = iter(loader)
        for _ in range(skip):  # (a plain iterable has no schedule to walk: its skipped batches are made and dropped)
            next(it)
        return it

    def _check_loader(self, loader: object) -> None:
        state = {k: getattr(loader, k) for k in ("seed", "batch_size", "n", "window", "noise_seed") if hasattr(loader, k)}
        if self._loader_state is not None and self._loader_state.get("made_for") not in (None, state):
            msg = f"the checkpoint was written with a loader of {self._loader_state['made_for']}, this one is {state}: the epoch's schedule would differ"
            raise ValueError(msg)
        self._loader_state = {"made_for": state, "seed": state.get("seed"), "epoch": self.epoch, "noise_word": getattr(loader, "noise_word", None)}

    def _lr(self) -> float | None:
        return None if self.opt is None else float(self.opt.param_groups[0]["lr"])

    def _is_better(self, value: float) -> bool:
        best = self.best["value"]
        if not math.isfinite(value):
            return False
        return best is None or (value < best if self.mode == "min" else value > best)

    def _epoch_end(self, val_loader: Iterable[tuple[Tensor, ...]] | None, lr: float | None, started: float, epoch_started: float) -> dict[str, object]:
        metrics: dict[str, float] = {}
        if self.train_metrics is not None:
            metrics.update(self.train_metrics.compute(check=True))
        train_time = time.time() - epoch_started  # (the copy above waited for the epoch's last step)
        if val_loader is not None:
            metrics.update(self._validate(val_loader))
        value = metrics.get(self.monitor)
        if self.train_metrics is not None:
            self.train_metrics.reset(self.global_step)
        line = {"epoch": self.epoch, "global_step": self.global_step, "lr": lr, **metrics, "train_time": train_time, "wall_time": time.time() - started}
        if value is not None:
            if self.scheduler is not None:
                self.scheduler.step(value)
            if self.early_stopping is not None and self.early_stopping.step(value, self.epoch):
                self.should_stop = True
        improved = value is not None and self._is_better(float(value))
        if improved:
            self.best = {"value": float(value), "epoch": self.epoch, "global_step": self.global_step}
        # the files describe the state the NEXT epoch starts from
        self.epoch, self.batch_in_epoch = self.epoch + 1, 0
        if self._loader_state is not None:
            self._loader_state["epoch"] = self.epoch
        if improved or (value is None and self.best["value"] is None):
            self.save("best.ckpt")
        self.save("last.ckpt")
        if self.rank == 0:
            self.directory.mkdir(parents=True, exist_ok=True)
            with (self.directory / "metrics.jsonl").open("a") as f:
                strict = {k: (None if isinstance(v, float) and not math.isfinite(v) else v) for k, v in line.items()}
                f.write(json.dumps(strict, allow_nan=False) + "\n")  # (a non-finite metric is null: NaN is no JSON)
        self.history.append(line)
        return line

    def fit(self, train_loader: Iterable[tuple[Tensor, ...]], val_loader: Iterable[tuple[Tensor, ...]] | None = None,
            resume: str | Path | None = None) -> list[dict[str, object]]:
        """Train until ``max_epochs``, ``max_steps`` or early stopping; returns the epochs' metric lines (also in ``metrics.jsonl``)."""
        if resume is not None:
            self.load(resume)
        started = time.time()
        step_fn = self._own_step if self.train_step is None else self.train_step
        self.model.train()
        self._check_loader(train_loader)
        while self.epoch < self.max_epochs and not self.should_stop:
            if self.max_steps is not None and self.global_step >= self.max_steps:
                break
            lr, epoch_started = self._lr(), time.time()
            if self.train_metrics is not None and self.batch_in_epoch == 0:
                self.train_metrics.reset(self.global_step)
            stopped_inside = False
            for batch in self._epoch_batches(train_loader, self.epoch, self.batch_in_epoch):
                self._loader_state["noise_word"] = getattr(train_loader, "noise_word", None)
                logs = step_fn(batch)
                self._fold_train(logs, int(batch[0].shape[0]))
                self.global_step += 1
                self.batch_in_epoch += 1
                if self.global_step % self.check_every == 0:
                    self.train_metrics.check()
                at_limit = self.max_steps is not None and self.global_step >= self.max_steps
                if at_limit or (self.save_every is not None and self.global_step % self.save_every == 0):
                    if at_limit and self._epoch_is_over(train_loader):
                        break  # (the limit fell on the epoch's last step: the epoch ends as any other)
                    self.save("last.ckpt")
                    if at_limit:
                        stopped_inside = True
                        break
            if stopped_inside:
                self.train_metrics.check()
                return self.history
            self._epoch_end(val_loader, lr, started, epoch_started)
        return self.history

    def _epoch_is_over(self, loader: object) -> bool:
        try:
            return self.batch_in_epoch >= len(loader)  # type: ignore[arg-type]
        except TypeError:
            return False


__all__ = ["EarlyStopping", "EpochMetrics", "Trainer", "fold_reference", "parameter_names", "segment_runs"]
