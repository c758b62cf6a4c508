"""Particle-filter likelihood: the sampled posteriors of a likelihood step, weighted per frame and resampled in time.

The whole-trajectory bound of ``likelihood.py`` sums its log-weights over all ``T`` frames before it compares the ``S``
samples of a row, so after a few frames one sample carries all the weight.  A particle filter (sequential Monte Carlo, the FIVO
estimator) compares them frame by frame, resamples the particles in proportion to their weights when those have collapsed and carries
on from the survivors.  ``log Z`` stays a lower bound in expectation and ``Z`` unbiased.

Row ``b`` has ``S`` particles (``1 <= S <= 16``); particle ``(b, s)`` is scan row ``b * S + s``.  Time is cut into segments of
``resample_every = c >= 1`` frames (the last may be shorter), ``J = ceil(T / c)``.  Frame ``t`` is live iff ``t < valid[b]``; per live
frame and particle ``a``, ``v``, ``r`` and ``l = (a + v) + r`` are those of ``likelihood.py``.  Per row, in double and zero at the start:
``lw[s]``, ``base``, ``prev``.  On a live frame

    lw[s] += l[s];  top = max_s lw;  w_s = exp(lw_s - top);  sum_w = sum_s w_s (a left fold)
    L = base + (top + log sum_w) - log S

and eight planes ``[8, B, T]`` (``PLANES``), each exactly 0 on dead frames:

    0 smc          L - prev, then prev = L
    1 mean         (1 / S) sum_s l[s]
    2, 3, 4 audio, vision, latent   as planes 2, 3, 4 of ``likelihood.py``
    5 ess          sum_w^2 / sum_s w_s^2, before any resampling
    6 resampled    1 if the particles were resampled after this frame, else 0
    7 smc_prefix   L

Resampling is considered only at the last frame ``t`` of a segment that is not the last one.  It happens iff ``t`` is live,
``t + 1 < valid[b]`` and ``ess <= threshold * S`` (``0 <= threshold <= 1``: 0 never resamples, 1 always does).  It is systematic with one
uniform ``u = u_resample[b, t]``: ``c_s`` the left-fold prefix sums of ``w``, ``target_i = ((u + i) / S) * sum_w``,
``ancestor[b, i] = min(S - 1, #{s : c_s <= target_i})``; then ``base = L`` and ``lw[:] = 0``.  Otherwise the ancestors are the identity.
Slot ``i`` continues from the end-of-segment posterior state of slot ``ancestor[b, i]`` and draws its own ``u_post[b, i, t + 1 ...]``.

With ``threshold = 0`` planes 0, 2, 3, 4, 5, 7 are planes 0, 2, 3, 4, 5, 6 of ``likelihood.py`` for any ``c`` and plane 1 is its ``elbo``;
at ``S = 1`` ``smc`` equals ``mean`` up to the one rounding.  ``ParticleFilter.reference`` states the rule in torch, in float64;
``mtrssm_particle_fold`` (one segment) and ``mtrssm_particle_gather`` (the states by ancestor) are the kernels, used for GPU tensors;
elsewhere the torch rules run.
"""

from __future__ import annotations

import ctypes as C
import math

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.likelihood import HALF_LOG_2PI, LikelihoodBound
from multimodal_mtrssm_amd.skill import MAX_SAMPLES, MODALITIES, ForecastSkill, ObservingConfig, PlaneTable

PLANES = ("smc", "mean", "audio", "vision", "latent", "ess", "resampled", "smc_prefix")
TABLE_ROWS = PLANES[:7]  # what a ParticleTable folds by frame position


def _sum_s(x: Tensor) -> Tensor:
    """The sum over dim 1 (``s``) as a left fold."""
    total = x[:, 0]
    for i in range(1, x.shape[1]):
        total = total + x[:, i]
    return total


class ParticleFilter(ObservingConfig):
    """``ParticleFilter(samples=S, resample_every=c, threshold=..., observe=..., score=..., latent=...)``: ``S`` (1 .. 16) particles per
    row, proposed by the posterior that sees ``observe`` at every live step; after every ``c`` frames a row whose effective sample size
    is at most ``threshold * S`` is resampled.  ``score`` and ``latent`` switch the terms of the weights as in ``LikelihoodBound``, whose
    argument rules these are.  ``max_frames``: the decoders and the scorer run over chunks of whole rows of at most this many frames."""

    def __init__(self, samples: int = 1, resample_every: int = 1, threshold: float = 0.5, observe: str = "both",  # noqa: PLR0913
                 score: tuple[str, ...] = MODALITIES, latent: bool = True) -> None:  # noqa: FBT001, FBT002
        terms = LikelihoodBound(samples, observe, score, latent)  # (its refusals)
        if isinstance(resample_every, bool) or not isinstance(resample_every, int) or not 1 <= resample_every < 1 << 24:
            msg = f"resample_every must be an integer 1 <= c < 2^24, got {resample_every!r}"
            raise ValueError(msg)
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= float(threshold) <= 1.0:
            msg = f"threshold must be a number in [0, 1], got {threshold!r}"
            raise ValueError(msg)
        self.samples, self.observe, self.score, self.latent = terms.samples, terms.observe, terms.score, terms.latent
        self.resample_every, self.threshold = resample_every, float(threshold)
        self.max_frames = 4096
        self.group = None  # the process group ParticleTable.all_reduce uses (FlatDataParallel.particle binds it)

    def __repr__(self) -> str:
        return (f"ParticleFilter(samples={self.samples}, resample_every={self.resample_every}, threshold={self.threshold}, "
                f"observe={self.observe!r}, score={self.score!r}, latent={self.latent})")

    def plan(self):  # noqa: ANN201
        """The copies of a row are those of a likelihood step: own initial draws ``u_init (B, S, K)`` and own ``u_post (B, S, T, K)``."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(self.samples, self.bits, None, init="copy", post="copy")

    def noise_shapes(self, model, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # noqa: ANN001
        """The plan's uniforms and ``u_resample (B, T)``: one uniform per row and frame, read at the segment ends that resample."""
        return self.plan().noise_shapes(model, batch, steps) | {"u_resample": (batch, steps)}

    def segments(self, steps: int) -> list[tuple[int, int]]:
        """``(t0, t1)`` of the ``J = ceil(T / c)`` time segments."""
        c = self.resample_every
        return [(t0, min(steps, t0 + c)) for t0 in range(0, steps, c)]

    # -- the rule in torch, in float64 ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked_segment(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None,  # noqa: PLR0913
                         event_audio: int, event_vision: int, threshold: float) -> tuple[int, int, int]:
        b, s, c = LikelihoodBound._checked_bound(se_audio, se_vision, log_ratio, valid, event_audio, event_vision)  # noqa: SLF001
        if not 0.0 <= float(threshold) <= 1.0:
            msg = f"threshold must lie in [0, 1], got {threshold!r}"
            raise ValueError(msg)
        return b, s, c

    @staticmethod
    def _checked_uniform(u: Tensor | None, b: int, ref: Tensor) -> None:
        if u is None or u.dtype != torch.float32 or tuple(u.shape) != (b,) or u.device != ref.device:
            msg = f"a segment that may resample needs its uniforms u: float32 ({b},) on {ref.device}"
            raise ValueError(msg)

    @staticmethod
    def segment_reference(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None,  # noqa: PLR0913, PLR0914, PLR0917
                          u: Tensor | None, t0: int, threshold: float, last_segment: bool, carry: Tensor,  # noqa: FBT001
                          event_audio: int = 0, event_vision: int = 0) -> tuple[Tensor, Tensor, float]:
        """One segment of the rule in float64: the inputs are ``[B, S, c]`` (the frames ``t0 .. t0 + c - 1``), ``u`` ``[B]`` the
        uniforms of its last frame (not read by the last segment), ``carry`` double ``[B, S + 2]`` (``lw``, ``base``, ``prev``), which is
        UPDATED IN PLACE.  Returns the planes ``[8, B, c]`` (float64), the ancestors ``[B, S]`` (int32) and the margin: the smallest
        ``|target_i - c_s| / sum_w`` over the rows that resampled (``inf`` without one)."""
        b, s, c = ParticleFilter._checked_segment(se_audio, se_vision, log_ratio, valid, event_audio, event_vision, threshold)
        ref = next(x for x in (se_audio, se_vision, log_ratio) if x is not None)
        dev, f64 = ref.device, torch.float64
        if carry.dtype != f64 or tuple(carry.shape) != (b, s + 2) or carry.device != dev:
            msg = f"carry must be a float64 ({b}, {s + 2}) tensor on {dev}, got {carry.dtype} {tuple(carry.shape)}"
            raise ValueError(msg)
        if not last_segment:
            ParticleFilter._checked_uniform(u, b, ref)
        frames = torch.arange(t0, t0 + c, device=dev)
        left = torch.full((b,), 1 << 40, device=dev, dtype=torch.int64) if valid is None else valid.to(torch.int64).clamp(min=0)
        live = frames.unsqueeze(0) < left.unsqueeze(1)  # [B, c]
        zero = torch.zeros(b, s, c, dtype=f64, device=dev)

        def term(x: Tensor | None, const: float, sign: float) -> Tensor:
            if x is None:
                return zero
            return torch.where(live.unsqueeze(1), sign * x.to(f64) - const, zero)

        a = term(se_audio, HALF_LOG_2PI * event_audio, -1.0)
        v = term(se_vision, HALF_LOG_2PI * event_vision, -1.0)
        r = term(log_ratio, 0.0, 1.0)
        step = (a + v) + r
        lw, base, prev = carry[:, :s].clone(), carry[:, s].clone(), carry[:, s + 1].clone()
        planes = torch.zeros(len(PLANES), b, c, dtype=f64, device=dev)
        identity = torch.arange(s, device=dev, dtype=torch.int32).expand(b, s)
        ancestor, margin = identity.clone(), math.inf
        nothing = torch.zeros((), dtype=f64, device=dev)
        for j in range(c):
            on = live[:, j]
            lw = lw + step[:, :, j]
            top = lw.max(dim=1).values
            w = torch.exp(lw - top.unsqueeze(1))
            sum_w = _sum_s(w)
            now = base + (top + torch.log(sum_w)) - math.log(float(s))
            ess = (sum_w * sum_w) / _sum_s(w * w)
            rows = (now - prev, _sum_s(step[:, :, j]) / float(s), _sum_s(a[:, :, j]) / float(s), _sum_s(v[:, :, j]) / float(s),
                    _sum_s(r[:, :, j]) / float(s), ess, nothing, now)
            for p, x in enumerate(rows):
                planes[p, :, j] = torch.where(on, x, nothing)
            prev = torch.where(on, now, prev)
            if j == c - 1 and not last_segment:
                resample = on & (t0 + c < left) & (ess <= float(threshold) * float(s))
                prefix = torch.empty_like(w)
                run = torch.zeros(b, dtype=f64, device=dev)
                for k in range(s):
                    run = run + w[:, k]
                    prefix[:, k] = run
                slots = torch.arange(s, device=dev, dtype=f64)
                target = ((u.to(f64).unsqueeze(1) + slots) / float(s)) * sum_w.unsqueeze(1)  # [B, i]
                count = (prefix.unsqueeze(1) <= target.unsqueeze(2)).sum(dim=2)
                ancestor = torch.where(resample.unsqueeze(1), count.clamp(max=s - 1).to(torch.int32), identity)
                if bool(resample.any()):
                    gap = ((target.unsqueeze(2) - prefix.unsqueeze(1)).abs() / sum_w.reshape(b, 1, 1))[resample]
                    margin = float(gap.min())
                planes[6, :, j] = resample.to(f64)
                base = torch.where(resample, now, base)
                lw = torch.where(resample.unsqueeze(1), torch.zeros_like(lw), lw)
        carry[:, :s], carry[:, s], carry[:, s + 1] = lw, base, prev
        return planes, ancestor, margin

    @staticmethod
    def reference(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None = None,  # noqa: PLR0913
                  event_audio: int = 0, event_vision: int = 0, *, resample_every: int = 1, threshold: float = 0.5,
                  u_resample: Tensor | None = None, ancestors: Tensor | None = None) -> tuple[Tensor, Tensor, float]:
        """The rule over full ``[B, S, T]`` inputs in float64: the eight planes ``[8, B, T]``, the ancestors ``[B, S, J]`` (int32) and
        ``margin``, the smallest ``|target_i - c_s| / sum_w`` over all resamplings (``inf`` when nothing was resampled): how far the
        nearest decision between two ancestors was from flipping.  ``u_resample``: fp32 ``[B, T]`` (None only where nothing can
        resample: ``threshold = 0`` or one segment).  The inputs at frame ``t`` are those of the slot, as given -- the caller's
        trajectories already continue from their ancestors.  ``ancestors=`` (``[B, S, J]``) replays: the rule still says WHEN a row
        resamples (that depends on the weights only) but the given ancestors are returned instead of being decided, no uniform is
        read and the margin is ``inf``."""
        b, s, t = ParticleFilter._checked_segment(se_audio, se_vision, log_ratio, valid, event_audio, event_vision, threshold)
        ref = next(x for x in (se_audio, se_vision, log_ratio) if x is not None)
        c = int(resample_every)
        if c < 1:
            msg = f"resample_every must be >= 1, got {resample_every!r}"
            raise ValueError(msg)
        starts = list(range(0, t, c))
        if ancestors is not None and tuple(ancestors.shape) != (b, s, len(starts)):
            msg = f"ancestors must have shape {(b, s, len(starts))}, got {tuple(ancestors.shape)}"
            raise ValueError(msg)
        if u_resample is None and (ancestors is not None or float(threshold) == 0.0 or len(starts) == 1):
            u_resample = torch.full((b, t), 0.5, dtype=torch.float32, device=ref.device)
        if u_resample is None or tuple(u_resample.shape) != (b, t) or u_resample.dtype != torch.float32:
            msg = f"u_resample must be a float32 {(b, t)} tensor"
            raise ValueError(msg)
        carry = torch.zeros(b, s + 2, dtype=torch.float64, device=ref.device)
        planes, chosen, margin = [], [], math.inf
        for t0 in starts:
            t1 = min(t, t0 + c)
            cut = [None if x is None else x[:, :, t0:t1] for x in (se_audio, se_vision, log_ratio)]
            part, anc, gap = ParticleFilter.segment_reference(*cut, valid, u_resample[:, t1 - 1], t0, threshold, t1 == t, carry, event_audio,
                                                              event_vision)
            planes.append(part)
            chosen.append(anc)
            margin = min(margin, gap)
        found = torch.stack(chosen, dim=2)
        if ancestors is not None:
            return torch.cat(planes, dim=2), ancestors.to(torch.int32), math.inf
        return torch.cat(planes, dim=2), found, margin

    # -- kernels on the GPU, the rules elsewhere -----------------------------------------------------------------------------------------
    @staticmethod
    def new_carry(batch: int, samples: int, device: torch.device | str = "cpu") -> Tensor:
        """The fold's carried state of ``batch`` rows before their first segment: double ``[B, S + 2]`` (``lw``, ``base``, ``prev``), zero."""
        return torch.zeros(batch, samples + 2, dtype=torch.float64, device=device)

    @staticmethod
    def fold(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None, u: Tensor | None,  # noqa: PLR0913, PLR0917
             t0: int, threshold: float, last_segment: bool, carry: Tensor, event_audio: int = 0, event_vision: int = 0, *,  # noqa: FBT001
             planes: Tensor | None = None, ancestor: Tensor | None = None) -> tuple[Tensor, Tensor]:
        """One ``mtrssm_particle_fold`` launch on torch's current stream (non-GPU tensors: ``segment_reference``): folds the segment
        ``[B, S, c]`` that begins at frame ``t0`` into ``carry`` (double ``[B, S + 2]``, read and written) and returns its planes (fp32
        ``[8, B, c]``) and ancestors (int32 ``[B, S]``), written into ``planes`` / ``ancestor`` when given.  ``u``: the segment's column of
        ``u_resample``, fp32 ``[B]`` with any stride (e.g. ``u_resample[:, t0 + c - 1]``); None for the last segment."""
        b, s, c = ParticleFilter._checked_segment(se_audio, se_vision, log_ratio, valid, event_audio, event_vision, threshold)
        ref = next(x for x in (se_audio, se_vision, log_ratio) if x is not None)
        dev = ref.device
        if t0 < 0 or t0 + c >= 1 << 30:
            msg = f"the segment's frames {t0} .. {t0 + c - 1} must lie in [0, 2^30)"
            raise ValueError(msg)
        if carry.dtype != torch.float64 or tuple(carry.shape) != (b, s + 2) or not carry.is_contiguous() or carry.device != dev:
            msg = f"carry must be a contiguous float64 ({b}, {s + 2}) tensor on {dev}, got {carry.dtype} {tuple(carry.shape)}"
            raise ValueError(msg)
        if not last_segment:
            ParticleFilter._checked_uniform(u, b, ref)
        if planes is None:
            planes = torch.empty(len(PLANES), b, c, device=dev, dtype=torch.float32)
        if ancestor is None:
            ancestor = torch.empty(b, s, device=dev, dtype=torch.int32)
        if tuple(planes.shape) != (len(PLANES), b, c) or planes.dtype != torch.float32 or not planes.is_contiguous() or planes.device != dev:
            msg = f"planes must be a contiguous float32 [{len(PLANES)}, {b}, {c}] buffer on {dev}, got {planes.dtype} {tuple(planes.shape)}"
            raise ValueError(msg)
        if tuple(ancestor.shape) != (b, s) or ancestor.dtype != torch.int32 or not ancestor.is_contiguous() or ancestor.device != dev:
            msg = f"ancestor must be a contiguous int32 ({b}, {s}) buffer on {dev}, got {ancestor.dtype} {tuple(ancestor.shape)}"
            raise ValueError(msg)
        if not ref.is_cuda:
            got, anc, _ = ParticleFilter.segment_reference(se_audio, se_vision, log_ratio, valid, u, t0, threshold, last_segment, carry,
                                                           event_audio, event_vision)
            planes.copy_(got.to(torch.float32))
            ancestor.copy_(anc)
            return planes, ancestor
        se_audio, se_vision, log_ratio, valid = (None if x is None else x.contiguous() for x in (se_audio, se_vision, log_ratio, valid))
        stride = 1 if last_segment else max(1, u.stride(0))
        _lib.check(_lib.TIMERS.call("mtrssm_particle_fold", _lib.load().mtrssm_particle_fold, _lib.ptr(se_audio), _lib.ptr(se_vision),
                                    _lib.ptr(log_ratio), _lib.index_ptr(valid), None if last_segment else _lib.raw_ptr(u), stride, int(t0), b, s, c,
                                    int(event_audio), int(event_vision), float(threshold), int(bool(last_segment)), _lib.raw_ptr(carry),
                                    _lib.ptr(planes), _lib.index_ptr(ancestor), _lib.stream_ptr(dev),
                                    nbytes=4.0 * b * c * (3 * s + len(PLANES)) + 16.0 * b * (s + 2) + 4.0 * b * s), "mtrssm_particle_fold")
        return planes, ancestor

    @staticmethod
    def gather_reference(last: list[Tensor], ancestor: Tensor) -> list[Tensor]:
        """``out[k][b * S + i] = last[k][b * S + ancestor[b, i], steps - 1]`` for scan outputs ``[B * S, steps, W]``."""
        b, s = ancestor.shape
        rows = (torch.arange(b, device=ancestor.device).unsqueeze(1) * s + ancestor.to(torch.int64).clamp(0, s - 1)).reshape(-1)
        return [x.detach()[:, -1].index_select(0, rows) for x in last]

    @staticmethod
    def gather(last: list[Tensor], ancestor: Tensor, out: list[Tensor] | None = None) -> list[Tensor]:
        """One ``mtrssm_particle_gather`` launch on torch's current stream for all tensors of a state (non-GPU tensors:
        ``gather_reference``): ``last[k]`` is a contiguous fp32 scan output ``[B * S, steps, W_k]``, ``ancestor`` int32 ``[B, S]``; returns
        the states ``[B * S, W_k]`` the next segment starts from (written into ``out`` when given; never in place)."""
        if ancestor.dim() != 2 or ancestor.dtype != torch.int32 or not 1 <= ancestor.shape[1] <= MAX_SAMPLES:  # noqa: PLR2004
            msg = f"ancestor must be an int32 [B, S] tensor with 1 <= S <= {MAX_SAMPLES}, got {ancestor.dtype} {tuple(ancestor.shape)}"
            raise ValueError(msg)
        b, s = ancestor.shape
        if not 0 < len(last) <= _lib.STATE_MAX:
            msg = f"a state table holds 1 .. {_lib.STATE_MAX} tensors, got {len(last)}"
            raise ValueError(msg)
        steps = last[0].shape[1] if last[0].dim() == 3 else 0  # noqa: PLR2004
        for x in last:
            if x.dim() != 3 or tuple(x.shape[:2]) != (b * s, steps) or steps < 1 or x.shape[2] < 1 or x.device != ancestor.device:  # noqa: PLR2004
                msg = f"particle_gather: scan output {tuple(x.shape)} is not [{b * s}, {steps}, W] on {ancestor.device}"
                raise ValueError(msg)
        if out is None:
            out = [torch.empty(b * s, x.shape[2], device=x.device, dtype=torch.float32) for x in last]
        for x, o in zip(last, out, strict=True):
            if tuple(o.shape) != (b * s, x.shape[2]) or o.dtype != torch.float32 or not o.is_contiguous() or o.device != x.device:
                msg = f"particle_gather: out {tuple(o.shape)} does not match the scan output {tuple(x.shape)}"
                raise ValueError(msg)
        if not ancestor.is_cuda:
            for o, got in zip(out, ParticleFilter.gather_reference(last, ancestor), strict=True):
                o.copy_(got)
            return out
        srcs = [x.detach() for x in last]
        table = _lib.StateTable()
        table.count = len(srcs)
        for k, (src, dst) in enumerate(zip(srcs, out, strict=True)):
            table.width[k] = dst.shape[-1]
            table.src_stride[k] = src.stride(0)
            table.src[k] = _lib.ptr(src)  # (contiguous fp32 on the GPU, or MtrssmLibraryError)
            table.alt[k] = None
            table.dst[k] = _lib.ptr(dst)
        moved = 8.0 * b * s * sum(o.shape[1] for o in out)
        _lib.check(_lib.TIMERS.call("mtrssm_particle_gather", _lib.load().mtrssm_particle_gather, C.byref(table),
                                    _lib.index_ptr(ancestor.contiguous()), b, s, steps, _lib.stream_ptr(ancestor.device), nbytes=moved),
                   "mtrssm_particle_gather")
        return out


class ParticleTable(PlaneTable):
    """The accumulated particle-filter bound of any number of steps in ONE fp32 buffer ``[7 + 1, T]``: the planes ``TABLE_ROWS`` (smc,
    mean, audio, vision, latent, ess, resampled) summed by frame position, then the counts of live frames.  A step run with
    ``keep_states`` also leaves ``planes`` ``[8, B, T]``, ``ancestors`` int32 ``[B, S, J]`` and ``inputs`` -- the fp32 ``se_audio``,
    ``se_vision`` and ``ratio`` ``[B, S, T]`` as the fold saw them (None for a term that is off)."""

    ROWS = len(TABLE_ROWS)

    def __init__(self, steps: int, device: torch.device | str = "cpu") -> None:
        super().__init__(steps, device)
        self.ancestors: Tensor | None = None
        self.inputs: dict[str, Tensor | None] | None = None

    def fold(self, planes: Tensor, valid: Tensor | None = None) -> ParticleTable:
        """Adds a step's planes (``[8, B, T]`` or their first seven) by frame position: ``mtrssm_horizon_table`` with ``context = 1``."""
        if planes.dim() != 3 or planes.shape[0] < self.ROWS or planes.shape[2] != self.steps:  # noqa: PLR2004
            msg = f"planes must be [>= {self.ROWS}, B, {self.steps}], got {tuple(planes.shape)}"
            raise ValueError(msg)
        context = torch.ones(planes.shape[1], dtype=torch.int32, device=planes.device)
        ForecastSkill.table_add(planes[: self.ROWS], context, valid, self.sums, self.counts)
        return self

    def curves(self) -> dict[str, Tensor]:
        """``sums / counts`` per plane, ``[T]`` each: the mean over the rows that are live at frame ``t``; an empty bin gives NaN."""
        return {name: self._mean(row, self.counts) for name, row in zip(TABLE_ROWS, self.sums, strict=True)}

    def per_frame(self) -> dict[str, Tensor]:
        """Each plane's summed row over the summed counts: nats per live frame (``ess``: its mean, ``resampled``: the fraction of live
        frames after which a row was resampled); NaN for an empty table."""
        total = self.counts.sum()
        return {name: self._mean(row.sum(), total) for name, row in zip(TABLE_ROWS, self.sums, strict=True)}

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix/{smc,mean,audio,vision,latent,ess,resampled}``: ``per_frame`` as a flat dict."""
        return {f"{prefix}/{name}": value for name, value in self.per_frame().items()}


__all__ = ["PLANES", "TABLE_ROWS", "ParticleFilter", "ParticleTable"]
