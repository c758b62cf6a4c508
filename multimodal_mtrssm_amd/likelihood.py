"""Held-out likelihood: the importance-weighted bound of sampled posterior trajectories.

A *likelihood step* gives row ``b`` ``S`` sampled posterior trajectories (``1 <= S <= 16``; the proposal sees ``observe`` at every live
step).  Frame ``t`` is live iff ``t < valid[b]``.  For a live frame and sample ``s``:

    a[b, s, t] = -se_audio[b, s, t] - 0.5 E_a log 2 pi        se: the data term ``mtrssm_ensemble_score`` writes into ``se_samples``,
    v[b, s, t] likewise for vision                            E the modality's C * H * W
    r[b, s, t] = sum_levels sum_k ( log p_k(c*) - log q_k(c*) )

``p`` / ``q`` are the per-categorical softmaxes of the rollout's ``prior_logits`` / ``post_logits`` and ``c*`` the class the posterior
sample took: the first ``c`` with ``post_stoch > 0.5``.  MRSSM has one level, MMTRSSM two (``_l``, ``_h``).  ``kl_coeff``, ``w_kl_h``,
balancing, free bits and ``recon_weights`` do not enter: this is a likelihood bound, not the training loss.  The initial latent is drawn
per copy from the prior head, so its ratio is 1 and it contributes nothing.

``l = (a + v) + r`` over the terms that are switched on, ``cum[b, s, t] = sum_{t' <= t} l[b, s, t']`` a left fold; a dead frame adds 0.
Per ``(b, t)`` eight planes ``[8, B, T]`` (``PLANES``), each exactly 0 on dead frames:

    0 iw            L[t] - L[t-1],  L[t] = logsumexp_s cum[., t] - log S  (= max + log sum exp(cum - max) - log S),  L[-1] = 0
    1 elbo          M[t] - M[t-1],  M[t] = (1 / S) sum_s cum[s, t]
    2, 3, 4 audio, vision, latent   (1 / S) sum_s of a, v, r at frame t; 0 when that term is off
    5 ess           (sum_s w)^2 / sum_s w^2,  w = exp(cum[s, t] - max_s cum[., t])
    6, 7 iw_prefix, elbo_prefix     L[t], M[t]

``L[t] >= M[t]`` (Jensen); at ``S = 1`` planes 0 and 6 equal planes 1 and 7 bit for bit; ``elbo = audio + vision + latent``.
``LikelihoodBound.reference_ratio`` and ``LikelihoodBound.reference`` state the two rules in torch, in float64;
``mtrssm_latent_log_ratio`` and ``mtrssm_iw_bound`` are the kernels, used for GPU tensors; elsewhere the torch rule runs.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.skill import MAX_SAMPLES, MODALITIES, OBSERVE_BITS, ForecastSkill, ObservingConfig, PlaneTable

PLANES = ("iw", "elbo", "audio", "vision", "latent", "ess", "iw_prefix", "elbo_prefix")
TABLE_ROWS = PLANES[:6]  # what a LikelihoodTable folds by frame position
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


class LikelihoodBound(ObservingConfig):
    """``LikelihoodBound(samples=S, observe=..., score=..., latent=...)``: ``S`` (1 .. 16) posterior trajectories per row, sampled
    from the posterior that sees ``observe`` (both modalities, audio only or vision only) at every live step; ``score`` names the
    modalities whose data terms enter and ``latent`` switches the latent log-ratio.  ``score=("vision",), latent=False,
    observe="audio"`` is the conditional estimate ``log (1 / S) sum_s p(x_v | z_s)``, ``z_s ~ q(z | x_a)``.  ``max_frames``: the decoders
    and the scorer run over chunks of whole rows (all ``S`` copies of a row together) of at most this many frames."""

    def __init__(self, samples: int = 1, observe: str = "both", score: tuple[str, ...] = MODALITIES, latent: bool = True) -> None:  # noqa: FBT001, FBT002
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= MAX_SAMPLES:
            msg = f"samples must be an integer in 1 .. {MAX_SAMPLES}, got {samples!r}"
            raise ValueError(msg)
        if observe not in OBSERVE_BITS:
            msg = f"observe must be one of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        if isinstance(score, str) or any(m not in MODALITIES for m in score) or len(set(score)) != len(tuple(score)):
            msg = f"score must be a tuple of distinct modalities out of {MODALITIES}, got {score!r}"
            raise ValueError(msg)
        if not isinstance(latent, bool):
            msg = f"latent must be a bool, got {latent!r}"
            raise ValueError(msg)
        if not score and not latent:
            msg = "nothing to score: give a modality in score or latent=True"
            raise ValueError(msg)
        self.samples, self.observe, self.latent = samples, observe, latent
        self.score = tuple(m for m in MODALITIES if m in score)
        self.max_frames = 4096
        self.group = None  # the process group LikelihoodTable.all_reduce uses (FlatDataParallel.likelihood binds it)

    def __repr__(self) -> str:
        return f"LikelihoodBound(samples={self.samples}, observe={self.observe!r}, score={self.score!r}, latent={self.latent})"

    def plan(self):  # noqa: ANN201
        """``S`` copies of a row observe ``observe`` on every live frame; each has its own initial draw ``u_init (B, S, K)`` and its own
        posterior draws ``u_post (B, S, T, K)``."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(self.samples, self.bits, None, init="copy", post="copy")

    # -- the rules in torch, in float64 ------------------------------------------------------------------------------------------------
    @staticmethod
    def _checked_ratio(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, cats: int, classes: int) -> int:
        if cats < 1 or classes < 1:
            msg = f"need K, C >= 1, got {cats}, {classes}"
            raise ValueError(msg)
        if post_logits.dim() < 2 or post_logits.shape[-1] != cats * classes or post_logits.numel() == 0:  # noqa: PLR2004
            msg = f"the logits must be [..., {cats * classes}] (K = {cats} categoricals of C = {classes} classes), got {tuple(post_logits.shape)}"
            raise ValueError(msg)
        if prior_logits.shape != post_logits.shape or stoch.shape != post_logits.shape:
            msg = f"post_logits, prior_logits and stoch must share a shape, got {tuple(post_logits.shape)}, {tuple(prior_logits.shape)}, {tuple(stoch.shape)}"
            raise ValueError(msg)
        rows = post_logits.numel() // (cats * classes)
        if post_logits.numel() >= 1 << 31:
            msg = f"{rows} x {cats} x {classes} logits: rows * K * C must stay below 2^31"
            raise ValueError(msg)
        return rows

    @staticmethod
    def reference_ratio(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, cats: int, classes: int) -> Tensor:
        """``sum_k ( log p_k(c*) - log q_k(c*) )`` in float64, of the leading shape: the inputs are ``[..., K * C]``, ``c*`` is the first
        class with ``stoch > 0.5`` (class 0 when there is none); categoricals are summed in ascending ``k``."""
        LikelihoodBound._checked_ratio(post_logits, prior_logits, stoch, cats, classes)
        lead = post_logits.shape[:-1]
        q = post_logits.to(torch.float64).reshape(*lead, cats, classes)
        p = prior_logits.to(torch.float64).reshape(*lead, cats, classes)
        star = (stoch.reshape(*lead, cats, classes) > 0.5).to(torch.int8).argmax(-1, keepdim=True)  # noqa: PLR2004  (the first maximum)

        def log_prob(x: Tensor) -> Tensor:
            m = x.max(-1, keepdim=True).values
            total = torch.exp(x[..., :1] - m)
            for c in range(1, classes):  # (a left fold, as the kernel's)
                total = total + torch.exp(x[..., c : c + 1] - m)
            return (x.gather(-1, star) - m) - torch.log(total)

        diff = (log_prob(p) - log_prob(q)).squeeze(-1)
        out = diff[..., 0]
        for k in range(1, cats):
            out = out + diff[..., k]
        return out

    @staticmethod
    def _checked_bound(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None,
                       event_audio: int, event_vision: int) -> tuple[int, int, int]:
        given = [x for x in (se_audio, se_vision, log_ratio) if x is not None]
        if not given:
            msg = "give at least one of se_audio, se_vision, log_ratio"
            raise ValueError(msg)
        ref = given[0]
        if ref.dim() != 3 or any(x.shape != ref.shape or x.device != ref.device for x in given):  # noqa: PLR2004
            msg = f"se_audio, se_vision and log_ratio must share one [B, S, T] shape and device, got {[tuple(x.shape) for x in given]}"
            raise ValueError(msg)
        b, s, t = ref.shape
        if not 1 <= s <= MAX_SAMPLES or min(b, t) < 1:
            msg = f"need B, T >= 1 and 1 <= S <= {MAX_SAMPLES}, got {tuple(ref.shape)}"
            raise ValueError(msg)
        if b * t >= 1 << 24:
            msg = f"{b} x {t} frames: B * T must stay below 2^24"
            raise ValueError(msg)
        if valid is not None and (valid.dtype != torch.int32 or tuple(valid.shape) != (b,)):
            msg = f"valid must be an int32 tensor of shape ({b},), got {valid.dtype} {tuple(valid.shape)}"
            raise ValueError(msg)
        if (se_audio is not None and event_audio < 1) or (se_vision is not None and event_vision < 1):
            msg = f"a data term needs its event size E >= 1, got event_audio {event_audio}, event_vision {event_vision}"
            raise ValueError(msg)
        return b, s, t

    @staticmethod
    def reference(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None = None,  # noqa: PLR0913, PLR0914
                  event_audio: int = 0, event_vision: int = 0) -> Tensor:
        """The eight planes ``[8, B, T]`` in float64: the inputs are ``[B, S, T]`` (None: that term is off), ``valid`` int32 ``[B]`` (None:
        every frame is live).  The fold over ``t`` and the sums over ``s`` are left folds."""
        b, s, t = LikelihoodBound._checked_bound(se_audio, se_vision, log_ratio, valid, event_audio, event_vision)
        ref = next(x for x in (se_audio, se_vision, log_ratio) if x is not None)
        dev = ref.device
        live = torch.ones(b, t, dtype=torch.bool, device=dev) if valid is None else torch.arange(t, device=dev) < valid.unsqueeze(1)
        zero = torch.zeros(b, s, t, dtype=torch.float64, device=dev)

        def term(x: Tensor | None, const: float, sign: float) -> Tensor:
            if x is None:
                return zero
            return torch.where(live.unsqueeze(1), sign * x.to(torch.float64) - const, zero)

        a = term(se_audio, HALF_LOG_2PI * event_audio, -1.0)
        v = term(se_vision, HALF_LOG_2PI * event_vision, -1.0)
        r = term(log_ratio, 0.0, 1.0)
        step = (a + v) + r
        cum = torch.empty_like(step)
        run = torch.zeros(b, s, dtype=torch.float64, device=dev)
        for i in range(t):
            run = run + step[:, :, i]
            cum[:, :, i] = run

        def fold(x: Tensor) -> Tensor:  # sum over s of [B, S, T], a left fold
            total = x[:, 0]
            for i in range(1, s):
                total = total + x[:, i]
            return total

        top = cum.max(dim=1).values
        w = torch.exp(cum - top.unsqueeze(1))
        sum_w = fold(w)
        prefix_iw = (top + torch.log(sum_w)) - math.log(float(s))
        prefix_elbo = fold(cum) / float(s)
        first = torch.zeros(b, 1, dtype=torch.float64, device=dev)
        planes = torch.stack([
            prefix_iw - torch.cat([first, prefix_iw[:, :-1]], dim=1), prefix_elbo - torch.cat([first, prefix_elbo[:, :-1]], dim=1),
            fold(a) / float(s), fold(v) / float(s), fold(r) / float(s), (sum_w * sum_w) / fold(w * w), prefix_iw, prefix_elbo])
        return torch.where(live.unsqueeze(0), planes, torch.zeros((), dtype=torch.float64, device=dev))

    # -- kernels on the GPU, the rules elsewhere -------------------------------------------------------------------------------------------
    @staticmethod
    def log_ratio(post_logits: Tensor, prior_logits: Tensor, stoch: Tensor, cats: int, classes: int, *, out: Tensor | None = None,  # noqa: PLR0913
                  accumulate: bool = False) -> Tensor:
        """One ``mtrssm_latent_log_ratio`` launch on torch's current stream (non-GPU tensors: ``reference_ratio``): fp32, of the inputs'
        leading shape.  ``accumulate`` adds onto ``out`` (in double, rounded once) instead of overwriting it."""
        rows = LikelihoodBound._checked_ratio(post_logits, prior_logits, stoch, cats, classes)
        lead = tuple(post_logits.shape[:-1])
        if accumulate and out is None:
            msg = "accumulate needs the out buffer it adds onto"
            raise ValueError(msg)
        if out is None:
            out = torch.empty(lead, device=post_logits.device, dtype=torch.float32)
        if tuple(out.shape) != lead or out.dtype != torch.float32 or not out.is_contiguous() or out.device != post_logits.device:
            msg = f"out must be a contiguous float32 {lead} buffer on {post_logits.device}, got {out.dtype} {tuple(out.shape)} on {out.device}"
            raise ValueError(msg)
        if not post_logits.is_cuda:
            got = LikelihoodBound.reference_ratio(post_logits, prior_logits, stoch, cats, classes)
            out.copy_((out.to(torch.float64) + got if accumulate else got).to(torch.float32))
            return out
        post_logits, prior_logits, stoch = post_logits.contiguous(), prior_logits.contiguous(), stoch.contiguous()
        _lib.check(_lib.TIMERS.call("mtrssm_latent_log_ratio", _lib.load().mtrssm_latent_log_ratio, _lib.ptr(post_logits), _lib.ptr(prior_logits),
                                    _lib.ptr(stoch), rows, cats, classes, int(accumulate), _lib.ptr(out), _lib.stream_ptr(out.device),
                                    nbytes=12.0 * rows * cats * classes), "mtrssm_latent_log_ratio")
        return out

    @staticmethod
    def bound(se_audio: Tensor | None, se_vision: Tensor | None, log_ratio: Tensor | None, valid: Tensor | None = None,  # noqa: PLR0913
              event_audio: int = 0, event_vision: int = 0, *, out: Tensor | None = None) -> Tensor:
        """One ``mtrssm_iw_bound`` launch on torch's current stream (non-GPU tensors: ``reference``): the eight planes, fp32
        ``[8, B, T]`` (``out``: the buffer they are written to)."""
        b, s, t = LikelihoodBound._checked_bound(se_audio, se_vision, log_ratio, valid, event_audio, event_vision)
        ref = next(x for x in (se_audio, se_vision, log_ratio) if x is not None)
        if out is None:
            out = torch.empty(len(PLANES), b, t, device=ref.device, dtype=torch.float32)
        if tuple(out.shape) != (len(PLANES), b, t) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != ref.device:
            msg = f"out must be a contiguous float32 [{len(PLANES)}, {b}, {t}] buffer on {ref.device}, got {out.dtype} {tuple(out.shape)}"
            raise ValueError(msg)
        if not ref.is_cuda:
            out.copy_(LikelihoodBound.reference(se_audio, se_vision, log_ratio, valid, event_audio, event_vision).to(torch.float32))
            return out
        se_audio, se_vision, log_ratio, valid = (None if x is None else x.contiguous() for x in (se_audio, se_vision, log_ratio, valid))
        _lib.check(_lib.TIMERS.call("mtrssm_iw_bound", _lib.load().mtrssm_iw_bound, _lib.ptr(se_audio), _lib.ptr(se_vision), _lib.ptr(log_ratio),
                                    _lib.index_ptr(valid), b, s, t, int(event_audio), int(event_vision), _lib.ptr(out), _lib.stream_ptr(ref.device),
                                    nbytes=4.0 * b * t * (3 * s + len(PLANES))), "mtrssm_iw_bound")
        return out


class LikelihoodTable(PlaneTable):
    """The accumulated bound of any number of likelihood steps in ONE fp32 buffer ``[6 + 1, T]``: the planes ``TABLE_ROWS`` (iw, elbo,
    audio, vision, latent, ess) summed by frame position, then the counts of live frames."""

    ROWS = len(TABLE_ROWS)

    def fold(self, planes: Tensor, valid: Tensor | None = None) -> LikelihoodTable:
        """Adds a step's planes (``[8, B, T]`` or their first six) by frame position: ``mtrssm_horizon_table`` with ``context = 1``, whose
        bin ``h`` is then the frame ``t``."""
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
        """Each plane's summed row over the summed counts: nats per live frame (``ess``: its mean); NaN for an empty table."""
        total = self.counts.sum()
        return {name: self._mean(row.sum(), total) for name, row in zip(TABLE_ROWS, self.sums, strict=True)}

    def scalars(self, prefix: str) -> dict[str, Tensor]:
        """``prefix/{iw,elbo,audio,vision,latent,ess,gap}``: ``per_frame`` as a flat dict, ``gap = iw - elbo`` (>= 0 up to rounding)."""
        per = self.per_frame()
        out = {f"{prefix}/{name}": value for name, value in per.items()}
        out[f"{prefix}/gap"] = per["iw"] - per["elbo"]
        return out


__all__ = ["PLANES", "TABLE_ROWS", "LikelihoodBound", "LikelihoodTable"]
