"""``MoPoE_MRSSM`` / ``MoPoE_MMTRSSM`` with the reference's Python surface, on HIP kernels.

Drop-in for ``multimodal_rssm.models.mrssm.mopoe_mrssm.MoPoE_MRSSM``
(``mrssm/mopoe_mrssm/core.py:12-355`` over ``models/core.py:13-266``) and
``multimodal_rssm.models.mmtrssm.mopoe_mmtrssm.MoPoE_MMTRSSM`` (``mmtrssm/mopoe_mmtrssm/core.py:77-610``):
same kwargs-only constructors, method names, loss-dict keys, state-dict names, ``TypeError`` when
``observations`` is not a tuple.  A YAML ``class_path`` can name these classes directly
(INTEGRATION.md).

What differs underneath: the T loop is one persistent HIP launch (``scan.py``); encoders and decoders
see all B*T frames as one batch; the KL term comes out of the scan kernel; the encoder runs once per
``shared_step`` (the reference encodes frame 0 twice, ``core.py:132`` and ``mrssm core.py:215-216`` -- same
values, and the gradient of both uses is accumulated).  Sampling noise is explicit: every rollout
takes an optional ``noise`` dict of uniforms and draws ``torch.rand`` on the device otherwise.
"""

from __future__ import annotations

import torch
from torch import Tensor, nn

from multimodal_mtrssm_amd import cnn, conv, scan
from multimodal_mtrssm_amd._shared import _check_lengths, _masked_mean_embed, _pairable, _rand
from multimodal_mtrssm_amd.carry import StateCarry
from multimodal_mtrssm_amd.census import CensusTable, LatentCensus
from multimodal_mtrssm_amd.digits import DigitClassifier
from multimodal_mtrssm_amd.frechet import FrechetDistance, FrechetTable
from multimodal_mtrssm_amd.distributions import MultiOneHot, MultiOneHotFactory, check_unimix, draw_uniforms, kl_divergence, onehot_from_uniforms
from multimodal_mtrssm_amd.dropout import ModalityDropout, StepMask, ragged_step_mask
from multimodal_mtrssm_amd.evaluation import _Evaluators
from multimodal_mtrssm_amd.experts import ExpertWeights
from multimodal_mtrssm_amd.forecast import Forecast
from multimodal_mtrssm_amd.overshoot import LatentOvershoot, OvershootTable, OvershootTerms
from multimodal_mtrssm_amd.likelihood import LikelihoodBound, LikelihoodTable
from multimodal_mtrssm_amd.networks import MTRNN, Representation, Transition
from multimodal_mtrssm_amd.objective import likelihood
from multimodal_mtrssm_amd.particle import ParticleFilter, ParticleTable
from multimodal_mtrssm_amd.schedule import ElboSchedule, ElboTerms
from multimodal_mtrssm_amd.skill import ForecastSkill, SkillTable
from multimodal_mtrssm_amd.state import MTState, State

try:  # the real trainer, when it is installed next to the reference
    from lightning import LightningModule as _Base
except ImportError:  # this image: a LightningModule-shaped nn.Module

    class _Base(nn.Module):  # type: ignore[no-redef]
        @property
        def device(self) -> torch.device:
            for p in self.parameters():
                return p.device
            return torch.device("cpu")

        def log_dict(self, *args, **kwargs) -> None:  # noqa: ANN002, ANN003
            return None


Noise = dict[str, Tensor | None]

def _st_onehot(dist: MultiOneHot, u: Tensor | None) -> Tensor:
    """Straight-through one-hot sample of ``dist`` from uniforms ``u`` (drawn on device when None)."""
    if u is None:
        return dist.rsample()
    onehot = onehot_from_uniforms(dist.probs.detach(), u.to(dist.probs))
    return (onehot + (dist.probs - dist.probs.detach())).flatten(start_dim=-2)


class _CategoricalHead(torch.autograd.Function):
    """Initial-state categorical head in ONE launch (``mtrssm_categorical_sample_fwd``): flat logits + uniforms ->
    (straight-through sample, log-probabilities, probabilities).  Same values as ``factory(logits)`` + ``_st_onehot`` -- a dozen
    eager launches per level --, same gradients: the sample's gradient flows into the probabilities (``onehot + p - p.detach()``)."""

    @staticmethod
    def forward(ctx, logits: Tensor, u: Tensor, cats: int, classes: int):  # noqa: ANN001, ANN205
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

        ctx.set_materialize_grads(False)
        logits, u = logits.contiguous().float(), u.contiguous().float()
        rows = logits.numel() // (cats * classes)
        logp = torch.empty(*logits.shape[:-1], cats, classes, device=logits.device, dtype=torch.float32)
        probs, onehot = torch.empty_like(logp), torch.empty_like(logits)
        _lib.check(_lib.load().mtrssm_categorical_sample_fwd(_lib.ptr(logits), _lib.ptr(u), rows, cats, classes, _lib.ptr(logp), _lib.ptr(probs),
                                                             _lib.ptr(onehot), _lib.stream_ptr(logits.device)), "mtrssm_categorical_sample_fwd")
        ctx.save_for_backward(probs)
        ctx.dims = (rows, cats, classes)
        return onehot, logp, probs

    @staticmethod
    def backward(ctx, g_stoch, g_logp, g_probs):  # noqa: ANN001, ANN205
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

        (probs,) = ctx.saved_tensors
        rows, cats, classes = ctx.dims
        gp = None
        if g_stoch is not None:
            gp = g_stoch.reshape(probs.shape)
        if g_probs is not None:
            gp = g_probs if gp is None else gp + g_probs
        if gp is None and g_logp is None:
            return None, None, None, None
        gp = None if gp is None else gp.contiguous().float()
        gl = None if g_logp is None else g_logp.contiguous().float()
        d = torch.empty(*probs.shape[:-2], cats * classes, device=probs.device, dtype=torch.float32)
        _lib.check(_lib.load().mtrssm_categorical_sample_bwd(_lib.ptr(probs), _lib.ptr(gp), _lib.ptr(gl), rows, cats, classes, _lib.ptr(d),
                                                             _lib.stream_ptr(probs.device)), "mtrssm_categorical_sample_bwd")
        return d, None, None, None


FUSED_INITIAL_STATE = True  # False: the initial state layer by layer (A/B runs, tests)


def _initial_state_problem(ea, ev, mask0, u, params, acts, depths, cats: int, classes: int):  # noqa: ANN001, ANN202, PLR0913
    """The ``MtrssmInitialState`` of one call with its extents, strides, activations and depths set and every pointer NULL
    (``_InitialState`` fills them in), or None where an operand is not what the kernels take (then the layer-by-layer path
    runs).  ``u`` may be None: whether the kernels apply is decided BEFORE the uniforms are drawn, so that a refused call leaves
    the draw to the path that runs.  ``params``: init_proj.0 / .2 and prior head .0 / .2 weights and biases; the embeddings are
    ``[B, E]`` views (frame 0 of ``[B, T, E]``: read in place through their row stride)."""
    from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

    ref = ea if ea is not None else ev
    if ref is None or any(p is None for p in params) or any(a is None for a in acts):
        return None
    tensors = [t for t in (ea, ev, u, *params) if t is not None]
    if not all(t.is_cuda and t.dtype == torch.float32 for t in tensors) or ref.dim() != 2 or any(t.stride(-1) != 1 for t in tensors):  # noqa: PLR2004
        return None
    if any(e is not None and (e.shape != ref.shape or (e.shape[0] > 1 and e.stride(0) < e.shape[1])) for e in (ea, ev)):
        return None
    if mask0 is not None and (mask0.dtype != torch.bool or tuple(mask0.shape) != (ref.shape[0], 2) or not mask0.is_contiguous()):
        return None
    wi1, bi1, wi2, bi2, wp1, bp1, wp2, bp2 = params
    B, E = ref.shape
    cells, D, H, S = wi1.shape[0], wi2.shape[0], wp1.shape[0], wp2.shape[0]
    if (wi1.shape[1], wi2.shape[1], wp1.shape[1], wp2.shape[1], S) != (E, cells, D, H, cats * classes):
        return None
    if u is not None and (tuple(u.shape) != (B, cats) or not u.is_contiguous()):
        return None
    if any(b.shape != (w.shape[0],) or not b.is_contiguous() for w, b in ((wi1, bi1), (wi2, bi2), (wp1, bp1), (wp2, bp2))):
        return None
    p = _lib.InitialState()
    p.ea_stride = 0 if ea is None else max(int(ea.stride(0)), E)
    p.ev_stride = 0 if ev is None else max(int(ev.stride(0)), E)
    p.ld_wi1, p.ld_wi2, p.ld_wp1, p.ld_wp2 = (max(int(w.stride(0)), w.shape[1]) for w in (wi1, wi2, wp1, wp2))
    p.B, p.E, p.cells, p.D, p.H, p.K, p.C = B, E, cells, D, H, cats, classes
    p.act_i, p.act_p = acts
    p.depth_i, p.depth_p = depths
    if not _lib.load().mtrssm_initial_state_supported(p):
        return None
    return p


class _InitialState(torch.autograd.Function):
    """The whole initial state -- masked mean of the frame-0 embeddings, ``init_proj``, the prior head, the categorical head --
    in ONE launch each way (``mtrssm_initial_state_fwd`` / ``_bwd``, csrc/init_state.hip).  Same values as the layer-by-layer
    path (``MLP.forward`` + ``_CategoricalHead``) up to the order of the fp32 sums.  The weight and bias gradients stay GEMMs on
    the pre-activation gradients the backward kernel leaves behind: ``linear.weight_grad``, straight into the flat gradient
    buffer and deferred to the end of the pass like every other Linear's.  ``problem``: ``_initial_state_problem``'s struct for
    exactly these operands (its bytes are kept; every tensor the backward reads goes through ``save_for_backward``; the
    embeddings are not among them: the backward kernel only asks which of the two was given)."""

    @staticmethod
    def forward(ctx, problem, mask0, ea, ev, u, wi1, bi1, wi2, bi2, wp1, bp1, wp2, bp2):  # noqa: ANN001, ANN205, PLR0913
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

        ctx.set_materialize_grads(False)
        params = (wi1, bi1, wi2, bi2, wp1, bp1, wp2, bp2)
        p = type(problem).from_buffer_copy(problem)
        new = lambda *shape: torch.empty(shape, device=u.device, dtype=torch.float32)  # noqa: E731
        e, z1, deter0, zp = new(p.B, p.E), new(p.B, p.cells), new(p.B, p.D), new(p.B, p.H)
        logp, probs, stoch = new(p.B, p.K, p.C), new(p.B, p.K, p.C), new(p.B, p.K * p.C)
        p.ea, p.ev, p.mask0, p.u = _lib.raw_ptr(ea), _lib.raw_ptr(ev), _lib.raw_ptr(mask0), _lib.ptr(u)
        p.wi1, p.bi1, p.wi2, p.bi2, p.wp1, p.bp1, p.wp2, p.bp2 = map(_lib.raw_ptr, params)
        p.e, p.z1, p.deter0, p.zp, p.logp, p.probs, p.stoch = map(_lib.ptr, (e, z1, deter0, zp, logp, probs, stoch))
        _lib.check(_lib.TIMERS.call("mtrssm_initial_state_fwd", _lib.load().mtrssm_initial_state_fwd, p, _lib.stream_ptr(u.device)),
                   "mtrssm_initial_state_fwd")
        ctx.plan, ctx.given, ctx.has_mask = bytes(problem), (ea is not None, ev is not None), mask0 is not None
        saved = (e, z1, deter0, zp, probs, *params) + ((mask0,) if mask0 is not None else ())
        ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(e)
        return deter0, stoch, logp, probs, e

    @staticmethod
    def backward(ctx, g_deter0, g_stoch, g_logp, g_probs, _g_e):  # noqa: ANN001, ANN205
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415
        from multimodal_mtrssm_amd.linear import weight_grad  # noqa: PLC0415

        if g_deter0 is None and g_stoch is None and g_logp is None and g_probs is None:
            return (None,) * 13
        e, z1, deter0, zp, probs, *rest = ctx.saved_tensors
        params, mask0 = rest[:8], (rest[8] if ctx.has_mask else None)
        p = _lib.InitialState.from_buffer_copy(ctx.plan)
        new = lambda *shape: torch.empty(shape, device=e.device, dtype=torch.float32)  # noqa: E731
        gs = [None if g is None else g.contiguous().float() for g in (g_deter0, g_stoch, g_logp, g_probs)]
        d_logits, d_zp, g_deter, d_z1 = new(p.B, p.K * p.C), new(p.B, p.H), new(p.B, p.D), new(p.B, p.cells)
        g_ea = new(p.B, p.E) if ctx.needs_input_grad[2] else None
        g_ev = new(p.B, p.E) if ctx.needs_input_grad[3] else None
        # (the backward kernel reads of ea / ev only whether each was given: the mean embedding stands in for the pointer)
        p.ea, p.ev = (_lib.ptr(e) if given else None for given in ctx.given)
        p.ea_stride, p.ev_stride = (p.E if given else 0 for given in ctx.given)
        p.mask0 = _lib.raw_ptr(mask0)
        p.wi1, p.bi1, p.wi2, p.bi2, p.wp1, p.bp1, p.wp2, p.bp2 = map(_lib.raw_ptr, params)
        p.z1, p.zp, p.probs = _lib.ptr(z1), _lib.ptr(zp), _lib.ptr(probs)
        p.g_deter0, p.g_stoch0, p.g_logp, p.g_probs = map(_lib.ptr, gs)
        p.d_logits, p.d_zp, p.g_deter, p.d_z1, p.g_ea, p.g_ev = map(_lib.ptr, (d_logits, d_zp, g_deter, d_z1, g_ea, g_ev))
        _lib.check(_lib.TIMERS.call("mtrssm_initial_state_bwd", _lib.load().mtrssm_initial_state_bwd, p, _lib.stream_ptr(e.device)),
                   "mtrssm_initial_state_bwd")
        wi1, bi1, wi2, bi2, wp1, bp1, wp2, bp2 = params
        need = ctx.needs_input_grad
        grads = []
        for j, (gy, x, w, b, act) in enumerate(((d_z1, e, wi1, bi1, 0), (g_deter, z1, wi2, bi2, p.act_i), (d_zp, deter0, wp1, bp1, 0),
                                                (d_logits, zp, wp2, bp2, p.act_p))):
            grads += weight_grad(gy, x, w, b, act_x=act, want_weight=need[5 + 2 * j], want_bias=need[6 + 2 * j])
        return (None, None, g_ea, g_ev, None, *grads)


class _ElboEpilogue(torch.autograd.Function):
    """``recon = nll_a + nll_v; kl_j = coeff_j mean(kl_bt_j); loss = recon + sum kl_j`` in one launch each way instead of the eager
    add / mean / mul / add chain and its autograd nodes.  ``live`` / ``count`` given (ragged batches):
    ``kl_j = coeff_j sum(live kl_bt_j) / count``, ``live`` float ``[B * T]`` in {0, 1}, ``count`` a device scalar.  Without ``sched`` the
    result is ``(recon, k_0, k_1, loss)`` (``mtrssm_elbo_combine_fwd / _bwd`` or ``mtrssm_elbo_combine_counted_fwd / _bwd``).  Under an
    ``ElboSchedule`` (``mtrssm_elbo_schedule_fwd / _bwd``) it is ``(recon, k_0, k_1, loss, beta, stats)``, ``stats``
    float32 ``[4]`` = raw_0, raw_1, active_0, active_1; ``beta`` and ``stats`` carry no gradient and the backward reads the stored ``beta``."""

    @staticmethod
    def forward(ctx, nll_a: Tensor, nll_v: Tensor, kl0: Tensor, kl1: Tensor | None, live: Tensor | None, count: Tensor | None,  # noqa: ANN001, ANN205, PLR0913
                step: Tensor | None, sched: ElboSchedule | None, c0: float, c1: float):
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

        ctx.set_materialize_grads(False)
        nll_a, nll_v, kl0, kl1, live, count, step = (None if t is None else t.contiguous().float() for t in (nll_a, nll_v, kl0, kl1, live, count, step))
        n = kl0.numel()
        if (live is None) != (count is None):
            msg = "live and count come together (both None: every step is live)"
            raise ValueError(msg)
        if live is not None and (live.numel() != n or count.numel() != 1):
            msg = f"live must have one entry per KL step ({n}), count one; got {live.numel()} and {count.numel()}"
            raise ValueError(msg)
        if kl1 is not None and kl1.numel() != n:
            msg = f"the two KL planes must have the same number of steps, got {n} and {kl1.numel()}"
            raise ValueError(msg)
        if step is not None and step.numel() != 1:
            msg = f"step must be one device scalar, got {step.numel()} entries"
            raise ValueError(msg)
        lib, ptr, stream = _lib.load(), _lib.ptr, _lib.stream_ptr(kl0.device)
        outs = [torch.empty((), device=kl0.device, dtype=torch.float32) for _ in range(4 if sched is None else 5)]
        planes = (ptr(nll_a), ptr(nll_v), ptr(kl0), ptr(kl1))
        four = (ptr(outs[0]), ptr(outs[1]), ptr(outs[2]) if kl1 is not None else None, ptr(outs[3]))  # (no kl1: k_1 is left unwritten)
        par, extra = (float(c0), float(c1)), ()
        if sched is not None:
            par = _lib.ElboSchedule(float(c0), float(c1), sched.free_nats, sched.free_nats_h, sched.recon_weights[0], sched.recon_weights[1],
                                    sched.beta_start, float(sched.warmup_steps))
            stats = torch.empty(4, device=kl0.device, dtype=torch.float32)
            _lib.check(lib.mtrssm_elbo_schedule_fwd(*planes, ptr(live), ptr(count), ptr(step), n, par, *map(ptr, outs), ptr(stats), stream),
                       "mtrssm_elbo_schedule_fwd")
            ctx.save_for_backward(kl0, kl1, live, count, outs[4])
            ctx.mark_non_differentiable(outs[4], stats)
            extra = (stats,)
        elif live is not None:
            _lib.check(lib.mtrssm_elbo_combine_counted_fwd(*planes, ptr(live), ptr(count), n, *par, *four, stream), "mtrssm_elbo_combine_counted_fwd")
            ctx.save_for_backward(None, None, live, count, None)
        else:
            _lib.check(lib.mtrssm_elbo_combine_fwd(*planes, n, *par, *four, stream), "mtrssm_elbo_combine_fwd")
            ctx.save_for_backward(None, None, None, None, None)
        ctx.meta = (kl0.shape, None if kl1 is None else kl1.shape, n, par, sched is not None)
        ctx.dev = kl0.device
        return (*outs, *extra)

    @staticmethod
    def backward(ctx, g_recon, g_k0, g_k1, g_loss, *_g_beta_stats):  # noqa: ANN001, ANN002, ANN205
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415

        shape0, shape1, n, par, scheduled = ctx.meta
        kl0, kl1, live, count, beta = ctx.saved_tensors
        lib, ptr, stream = _lib.load(), _lib.ptr, _lib.stream_ptr(ctx.dev)
        g_a, g_v = (torch.empty((), device=ctx.dev, dtype=torch.float32) for _ in range(2))
        g_kl0 = torch.empty(shape0, device=ctx.dev, dtype=torch.float32)
        g_kl1 = None if shape1 is None else torch.empty(shape1, device=ctx.dev, dtype=torch.float32)
        opt = lambda t: None if t is None else ptr(t.contiguous().float())  # noqa: E731
        gs = (opt(g_recon), opt(g_k0), opt(g_k1) if shape1 is not None else None, opt(g_loss))
        grads = (ptr(g_a), ptr(g_v), ptr(g_kl0), ptr(g_kl1))
        if scheduled:
            _lib.check(lib.mtrssm_elbo_schedule_bwd(*gs, ptr(kl0), ptr(kl1), ptr(live), ptr(count), ptr(beta), n, par, *grads, stream),
                       "mtrssm_elbo_schedule_bwd")
        elif live is not None:
            _lib.check(lib.mtrssm_elbo_combine_counted_bwd(*gs, ptr(live), ptr(count), n, *par, *grads, stream), "mtrssm_elbo_combine_counted_bwd")
        else:
            _lib.check(lib.mtrssm_elbo_combine_bwd(*gs, n, *par, *grads, stream), "mtrssm_elbo_combine_bwd")
        return g_a, g_v, g_kl0, g_kl1, None, None, None, None, None, None


# The three call shapes of the epilogue (plain, counted, scheduled): every one is _ElboEpilogue.
_ElboScheduled = _ElboEpilogue


class _ElboCombineCounted:
    @staticmethod
    def apply(nll_a: Tensor, nll_v: Tensor, kl0: Tensor, kl1: Tensor | None, live: Tensor, count: Tensor, c0: float, c1: float):  # noqa: ANN205, PLR0913
        return _ElboEpilogue.apply(nll_a, nll_v, kl0, kl1, live, count, None, None, c0, c1)


class _ElboCombine:
    @staticmethod
    def apply(nll_a: Tensor, nll_v: Tensor, kl0: Tensor, kl1: Tensor | None, c0: float, c1: float):  # noqa: ANN205, PLR0913
        return _ElboEpilogue.apply(nll_a, nll_v, kl0, kl1, None, None, None, None, c0, c1)


def _elbo_scheduled(nll_a: Tensor, nll_v: Tensor, kl0: Tensor, c0: float, kl1: Tensor | None, c1: float, step_mask: StepMask | None,  # noqa: PLR0913
                    schedule: ElboSchedule) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``_elbo`` under ``schedule``: the new pair on the GPU, the rule in eager torch elsewhere; ``schedule.stats`` keeps the rest."""
    if not isinstance(schedule, ElboSchedule):
        msg = f"elbo_schedule must be an ElboSchedule, got {type(schedule).__name__}"
        raise ValueError(msg)
    live = count = None
    if step_mask is not None and step_mask.live is not None:
        live, count = step_mask.live, step_mask.count_live
    step = schedule.step_on(kl0.device)
    if kl0.is_cuda and nll_a.dim() == 0 and nll_v.dim() == 0:
        recon, k0, k1, loss, beta, stats = _ElboScheduled.apply(nll_a, nll_v, kl0, kl1, live, count, step, schedule, c0, c1)
        terms = ElboTerms(recon, k0, k1, loss, beta, stats[0], stats[1], stats[2], stats[3])
    else:
        terms = schedule.reference(nll_a, nll_v, kl0, c0, kl1, c1, live, count, step)
    schedule.record(terms, higher=kl1 is not None)
    return terms.recon, terms.k0, terms.k1, terms.loss


def _elbo(nll_a: Tensor, nll_v: Tensor, kl0: Tensor, c0: float, kl1: Tensor | None = None, c1: float = 0.0,  # noqa: PLR0913
          step_mask: StepMask | None = None, schedule: ElboSchedule | None = None) -> tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(recon, kl_0, kl_1, loss)``; on the GPU one fused launch, elsewhere the eager arithmetic of the reference.  A ``step_mask``
    that carries ``live`` (a ragged batch) takes the counted epilogue: the KL sums over live steps / ``count_live``.  With a
    ``schedule`` the terms are weighed by its rule: ``kl_j`` is the clipped, beta-weighted term, ``recon`` the
    weighted sum, and ``schedule.stats`` holds ``beta``, the active fractions and the unscheduled KL terms."""
    if schedule is not None:
        return _elbo_scheduled(nll_a, nll_v, kl0, c0, kl1, c1, step_mask, schedule)
    if step_mask is not None and step_mask.live is not None:
        if kl0.is_cuda and nll_a.dim() == 0 and nll_v.dim() == 0:
            return _ElboCombineCounted.apply(nll_a, nll_v, kl0, kl1, step_mask.live, step_mask.count_live, c0, c1)
        live, count = step_mask.live.reshape(kl0.shape).to(kl0), step_mask.count_live.to(kl0)  # the same rule in eager arithmetic
        zero = torch.zeros((), device=kl0.device)
        recon = nll_a + nll_v
        k0 = torch.where(count > 0, (kl0 * live).sum() / count * c0, zero)
        k1 = torch.where(count > 0, (kl1 * live).sum() / count * c1, zero) if kl1 is not None else zero
        return recon, k0, k1, recon + k0 + (k1 if kl1 is not None else 0.0)
    if kl0.is_cuda and nll_a.dim() == 0 and nll_v.dim() == 0:
        return _ElboCombine.apply(nll_a, nll_v, kl0, kl1, c0, c1)
    recon = nll_a + nll_v
    k0 = kl0.mean().mul(c0)
    k1 = kl1.mean().mul(c1) if kl1 is not None else torch.zeros((), device=kl0.device)
    return recon, k0, k1, recon + k0 + (k1 if kl1 is not None else 0.0)


def _sampled_head(factory, logits: Tensor, u: Tensor | None) -> tuple[MultiOneHot, Tensor]:  # noqa: ANN001
    """``(factory(logits), straight-through sample)``: one fused launch on the GPU when the uniforms are given."""
    if not logits.is_cuda:
        dist = factory.unmixed(logits)  # (the initial state's head: never uniform-mixed)
        return dist, _st_onehot(dist, u)
    if u is None:  # (the draw MultiOneHot.rsample would make: injected noise tape or the device generator)
        u = draw_uniforms((*logits.shape[:-1], factory.category_size), logits)
    stoch, logp, probs = _CategoricalHead.apply(logits, u.to(logits), factory.category_size, factory.class_size)
    return MultiOneHot(logp, probs), stoch


def _check_modality_mask(mask: Tensor, B: int, T: int | None, device: torch.device, *, first_step: bool) -> None:  # noqa: N803
    """Host-side checks of a modality mask (DESIGN.md "Missing modalities"): bool ``[B, T, 2]`` (``[B, 2]`` when ``T`` is
    None) on ``device``; ``first_step``: every row observes something at t = 0 (the initial state averages those embeddings)."""
    shape = (B, 2) if T is None else (B, T, 2)
    if not isinstance(mask, Tensor) or mask.dtype != torch.bool:
        msg = f"modality_mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask))}"
        raise ValueError(msg)
    if tuple(mask.shape) != shape:
        msg = f"modality_mask must have shape {shape} (ordered audio, vision), got {tuple(mask.shape)}"
        raise ValueError(msg)
    if mask.device != torch.device(device):
        msg = f"modality_mask is on {mask.device}, the model's tensors on {device}"
        raise ValueError(msg)
    if first_step:
        m0 = mask if T is None else mask[:, 0]
        if not bool(m0.any(dim=-1).all()):
            msg = "modality_mask: every row must observe at least one modality at t = 0 (the initial state needs an embedding)"
            raise ValueError(msg)


def _absent_mask(observations: tuple, B: int, T: int, device: torch.device) -> Tensor:  # noqa: N803
    """The mask an observation tuple with ``None`` entries stands for: a None modality is absent at every step."""
    present = torch.tensor([observations[0] is not None, observations[1] is not None], device=device)
    return present.expand(B, T, 2)


def _resolve_modality_mask(observations: tuple, mask: Tensor | None, B: int, T: int, device: torch.device) -> Tensor | None:  # noqa: N803
    """Validated mask of a rollout (None: both modalities everywhere, the unmasked kernels).  A None observation must be
    masked out at every step."""
    if observations[0] is None and observations[1] is None:
        msg = "observations: at least one of (audio_obs, vision_obs) must be given"
        raise ValueError(msg)
    if mask is None:
        if observations[0] is None or observations[1] is None:
            return _absent_mask(observations, B, T, device)
        return None
    _check_modality_mask(mask, B, T, device, first_step=False)
    for j, name in enumerate(("audio", "vision")):
        if observations[j] is None and bool(mask[..., j].any()):
            msg = f"modality_mask marks {name} present, but observations carries None for it"
            raise ValueError(msg)
    return mask


def check_ragged_rows(valid_host: Tensor, reset_host: Tensor | None) -> None:
    """The host rule of a ragged step: a row that resets needs a frame at t = 0 -- ``reset_host[b]`` implies
    ``valid_host[b] >= 1`` (``reset_host`` None: every row resets).  Raises before anything is launched."""
    empty = valid_host.to("cpu") < 1
    if reset_host is not None:
        if tuple(reset_host.shape) != tuple(valid_host.shape):
            msg = f"reset {tuple(reset_host.shape)} and valid {tuple(valid_host.shape)} do not match"
            raise ValueError(msg)
        empty = empty & reset_host.to("cpu", torch.bool)
    if bool(empty.any()):
        msg = (f"rows {empty.nonzero().flatten().tolist()} start an episode (reset) with no valid frame: a row may have nothing at "
               "t = 0 only when it continues from the carry")
        raise ValueError(msg)


class MoPoE_MRSSM(_Evaluators, _Base):  # noqa: N801
    """Multimodal RSSM with MoPoE posteriors: PoE of {audio, vision}, then MoE over {A, V, A+V}."""

    def __setattr__(self, name: str, value: object) -> None:
        if name == "frechet_classifier":  # an evaluation tool, not a part of the model: no submodule, no state-dict keys
            object.__setattr__(self, name, value)
            return
        super().__setattr__(name, value)

    def __init__(  # noqa: PLR0913
        self,
        *,
        audio_representation: Representation,
        vision_representation: Representation,
        transition: Transition,
        audio_encoder: nn.Module,
        vision_encoder: nn.Module,
        audio_decoder: nn.Module,
        vision_decoder: nn.Module,
        init_proj: nn.Module,
        kl_coeff: float,
        use_kl_balancing: bool,
        unimix: float = 0.0,
    ) -> None:
        super().__init__()
        # registration order and the double registration of the audio head follow the reference
        # (core.py:27-29, mrssm core.py:55-60): checkpoints carry both `representation.*` and `audio_representation.*`
        self.representation = audio_representation
        self.transition = transition
        self.init_proj = init_proj
        self.kl_coeff = kl_coeff
        self.use_kl_balancing = use_kl_balancing
        self.audio_representation = audio_representation
        self.vision_representation = vision_representation
        self.audio_encoder = audio_encoder
        self.vision_encoder = vision_encoder
        self.audio_decoder = audio_decoder
        self.vision_decoder = vision_decoder
        self.scan_rows_per_block = 0  # 0 = library default (tuning knobs)
        self.scan_threads = 0
        self.modality_dropout: ModalityDropout | None = None  # training_step samples a modality mask with it
        self.state_carry: StateCarry | None = None  # training_step / validation_step continue from its "train" / "val" set
        self.forecast: Forecast | None = None  # training_step trains the forecast objective with it
        self.val_forecast: Forecast | None = None  # validation_step adds a forecast step at this (fixed) context and logs val/forecast/*
        self.elbo_schedule: ElboSchedule | None = None  # training_step (never validation_step) weighs the loss terms with it
        self.val_skill: ForecastSkill | None = None  # validation_step adds a skill step into self.skill_table
        self.skill_table: SkillTable | None = None  # ... logged as val/skill/* and cleared by on_validation_epoch_end
        self.val_likelihood: LikelihoodBound | None = None  # validation_step adds a likelihood step into self.likelihood_table
        self.likelihood_table: LikelihoodTable | None = None  # ... logged as val/loglik/* and cleared by on_validation_epoch_end
        self.val_particle: ParticleFilter | None = None  # validation_step adds a particle-filter step into self.particle_table
        self.particle_table: ParticleTable | None = None  # ... logged as val/smc/* and cleared by on_validation_epoch_end
        self.overshoot: LatentOvershoot | None = None  # training_step adds the latent-overshooting term with it
        self.val_overshoot: LatentOvershoot | None = None  # validation_step adds an overshoot pass into self.overshoot_table
        self.overshoot_table: OvershootTable | None = None  # ... logged as val/overshoot/* and cleared by on_validation_epoch_end
        self._overshoot_terms_last: list[OvershootTerms] | None = None  # the last overshoot step's terms per level (detached use only)
        self.val_census: LatentCensus | None = None  # validation_step adds a census step into self.census_table
        self.census_table: CensusTable | None = None  # ... logged as val/latent/* and cleared by on_validation_epoch_end
        self.val_frechet: FrechetDistance | None = None  # validation_step adds a Frechet step into self.frechet_table
        self.frechet_table: FrechetTable | None = None  # ... logged as val/frechet/* and cleared by on_validation_epoch_end
        self.frechet_classifier: DigitClassifier | None = None  # the reader of val_frechet's features="reader" (not a submodule)
        # weighted MoPoE: assign an ExpertWeights (a submodule: before FlatParameters is built); None = 1/3 each, no new
        # state-dict keys.  After every posterior rollout with weights, weights_timeseries is ExpertWeights.table(...) [B, T, 3]
        self.expert_weights: ExpertWeights | None = None
        self.weights_timeseries: Tensor | None = None
        self._weights_both: Tensor | None = None  # bool [B, T]: where weights_timeseries belongs to a step with both modalities
        self.unimix = unimix  # uniform mixing of every categorical the scans form; config, not checkpoint

    def _distribution_factories(self) -> list[MultiOneHotFactory]:
        owned = [self.transition.distribution_factory, self.audio_representation.distribution_factory,
                 self.vision_representation.distribution_factory]
        return owned + [f for f in (getattr(self, "l_dist", None), getattr(self, "h_dist", None)) if f is not None]

    @property
    def unimix(self) -> float:
        """eps of the uniform mixing ``(1 - eps) softmax + eps / C`` of every prior and posterior categorical:
        one value on every distribution factory the model owns; 0 = off.  No parameter, buffer or state-dict key."""
        return scan.unimix_of(*self._distribution_factories())

    @unimix.setter
    def unimix(self, value: float) -> None:
        eps = check_unimix(value)
        for factory in self._distribution_factories():
            factory.unimix = eps

    # -- batch accessors (mrssm core.py:310-355) --------------------------------------------
    @staticmethod
    def get_observations_from_batch(batch: tuple[Tensor, ...]) -> tuple[Tensor, Tensor]:
        return batch[1], batch[2]

    @staticmethod
    def get_initial_observation(observations: tuple[Tensor, Tensor]) -> tuple[Tensor, Tensor]:
        audio_obs, vision_obs = observations
        return audio_obs[:, 0], vision_obs[:, 0]

    @staticmethod
    def get_targets_from_batch(batch: tuple[Tensor, ...]) -> dict[str, Tensor]:
        return {"recon/audio": batch[4], "recon/vision": batch[5]}

    @staticmethod
    def get_modality_mask_from_batch(batch: tuple[Tensor, ...]) -> Tensor | None:
        """The optional 7th batch entry: bool ``[B, T, 2]`` (audio, vision), True = observed.  None for the reference's
        6-tuple (both modalities everywhere)."""
        return batch[6] if len(batch) > 6 else None  # noqa: PLR2004

    # -- encoders / decoders / losses ---------------------------------------------------------
    def encode_observation(self, observation: tuple[Tensor, Tensor] | Tensor, modality_mask: Tensor | None = None) -> Tensor:
        """Fused t = 0 embedding: the mean of the present modalities' embeddings (``modality_mask``: bool ``[B, 2]``; a None
        entry of the tuple is absent for every row and its encoder is not run)."""
        if isinstance(observation, tuple):
            audio_obs, vision_obs = observation
            ea = None if audio_obs is None else self.audio_encoder(audio_obs)
            ev = None if vision_obs is None else self.vision_encoder(vision_obs)
            if ea is None and ev is None:
                msg = "observation: at least one of (audio_obs, vision_obs) must be given"
                raise ValueError(msg)
            return _masked_mean_embed(ea, ev, modality_mask)
        return observation

    def decode_state(self, state: State | MTState) -> dict[str, Tensor]:
        return {"recon/audio": self.audio_decoder(state.feature), "recon/vision": self.vision_decoder(state.feature)}

    @staticmethod
    def compute_reconstruction_loss(reconstructions: dict[str, Tensor], targets: dict[str, Tensor],
                                    modality_mask: Tensor | None = None) -> dict[str, Tensor]:
        """``mrssm core.py:279-308``.  ``modality_mask`` (bool ``[B, T, 2]``): each modality's NLL averages over the frames
        where it is present (0 where it is present nowhere)."""
        fa = fv = None
        if modality_mask is not None:
            fa, fv = modality_mask[..., 0], modality_mask[..., 1]
        audio = likelihood(prediction=reconstructions["recon/audio"], target=targets["recon/audio"], event_ndims=3, frame_mask=fa)
        vision = likelihood(prediction=reconstructions["recon/vision"], target=targets["recon/vision"], event_ndims=3, frame_mask=fv)
        return {"recon": audio + vision, "recon/audio": audio, "recon/vision": vision}

    def _encode_both(self, audio_obs: Tensor, vision_obs: Tensor) -> tuple[Tensor, Tensor]:
        """Both encoders over all B*T frames; equal-shaped residual blocks of the two stacks share launches."""
        if _pairable(self.audio_encoder, self.vision_encoder, cnn.Encoder):
            return cnn.encode_pair(self.audio_encoder, self.vision_encoder, audio_obs, vision_obs)
        return self.audio_encoder(audio_obs), self.vision_encoder(vision_obs)

    def _reconstruction_losses(self, feature: Tensor, targets: dict[str, Tensor], *, sum_recon: bool = True,
                               modality_mask: Tensor | None = None, step_mask: StepMask | None = None) -> dict[str, Tensor]:
        """``decode_state`` + ``compute_reconstruction_loss`` (``mrssm core.py:262-308``).  With this package's decoders the
        out_activation (Tanh) is applied inside the NLL kernels: the activated reconstructions are never written in training."""
        da, dv = self.audio_decoder, self.vision_decoder
        fused = isinstance(da, cnn.Decoder) and isinstance(dv, cnn.Decoder) and da.out_act_id is not None and dv.out_act_id is not None
        if fused and _pairable(da, dv, cnn.Decoder):
            pa, pv = cnn.decode_pair(da, dv, feature, feature, raw=True)
        elif fused:
            pa, pv = da(feature, raw=True), dv(feature, raw=True)
        else:
            pa, pv = da(feature), dv(feature)
        fa = fv = ca = cv = None
        if modality_mask is not None:
            fa, fv = modality_mask[..., 0], modality_mask[..., 1]
        if step_mask is not None:  # (the planes and counts exist already: nothing is derived from a bool mask here)
            ca, cv = (step_mask.present_audio, step_mask.count_audio), (step_mask.present_vision, step_mask.count_vision)
        audio = likelihood(prediction=pa, target=targets["recon/audio"], event_ndims=3, out_act=da.out_act_id if fused else 0,
                           frame_mask=fa, frame_present=ca)
        vision = likelihood(prediction=pv, target=targets["recon/vision"], event_ndims=3, out_act=dv.out_act_id if fused else 0,
                            frame_mask=fv, frame_present=cv)
        if not sum_recon:  # (shared_step adds them in its fused scalar epilogue)
            return {"recon/audio": audio, "recon/vision": vision}
        return {"recon": audio + vision, "recon/audio": audio, "recon/vision": vision}

    # -- states ---------------------------------------------------------------------------------
    def _initial_fused(self, ea: Tensor | None, ev: Tensor | None, mask0: Tensor | None, u_init: Tensor | None) -> State | None:
        """The initial state of the mean embedding of (``ea``, ``ev``) -- ``[B, E]`` each, one may be None -- in one launch
        (``_InitialState``), or None where the kernels do not apply (then the caller runs the layer-by-layer path)."""
        from multimodal_mtrssm_amd import _lib  # noqa: PLC0415
        from multimodal_mtrssm_amd.networks import MLP  # noqa: PLC0415

        proj, head = self.init_proj, self.transition.rnn_to_prior_projector
        ref = ea if ea is not None else ev
        if not FUSED_INITIAL_STATE or ref is None or not ref.is_cuda or not isinstance(proj, MLP) or not isinstance(head, MLP):
            return None
        if len(proj) != 3 or len(head) != 3 or proj.activate_last_layer or head.activate_last_layer:  # noqa: PLR2004
            return None
        factory = self.representation.distribution_factory
        params = (proj[0].weight, proj[0].bias, proj[2].weight, proj[2].bias, head[0].weight, head[0].bias, head[2].weight, head[2].bias)
        acts = (_lib.ACT_IDS.get(proj.activation_name), _lib.ACT_IDS.get(head.activation_name))
        u = None if u_init is None else u_init.to(ref).contiguous()
        problem = _initial_state_problem(ea, ev, mask0, u, params, acts, (proj.depth, head.depth), factory.category_size, factory.class_size)
        if problem is None:
            return None  # (nothing has been drawn: the layer-by-layer path makes its own draw)
        if u is None:  # (the draw MultiOneHot.rsample would make: injected noise tape or the device generator)
            u = draw_uniforms((ref.shape[0], factory.category_size), ref).contiguous()
        deter, stoch, logp, probs, _ = _InitialState.apply(problem, mask0, ea, ev, u, *params)
        return State(deter=deter, distribution=MultiOneHot(logp, probs), stoch=stoch)

    def _initial_from_embed(self, obs_embed: Tensor, u_init: Tensor | None) -> State:
        fused = self._initial_fused(obs_embed, None, None, u_init) if obs_embed.dim() == 2 else None  # noqa: PLR2004
        if fused is not None:
            return fused
        deter = self.init_proj(obs_embed)
        logits = self.transition.rnn_to_prior_projector(deter)
        dist, stoch = _sampled_head(self.representation.distribution_factory, logits, u_init)
        return State(deter=deter, distribution=dist, stoch=stoch)

    def _initial_embed(self, observation: tuple[Tensor, Tensor] | Tensor, modality_mask: Tensor | None) -> Tensor:
        if modality_mask is not None:
            if not isinstance(observation, tuple):
                msg = "modality_mask needs the (audio_obs, vision_obs) tuple"
                raise ValueError(msg)
            ref = observation[0] if observation[0] is not None else observation[1]
            _check_modality_mask(modality_mask, ref.shape[0], None, ref.device, first_step=True)
            for j, name in enumerate(("audio", "vision")):
                if observation[j] is None and bool(modality_mask[:, j].any()):
                    msg = f"modality_mask marks {name} present, but the observation carries None for it"
                    raise ValueError(msg)
        return self.encode_observation(observation, modality_mask)

    def initial_state(self, observation: tuple[Tensor, Tensor] | Tensor, noise: Noise | None = None,
                      modality_mask: Tensor | None = None) -> State:
        """``core.py:121-135``: fused embedding -> ``init_proj`` -> prior head -> sampled State.  ``modality_mask``: bool
        ``[B, 2]`` (audio, vision) of the t = 0 frame; the embedding is the mean over the present modalities."""
        u = None if noise is None else noise.get("u_init")
        return self._initial_from_embed(self._initial_embed(observation, modality_mask), u).to(self.device)

    def noise_shapes(self, batch: int, steps: int) -> dict[str, tuple[int, ...]]:
        """Uniforms one ``shared_step`` consumes (one per categorical and draw; row = batch row).  Data-parallel runs
        draw them for the GLOBAL batch and slice rows (``parallel.GlobalRowNoise``) so results do not depend on the rank count."""
        k = self.transition.distribution_factory.category_size
        return self._with_mask_noise({"u_init": (batch, k), "u_post": (batch, steps, k)}, batch, steps)

    def _with_mask_noise(self, shapes: dict[str, tuple[int, ...]], batch: int, steps: int) -> dict[str, tuple[int, ...]]:
        """With ``self.modality_dropout`` set, the key ``u_mask`` joins (``GlobalRowNoise`` hands every rank ALL its rows: the
        sampler counts the global batch's present frames), with ``self.forecast`` set ``u_context`` (likewise); without, ``shapes``
        as it is.  With ``self.overshoot`` set ``u_overshoot`` (MMTRSSM: ``u_overshoot_l`` / ``u_overshoot_h``) joins, batch row first."""
        if self.modality_dropout is not None:
            shapes["u_mask"] = self.modality_dropout.noise_shape(batch, steps)
        if self.forecast is not None:
            shapes["u_context"] = self.forecast.noise_shape(batch)
        if self.overshoot is not None:
            for key in self._POST_KEYS:
                shapes[self._overshoot_key(key)] = self.overshoot.noise_shape(batch, steps, self._category_size_of(key))
        return shapes

    def _rollout_embedded(self, actions: Tensor, audio_embed: Tensor | None, vision_embed: Tensor | None, prev_state: State,  # noqa: PLR0913
                          noise: Noise | None, *, sample_prior: bool, modality: Tensor | None = None,
                          expert_log_weights: Tensor | None = None) -> dict[str, Tensor]:
        noise = noise or {}
        B, T = actions.shape[:2]
        K = self.transition.distribution_factory.category_size
        logw = self._expert_logw(audio_embed, vision_embed, expert_log_weights, B, T)
        self._report_weights(logw, modality, B, T, actions.device)
        u_post = noise.get("u_post")
        u_prior = noise.get("u_prior")
        if u_post is None:
            u_post = _rand(actions, B, T, K)
        if u_prior is None and sample_prior:
            u_prior = _rand(actions, B, T, K)
        return scan.mrssm_posterior_rollout(
            self.transition, self.audio_representation, self.vision_representation, actions, audio_embed, vision_embed,
            prev_state.deter, prev_state.stoch, u_post, u_prior, balancing=bool(self.use_kl_balancing),
            rows_per_block=self.scan_rows_per_block, threads=self.scan_threads, modality=modality, expert_logw=logw,
        )

    def _expert_logw(self, audio_embed: Tensor | None, vision_embed: Tensor | None, explicit: Tensor | None, B: int, T: int) -> Tensor | None:  # noqa: N803, PLR0913
        """The scan's expert log-weights ``[B, T, 3]``: ``explicit`` ones, else the model's gate on the two embeddings, else None (1/3
        each).  A modality that is absent at every step (None) leaves no step with both: the gate is not run."""
        if audio_embed is None or vision_embed is None:
            return None
        if explicit is not None:
            return scan.check_expert_logw(explicit, B, T)
        if self.expert_weights is None:
            return None
        return self.expert_weights(audio_embed, vision_embed)

    def _report_weights(self, logw: Tensor | None, codes: Tensor | None, B: int, T: int, device: torch.device) -> None:  # noqa: N803, PLR0913
        """``weights_timeseries`` of a weighted rollout (detached; a model without weights keeps None)."""
        if logw is None and self.expert_weights is None:
            return
        with torch.no_grad():
            if codes is None:
                codes = torch.full((B, T), 3, device=device, dtype=torch.int32)
            self._weights_both = (codes & 3) == 3  # noqa: PLR2004
            self.weights_timeseries = ExpertWeights.table(logw, codes & 3)

    def _posterior_from_rollout(self, out: dict[str, Tensor]) -> State:
        post = State(deter=out["deter"], distribution=self.audio_representation.distribution_factory.unmixed(out["post_logits"]), stoch=out["post_stoch"])
        post.kl_per_step = out["kl"]  # sum_K KL(q||p) per (b, t), straight from the scan kernel
        return post

    def _states_from_rollout(self, out: dict[str, Tensor]) -> tuple[State, State]:
        factory = self.audio_representation.distribution_factory
        prior = State(deter=out["deter"], distribution=factory.unmixed(out["prior_logits"]), stoch=out["prior_stoch"])
        return self._posterior_from_rollout(out), prior

    def rollout_representation(
        self,
        *,
        actions: Tensor,
        observations: Tensor | tuple[Tensor, ...],
        prev_state: State,
        noise: Noise | None = None,
        modality_mask: Tensor | None = None,
        lengths: Tensor | None = None,
        expert_log_weights: Tensor | None = None,
    ) -> tuple[State, State]:
        """``mrssm core.py:184-260``: returns (mixed posterior, prior), each ``[B, T, .]``.

        ``modality_mask``: optional bool ``[B, T, 2]`` (audio, vision), True = observed.  At each (b, t) the posterior mixes
        the present modalities only; with none present it is the prior (DESIGN.md "Missing modalities").  An entry of
        ``observations`` may be None: that modality is absent at every step and its encoder is not run.  ``lengths`` (int32 ``[B]`` on
        the device) instead of a mask: both modalities on a row's first ``lengths[b]`` steps, none after.  ``expert_log_weights``
        (fp32 ``[B, T, 3]``): explicit log-weights of the (audio, vision, fused) experts where both are
        present, instead of ``self.expert_weights``' (analysis, tests)."""
        if not isinstance(observations, tuple):
            msg = "MoPoE-MRSSM requires tuple of (audio_obs, vision_obs)"
            raise TypeError(msg)
        audio_obs, vision_obs = observations
        B, T = actions.shape[:2]
        codes = self._rollout_codes(observations, modality_mask, lengths, B, T, actions.device)
        audio_embed = None if audio_obs is None else self.audio_encoder(audio_obs)
        vision_embed = None if vision_obs is None else self.vision_encoder(vision_obs)
        out = self._rollout_embedded(actions, audio_embed, vision_embed, prev_state, noise, sample_prior=True, modality=codes,
                                     expert_log_weights=expert_log_weights)
        return self._states_from_rollout(out)

    @staticmethod
    def _rollout_codes(observations: tuple, modality_mask: Tensor | None, lengths: Tensor | None, B: int, T: int,  # noqa: N803, PLR0913
                       device: torch.device) -> Tensor | None:
        """The scans' codes of a rollout: from a modality mask (None: the unmasked kernels), or from ``lengths`` (int32 ``[B]`` on the
        device: row b observes both modalities on its first ``lengths[b]`` steps and nothing after)."""
        if lengths is None:
            mask = _resolve_modality_mask(observations, modality_mask, B, T, device)
            return None if mask is None else scan.modality_codes(mask)
        if modality_mask is not None or observations[0] is None or observations[1] is None:
            msg = "give lengths or a modality_mask (or a None observation), not both"
            raise ValueError(msg)
        _check_lengths(lengths, B, device)
        return ragged_step_mask(lengths, None, T).codes

    def rollout_transition(self, *, actions: Tensor, prev_state: State, noise: Noise | None = None) -> State:
        """``core.py:170-185``: prior-only rollout (callbacks / evaluation)."""
        u = None if noise is None else noise.get("u_prior")
        out = scan.mrssm_prior_rollout(self.transition, actions, prev_state.deter, prev_state.stoch, u,
                                       rows_per_block=self.scan_rows_per_block, threads=self.scan_threads)
        dist = self.transition.distribution_factory.unmixed(out["prior_logits"])
        return State(deter=out["deter"], distribution=dist, stoch=out["prior_stoch"])

    @torch.no_grad()
    def forecast_rollout(self, *, actions: Tensor, observations: tuple[Tensor, Tensor], context: int, prev_state: State | MTState,  # noqa: PLR0913
                         noise: Noise | None = None, lengths: Tensor | None = None) -> State | MTState:
        """Observe the first ``context`` frames, then run open loop: ONE masked posterior rollout (both modalities on steps
        ``t < context``, none after, where the scans take posterior = prior), returned as the posterior state sequence ``[B, T, .]``.
        It is the logging callback's ``rollout_representation`` -> ``[:, context - 1]`` -> ``rollout_transition`` -> ``cat_states`` in one
        launch, the tail sampled with ``noise["u_post"][:, context:]`` (MMTRSSM: ``u_post_l`` / ``u_post_h``).  ``lengths`` (int32
        ``[B]`` on the device): nothing is observed at or past a row's end either."""
        if not isinstance(observations, tuple) or observations[0] is None or observations[1] is None:
            msg = "forecast_rollout requires the tuple (audio_obs, vision_obs), both given"
            raise TypeError(msg)
        B, T = actions.shape[:2]
        if lengths is not None:
            _check_lengths(lengths, B, actions.device)
        sm = Forecast(context).sample(torch.zeros(B, device=actions.device), T, lengths)  # (a fixed context: the uniforms do not matter)
        audio_embed, vision_embed = self.audio_encoder(observations[0]), self.vision_encoder(observations[1])
        out = self._rollout_embedded(actions, audio_embed, vision_embed, prev_state, noise, sample_prior=False, modality=sm.codes)
        return self._posterior_from_rollout(out)

    def _initial_for_step(self, obs_embed: Tensor, noise: Noise | None) -> State | MTState:
        """``_initial_from_embed`` with the step's noise dict (the two models take their initial uniforms differently)."""
        return self._initial_from_embed(obs_embed, None if noise is None else noise.get("u_init"))

    @staticmethod
    def _feature_of(out: dict[str, Tensor]) -> Tensor:
        """What the decoders read of a posterior rollout."""
        return torch.cat([out["deter"], out["post_stoch"]], dim=-1)

    _POST_KEYS = ("u_post",)  # the rollout's posterior uniforms; a skill step composes each with its "u_tail" twin (evaluation.CopyPlan)

    def _category_size_of(self, key: str) -> int:  # noqa: ARG002
        return self.transition.distribution_factory.category_size

    # -- train / val ----------------------------------------------------------------------------
    def _dropout_uniforms(self, batch: tuple[Tensor, ...], noise: Noise | None, modality_dropout: ModalityDropout, world: int) -> Tensor:
        """``noise["u_mask"]`` of the GLOBAL batch (``world`` ranks of the batch's rows), drawn here when absent on one rank."""
        B, T = batch[0].shape[:2]
        u = None if noise is None else noise.get("u_mask")
        if u is None:
            if world > 1:
                msg = "modality_dropout on more than one rank needs noise['u_mask'] of the global batch (GlobalRowNoise.draw)"
                raise ValueError(msg)
            u = _rand(batch[0], *modality_dropout.noise_shape(B, T))
        if u.shape[0] != B * world:
            msg = f"noise['u_mask'] has {u.shape[0]} rows, the global batch {B} x {world}"
            raise ValueError(msg)
        return u

    def _forecast_step_mask(self, batch: tuple[Tensor, ...], noise: Noise | None, forecast: Forecast,  # noqa: PLR0913
                            modality_dropout: ModalityDropout | None, lengths: Tensor | None = None,
                            ragged: tuple[Tensor, int, int] | None = None) -> StepMask:
        """The masks of a forecast step, one launch, nothing read back: the sampled context AND the lengths (when
        the step has them) AND the dropout rule.  ``ragged``: ``_lengths_of``'s result when the caller has checked the lengths already."""
        if not isinstance(forecast, Forecast):
            msg = f"forecast must be a Forecast, got {type(forecast).__name__}"
            raise ValueError(msg)
        if modality_dropout is not None and not isinstance(modality_dropout, ModalityDropout):
            msg = f"modality_dropout must be a ModalityDropout, got {type(modality_dropout).__name__}"
            raise ValueError(msg)
        B, T = batch[0].shape[:2]
        if lengths is not None and forecast.world != 1:
            msg = "lengths= describes one rank's own rows: with data parallelism use a batch that carries valid_global"
            raise ValueError(msg)
        if ragged is None:
            ragged = self._lengths_of(batch, lengths, modality_dropout, None)  # (no carry: every row resets)
        if ragged is not None:
            valid, world, rank = ragged
            _check_lengths(valid, B * world, batch[0].device)
        else:
            valid, world, rank = None, forecast.world, forecast.rank
        for what, bound in (("forecast", forecast), ("modality_dropout", modality_dropout)):
            if bound is not None and (bound.world not in (1, world) or (bound.world == world and bound.rank != rank)):
                msg = f"{what} is bound to rank {bound.rank} of {bound.world}, the batch to rank {rank} of {world}"
                raise ValueError(msg)
        u_context = None if noise is None else noise.get("u_context")
        if u_context is None:
            if forecast.fixed:  # (every row observes the same number of frames: no draw)
                u_context = torch.zeros(B * world, device=batch[0].device)
            elif world > 1:
                msg = "forecast on more than one rank needs noise['u_context'] of the global batch (GlobalRowNoise.draw)"
                raise ValueError(msg)
            else:
                u_context = _rand(batch[0], *forecast.noise_shape(B))
        if u_context.shape[0] != B * world:
            msg = f"noise['u_context'] has {u_context.shape[0]} rows, the global batch {B} x {world}"
            raise ValueError(msg)
        u_mask = None if modality_dropout is None else self._dropout_uniforms(batch, noise, modality_dropout, world)
        return forecast.sample(u_context, T, valid, u_mask, modality_dropout, world=world, rank=rank)

    def _ragged_step_mask(self, batch: tuple[Tensor, ...], noise: Noise | None, modality_dropout: ModalityDropout | None,  # noqa: PLR0913
                          valid_global: Tensor, world: int, rank: int) -> StepMask:
        """The masks of a ragged step from the GLOBAL batch's live-step counts, one launch, nothing read back:
        lengths AND the dropout rule (``noise["u_mask"]``, drawn here when absent on one rank)."""
        B, T = batch[0].shape[:2]
        _check_lengths(valid_global, B * world, batch[0].device)
        u = None
        if modality_dropout is not None:
            if not isinstance(modality_dropout, ModalityDropout):
                msg = f"modality_dropout must be a ModalityDropout, got {type(modality_dropout).__name__}"
                raise ValueError(msg)
            if modality_dropout.world not in (1, world) or (modality_dropout.world == world and modality_dropout.rank != rank):
                msg = f"modality_dropout is bound to rank {modality_dropout.rank} of {modality_dropout.world}, the batch to rank {rank} of {world}"
                raise ValueError(msg)
            u = self._dropout_uniforms(batch, noise, modality_dropout, world)
        return ragged_step_mask(valid_global, u, T, modality_dropout, world=world, rank=rank)

    def _lengths_of(self, batch: tuple[Tensor, ...], lengths: Tensor | None, modality_dropout: ModalityDropout | None,
                    reset_host: Tensor | None, *, trust_reset: bool = False) -> tuple[Tensor, int, int] | None:
        """``(valid_global, world, rank)`` of a ragged step, None for a step without lengths.  An explicit ``lengths`` is one rank's
        own (int32 ``[B]`` on the device, trusted); a batch's ``valid_global`` comes with its host copy, on which the t = 0 rule is
        checked here against ``reset_host`` (None: every row resets; ``trust_reset``: the reset only exists on the device, no check)."""
        B = batch[0].shape[0]
        if lengths is not None:
            _check_lengths(lengths, B, batch[0].device)
            if modality_dropout is not None and getattr(modality_dropout, "world", 1) != 1:
                msg = "lengths= describes one rank's own rows: with data parallelism use a batch that carries valid_global"
                raise ValueError(msg)
            return lengths, 1, 0
        valid_global = getattr(batch, "valid_global", None)
        if valid_global is None:
            return None
        if valid_global.numel() % B:
            msg = f"valid_global has {valid_global.numel()} rows, no multiple of the batch's {B}"
            raise ValueError(msg)
        world = valid_global.numel() // B
        rank = int(getattr(batch, "row0", 0)) // B
        valid_host = getattr(batch, "valid_host", None)
        if valid_host is not None and not trust_reset:
            check_ragged_rows(valid_host, reset_host)
        return valid_global, world, rank

    def _step_mask(self, batch: tuple[Tensor, ...], noise: Noise | None, modality_mask: Tensor | None,  # noqa: PLR0913
                   modality_dropout: ModalityDropout | None, lengths: Tensor | None = None, reset_host: Tensor | None = None, *,
                   trust_reset: bool = False) -> StepMask | None:
        """The masks of a training step (None: every modality everywhere, the unmasked kernels).  A caller's mask (the kwarg,
        else the batch's 7th entry) is validated on the host; a dropout's comes from its sampler kernel with no host round trip
        (the rule itself keeps a modality at t = 0).  ``lengths`` (or a batch that carries ``valid_global``): the ragged step's
        masks, lengths AND dropout, from ``mtrssm_step_mask_ragged``."""
        mask = modality_mask if modality_mask is not None else self.get_modality_mask_from_batch(batch)
        B, T = batch[0].shape[:2]
        ragged = self._lengths_of(batch, lengths, modality_dropout, reset_host, trust_reset=trust_reset)
        if ragged is not None:
            if mask is not None:
                msg = "give lengths (or a batch that carries them) or a modality_mask, not both"
                raise ValueError(msg)
            return self._ragged_step_mask(batch, noise, modality_dropout, *ragged)
        if modality_dropout is None:
            if mask is None:
                return None
            _check_modality_mask(mask, B, T, batch[0].device, first_step=True)
            return StepMask.from_mask(mask)
        if mask is not None:
            msg = "give a modality_mask (or a 7-tuple batch) or a modality_dropout, not both"
            raise ValueError(msg)
        if not isinstance(modality_dropout, ModalityDropout):
            msg = f"modality_dropout must be a ModalityDropout, got {type(modality_dropout).__name__}"
            raise ValueError(msg)
        return modality_dropout.sample(self._dropout_uniforms(batch, noise, modality_dropout, modality_dropout.world), T).step_mask()

    @staticmethod
    def _overshoot_key(post_key: str) -> str:
        """``u_post`` -> ``u_overshoot``, ``u_post_l`` -> ``u_overshoot_l``: the uniforms of a level's overshoot rows."""
        return "u_overshoot" + post_key[len("u_post"):]

    def _overshoot_plan(self, batch: tuple[Tensor, ...], overshoot: LatentOvershoot, lengths: Tensor | None,
                        modality_dropout: ModalityDropout | None) -> tuple[LatentOvershoot, Tensor | None, int]:
        """``(overshoot bound to the batch's rank, valid of ALL global rows or None, row0)`` of a step; host rules only."""
        if not isinstance(overshoot, LatentOvershoot):
            msg = f"overshoot must be a LatentOvershoot, got {type(overshoot).__name__}"
            raise ValueError(msg)
        B, T = batch[0].shape[:2]
        overshoot.rows(T)  # (offset <= T - 2, or ValueError)
        if lengths is not None and overshoot.world != 1:
            msg = "lengths= describes one rank's own rows: with data parallelism use a batch that carries valid_global"
            raise ValueError(msg)
        ragged = self._lengths_of(batch, lengths, modality_dropout, None, trust_reset=True)  # (the step's mask checked the t = 0 rule)
        valid, world, rank = (None, overshoot.world, overshoot.rank) if ragged is None else ragged
        if overshoot.world not in (1, world) or (overshoot.world == world and overshoot.rank != rank):
            msg = f"overshoot is bound to rank {overshoot.rank} of {overshoot.world}, the batch to rank {rank} of {world}"
            raise ValueError(msg)
        bound = overshoot if overshoot.world == world else overshoot.for_rank(world, rank)
        return bound, valid, rank * B

    def _overshoot_terms(self, actions: Tensor, out: dict[str, Tensor], noise: Noise | None,
                         plan: tuple[LatentOvershoot, Tensor | None, int]) -> list[OvershootTerms]:
        """The overshoot pass behind the closed-loop scan ``out``: gather the start states and action windows, roll the
        ``B * N`` rows ``D`` steps open loop (modality code 0, no embeddings) and take the KL pair per latent level.  Nothing is read
        back."""
        from types import SimpleNamespace  # noqa: PLC0415

        lo, valid, row0 = plan
        noise = noise or {}
        B, T = actions.shape[:2]
        n, d = lo.rows(T), lo.depth
        starts, windows = lo.gather([out[self._LAST_KEYS[k]] for k in self._FRESH_KEYS], actions)
        state = SimpleNamespace(**dict(zip(self._FRESH_KEYS, starts, strict=True)))
        os_noise: dict[str, Tensor] = {}
        for key in self._POST_KEYS:
            k = self._category_size_of(key)
            u = noise.get(self._overshoot_key(key))
            if u is None:
                u = _rand(actions, B, n, d, k)
            if tuple(u.shape) != (B, n, d, k):
                msg = f"noise[{self._overshoot_key(key)!r}] must have shape {(B, n, d, k)}, got {tuple(u.shape)}"
                raise ValueError(msg)
            os_noise[key] = u.to(actions).reshape(B * n, d, k)
        codes = torch.zeros(B * n, d, dtype=torch.int32, device=actions.device)
        reported = (self.weights_timeseries, self._weights_both)  # (the closed-loop step's: the overshoot rows have no gate to report)
        os_out = self._rollout_embedded(windows, None, None, state, os_noise, sample_prior=False, modality=codes)
        self.weights_timeseries, self._weights_both = reported
        weights = lo.kl_weights(bool(self.use_kl_balancing))
        terms = []
        for key in self._POST_KEYS:
            level = key[len("u_post"):]
            terms.append(lo.kl(out["post_logits" + level], os_out["prior_logits" + level], self._category_size_of(key), valid, row0, weights))
        self._overshoot_terms_last = terms
        return terms

    def _add_overshoot(self, result: dict[str, Tensor], terms: list[OvershootTerms], lo: LatentOvershoot,
                       schedule: ElboSchedule | None) -> dict[str, Tensor]:
        """``loss += kl_coeff * weight * (overshoot [+ w_kl_h * overshoot_h])``, times the step's beta under a schedule; free nats do
        not apply.  The new keys come after the existing ones."""
        extra = terms[0].term
        if len(terms) > 1:
            extra = extra + float(self.w_kl_h) * terms[1].term
        extra = extra * (float(self.kl_coeff) * lo.weight)
        if schedule is not None:
            extra = extra * schedule.stats["beta"].to(extra)
        result["loss"] = result["loss"] + extra
        result["overshoot"] = terms[0].term
        if len(terms) > 1:
            result["overshoot_h"] = terms[1].term
        return result

    def shared_step(self, batch: tuple[Tensor, ...], noise: Noise | None = None, modality_mask: Tensor | None = None,  # noqa: PLR0913
                    modality_dropout: ModalityDropout | None = None, state_carry: StateCarry | None = None,
                    reset: Tensor | None = None, *, carry_prefix: str = "train", lengths: Tensor | None = None,
                    forecast: Forecast | None = None, elbo_schedule: ElboSchedule | None = None,
                    expert_log_weights: Tensor | None = None, overshoot: LatentOvershoot | None = None) -> dict[str, Tensor]:
        """``core.py:187-221``: ``loss = recon + kl_coeff * KL(post || prior)`` (MMTRSSM, ``mmtrssm core.py:563-606``:
        ``recon + kl_coeff KL_l + kl_coeff w_kl_h KL_h``).  ``modality_mask`` (or a 7th batch entry, bool ``[B, T, 2]``): each
        recon term averages over the frames where its modality is present; the KL stays the mean over all B*T (0 on steps with
        no modality).  ``modality_dropout``: the mask is sampled on the device from ``noise["u_mask"]`` (drawn here when
        absent) and each recon sum is divided by the GLOBAL batch's present frames / world.

        ``state_carry``: rows with ``reset[b]`` False start from the posterior the previous step of
        ``carry_prefix``'s set ended with instead of the chunk's own frame 0; afterwards the posterior at t = T - 1 (detached) is
        saved there.  ``reset`` (bool ``[B]``) defaults to ``batch.reset`` of an ``EpisodeBatch``; a host tensor is also checked
        against the carry's rules, a device tensor is trusted (an empty carry refuses it).

        ``lengths`` (int32 ``[B]`` on the device, default: the ``valid`` / ``valid_global`` of a batch made by a
        loader with lengths): row b has ``lengths[b]`` live steps.  A dead step has no modality (posterior = prior, KL 0), no
        reconstruction term and zero gradient; each term is divided by the GLOBAL batch's count of its frames / world, the KL by the
        live steps; the carry saves each row's last live step.  A row may be empty only when it does not reset (without a
        ``state_carry`` every row resets).

        ``forecast`` (a ``Forecast``): each row observes a context of ``c_b`` frames sampled from
        ``noise["u_context"]`` (drawn here when absent) and runs open loop after it; both modalities are reconstructed on every live
        frame, the KL sums over the observed steps / their count.  Alone, with ``modality_dropout`` and / or with lengths; not with a
        modality mask (it already says what is seen) nor with a ``state_carry`` (the state it would save is an open-loop state).

        ``elbo_schedule`` (an ``ElboSchedule``): free nats per step, a beta warm-up and per-modality weights in the
        scalar epilogue, with every option above.  ``kl`` (``kl_h``) is then the clipped, beta-weighted term and ``recon`` the weighted
        sum, so ``loss = recon + kl (+ kl_h)`` still holds; ``recon/audio`` and ``recon/vision`` stay unweighted; the dict gains ``kl_raw``
        (``kl_h_raw``), the unscheduled term, after the existing keys.

        ``expert_log_weights``: explicit expert log-weights as in ``rollout_representation``; a weighted model
        (``self.expert_weights``) needs none, its gate runs inside the step.

        ``overshoot`` (a ``LatentOvershoot``): behind the closed-loop scan the posterior states at every
        ``stride``-th frame start ``depth`` open-loop steps (uniforms ``noise["u_overshoot"]``, MMTRSSM ``u_overshoot_l`` / ``_h``,
        drawn here when absent) and ``loss += kl_coeff * weight * overshoot (+ kl_coeff * weight * w_kl_h * overshoot_h)``, times the
        step's beta under an ``elbo_schedule``; the dict gains ``overshoot`` (``overshoot_h``) after the existing keys.  With every
        option above except ``forecast`` (its tail's states are not posteriors)."""
        if forecast is not None and overshoot is not None:
            msg = "overshoot= does not combine with forecast=: the states of a forecast step's tail are not posteriors"
            raise ValueError(msg)
        plan = None if overshoot is None else self._overshoot_plan(batch, overshoot, lengths, modality_dropout)
        if forecast is not None:
            if modality_mask is not None or self.get_modality_mask_from_batch(batch) is not None:
                msg = "forecast= decides what the model observes: a modality_mask (or a 7-tuple batch) already says what is seen, give one of them"
                raise ValueError(msg)
            if state_carry is not None:
                msg = "forecast= does not combine with state_carry: the state a forecast step ends with is an open-loop state, not one to continue from"
                raise ValueError(msg)
            return self._elbo_step(batch, noise, self._forecast_step_mask(batch, noise, forecast, modality_dropout, lengths), schedule=elbo_schedule,
                                   expert_log_weights=expert_log_weights)
        reset_host = None  # without a carry every row starts from its fresh state: every row resets
        if state_carry is not None:
            reset_host = getattr(batch, "reset_host", None) if reset is None else (None if reset.is_cuda else reset)
        on_device = state_carry is not None and isinstance(reset, Tensor) and reset.is_cuda  # (trusted, as the carry trusts it)
        sm = self._step_mask(batch, noise, modality_mask, modality_dropout, lengths, reset_host, trust_reset=on_device)
        if state_carry is None:
            return self._elbo_step(batch, noise, sm, schedule=elbo_schedule, expert_log_weights=expert_log_weights, overshoot=plan)
        return self._elbo_step(batch, noise, sm, self._carry_of(batch, state_carry, reset, carry_prefix), schedule=elbo_schedule,
                               expert_log_weights=expert_log_weights, overshoot=plan)

    @staticmethod
    def _carry_of(batch: tuple[Tensor, ...], state_carry: StateCarry, reset: Tensor | None, prefix: str) -> tuple[StateCarry, str, Tensor]:
        """Validated ``(carry, prefix, reset on the device)`` of a step; host rules only, nothing is read back."""
        if not isinstance(state_carry, StateCarry):
            msg = f"state_carry must be a StateCarry, got {type(state_carry).__name__}"
            raise ValueError(msg)
        dev = batch[0].device
        if reset is None:
            reset, reset_host = getattr(batch, "reset", None), getattr(batch, "reset_host", None)
            if reset is None:
                msg = "state_carry needs reset= (bool [B]) or a batch that carries one (an EpisodeBatch of a windowed loader)"
                raise ValueError(msg)
        elif not isinstance(reset, Tensor) or reset.dtype != torch.bool:
            msg = f"reset must be a bool tensor, got {getattr(reset, 'dtype', type(reset))}"
            raise ValueError(msg)
        else:
            reset_host = None if reset.is_cuda else reset
        if tuple(reset.shape) != (batch[0].shape[0],):
            msg = f"reset must have shape ({batch[0].shape[0]},), got {tuple(reset.shape)}"
            raise ValueError(msg)
        state_carry.check(prefix, batch[0].shape[0], reset_host)
        return state_carry, prefix, reset.to(dev).contiguous()

    _FRESH_KEYS = ("deter", "stoch")  # State attributes the scan starts from
    _INIT_KEYS = ("u_init",)  # the initial state's uniforms
    _LAST_KEYS = {"deter": "deter", "stoch": "post_stoch"}  # ... and the scan outputs that continue them

    def _state0(self, fresh: State | MTState, carry: tuple[StateCarry, str, Tensor] | None) -> State | MTState:
        """The scan's initial state: ``fresh`` (computed for all rows, so the launch sequence is static), or per row the carried one."""
        if carry is None:
            return fresh
        sc, prefix, reset = carry
        got = sc.select(prefix, reset, {k: getattr(fresh, k) for k in self._FRESH_KEYS})
        return self._state_like(fresh, got)

    @staticmethod
    def _state_like(fresh: State, got: dict[str, Tensor]) -> State:
        return State(deter=got["deter"], distribution=fresh.distribution, stoch=got["stoch"])

    def _save_carry(self, out: dict[str, Tensor], carry: tuple[StateCarry, str, Tensor] | None, last: Tensor | None = None) -> None:
        if carry is not None:
            carry[0].save(carry[1], {k: out[v] for k, v in self._LAST_KEYS.items()}, last)

    def _elbo_step(self, batch: tuple[Tensor, ...], noise: Noise | None, sm: StepMask | None,
                   carry: tuple[StateCarry, str, Tensor] | None = None, schedule: ElboSchedule | None = None,
                   expert_log_weights: Tensor | None = None,
                   overshoot: tuple[LatentOvershoot, Tensor | None, int] | None = None) -> dict[str, Tensor]:
        """``shared_step`` behind the mask handling (the captured step enters here with a mask it validated itself)."""
        action_input = batch[0]
        audio_obs, vision_obs = self.get_observations_from_batch(batch)
        conv.begin_step(audio_obs.device)
        audio_embed, vision_embed = self._encode_both(audio_obs, vision_obs)
        u_init = None if noise is None else noise.get("u_init")
        mask0 = None if sm is None else sm.mask0
        state0 = self._initial_fused(audio_embed[:, 0], vision_embed[:, 0], mask0, u_init)  # (the mean is inside the launch)
        if state0 is None:
            state0 = self._initial_from_embed(_masked_mean_embed(audio_embed[:, 0], vision_embed[:, 0], mask0), u_init)
        state0 = self._state0(state0, carry)
        out = self._rollout_embedded(action_input, audio_embed, vision_embed, state0, noise, sample_prior=False,
                                     modality=None if sm is None else sm.codes, expert_log_weights=expert_log_weights)
        self._save_carry(out, carry, None if sm is None else sm.last)
        feature = torch.cat([out["deter"], out["post_stoch"]], dim=-1)
        parts = self._reconstruction_losses(feature, self.get_targets_from_batch(batch), sum_recon=False, step_mask=sm)
        recon, kl_div, _, loss = _elbo(parts["recon/audio"], parts["recon/vision"], out["kl"], float(self.kl_coeff), step_mask=sm, schedule=schedule)
        result = {"recon": recon, **parts, "kl": kl_div, "loss": loss}
        if schedule is not None:
            result["kl_raw"] = schedule.stats["kl_raw"]
        if overshoot is not None:
            return self._add_overshoot(result, self._overshoot_terms(action_input, out, noise, overshoot), overshoot[0], schedule)
        return result

    def _step(self, batch: tuple[Tensor, ...], prefix: str, *, with_loss_key: bool, modality_dropout: ModalityDropout | None = None,  # noqa: PLR0913
              forecast: Forecast | None = None, elbo_schedule: ElboSchedule | None = None,
              overshoot: LatentOvershoot | None = None) -> dict[str, Tensor]:
        if forecast is not None:  # (with a state_carry or an overshoot set too, shared_step refuses)
            loss_dict = self.shared_step(batch, modality_dropout=modality_dropout, state_carry=self.state_carry, forecast=forecast,
                                         elbo_schedule=elbo_schedule, overshoot=overshoot)
        elif self.state_carry is None:
            loss_dict = self.shared_step(batch, modality_dropout=modality_dropout, elbo_schedule=elbo_schedule, overshoot=overshoot)
        else:
            loss_dict = self.shared_step(batch, modality_dropout=modality_dropout, state_carry=self.state_carry, carry_prefix=prefix,
                                         elbo_schedule=elbo_schedule, overshoot=overshoot)
        renamed = {"loss": loss_dict["loss"]} if with_loss_key else {}
        renamed[f"{prefix}/loss"] = loss_dict["loss"]
        for key, value in loss_dict.items():
            if key != "loss":
                renamed[f"{prefix}/{key}"] = value
        self.log_dict(renamed, prog_bar=True, sync_dist=True, on_step=False, on_epoch=True)
        return renamed

    def training_step(self, batch: tuple[Tensor, ...], _: int = 0) -> dict[str, Tensor]:
        return self._step(batch, "train", with_loss_key=True, modality_dropout=self.modality_dropout, forecast=self.forecast,
                          elbo_schedule=self.elbo_schedule, overshoot=self.overshoot)

    def validation_step(self, batch: tuple[Tensor, ...], _batch_index: int = 0) -> dict[str, Tensor]:
        """``val/*`` of the closed-loop step; with ``self.val_forecast`` set, a second step on the same batch observes that context and
        forecasts the rest (from the chunk's own frame 0, no carry), logged as ``val/forecast/*``.  ``self.elbo_schedule`` is not used
        here: ``val/loss`` stays the plain ELBO that schedulers and checkpointing monitor."""
        logged = self._step(batch, "val", with_loss_key=False)
        if self.expert_weights is not None and self.weights_timeseries is not None:
            # the closed-loop step's reported weights, averaged over the live frames where both modalities are present
            both = self._weights_both.unsqueeze(-1).to(torch.float32)
            mean = (self.weights_timeseries * both).sum(dim=(0, 1)) / both.sum().clamp(min=1.0)
            weights = {f"val/weights/{name}": mean[i] for i, name in enumerate(("audio", "vision", "fused"))}
            self.log_dict(weights, prog_bar=False, sync_dist=True, on_step=False, on_epoch=True)
            logged.update(weights)
        if self.val_forecast is not None:
            fore = {f"val/forecast/{k}": v for k, v in self.shared_step(batch, forecast=self.val_forecast).items()}
            self.log_dict(fore, prog_bar=False, sync_dist=True, on_step=False, on_epoch=True)
            logged.update(fore)
        if self.val_skill is not None:  # (after everything above: the draws of val/* are what they are without it)
            self.skill_table = self.forecast_skill(batch, self.val_skill, table=self.skill_table)
        if self.val_likelihood is not None:  # (last, for the same reason)
            self.likelihood_table = self.likelihood_bound(batch, self.val_likelihood, table=self.likelihood_table)
        if self.val_particle is not None:  # (after the likelihood step: every draw above is what it is without it)
            self.particle_table = self.particle_filter(batch, self.val_particle, table=self.particle_table)
        if self.val_overshoot is not None:  # (last: every draw above is what it is without it)
            with torch.no_grad():
                self.shared_step(batch, overshoot=self.val_overshoot)
            terms = self._overshoot_terms_last
            if self.overshoot_table is None:
                self.overshoot_table = OvershootTable(len(terms), self.val_overshoot.depth, terms[0].table.device)
            self.overshoot_table.fold([t.table for t in terms])
        if self.val_census is not None:  # (last: every draw above is what it is without it)
            self.census_table = self.latent_census(batch, self.val_census, table=self.census_table)
        if self.val_frechet is not None:  # (last: every draw above is what it is without it)
            self.frechet_table = self.frechet_distance(batch, self.val_frechet, self.frechet_classifier, table=self.frechet_table)
        return logged

    def on_validation_epoch_end(self) -> dict[str, Tensor]:
        """Logs the epoch's ``val/skill/{audio,vision}/{mean,ens,best,spread}/{obs,h1,h2,h4,h8}`` and
        ``val/loglik/{iw,elbo,audio,vision,latent,ess,gap}`` and ``val/smc/{smc,mean,audio,vision,latent,ess,resampled}`` (each table
        all-reduced once when a process group is initialised; the group is the one ``FlatDataParallel.skill`` / ``.likelihood`` /
        ``.particle`` bound) and clears the tables; likewise ``val/overshoot/*``, the census's ``val/latent/*`` (``CensusTable.scalars``)
        and the Frechet distances ``val/frechet/*`` (``FrechetTable.scalars``).
        Without a table: nothing."""
        logged: dict[str, Tensor] = {}
        table, self.skill_table = self.skill_table, None
        if table is not None:
            table.all_reduce(getattr(self.val_skill, "group", None))
            logged.update(table.scalars("val/skill"))
        loglik, self.likelihood_table = self.likelihood_table, None
        if loglik is not None:
            loglik.all_reduce(getattr(self.val_likelihood, "group", None))
            logged.update(loglik.scalars("val/loglik"))
        smc, self.particle_table = self.particle_table, None
        if smc is not None:
            smc.all_reduce(getattr(self.val_particle, "group", None))
            logged.update(smc.scalars("val/smc"))
        curve, self.overshoot_table = self.overshoot_table, None
        if curve is not None:
            curve.all_reduce(getattr(self.val_overshoot, "group", None))
            logged.update(curve.scalars("val/overshoot"))
        census, self.census_table = self.census_table, None
        if census is not None:
            census.all_reduce(getattr(self.val_census, "group", None))
            logged.update(census.scalars("val/latent"))
        moments, self.frechet_table = self.frechet_table, None
        if moments is not None:
            moments.all_reduce(getattr(self.val_frechet, "group", None))
            logged.update(moments.scalars("val/frechet"))
        if logged:
            self.log_dict(logged, prog_bar=False, sync_dist=False, on_step=False, on_epoch=True)
        return logged


class MoPoE_MMTRSSM(MoPoE_MRSSM):  # noqa: N801
    """Two-timescale variant: MTRNN lower (tau_l) / higher (tau_h) levels, MoPoE on the lower level."""

    def __init__(  # noqa: PLR0913
        self,
        *,
        audio_representation: Representation,
        vision_representation: Representation,
        audio_encoder: nn.Module,
        vision_encoder: nn.Module,
        audio_decoder: nn.Module,
        vision_decoder: nn.Module,
        init_proj: nn.Module,
        kl_coeff: float,
        use_kl_balancing: bool,
        action_size: int,
        hd_dim: int,
        hs_dim: int,
        ld_dim: int,
        ls_dim: int,
        l_tau: float,
        h_tau: float,
        l_prior: nn.Module,
        l_posterior: nn.Module,
        h_prior: nn.Module,
        h_posterior: nn.Module,
        l_dist: MultiOneHotFactory,
        h_dist: MultiOneHotFactory,
        w_kl_h: float = 1.0,
        unimix: float = 0.0,
    ) -> None:
        # the reference registers a never-trained Transition (A=1, S=1) for its base class (core.py:143-151);
        # kept so that state-dicts interchange
        dummy_transition = Transition(deterministic_size=ld_dim, hidden_size=ld_dim, action_size=1,
                                      distribution_config=[1, 1], activation_name="ELU")
        super().__init__(
            audio_representation=audio_representation, vision_representation=vision_representation,
            transition=dummy_transition, audio_encoder=audio_encoder, vision_encoder=vision_encoder,
            audio_decoder=audio_decoder, vision_decoder=vision_decoder, init_proj=init_proj, kl_coeff=kl_coeff,
            use_kl_balancing=use_kl_balancing, unimix=unimix,
        )
        self.action_dim = action_size
        self.hd_dim, self.hs_dim, self.ld_dim, self.ls_dim = hd_dim, hs_dim, ld_dim, ls_dim
        self.w_kl_h = w_kl_h
        self.l_rnn = MTRNN(input_dim=action_size + ls_dim + hs_dim, hidden_dim=ld_dim, tau=l_tau)
        self.h_rnn = MTRNN(input_dim=hs_dim, hidden_dim=hd_dim, tau=h_tau)
        self.l_prior = l_prior
        self.l_posterior = l_posterior  # registered, never used on the path upstream either (core.py:188)
        self.h_prior = h_prior
        self.h_posterior = h_posterior
        self.l_dist = l_dist
        self.h_dist = h_dist
        self.unimix = unimix  # (again: now l_dist and h_dist are among the factories)

    @property
    def feature_dim(self) -> int:
        return self.hd_dim + self.hs_dim + self.ld_dim + self.ls_dim

    def _initial_from_embed(self, obs_embed: Tensor, noise: Noise | None) -> MTState:  # type: ignore[override]
        h = self.init_proj(obs_embed)
        higher, lower = h[..., : self.hd_dim], h[..., self.hd_dim :]
        noise = noise or {}
        h_dist, stoch_h = _sampled_head(self.h_dist, self.h_prior(higher), noise.get("u_init_h"))
        l_dist, stoch_l = _sampled_head(self.l_dist, self.l_prior(lower), noise.get("u_init_l"))
        return MTState(
            deter_h=higher, deter_l=lower, distribution_h=h_dist, distribution_l=l_dist, hidden_h=higher, hidden_l=lower,
            stoch_h=stoch_h, stoch_l=stoch_l,
        )

    def initial_state(self, observation: tuple[Tensor, Tensor] | Tensor, noise: Noise | None = None,  # type: ignore[override]
                      modality_mask: Tensor | None = None) -> MTState:
        """``mmtrssm core.py:321-362``: ``init_proj`` output split into raw hiddens = deters (no tanh at t=0).
        ``modality_mask``: as ``MoPoE_MRSSM.initial_state``."""
        obs_embed = self._initial_embed(observation, modality_mask) if isinstance(observation, tuple) else observation
        return self._initial_from_embed(obs_embed, noise).to(obs_embed.device)

    def noise_shapes(self, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # type: ignore[override]
        kl, kh = self.l_dist.category_size, self.h_dist.category_size
        return self._with_mask_noise({"u_init_h": (batch, kh), "u_init_l": (batch, kl), "u_post_l": (batch, steps, kl),
                                      "u_post_h": (batch, steps, kh)}, batch, steps)

    @staticmethod
    def _state_dict_of(state: MTState) -> dict[str, Tensor]:
        return {"deter_l": state.deter_l, "deter_h": state.deter_h, "hidden_l": state.hidden_l, "hidden_h": state.hidden_h,
                "stoch_l": state.stoch_l, "stoch_h": state.stoch_h}

    def _rollout_embedded(self, actions: Tensor, audio_embed: Tensor | None, vision_embed: Tensor | None,  # type: ignore[override]  # noqa: PLR0913
                          prev_state: MTState, noise: Noise | None, *, sample_prior: bool,
                          modality: Tensor | None = None, expert_log_weights: Tensor | None = None) -> dict[str, Tensor]:
        noise = dict(noise or {})
        B, T = actions.shape[:2]
        logw = self._expert_logw(audio_embed, vision_embed, expert_log_weights, B, T)
        self._report_weights(logw, modality, B, T, actions.device)
        KL, KH = self.l_dist.category_size, self.h_dist.category_size
        for key, k in (("u_post_l", KL), ("u_post_h", KH)):
            if noise.get(key) is None:
                noise[key] = _rand(actions, B, T, k)
        if sample_prior:
            for key, k in (("u_prior_l", KL), ("u_prior_h", KH)):
                if noise.get(key) is None:
                    noise[key] = _rand(actions, B, T, k)
        return scan.mmtrssm_posterior_rollout(self, actions, audio_embed, vision_embed, self._state_dict_of(prev_state), noise,
                                              rows_per_block=self.scan_rows_per_block, threads=self.scan_threads, modality=modality,
                                              expert_logw=logw)

    def _posterior_from_rollout(self, out: dict[str, Tensor]) -> MTState:  # type: ignore[override]
        post = MTState(distribution_h=self.h_dist.unmixed(out["post_logits_h"]), distribution_l=self.l_dist.unmixed(out["post_logits_l"]),
                       stoch_h=out["post_stoch_h"], stoch_l=out["post_stoch_l"], deter_h=out["deter_h"], deter_l=out["deter_l"],
                       hidden_h=out["hidden_h"], hidden_l=out["hidden_l"])
        post.kl_per_step, post.kl_h_per_step = out["kl_l"], out["kl_h"]
        return post

    def _states_from_rollout(self, out: dict[str, Tensor]) -> tuple[MTState, MTState]:  # type: ignore[override]
        prior = MTState(distribution_h=self.h_dist.unmixed(out["prior_logits_h"]), distribution_l=self.l_dist.unmixed(out["prior_logits_l"]),
                        stoch_h=out["prior_stoch_h"], stoch_l=out["prior_stoch_l"], deter_h=out["deter_h"], deter_l=out["deter_l"],
                        hidden_h=out["hidden_h"], hidden_l=out["hidden_l"])
        return self._posterior_from_rollout(out), prior

    def rollout_representation(  # type: ignore[override]
        self,
        *,
        actions: Tensor,
        observations: Tensor | tuple[Tensor, ...],
        prev_state: MTState,
        noise: Noise | None = None,
        modality_mask: Tensor | None = None,
        lengths: Tensor | None = None,
        expert_log_weights: Tensor | None = None,
    ) -> tuple[MTState, MTState]:
        """``mmtrssm core.py:364-494``.

        ``modality_mask``: optional bool ``[B, T, 2]`` (audio, vision), True = observed.  At each (b, t) the posterior mixes
        the present modalities only; with none present it is the prior (DESIGN.md "Missing modalities").  An entry of
        ``observations`` may be None: that modality is absent at every step and its encoder is not run.  ``lengths`` (int32 ``[B]`` on
        the device) instead of a mask: both modalities on a row's first ``lengths[b]`` steps, none after.  ``expert_log_weights``
        (fp32 ``[B, T, 3]``): explicit log-weights of the (audio, vision, fused) experts where both are
        present, instead of ``self.expert_weights``' (analysis, tests)."""
        if not isinstance(observations, tuple):
            msg = "MoPoE-MMTRSSM requires tuple of (audio_obs, vision_obs)"
            raise TypeError(msg)
        audio_obs, vision_obs = observations
        B, T = actions.shape[:2]
        codes = self._rollout_codes(observations, modality_mask, lengths, B, T, actions.device)
        audio_embed = None if audio_obs is None else self.audio_encoder(audio_obs)
        vision_embed = None if vision_obs is None else self.vision_encoder(vision_obs)
        out = self._rollout_embedded(actions, audio_embed, vision_embed, prev_state, noise, sample_prior=True, modality=codes,
                                     expert_log_weights=expert_log_weights)
        return self._states_from_rollout(out)

    def rollout_transition(self, *, actions: Tensor, prev_state: MTState, noise: Noise | None = None) -> MTState:  # type: ignore[override]
        """``mmtrssm core.py:496-544``."""
        out = scan.mmtrssm_prior_rollout(self, actions, self._state_dict_of(prev_state), noise or {},
                                         rows_per_block=self.scan_rows_per_block, threads=self.scan_threads)
        return MTState(
            deter_h=out["deter_h"], deter_l=out["deter_l"], distribution_h=self.h_dist.unmixed(out["prior_logits_h"]),
            distribution_l=self.l_dist.unmixed(out["prior_logits_l"]), hidden_h=out["hidden_h"], hidden_l=out["hidden_l"],
            stoch_h=out["prior_stoch_h"], stoch_l=out["prior_stoch_l"],
        )

    def _initial_for_step(self, obs_embed: Tensor, noise: Noise | None) -> MTState:  # type: ignore[override]
        return self._initial_from_embed(obs_embed, noise)

    @staticmethod
    def _feature_of(out: dict[str, Tensor]) -> Tensor:
        return torch.cat([out["deter_h"], out["post_stoch_h"], out["deter_l"], out["post_stoch_l"]], dim=-1)

    _POST_KEYS = ("u_post_l", "u_post_h")

    def _category_size_of(self, key: str) -> int:
        return (self.l_dist if key.endswith("_l") else self.h_dist).category_size

    _FRESH_KEYS = ("deter_l", "deter_h", "stoch_l", "stoch_h", "hidden_l", "hidden_h")
    _INIT_KEYS = ("u_init_h", "u_init_l")

    def _latent_levels(self) -> tuple[tuple[str, MultiOneHotFactory], ...]:
        return (("_l", self.l_dist), ("_h", self.h_dist))
    _LAST_KEYS = {"deter_l": "deter_l", "deter_h": "deter_h", "stoch_l": "post_stoch_l", "stoch_h": "post_stoch_h", "hidden_l": "hidden_l",  # noqa: RUF012
                  "hidden_h": "hidden_h"}

    @staticmethod
    def _state_like(fresh: MTState, got: dict[str, Tensor]) -> MTState:  # type: ignore[override]
        return MTState(distribution_h=fresh.distribution_h, distribution_l=fresh.distribution_l, **got)

    def _elbo_step(self, batch: tuple[Tensor, ...], noise: Noise | None, sm: StepMask | None,
                   carry: tuple[StateCarry, str, Tensor] | None = None, schedule: ElboSchedule | None = None,
                   expert_log_weights: Tensor | None = None,
                   overshoot: tuple[LatentOvershoot, Tensor | None, int] | None = None) -> dict[str, Tensor]:
        """``mmtrssm core.py:563-606``: ``loss = recon + kl_coeff KL_l + kl_coeff w_kl_h KL_h`` (``shared_step``'s body)."""
        action_input = batch[0]
        audio_obs, vision_obs = self.get_observations_from_batch(batch)
        conv.begin_step(audio_obs.device)
        audio_embed, vision_embed = self._encode_both(audio_obs, vision_obs)
        state0 = self._initial_from_embed(_masked_mean_embed(audio_embed[:, 0], vision_embed[:, 0], None if sm is None else sm.mask0),
                                          noise)
        state0 = self._state0(state0, carry)
        out = self._rollout_embedded(action_input, audio_embed, vision_embed, state0, noise, sample_prior=False,
                                     modality=None if sm is None else sm.codes, expert_log_weights=expert_log_weights)
        self._save_carry(out, carry, None if sm is None else sm.last)
        feature = torch.cat([out["deter_h"], out["post_stoch_h"], out["deter_l"], out["post_stoch_l"]], dim=-1)
        parts = self._reconstruction_losses(feature, self.get_targets_from_batch(batch), sum_recon=False, step_mask=sm)
        recon, kl_div_l, kl_div_h, loss = _elbo(parts["recon/audio"], parts["recon/vision"], out["kl_l"], float(self.kl_coeff), out["kl_h"],
                                                float(self.kl_coeff * self.w_kl_h), step_mask=sm, schedule=schedule)
        result = {"recon": recon, **parts, "kl": kl_div_l, "kl_h": kl_div_h, "loss": loss}
        if schedule is not None:
            result.update({"kl_raw": schedule.stats["kl_raw"], "kl_h_raw": schedule.stats["kl_h_raw"]})
        if overshoot is not None:
            return self._add_overshoot(result, self._overshoot_terms(action_input, out, noise, overshoot), overshoot[0], schedule)
        return result


def _gate_for(model: MoPoE_MRSSM, mode: str) -> ExpertWeights:
    return ExpertWeights(mode, model.audio_representation.obs_embed_size if mode == "gated" else None)


class WeightedMoPoE_MRSSM(MoPoE_MRSSM):  # noqa: N801
    """``MoPoE_MRSSM`` with learned weights of the (audio, vision, fused) experts: the class a YAML names,
    ``init_args`` gaining ``expert_weights: gated`` (a gate on the two embeddings of a frame) or ``static`` (one learned triple)."""

    def __init__(self, *, expert_weights: str = "gated", **kw) -> None:  # noqa: ANN003
        super().__init__(**kw)
        self.expert_weights = _gate_for(self, expert_weights)


class WeightedMoPoE_MMTRSSM(MoPoE_MMTRSSM):  # noqa: N801
    """``MoPoE_MMTRSSM`` with learned expert weights on the lower level's mixture; ``expert_weights`` as ``WeightedMoPoE_MRSSM``."""

    def __init__(self, *, expert_weights: str = "gated", **kw) -> None:  # noqa: ANN003
        super().__init__(**kw)
        self.expert_weights = _gate_for(self, expert_weights)


__all__ = ["MoPoE_MMTRSSM", "MoPoE_MRSSM", "WeightedMoPoE_MMTRSSM", "WeightedMoPoE_MRSSM", "check_ragged_rows", "kl_divergence"]
