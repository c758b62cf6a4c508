"""How the terms of the ELBO are weighed: KL free bits, a beta warm-up, per-modality reconstruction weights.

The rule (``ElboSchedule.reference`` is its statement in torch, ``mtrssm_elbo_schedule_fwd / _bwd`` the kernels).  Inputs of a step: the
scalars ``nll_a``, ``nll_v``; the per-(b, t) planes ``kl_0`` (MRSSM ``kl`` / MMTRSSM ``kl_l``) and ``kl_1`` (MMTRSSM ``kl_h``) of ``n = B * T``
entries with their coefficients ``c_0 = kl_coeff``, ``c_1 = kl_coeff * w_kl_h``; optionally ``live`` in {0, 1} and the device scalar
``count`` of a ``StepMask`` (``N = count``; without them every step is live and ``N = n``); the device scalar ``step``, the optimizer steps
taken so far.  Every operand is an fp32 value and every operation is rounded on its own::

    beta      = 1 if warmup_steps == 0 else beta_start + (1 - beta_start) * min(step / warmup_steps, 1)
    recon     = w_a * nll_a + w_v * nll_v
    clip_j[i] = free_j if kl_j[i] < free_j else kl_j[i]
    k_j       = (sum over live i of clip_j[i]) / N * c_j * beta          (0 when N <= 0)
    raw_j     = (sum over live i of kl_j[i]) / N * c_j                   (the unscheduled term; not differentiable)
    active_j  = #{live i: not kl_j[i] < free_j} / N                      (not differentiable)
    loss      = recon + k_0 + k_1

    g_nll_a   = w_a * (g_recon + g_loss),   g_nll_v = w_v * (g_recon + g_loss)
    g_kl_j[i] = (g_k_j + g_loss) * c_j * beta / N   where live[i] and not kl_j[i] < free_j, an explicit 0 elsewhere and when N <= 0

The free nats act per (b, t) on the step's KL summed over its categoricals: element-wise, so sharding the batch changes nothing.  The
tie ``kl == free`` passes the gradient, as ``torch.where(kl < free, free, kl)`` does.  ``beta`` is decided on the device: bound to
``FlatAdamW.state[1:2]`` one captured graph serves the whole warm-up, a step the optimizer skipped does not advance it, and
``FlatAdamW.load_state_dict`` resumes it.  With all defaults the rule is the plain ELBO epilogue, bit for bit.
"""

from __future__ import annotations

import math
from typing import NamedTuple

import torch
from torch import Tensor

_MAX_WARMUP = 1 << 24  # every step count below it is an exact fp32 value


class ElboTerms(NamedTuple):
    """One step under the rule: the four loss scalars of the epilogue, the ``beta`` it used and the statistics (no gradient)."""

    recon: Tensor
    k0: Tensor
    k1: Tensor
    loss: Tensor
    beta: Tensor
    raw0: Tensor
    raw1: Tensor
    active0: Tensor
    active1: Tensor


def _f32(x: float, device: torch.device) -> Tensor:
    return torch.tensor(float(x), dtype=torch.float32, device=device)


class _Rule(torch.autograd.Function):
    """The rule in torch operations, each rounded on its own; its backward is the rule's own formula (not autograd's chain), so the
    gradient planes are the kernel's bit for bit."""

    @staticmethod
    def forward(ctx, nll_a, nll_v, kl0, kl1, live, count, step, sched, c0, c1):  # noqa: ANN001, ANN205, PLR0913
        ctx.set_materialize_grads(False)
        dev = kl0.device
        f = lambda x: _f32(x, dev)  # noqa: E731
        zero, one = f(0.0), f(1.0)
        nll_a, nll_v, kl0 = nll_a.float(), nll_v.float(), kl0.float()
        kl1 = None if kl1 is None else kl1.float()
        if live is None:
            on, cnt = None, f(kl0.numel())
        else:
            on, cnt = live.reshape(kl0.shape) != 0, count.reshape(()).float()
        some = cnt > 0
        if sched.warmup_steps == 0:
            beta = one.clone()
        else:
            r = step.reshape(()).float() / f(sched.warmup_steps)
            beta = f(sched.beta_start) + (one - f(sched.beta_start)) * torch.where(r > one, one, r)
        w_a, w_v = (f(w) for w in sched.recon_weights)
        recon = w_a * nll_a + w_v * nll_v

        def term(kl: Tensor | None, free: float, c: float) -> tuple[Tensor, Tensor, Tensor, Tensor | None]:
            if kl is None:
                return zero.clone(), zero.clone(), zero.clone(), None
            low = kl < f(free)
            clip = torch.where(low, f(free), kl)
            keep = ~low if on is None else on & ~low
            s_clip = (clip if on is None else torch.where(on, clip, zero)).sum()
            s_raw = (kl if on is None else torch.where(on, kl, zero)).sum()
            k = torch.where(some, s_clip / cnt * f(c) * beta, zero)
            raw = torch.where(some, s_raw / cnt * f(c), zero)
            active = torch.where(some, keep.sum().float() / cnt, zero)
            return k, raw, active, keep

        k0, raw0, active0, keep0 = term(kl0, sched.free_nats, c0)
        k1, raw1, active1, keep1 = term(kl1, sched.free_nats_h, c1)
        loss = recon + k0 + k1
        ctx.save_for_backward(keep0, keep1, cnt, beta)
        ctx.consts = (w_a, w_v, f(c0), f(c1))
        ctx.mark_non_differentiable(beta, raw0, raw1, active0, active1)
        return recon, k0, k1, loss, beta, raw0, raw1, active0, active1

    @staticmethod
    def backward(ctx, g_recon, g_k0, g_k1, g_loss, *_):  # noqa: ANN001, ANN002, ANN205
        keep0, keep1, cnt, beta = ctx.saved_tensors
        w_a, w_v, c0, c1 = ctx.consts
        zero = torch.zeros((), dtype=torch.float32, device=cnt.device)
        opt = lambda g: zero if g is None else g.float()  # noqa: E731
        gl = opt(g_loss)
        gn = opt(g_recon) + gl

        def plane(keep: Tensor | None, g_k: Tensor | None, c: Tensor) -> Tensor | None:
            if keep is None:
                return None
            v = torch.where(cnt > 0, (opt(g_k) + gl) * c * beta / cnt, zero)
            return torch.where(keep, v, zero)

        return w_a * gn, w_v * gn, plane(keep0, g_k0, c0), plane(keep1, g_k1, c1), None, None, None, None, None, None


class ElboSchedule:
    """``ElboSchedule(free_nats, free_nats_h, beta_start, warmup_steps, recon_weights)``: the KL of a step below ``free_nats`` (MMTRSSM's
    higher level: ``free_nats_h``) is held at the threshold and gets no gradient; the KL terms are scaled by ``beta``, which rises
    linearly from ``beta_start`` to 1 over ``warmup_steps`` optimizer steps (0: no warm-up, beta = 1); the audio and vision NLL are
    weighted ``recon_weights = (w_a, w_v)``.  The defaults are the plain ELBO.

    ``bind(opt)`` takes ``FlatAdamW``'s device-resident count of steps taken as ``step`` (a view: a captured graph sees a new beta on
    every replay); ``set_step(k)`` fills an own tensor for callers without one.  ``stats`` holds the last step's device tensors
    ``beta``, ``active`` and ``active_h`` (the fraction of live steps at or above the threshold); nothing is read back.  The stats of
    a captured step live in the graph's memory: ``CapturedTrainStep.close()`` empties ``stats``."""

    def __init__(self, free_nats: float = 0.0, free_nats_h: float = 0.0, beta_start: float = 1.0, warmup_steps: int = 0,  # noqa: PLR0913
                 recon_weights: tuple[float, float] = (1.0, 1.0)) -> None:
        for name, v in (("free_nats", free_nats), ("free_nats_h", free_nats_h)):
            if not self._number(v) or not math.isfinite(v) or v < 0.0:
                msg = f"{name} must be a finite number >= 0, got {v!r}"
                raise ValueError(msg)
        if not self._number(beta_start) or not 0.0 <= beta_start <= 1.0:
            msg = f"beta_start must lie in [0, 1], got {beta_start!r}"
            raise ValueError(msg)
        if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or not 0 <= warmup_steps < _MAX_WARMUP:
            msg = f"warmup_steps must be an integer with 0 <= warmup_steps < 2^24, got {warmup_steps!r}"
            raise ValueError(msg)
        weights = tuple(recon_weights) if isinstance(recon_weights, (tuple, list)) else ()
        if len(weights) != 2 or any(not self._number(w) or not math.isfinite(w) or w < 0.0 for w in weights):  # noqa: PLR2004
            msg = f"recon_weights must be a pair of finite numbers >= 0 (audio, vision), got {recon_weights!r}"
            raise ValueError(msg)
        self.free_nats, self.free_nats_h = float(free_nats), float(free_nats_h)
        self.beta_start, self.warmup_steps = float(beta_start), warmup_steps
        self.recon_weights = (float(weights[0]), float(weights[1]))
        self.stats: dict[str, Tensor] = {}
        self._step: Tensor | None = None
        self._own = False  # (the step tensor is this schedule's own, filled by set_step)

    @staticmethod
    def _number(v: object) -> bool:
        return isinstance(v, (int, float)) and not isinstance(v, bool)

    def __repr__(self) -> str:
        return (f"ElboSchedule(free_nats={self.free_nats}, free_nats_h={self.free_nats_h}, beta_start={self.beta_start}, "
                f"warmup_steps={self.warmup_steps}, recon_weights={self.recon_weights})")

    # -- the step count ---------------------------------------------------------------------------
    def bind(self, opt: object) -> ElboSchedule:
        """Read ``step`` from ``opt.state[1:2]``, ``FlatAdamW``'s "steps taken" on the device: a view, not a copy."""
        state = getattr(opt, "state", None)
        if not isinstance(state, Tensor) or state.dtype != torch.float32 or state.dim() != 1 or state.numel() < 2:  # noqa: PLR2004
            msg = f"bind needs an optimizer with the device-resident state of FlatAdamW (float32 [lr, steps taken, ...]), got {type(opt).__name__}"
            raise ValueError(msg)
        self._step, self._own = state[1:2], False
        return self

    def set_step(self, k: int, device: torch.device | str | None = None) -> ElboSchedule:
        """For callers without a ``FlatAdamW``: ``step = k`` in an own tensor, filled eagerly (not inside a graph capture)."""
        if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k < _MAX_WARMUP:
            msg = f"step must be an integer with 0 <= step < 2^24, got {k!r}"
            raise ValueError(msg)
        if self._own and self._step is not None and (device is None or self._same_device(self._step.device, torch.device(device))):
            self._step.fill_(float(k))  # (the SAME tensor: a graph captured on it sees the new value)
        else:
            self._step, self._own = torch.full((1,), float(k), dtype=torch.float32, device=device or "cpu"), True
        return self

    @staticmethod
    def _same_device(have: torch.device, want: torch.device) -> bool:
        """``want`` names the device ``have`` is on; an index left out ("cuda") stands for the current device of that type."""
        if have.type != want.type:
            return False
        if want.index is None or have.index is None:
            index = torch.cuda.current_device() if have.type == "cuda" else 0
            return (index if have.index is None else have.index) == (index if want.index is None else want.index)
        return have.index == want.index

    def step_on(self, device: torch.device) -> Tensor | None:
        """The ``step`` scalar the epilogue on ``device`` reads; None without a warm-up (nothing is read then)."""
        if self.warmup_steps == 0:
            return None
        if self._step is None:
            msg = "warmup_steps > 0 needs the steps taken so far: bind(opt) to a FlatAdamW, or set_step(k)"
            raise ValueError(msg)
        if not self._same_device(self._step.device, torch.device(device)):
            if not self._own:
                msg = f"the schedule is bound to an optimizer on {self._step.device}, the step runs on {device}"
                raise ValueError(msg)
            self._step = self._step.to(device)
        return self._step

    # -- the rule ------------------------------------------------------------------------------------
    def reference(self, nll_a: Tensor, nll_v: Tensor, kl0: Tensor, c0: float, kl1: Tensor | None = None, c1: float = 0.0,  # noqa: PLR0913
                  live: Tensor | None = None, count: Tensor | None = None, step: Tensor | None = None) -> ElboTerms:
        """The rule in torch, on any device, differentiable in the NLLs and the KL planes.  ``step`` defaults to the bound one."""
        if (live is None) != (count is None):
            msg = "live and count come together (neither: every step is live)"
            raise ValueError(msg)
        if step is None:
            step = self.step_on(kl0.device)
        return ElboTerms(*_Rule.apply(nll_a, nll_v, kl0, kl1, live, count, step, self, float(c0), float(c1)))

    def record(self, terms: ElboTerms, *, higher: bool) -> None:
        """Keep the last step's ``beta`` / ``active`` (/ ``active_h``) and its unscheduled KL terms, all device tensors."""
        self.stats = {"beta": terms.beta, "active": terms.active0, "kl_raw": terms.raw0}
        if higher:
            self.stats.update({"active_h": terms.active1, "kl_h_raw": terms.raw1})


__all__ = ["ElboSchedule", "ElboTerms"]
