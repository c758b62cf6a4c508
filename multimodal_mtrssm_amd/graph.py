"""The whole train step as ONE captured hipGraph.

One MoPoE-MRSSM train step is a chain of a few hundred small dependent launches (encoders, the scan,
decoders, their backward, the optimizer); enqueued one by one the host needs about as long as the GPU
(DESIGN.md section 4).  ``CapturedTrainStep`` records

    zero_grad -> shared_step -> backward [-> clip + AdamW when there is one rank]

once (``torch.cuda.graph`` = ``hipStreamBeginCapture`` on a side stream; the library's launches go to torch's
current stream, so they are captured like torch's own) and replays it with one ``hipGraphLaunch`` per step.
What makes that legal here:

* every scalar the kernels need lives in device memory (``FlatAdamW.state``: learning rate, step count, bias
  corrections), so nothing is frozen into the graph that changes between steps;
* the sampling uniforms are drawn OUTSIDE the graph into fixed buffers (``GlobalRowNoise.draw(out=...)``) and the
  batch is copied into fixed buffers, which the captured kernels read;
* the conv layer's zeroed accumulation chunks and packed-weight buffers are (re)created inside the capture
  (``conv.reset_scratch``), so each replay starts from the state the capture started from.

Masked steps are captured in one of two modes, fixed for the graph's life:

* ``modality_dropout=``: the ``u_mask`` uniforms are drawn outside the graph with the others; the sampler launch and everything
  downstream of it is inside, so every replay trains on a fresh mask with no host round trip;
* ``masked=True``: batches are 7-tuples; ``step`` validates the mask's t = 0 frame on the host and copies the mask into a fixed
  buffer, from which the captured region derives the scans' codes and the NLL's planes.

``state_carry=`` adds truncated BPTT to any of the three: ``step`` checks the carry's host rules on the
batch's ``reset_host`` and copies ``batch.reset`` into a fixed buffer; ``mtrssm_state_select`` and ``mtrssm_state_save`` are inside
the graph and read ``reset`` on the device, so ONE graph serves the first chunk of an episode and every later one.

``ragged=True`` captures the step over episodes of different lengths, alone or with ``modality_dropout=`` and
``state_carry=``: batches carry ``valid`` (an ``EpisodeBatch`` of a loader with lengths); ``step`` checks on the host that no row
resets with nothing at t = 0 and copies ``valid_global`` into a fixed buffer; the mask launch, the counted ELBO epilogue and the
save at each row's last live step are inside the graph.  A graph is ragged or not for life.

``forecast=`` captures the forecast objective, alone or with ``modality_dropout=`` and ``ragged=True``: the
``u_context`` uniforms are drawn outside the graph into a fixed buffer with the others; the sampler launch and everything behind it is
inside, so every replay trains on freshly sampled contexts.  It does not combine with ``masked=True`` (a caller's mask already says
what is seen) nor with ``state_carry=`` (the state such a step ends with is an open-loop state).

``elbo_schedule=`` weighs the loss terms inside the capture, with every mode above: the schedule is bound to the
optimizer's device-resident count of steps taken, which the captured epilogue reads, so every replay sees its own beta (the warm-up
steps of the construction put that count back with the rest of ``opt.state``).

``overshoot=`` captures the latent-overshooting term with every mode above except ``forecast=``: the
``u_overshoot`` uniforms are drawn outside the graph into fixed buffers with the others; the gather, the overshoot rows' scan and the
KL pair are inside.

Observations that are ``None`` stay eager-only: a capture cannot drop an encoder per step.

With more than one rank the gradient all-reduce (RCCL) and the optimizer run eagerly after the replay: the
exchange stays a plain ``torch.distributed`` call.
"""

from __future__ import annotations

import torch
from torch import Tensor

from multimodal_mtrssm_amd import conv, scan
from multimodal_mtrssm_amd.carry import StateCarry
from multimodal_mtrssm_amd.core import _check_modality_mask, check_ragged_rows
from multimodal_mtrssm_amd.dropout import ModalityDropout, StepMask
from multimodal_mtrssm_amd.forecast import Forecast
from multimodal_mtrssm_amd.optim import FlatAdamW, FlatParameters
from multimodal_mtrssm_amd.overshoot import LatentOvershoot
from multimodal_mtrssm_amd.parallel import FlatDataParallel, GlobalRowNoise
from multimodal_mtrssm_amd.schedule import ElboSchedule


def _refuse_modality_mask(model: torch.nn.Module, batch: tuple[Tensor, ...]) -> None:
    """The captured step runs the unmasked kernels: a batch that carries a modality mask (7th entry) would be trained as if
    every modality were present.  Refused instead (run such batches eagerly: ``model.shared_step``)."""
    if model.get_modality_mask_from_batch(batch) is not None:
        msg = ("CapturedTrainStep without masked=True does not take a modality mask (a 7-tuple batch): capture with masked=True "
               "(or modality_dropout=), or train masked batches with the eager step")
        raise NotImplementedError(msg)


class CapturedTrainStep:
    """``step(batch)`` = one train step of ``model`` on a batch of the captured shape; returns the loss scalars
    (device tensors, averaged over ranks) exactly as the eager sequence would.

    Construction runs ``warmup`` real steps on the capture stream (every lazy allocation, plan entry and workspace must
    exist before the capture) and then puts parameters, Adam moments, the device-side step count and the noise generator
    BACK where they were: a run with the graph is step for step the eager run.  ``close()`` (or garbage collection) releases
    the pin on the conv layer's packed-weight plan.

    ``modality_dropout`` (a ``ModalityDropout``) or ``masked=True`` capture the masked step (module docstring); the graph then
    takes only that kind of batch, an unmasked graph only 6-tuples.

    ``state_carry`` (a ``StateCarry`` of the batch's rows): the step continues its ``"train"`` set (module docstring).  The warm-up
    steps reset every row and leave the carry as they found it; a carry that was empty is empty after construction.

    ``elbo_schedule`` (an ``ElboSchedule``): the constructor calls ``elbo_schedule.bind(opt)`` on the CALLER's object -- whatever it
    was bound to or set to before, it reads this optimizer's steps taken from now on.  Its ``stats`` are tensors of the graph's
    memory, rewritten by every replay and valid while the capture lives; ``close()`` empties them."""

    def __init__(self, model: torch.nn.Module, flat: FlatParameters, opt: FlatAdamW, dp: FlatDataParallel,  # noqa: PLR0913
                 batch: tuple[Tensor, ...], noise: GlobalRowNoise, *, warmup: int = 3,
                 modality_dropout: ModalityDropout | None = None, masked: bool = False, state_carry: StateCarry | None = None,
                 ragged: bool = False, forecast: Forecast | None = None, elbo_schedule: ElboSchedule | None = None,
                 overshoot: LatentOvershoot | None = None) -> None:
        if state_carry is not None and not isinstance(state_carry, StateCarry):
            msg = f"state_carry must be a StateCarry, got {type(state_carry).__name__}"
            raise ValueError(msg)
        if modality_dropout is not None and masked:
            msg = "give modality_dropout= (the graph samples its masks) or masked=True (the batches carry them), not both"
            raise ValueError(msg)
        if modality_dropout is not None and not isinstance(modality_dropout, ModalityDropout):
            msg = f"modality_dropout must be a ModalityDropout, got {type(modality_dropout).__name__}"
            raise ValueError(msg)
        if ragged and masked:
            msg = "ragged=True builds its masks from the batch's lengths: it does not combine with masked=True"
            raise ValueError(msg)
        if forecast is not None and not isinstance(forecast, Forecast):
            msg = f"forecast must be a Forecast, got {type(forecast).__name__}"
            raise ValueError(msg)
        if forecast is not None and masked:
            msg = "forecast= decides what the model observes: it does not combine with masked=True (the batches' masks already say what is seen)"
            raise ValueError(msg)
        if forecast is not None and state_carry is not None:
            msg = "forecast= does not combine with state_carry=: the state a forecast step ends with is an open-loop state"
            raise ValueError(msg)
        if overshoot is not None and not isinstance(overshoot, LatentOvershoot):
            msg = f"overshoot must be a LatentOvershoot, got {type(overshoot).__name__}"
            raise ValueError(msg)
        if overshoot is not None and forecast is not None:
            msg = "overshoot= does not combine with forecast=: the states of a forecast step's tail are not posteriors"
            raise ValueError(msg)
        if elbo_schedule is not None and not isinstance(elbo_schedule, ElboSchedule):
            msg = f"elbo_schedule must be an ElboSchedule, got {type(elbo_schedule).__name__}"
            raise ValueError(msg)
        self.model, self.masked, self.dropout, self.ragged = model, bool(masked), modality_dropout, bool(ragged)
        self.schedule = None if elbo_schedule is None else elbo_schedule.bind(opt)  # (beta follows opt.state[1], read on the device)
        self.forecast = None if forecast is None else forecast.for_rank(dp.world, dp.rank)
        self.overshoot = None if overshoot is None else overshoot.for_rank(dp.world, dp.rank)
        self._check_batch_kind(batch)
        self.flat, self.opt, self.dp, self.noise = flat, opt, dp, noise
        b, t = batch[0].shape[:2]
        dev = batch[0].device
        self.mask: Tensor | None = None
        if self.masked:
            _check_modality_mask(batch[6], b, t, dev, first_step=True)
            self.mask = batch[6].clone()
        self.batch = tuple(x.clone() for x in batch[:6])
        self.carry = state_carry
        self.reset: Tensor | None = None
        if state_carry is not None:
            state_carry.check("train", b, torch.ones(b, dtype=torch.bool))  # (the batch size; the warm-up resets every row)
            self.reset = torch.ones(b, dtype=torch.bool, device=dev)
        self.valid_global: Tensor | None = None
        if self.ragged:
            check_ragged_rows(self._valid_host(batch), None)  # (the warm-up resets every row)
            if batch.valid_global.numel() != b * dp.world:
                msg = f"the batch's valid_global has {batch.valid_global.numel()} rows, the global batch {b} x {dp.world}"
                raise ValueError(msg)
            self.valid_global = batch.valid_global.to(dev, torch.int32).clone()
        self.shapes = dict(model.noise_shapes(b, t))
        if self.dropout is not None:
            self.dropout = self.dropout.for_rank(dp.world, dp.rank)
            self.shapes["u_mask"] = self.dropout.noise_shape(b, t)
        if self.forecast is not None:
            self.shapes["u_context"] = self.forecast.noise_shape(b)
        if self.overshoot is not None:
            for key in model._POST_KEYS:  # noqa: SLF001
                self.shapes[model._overshoot_key(key)] = self.overshoot.noise_shape(b, t, model._category_size_of(key))  # noqa: SLF001
        # (a GLOBAL_KEYS entry keeps the rows of every rank: GlobalRowNoise.draw)
        self.uniforms = {k: torch.empty((s[0] * noise.world if k in noise.GLOBAL_KEYS else s[0], *s[1:]), device=dev, dtype=torch.float32)
                         for k, s in self.shapes.items()}
        self.fused_optimizer = dp.world == 1
        self.keys: list[str] = []
        self.graph: torch.cuda.CUDAGraph | None = None
        self._capture(warmup)

    def _check_batch_kind(self, batch: tuple[Tensor, ...]) -> None:
        """A graph is masked or unmasked for life: refuse the other kind of batch, and ``None`` observations always."""
        if batch[1] is None or batch[2] is None:
            msg = "CapturedTrainStep needs both observations: a None modality is eager-only (a capture cannot drop an encoder per step)"
            raise ValueError(msg)
        has_mask = self.model.get_modality_mask_from_batch(batch) is not None
        if self.masked and not has_mask:
            msg = "this CapturedTrainStep was captured with masked=True: every batch must be a 7-tuple carrying its modality mask"
            raise ValueError(msg)
        if self.dropout is not None and has_mask:
            msg = "this CapturedTrainStep samples its modality masks (modality_dropout=): it takes 6-tuple batches without a mask"
            raise ValueError(msg)
        if self.forecast is not None and has_mask:
            msg = "this CapturedTrainStep samples what is observed (forecast=): it takes 6-tuple batches without a mask"
            raise ValueError(msg)
        if not self.masked and self.dropout is None and self.forecast is None:
            _refuse_modality_mask(self.model, batch)
        has_valid = getattr(batch, "valid", None) is not None
        if self.ragged and not has_valid:
            msg = "this CapturedTrainStep was captured with ragged=True: every batch must carry valid (an EpisodeBatch of a loader with lengths)"
            raise ValueError(msg)
        if not self.ragged and has_valid:
            msg = "this CapturedTrainStep was captured without ragged=True: it does not take a batch that carries valid"
            raise ValueError(msg)

    @staticmethod
    def _valid_host(batch: tuple[Tensor, ...]) -> Tensor:
        valid_host = getattr(batch, "valid_host", None)
        if valid_host is None:
            msg = "a ragged CapturedTrainStep needs the batch's valid_host (the loader makes it): the t = 0 rule is checked on the host"
            raise ValueError(msg)
        return valid_host

    # the captured region -------------------------------------------------------------------------
    def _body(self) -> list[str]:
        self.opt.zero_grad()
        carry = None if self.carry is None else (self.carry, "train", self.reset)  # (its host rules were checked by step())
        plan = None  # (the overshoot term's rows: this rank's of the global batch, whose lengths a ragged graph holds)
        if self.overshoot is not None:
            plan = (self.overshoot, self.valid_global if self.ragged else None, self.dp.rank * self.batch[0].shape[0])
        if self.masked:  # (validated on the host by step(); codes, planes and counts are derived here, inside the capture)
            out = self.model._elbo_step(self.batch, self.uniforms, StepMask.from_mask(self.mask), carry, self.schedule, overshoot=plan)  # noqa: SLF001
        elif self.forecast is not None:  # (a ragged batch's host rule was checked by step(); context AND lengths AND dropout in one launch)
            ragged = (self.valid_global, self.dp.world, self.dp.rank) if self.ragged else None
            sm = self.model._forecast_step_mask(self.batch, self.uniforms, self.forecast, self.dropout, ragged=ragged)  # noqa: SLF001
            out = self.model._elbo_step(self.batch, self.uniforms, sm, schedule=self.schedule)  # noqa: SLF001
        elif self.ragged:  # (the host rule was checked by step(); lengths AND dropout in one launch, inside the capture)
            sm = self.model._ragged_step_mask(self.batch, self.uniforms, self.dropout, self.valid_global, self.dp.world, self.dp.rank)  # noqa: SLF001
            out = self.model._elbo_step(self.batch, self.uniforms, sm, carry, self.schedule, overshoot=plan)  # noqa: SLF001
        elif carry is not None:
            sm = self.model._step_mask(self.batch, self.uniforms, None, self.dropout)  # noqa: SLF001
            out = self.model._elbo_step(self.batch, self.uniforms, sm, carry, self.schedule, overshoot=plan)  # noqa: SLF001
        else:
            out = self.model.shared_step(self.batch, self.uniforms, modality_dropout=self.dropout, elbo_schedule=self.schedule,
                                         overshoot=self.overshoot)
        out["loss"].backward()
        keys = list(out)
        if self.fused_optimizer:
            self.dp.sync({k: out[k] for k in keys})  # one rank: only the scalars' copies into the gradient buffer's tail
            self.opt.step(grad_scale=self.dp.grad_scale, check=False)
        else:
            self.dp.stage_scalars({k: out[k] for k in keys})
        return keys

    def _tail(self) -> None:
        if not self.fused_optimizer:
            self.dp.reduce()
            self.opt.step(grad_scale=self.dp.grad_scale, check=False)

    def _capture(self, warmup: int) -> None:
        dev = self.batch[0].device
        # the warm-up steps are real steps: snapshot what they change and restore it afterwards
        snap = (self.flat.param.clone(), self.opt.exp_avg.clone(), self.opt.exp_avg_sq.clone(), self.opt.state.clone(), self.opt.steps,
                self.noise.gen.get_state(), None if self.carry is None else self.carry.snapshot())
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(1, warmup)):  # eager steps on the capture stream: every lazy allocation / plan entry exists
                self.noise.draw(self.shapes, out=self.uniforms)
                self.opt.sync_lr()
                self._body()
                self._tail()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            self.flat.param.copy_(snap[0])
            self.opt.exp_avg.copy_(snap[1])
            self.opt.exp_avg_sq.copy_(snap[2])
            self.opt.state.copy_(snap[3])
        self.opt.steps = snap[4]
        self.noise.gen.set_state(snap[5])
        if self.carry is not None:  # the warm-up steps saved their last posterior: put the carry back (an empty one is empty again)
            self.carry.restore(snap[6])
        conv.invalidate_packs()
        scan.STATUS.check()  # a warm-up step whose cooperative scan gave up must not be captured
        self.flat.check_views()
        self.opt.active_mask()  # built from what the warm-up steps touched; a fixed buffer from here on
        self.opt.sync_lr()  # (no draw here: the recorded step is not executed, and a draw would shift the stream of uniforms)
        conv.reset_scratch(pin=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            self.keys = self._body()
        if self.carry is not None:  # (the recorded, not executed, save marked the set filled on the host)
            self.carry.filled = dict(snap[6][1])
        conv.reset_scratch()
        self._pinned = True
        self.graph = graph  # capture records, it does not execute: the first step() runs it
        if self.fused_optimizer:
            self.opt.steps -= 1  # FlatAdamW.step counted the recorded (not executed) step on the host

    def close(self) -> None:
        """Drop the graph and the pin it holds on the conv layer's packed-weight plan; the schedule's ``stats`` (tensors of the graph's
        memory) are emptied."""
        self.graph = None
        if getattr(self, "schedule", None) is not None:
            self.schedule.stats = {}
        if getattr(self, "_pinned", False):
            self._pinned = False
            conv.unpin_scratch()

    def __del__(self) -> None:
        self.close()

    # one step ---------------------------------------------------------------------------------------
    def step(self, batch: tuple[Tensor, ...] | None = None) -> dict[str, Tensor]:
        scan.STATUS.poll()  # a cooperative scan launch of an earlier replay gave up (the device skipped that update): raise
        if batch is not None:
            self._check_batch_kind(batch)
            if self.masked:  # the t = 0 check reads the mask back: here, before the replay, never inside the capture
                _check_modality_mask(batch[6], *self.batch[0].shape[:2], self.batch[0].device, first_step=True)
        if self.ragged and batch is not None:  # host rule first: a row that resets with no valid frame raises before anything is replayed
            check_ragged_rows(self._valid_host(batch), None if self.carry is None else getattr(batch, "reset_host", None))
            if tuple(batch.valid_global.shape) != tuple(self.valid_global.shape):
                msg = f"valid_global must have shape {tuple(self.valid_global.shape)}, got {tuple(batch.valid_global.shape)}"
                raise ValueError(msg)
        if self.carry is not None:  # host rules first: a partial reset into an empty carry raises before anything is replayed
            reset = getattr(batch, "reset", None)
            if reset is None:
                msg = "this CapturedTrainStep carries state: step() needs an EpisodeBatch (its reset says which rows start an episode)"
                raise ValueError(msg)
            self.carry.check("train", reset.shape[0], getattr(batch, "reset_host", None))
            self.reset.copy_(reset)
        if batch is not None and batch[0] is not self.batch[0]:
            for dst, src in zip(self.batch, batch[:6], strict=True):
                dst.copy_(src)
        if batch is not None and self.masked and batch[6] is not self.mask:
            self.mask.copy_(batch[6])
        if batch is not None and self.ragged:
            self.valid_global.copy_(batch.valid_global)
        self.noise.draw(self.shapes, out=self.uniforms)
        self.opt.sync_lr()
        assert self.graph is not None
        self.graph.replay()
        if self.carry is not None:
            self.carry.filled["train"] = True  # host mirror of the replayed save
        self._tail()
        self.opt.steps += 1 if self.fused_optimizer else 0  # host mirror of the device-side step count
        scan.STATUS.post()
        if self.dp.world == 1:
            return {k: self.flat.tail[i] for i, k in enumerate(self.keys)}
        return {k: self.flat.tail[i] / self.dp.world for i, k in enumerate(self.keys)}
