"""The evaluation steps of the models: forecast skill, word transitions, held-out likelihood, latent
probes, episode panels, the latent census, the Frechet distance of sampled frames and the coherence of the two generated modalities.

Every one of them runs ONE masked posterior rollout over ``B x copies`` rows and then scores it.  What differs between them is what a
copy of a row is -- what it observes, up to which frame, whether it shares the row's uniforms, where it lies among the scan's rows -- and
that is a ``CopyPlan``, which every config object builds for itself (``ForecastSkill.plan()`` ...).  ``_Evaluators._evaluation_rollout``
turns a batch and a plan into the scan's outputs; the public methods are a guard, that rollout and a scorer.  A new evaluator adds a
plan and a scorer, not a rollout.

``_Evaluators`` is a mixin of ``core.MoPoE_MRSSM`` and reaches the model through ``self`` only; this module does not import ``core``.
"""

from __future__ import annotations

from collections.abc import Callable, Iterator
from dataclasses import dataclass

import torch
from torch import Tensor

from multimodal_mtrssm_amd import cnn, conv, digits, frechet, linear
from multimodal_mtrssm_amd._shared import _check_lengths, _masked_mean_embed, _pairable, _rand
from multimodal_mtrssm_amd.census import CensusTable, LatentCensus
from multimodal_mtrssm_amd.coherence import CoherenceTable, GenerationCoherence
from multimodal_mtrssm_amd.digits import DigitClassifier, word_counts
from multimodal_mtrssm_amd.distributions import MultiOneHotFactory
from multimodal_mtrssm_amd.forecast import Forecast
from multimodal_mtrssm_amd.frechet import FrechetDistance, FrechetTable
from multimodal_mtrssm_amd.likelihood import PLANES as LIKELIHOOD_PLANES
from multimodal_mtrssm_amd.likelihood import LikelihoodBound, LikelihoodTable
from multimodal_mtrssm_amd.panel import EpisodePanel, EpisodeVideo
from multimodal_mtrssm_amd.particle import PLANES as PARTICLE_PLANES
from multimodal_mtrssm_amd.particle import ParticleFilter, ParticleTable
from multimodal_mtrssm_amd.probe import LatentProbe, LinearProbe, ProbeTable, frame_labels
from multimodal_mtrssm_amd.skill import ForecastSkill, SkillTable, observed_bits
from multimodal_mtrssm_amd.words import TransitionTable, WordTransitions

Noise = dict[str, Tensor | None]
_LAYOUTS = {"init": ("row", "copy"), "post": ("row", "copy", "tail", "prior"), "order": ("row", "copy")}


@dataclass(frozen=True)
class CopyPlan:
    """What the copies of a row are in an evaluation rollout over ``B * copies`` rows.

    ``bits``: the modality code an observed step of a copy sees (bit 0 audio, bit 1 vision) -- one for all copies, or one per copy.
    ``context``: the frames a copy observes (None: every live frame; more than ``T``: as ``T``) -- one for all copies, or one per copy.
    ``init``: ``"row"`` the copies share the row's initial uniforms ``(B, K)``, ``"copy"`` each has its own ``(B, S, K)``.
    ``post``: ``"row"`` shared posterior uniforms ``(B, T, K)``; ``"copy"`` own ``(B, S, T, K)``; ``"tail"`` shared on the context, own
    ``u_tail (B, S, T, K)`` after it; ``"prior"`` no posterior step at all: own ``u_prior (B, S, 1, K)`` for one prior step (the reference
    protocol of ``word_transitions``).  ``order``: ``"row"`` copy ``s`` of row ``b`` is scan row ``b * S + s``, ``"copy"`` it is
    ``s * B + b``.  Everything here is plain torch on any device."""

    copies: int
    bits: int | tuple[int, ...]
    context: int | None | tuple[int | None, ...]
    init: str = "row"
    post: str = "row"
    order: str = "row"

    def __post_init__(self) -> None:
        for name, allowed in _LAYOUTS.items():
            if getattr(self, name) not in allowed:
                msg = f"{name} must be one of {allowed}, got {getattr(self, name)!r}"
                raise ValueError(msg)
        if self.copies < 1 or any(isinstance(v, tuple) and len(v) != self.copies for v in (self.bits, self.context)):
            msg = f"need copies >= 1 and one entry per copy, got {self}"
            raise ValueError(msg)
        if self.post == "tail" and not isinstance(self.context, int):
            msg = f"tail uniforms begin after ONE context, got {self.context!r}"
            raise ValueError(msg)

    def per_copy(self, value):  # noqa: ANN001, ANN201
        """``value`` (``bits`` or ``context``) as a tuple with one entry per copy."""
        return value if isinstance(value, tuple) else (value,) * self.copies

    @property
    def contexts(self) -> tuple[int | None, ...]:
        """The DISTINCT contexts, in the order of their first copy: one ``Forecast.sample`` launch each."""
        return tuple(dict.fromkeys(self.per_copy(self.context)))

    @property
    def shares_frame0(self) -> bool:
        """The copies of a row see the same modalities at frame 0 (every context observes it): one mean embedding per row."""
        return isinstance(self.bits, int)

    # -- rows ------------------------------------------------------------------------------------------------------------------------------
    def rows(self, x: Tensor) -> Tensor:
        """``[B, S, ...]`` -> the scan's rows ``[B * S, ...]``."""
        if self.order == "copy":
            x = x.transpose(0, 1)
        return x.reshape(x.shape[0] * x.shape[1], *x.shape[2:])

    def spread(self, x: Tensor) -> Tensor:
        """``[B, ...]`` -> ``[B * S, ...]``: every copy of a row gets the row's ``x`` (actions, embeddings, gate weights, states)."""
        return self.rows(x.unsqueeze(1).expand(x.shape[0], self.copies, *x.shape[1:]))

    def first(self, x: Tensor) -> Tensor:
        """``[B * S, ...]`` -> ``[B, ...]``: copy 0 of every row (a view)."""
        return x[: x.shape[0] // self.copies] if self.order == "copy" else x[:: self.copies]

    # -- uniforms --------------------------------------------------------------------------------------------------------------------------
    def uniforms(self, key: str, u: Tensor, layout: str, batch: int, *tail: int) -> Tensor:
        """``noise[key]`` as the scan's rows: ``layout`` ``"row"`` ``(B, *tail)`` is repeated for a row's copies, ``"copy"``
        ``(B, S, *tail)`` taken as it lies."""
        want = (batch, *tail) if layout == "row" else (batch, self.copies, *tail)
        if tuple(u.shape) != want:
            msg = f"noise[{key!r}] must have shape {want}, got {tuple(u.shape)}"
            raise ValueError(msg)
        return (self.spread(u) if layout == "row" else self.rows(u)).contiguous()

    def tail_uniforms(self, key: str, u_post: Tensor, u_tail: Tensor) -> Tensor:
        """``[B * S, T, K]``: copy ``s`` of row ``b`` reads ``u_post[b, t]`` on ``t < q`` and ``u_tail[b, s, t]`` from ``q`` on."""
        b, t, k = u_post.shape
        tail_key = key.replace("post", "tail")
        if tuple(u_tail.shape) != (b, self.copies, t, k):
            msg = f"noise[{tail_key!r}] must have shape {(b, self.copies, t, k)}, got {tuple(u_tail.shape)}"
            raise ValueError(msg)
        q = min(self.context, t)
        return self.rows(torch.cat([u_post[:, None, :q].expand(b, self.copies, q, k), u_tail[:, :, q:]], dim=2)).contiguous()

    def noise_shapes(self, model, batch: int, steps: int) -> dict[str, tuple[int, ...]]:  # noqa: ANN001
        """The uniforms of one step under this plan, batch dimension first, for either model (``model._INIT_KEYS`` / ``_POST_KEYS``)."""
        s = self.copies
        shapes = {key: (batch, *(() if self.init == "row" else (s,)), model._category_size_of(key)) for key in model._INIT_KEYS}  # noqa: SLF001
        sizes = {key: model._category_size_of(key) for key in model._POST_KEYS}  # noqa: SLF001
        if self.post == "prior":
            return shapes | {key.replace("post", "prior"): (batch, s, 1, k) for key, k in sizes.items()}
        shapes |= {key: (batch, s, steps, k) if self.post == "copy" else (batch, steps, k) for key, k in sizes.items()}
        if self.post == "tail":
            shapes |= {key.replace("post", "tail"): (batch, s, steps, k) for key, k in sizes.items()}
        return shapes

    # -- the expansion ---------------------------------------------------------------------------------------------------------------------
    def expand(self, base: dict[int | None, tuple[Tensor, Tensor]], noise: Noise | None,
               sizes: dict[str, int]) -> tuple[Tensor, Tensor, Noise, Callable[[Tensor], Tensor]]:
        """``(codes [B * S, T], mask0 [B * S, 2], noise, spread)`` of the scan's rows.  ``base``: per distinct context the ``codes``
        int32 ``[B, T]`` and ``mask0`` bool ``[B, 2]`` of a row that observes both modalities on that context.  ``sizes``: ``K`` of the
        uniforms to widen -- ``u_init*`` by ``init``, ``u_post*`` by ``post`` (``"tail"``: composed with their ``u_tail*`` twins).  A
        shared uniform that is absent is drawn per ROW; an absent own one is left to its consumer's draw."""
        if self.post == "prior":
            msg = "a plan without posterior uniforms (post='prior') has no posterior rollout to expand"
            raise ValueError(msg)
        per = [base[c][0] for c in self.per_copy(self.context)]
        ref = per[0]
        (b, t), dev = ref.shape, ref.device
        bits, seen = observed_bits(self.per_copy(self.bits), dev)
        stacked = ref[:, None, :] if len(self.contexts) == 1 else torch.stack(per, dim=1)
        codes = self.rows(stacked & bits[None, :, None]).contiguous()
        mask0 = self.rows(base[self.contexts[0]][1][:, None, :] & seen[None])  # (frame 0 is inside every context)
        noise = dict(noise or {})
        for key, k in sizes.items():
            layout, mid = (self.init, ()) if key.startswith("u_init") else (self.post, (t,))
            u = noise.get(key)
            if layout == "tail":
                u_tail = noise.get(key.replace("post", "tail"))
                u = _rand(ref, b, t, k) if u is None else u
                if tuple(u.shape) != (b, t, k):
                    msg = f"noise[{key!r}] must have shape {(b, t, k)}, got {tuple(u.shape)}"
                    raise ValueError(msg)
                noise[key] = self.tail_uniforms(key, u, _rand(ref, b, self.copies, t, k) if u_tail is None else u_tail)
            elif layout == "row":
                noise[key] = self.uniforms(key, _rand(ref, b, *mid, k) if u is None else u, "row", b, *mid, k)
            elif u is not None:
                noise[key] = self.uniforms(key, u, "copy", b, *mid, k)
        return codes, mask0, noise, self.spread


def _must_be(name: str, value: object, kind: type) -> None:
    if not isinstance(value, kind):
        msg = f"{name} must be a {kind.__name__}, got {type(value).__name__}"
        raise ValueError(msg)


def _check_labels(labels: Tensor, batch: tuple[Tensor, ...]) -> None:
    (b, t), dev = batch[0].shape[:2], batch[0].device
    if tuple(labels.shape) != (b, t) or labels.dtype not in (torch.int32, torch.int64) or labels.device != dev:
        msg = f"labels must be an int32 / int64 tensor of shape {(b, t)} on {dev}, got {labels.dtype} {tuple(labels.shape)} on {labels.device}"
        raise ValueError(msg)


def _row_chunks(rows: int, frames_per_row: int, max_frames: int) -> Iterator[tuple[int, int]]:
    """``(r0, r1)``: ``rows`` rows in chunks of whole rows of at most ``max_frames`` frames (one row at least)."""
    per = max(1, int(max_frames) // frames_per_row)
    for r0 in range(0, rows, per):
        yield r0, min(rows, r0 + per)


class _Evaluators:
    """The evaluation steps of ``MoPoE_MRSSM`` (and, through its overrides, ``MoPoE_MMTRSSM``)."""

    def _check_evaluation_step(self, batch: tuple[Tensor, ...], what: str, config: object, kind: type, table: object = None,  # noqa: PLR0913
                               table_kind: type | None = None) -> None:
        """The refusals every evaluation step shares: ``config`` (the argument ``what``) is a ``kind``; the batch carries no modality
        mask; no ``state_carry`` is set; a given ``table`` is a ``table_kind`` of the batch's steps (and of ``config.groups``, where a
        config has groups) on its device."""
        _must_be(what, config, kind)
        groups = getattr(config, "groups", None)
        if self.get_modality_mask_from_batch(batch) is not None:
            msg = "an evaluation step decides what the model observes: a masked (7-tuple) batch already says what is seen"
            raise ValueError(msg)
        if self.state_carry is not None:
            msg = "an evaluation step starts every row from its own frame 0: it does not combine with a set state_carry"
            raise ValueError(msg)
        steps, dev = batch[0].shape[1], batch[0].device
        if table is not None and (not isinstance(table, table_kind) or table.steps != steps or table.buffer.device != dev
                                  or (groups is not None and table.groups != groups)):
            of = f"{steps} steps" if groups is None else f"{groups} groups and {steps} steps"
            msg = f"table must be a {table_kind.__name__} of {of} on {dev}"
            raise ValueError(msg)

    def _local_lengths(self, batch: tuple[Tensor, ...], lengths: Tensor | None) -> Tensor | None:
        """This rank's rows' lengths (int32 ``[B]``) from ``lengths`` or a batch that carries ``valid_global``; None without either."""
        ragged = self._lengths_of(batch, lengths, None, None)
        if ragged is None:
            return None
        valid_global, world, rank = ragged
        rows = batch[0].shape[0]
        _check_lengths(valid_global, rows * world, batch[0].device)
        return valid_global[rank * rows : (rank + 1) * rows].contiguous()

    def _spread_state(self, state, spread: Callable[[Tensor], Tensor]):  # noqa: ANN001, ANN202
        return self._state_like(state, {k: spread(getattr(state, k)) for k in self._FRESH_KEYS})

    def _evaluation_inputs(self, batch: tuple[Tensor, ...], plan: CopyPlan, noise: Noise | None, lengths: Tensor | None,  # noqa: PLR0914
                           expert_log_weights: Tensor | None) -> tuple[dict[str, object], Tensor | None]:
        """What the rollout of an evaluation step reads, on the scan's ``B * copies`` rows: both encoders once, one ``Forecast.sample``
        per distinct context of ``plan``, its expansion, the initial state and the gate once per row.  Returns ``{"actions",
        "audio_embed", "vision_embed", "state0", "noise", "codes", "logw"}`` and the rows' lengths (or None).  The initial state is
        computed on ``B`` rows and spread when the copies share their frame-0 mask and their initial uniforms, else on the wide rows
        (from one mean embedding per row when they share the mask).  ``expert_log_weights``: ``[B, T, 3]``, or ``[B * copies, T, 3]``
        taken as it is."""
        actions = batch[0]
        audio_obs, vision_obs = self.get_observations_from_batch(batch)
        (B, T), dev = actions.shape[:2], actions.device  # noqa: N806
        valid = self._local_lengths(batch, lengths)
        conv.begin_step(dev)
        audio_embed, vision_embed = self._encode_both(audio_obs, vision_obs)
        zeros = torch.zeros(B, device=dev)  # (fixed contexts: the uniforms do not matter)
        base = {}
        for c in plan.contexts:
            sm = Forecast(T if c is None else c).sample(zeros, T, valid)
            base[c] = (sm.codes, sm.mask0)
        per_row = plan.shares_frame0 and plan.init == "row"
        keys = self._POST_KEYS if per_row else (*self._INIT_KEYS, *self._POST_KEYS)
        codes, mask0, wide_noise, spread = plan.expand(base, noise, {key: self._category_size_of(key) for key in keys})
        if plan.shares_frame0:
            embed0 = _masked_mean_embed(audio_embed[:, 0], vision_embed[:, 0], plan.first(mask0))
            if per_row:
                state0 = self._spread_state(self._initial_for_step(embed0, noise), spread)
            else:
                state0 = self._initial_for_step(spread(embed0), wide_noise)
        else:
            state0 = self._initial_for_step(_masked_mean_embed(spread(audio_embed[:, 0]), spread(vision_embed[:, 0]), mask0), wide_noise)
        if expert_log_weights is not None and expert_log_weights.shape[0] == B * plan.copies:
            logw = expert_log_weights  # (checked by the rollout)
        else:
            logw = self._expert_logw(audio_embed, vision_embed, expert_log_weights, B, T)  # the gate once per row ...
            logw = None if logw is None else spread(logw)  # ... repeated for its copies
        return {"actions": spread(actions), "audio_embed": spread(audio_embed), "vision_embed": spread(vision_embed), "state0": state0,
                "noise": wide_noise, "codes": codes, "logw": logw}, valid

    def _evaluation_rollout(self, batch: tuple[Tensor, ...], plan: CopyPlan, noise: Noise | None, lengths: Tensor | None,
                            expert_log_weights: Tensor | None) -> tuple[dict[str, Tensor], Tensor | None]:
        """The rollout of every evaluation step: ``_evaluation_inputs`` and ONE masked posterior rollout over ``B * copies`` rows.
        Returns the scan's outputs -- with ``"codes"``, the rows' modality codes -- and the rows' lengths (or None)."""
        with linear.ordered_sums():  # (no split reductions: two steps on the same rows agree bitwise, whatever their other rows)
            inp, valid = self._evaluation_inputs(batch, plan, noise, lengths, expert_log_weights)
            out = self._rollout_embedded(inp["actions"], inp["audio_embed"], inp["vision_embed"], inp["state0"], inp["noise"], sample_prior=False,
                                         modality=inp["codes"], expert_log_weights=inp["logw"])
        out["codes"] = inp["codes"]
        return out, valid

    # -- forecast skill -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forecast_skill(self, batch: tuple[Tensor, ...], skill: ForecastSkill, noise: Noise | None = None, lengths: Tensor | None = None,  # noqa: PLR0913, PLR0914
                       table: SkillTable | None = None, *, keep_states: bool = False, expert_log_weights: Tensor | None = None) -> SkillTable:
        """One skill step: observe ``skill.context`` frames (of ``skill.observe``), roll ``skill.samples`` sampled
        futures per row open loop in ONE masked posterior rollout over ``B * S`` rows (row ``b * S + s``; the copies of a row share
        ``noise["u_post"]`` on the context and read ``noise["u_tail"][b, s]`` after it), decode, and score every live frame of both
        modalities as an ensemble (``mtrssm_ensemble_score``); the planes are folded by horizon into ``table`` (a new one when None),
        which is returned.  ``best`` is the best sample per FRAME.  ``lengths`` (or a batch that carries ``valid_global``) as in
        ``forecast_rollout``: nothing is observed or scored at or past a row's end.  ``keep_states``: ``table.states`` is the posterior
        state sequence ``[B * S, T, .]`` and ``table.planes`` the step's score planes ``[8, B, T]``.  Every row starts from its own
        frame 0: no masked (7-tuple) batch, no ``state_carry``.  A weighted model runs its gate once per row and
        repeats the weights for the row's copies; ``expert_log_weights`` (fp32 ``[B, T, 3]``, or ``[B * S, T, 3]`` already repeated)
        gives them explicitly."""
        self._check_evaluation_step(batch, "skill", skill, ForecastSkill, table, SkillTable)
        actions = batch[0]
        targets = self.get_targets_from_batch(batch)
        B, T = actions.shape[:2]  # noqa: N806
        S, dev = skill.samples, actions.device  # noqa: N806
        out, valid = self._evaluation_rollout(batch, skill.plan(), noise, lengths, expert_log_weights)
        feature = self._feature_of(out)
        planes = torch.empty(SkillTable.ROWS, B, T, device=dev, dtype=torch.float32)
        for r0, r1 in _row_chunks(B, S * T, skill.max_frames):
            preds, acts = self._decode_for_score(feature[r0 * S : r1 * S])
            part = torch.empty(SkillTable.ROWS, r1 - r0, T, device=dev, dtype=torch.float32)
            for j, (pred, key) in enumerate(zip(preds, ("recon/audio", "recon/vision"), strict=True)):
                ForecastSkill.score(pred.reshape(r1 - r0, S, T, -1), targets[key][r0:r1].reshape(r1 - r0, T, -1),
                                    None if valid is None else valid[r0:r1], acts[j], out=part[4 * j : 4 * j + 4])
            planes[:, r0:r1] = part
        if table is None:
            table = SkillTable(T, dev)
        context = torch.full((B,), min(skill.context, (1 << 31) - 1), dtype=torch.int32, device=dev)
        ForecastSkill.table_add(planes, context, valid, table.sums, table.counts)
        table.planes = planes if keep_states else None
        table.states = self._posterior_from_rollout(out) if keep_states else None
        return table

    def _decode_for_score(self, feature: Tensor, *, audio: bool = True, vision: bool = True) -> tuple[tuple[Tensor | None, Tensor | None], tuple[int, int]]:
        """``(audio, vision)`` predictions of ``feature`` for the ensemble scorer and the output activations it applies while reading
        them: this package's decoders hand over their RAW output (paired when they pair).  A modality that is not asked for is None."""
        da, dv = self.audio_decoder, self.vision_decoder
        fused = isinstance(da, cnn.Decoder) and isinstance(dv, cnn.Decoder) and da.out_act_id is not None and dv.out_act_id is not None
        acts = (da.out_act_id, dv.out_act_id) if fused else (0, 0)
        if audio and vision and fused and _pairable(da, dv, cnn.Decoder):
            return cnn.decode_pair(da, dv, feature, feature, raw=True), acts
        kw = {"raw": True} if fused else {}
        return (da(feature, **kw) if audio else None, dv(feature, **kw) if vision else None), acts

    # -- episode panels -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def render_episodes(self, batch: tuple[Tensor, ...], panel: EpisodePanel, noise: Noise | None = None, lengths: Tensor | None = None, *,  # noqa: PLR0913, PLR0914
                        rows: Tensor | list[int] | None = None, frame0: int = 0, keep_states: bool = False,
                        expert_log_weights: Tensor | None = None) -> EpisodeVideo:
        """The episode panels of a batch: what the reference's logging callback shows per episode -- the open-loop
        prior, the observation and the closed-loop posterior, vision over audio -- as one finished uint8 video.  Both encoders run once,
        then ONE masked posterior rollout over ``2 N`` rows: rows ``[0, N)`` observe ``panel.observe`` on every live frame (the
        posterior), rows ``[N, 2 N)`` observe it on ``t < panel.query_length`` and nothing after (the prior).  Both halves start from the
        same initial state and read the same ``noise["u_post"]`` (MMTRSSM: the ``_l`` / ``_h`` pairs), so on the context the prior is
        the posterior bit for bit: the callback's ``cat_states([posterior[:, :q], prior])``.  Both halves are decoded in chunks of whole
        rows through the decoders' activated path and one ``mtrssm_episode_panel`` launch writes the video.  ``rows`` (an index tensor or
        list) picks the episodes before anything runs, ``noise`` and ``lengths`` with them; ``frame0`` is the number drawn on frame 0.
        ``lengths`` (or a batch that carries ``valid_global``): nothing is observed at or past a row's end and those frames are black.
        ``keep_states``: the video carries the rollout's posterior states ``[2 N, T, .]`` and the decoded frames.  No masked (7-tuple)
        batch, no ``state_carry``; a weighted model runs its gate once per row and repeats it for the row's second copy."""
        self._check_evaluation_step(batch, "panel", panel, EpisodePanel)
        dev = batch[0].device
        if rows is not None:
            pick = torch.as_tensor(rows, dtype=torch.int64, device=dev).reshape(-1)
            if pick.numel() == 0:
                msg = "rows picks no episode"
                raise ValueError(msg)
            lengths = self._local_lengths(batch, lengths)
            lengths = None if lengths is None else lengths.index_select(0, pick).contiguous()
            batch = tuple(b.index_select(0, pick) for b in batch[:6])
            noise = {k: (None if u is None else u.index_select(0, pick)) for k, u in (noise or {}).items()}
            if expert_log_weights is not None:
                expert_log_weights = expert_log_weights.index_select(0, pick)
        targets = self.get_targets_from_batch(batch)
        N, T = batch[0].shape[:2]  # noqa: N806
        plan = panel.plan()
        out, valid = self._evaluation_rollout(batch, plan, noise, lengths, expert_log_weights)
        feature = self._feature_of(out)  # [2 N, T, F]
        da, dv = self.audio_decoder, self.vision_decoder
        decoded: dict[str, Tensor] = {}
        for r0, r1 in _row_chunks(N, 2 * T, panel.max_frames):
            both = torch.cat([feature[r0:r1], feature[N + r0 : N + r1]], dim=0)
            ya, yv = cnn.decode_pair(da, dv, both, both) if _pairable(da, dv, cnn.Decoder) else (da(both), dv(both))
            for name, y in (("audio", ya), ("vision", yv)):
                y = y.to(torch.float32)  # noqa: PLW2901
                if (r0, r1) == (0, N):
                    decoded[f"posterior/{name}"], decoded[f"prior/{name}"] = y[:N], y[N:]
                    continue
                if r0 == 0:
                    decoded[f"posterior/{name}"] = torch.empty(N, *y.shape[1:], device=dev, dtype=torch.float32)
                    decoded[f"prior/{name}"] = torch.empty(N, *y.shape[1:], device=dev, dtype=torch.float32)
                decoded[f"posterior/{name}"][r0:r1], decoded[f"prior/{name}"][r0:r1] = y[: r1 - r0], y[r1 - r0 :]
        decoded["observation/audio"] = targets["recon/audio"].to(torch.float32).contiguous()
        decoded["observation/vision"] = targets["recon/vision"].to(torch.float32).contiguous()
        context = torch.full((N,), min(panel.query_length, (1 << 31) - 1), dtype=torch.int32, device=dev)
        frames = panel.render(decoded["observation/audio"], decoded["posterior/audio"], decoded["prior/audio"], decoded["observation/vision"],
                              decoded["posterior/vision"], decoded["prior/vision"], codes=plan.first(out["codes"]), valid=valid, context=context,
                              frame0=frame0)
        video = EpisodeVideo(frames, context, valid)
        if keep_states:
            video.states, video.decoded = self._posterior_from_rollout(out), decoded
        return video

    # -- held-out likelihood --------------------------------------------------------------------------------------------------
    def _latent_levels(self) -> tuple[tuple[str, MultiOneHotFactory], ...]:
        """The latent levels of a posterior rollout: the suffix of their scan outputs and the factory that knows their K and C."""
        return (("", self.transition.distribution_factory),)

    @torch.no_grad()
    def likelihood_bound(self, batch: tuple[Tensor, ...], bound: LikelihoodBound, noise: Noise | None = None, lengths: Tensor | None = None,  # noqa: PLR0913, PLR0914
                         table: LikelihoodTable | None = None, *, keep_states: bool = False,
                         expert_log_weights: Tensor | None = None) -> LikelihoodTable:
        """One likelihood step (``likelihood.py`` states the quantity): ``bound.samples`` posterior trajectories
        per row in ONE masked posterior rollout over ``B * S`` rows (row ``b * S + s``; the posterior sees ``bound.observe`` on every live
        step and nothing after a row's end; every copy starts from its row's frame 0 with its own ``noise["u_init"][b, s]`` and reads
        ``noise["u_post"][b, s]``), the latent log-ratio of the sampled classes (``mtrssm_latent_log_ratio``, one launch per level), the
        decoders over chunks of whole rows, the per-sample errors (``mtrssm_ensemble_score``) and the bound (``mtrssm_iw_bound``); the
        planes are folded by frame position into ``table`` (a new one when None), which is returned.  ``lengths`` (or a batch that
        carries ``valid_global``): nothing is observed or scored at or past a row's end.  ``keep_states``: ``table.states`` is the
        posterior state sequence ``[B * S, T, .]`` and ``table.planes`` the step's planes ``[8, B, T]``.  No masked (7-tuple) batch, no
        ``state_carry``.  A weighted model runs its gate as in ``forecast_skill``."""
        self._check_evaluation_step(batch, "bound", bound, LikelihoodBound, table, LikelihoodTable)
        actions = batch[0]
        targets = self.get_targets_from_batch(batch)
        B, T = actions.shape[:2]  # noqa: N806
        S, dev = bound.samples, actions.device  # noqa: N806
        out, valid = self._evaluation_rollout(batch, bound.plan(), noise, lengths, expert_log_weights)
        ratio = None
        if bound.latent:
            for suffix, factory in self._latent_levels():
                ratio = LikelihoodBound.log_ratio(out[f"post_logits{suffix}"], out[f"prior_logits{suffix}"], out[f"post_stoch{suffix}"],
                                                  factory.category_size, factory.class_size, out=ratio, accumulate=ratio is not None)
            ratio = ratio.reshape(B, S, T)
        if table is None:
            table = LikelihoodTable(T, dev)
        audio, vision = "audio" in bound.score, "vision" in bound.score
        feature = self._feature_of(out) if bound.score else None
        planes = torch.empty(len(LIKELIHOOD_PLANES), B, T, device=dev, dtype=torch.float32)
        for r0, r1 in _row_chunks(B, S * T, bound.max_frames if bound.score else B * S * T):  # (nothing to decode: one chunk)
            n = r1 - r0
            chunk_valid = None if valid is None else valid[r0:r1]
            se, events = [None, None], [0, 0]
            if bound.score:
                preds, acts = self._decode_for_score(feature[r0 * S : r1 * S], audio=audio, vision=vision)
                for j, (pred, key) in enumerate(zip(preds, ("recon/audio", "recon/vision"), strict=True)):
                    if pred is None:
                        continue
                    pred = pred.reshape(n, S, T, -1)  # noqa: PLW2901
                    events[j] = pred.shape[-1]
                    se[j] = ForecastSkill.score(pred, targets[key][r0:r1].reshape(n, T, -1), chunk_valid, acts[j], se_samples=True).se_samples
            part = planes if n == B else torch.empty(len(LIKELIHOOD_PLANES), n, T, device=dev, dtype=torch.float32)
            LikelihoodBound.bound(se[0], se[1], None if ratio is None else ratio[r0:r1], chunk_valid, events[0], events[1], out=part)
            table.fold(part, chunk_valid)
            if n != B:
                planes[:, r0:r1] = part
        table.planes = planes if keep_states else None
        table.states = self._posterior_from_rollout(out) if keep_states else None
        return table

    # -- particle-filter likelihood -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def particle_filter(self, batch: tuple[Tensor, ...], pf: ParticleFilter, noise: Noise | None = None, lengths: Tensor | None = None,  # noqa: PLR0913, PLR0914, PLR0915
                        table: ParticleTable | None = None, *, keep_states: bool = False,
                        expert_log_weights: Tensor | None = None) -> ParticleTable:
        """One particle-filter step (``particle.py`` states the quantity): ``pf.samples`` particles per row (scan
        row ``b * S + s``), proposed as the samples of ``likelihood_bound`` are.  Encoders, gate, codes and the initial state run once;
        then, per time segment of ``pf.resample_every`` frames: the masked posterior rollout of the segment from the carried particle
        states, the latent log-ratio (one launch per level), the decoders and the scorer over chunks of whole rows,
        ``mtrssm_particle_fold`` -- which carries the weights in double, decides the resampling on the device and writes the ancestors --
        and ``mtrssm_particle_gather`` of the scan's last step by ancestor.  Nothing is read back to the host.  Planes 0 .. 6 are folded
        by frame position into ``table`` (a new one when None), which is returned.  ``noise``: the plan's uniforms and ``u_resample``
        ``(B, T)`` (absent ones are drawn).  ``lengths`` (or a batch that carries ``valid_global``): nothing is observed, scored or
        resampled at or past a row's end.  ``keep_states``: ``table.planes`` ``[8, B, T]``, ``table.ancestors`` int32 ``[B, S, J]`` and
        ``table.inputs`` (``se_audio``, ``se_vision``, ``ratio``: fp32 ``[B, S, T]`` as the fold saw them, None for a term that is off).
        No masked (7-tuple) batch, no ``state_carry``; a weighted model runs its gate as in ``forecast_skill``."""
        self._check_evaluation_step(batch, "pf", pf, ParticleFilter, table, ParticleTable)
        targets = self.get_targets_from_batch(batch)
        B, T = batch[0].shape[:2]  # noqa: N806
        S, dev = pf.samples, batch[0].device  # noqa: N806
        inp, valid = self._evaluation_inputs(batch, pf.plan(), noise, lengths, expert_log_weights)
        u_resample = (noise or {}).get("u_resample")
        if u_resample is None:
            u_resample = _rand(batch[0], B, T)
        if tuple(u_resample.shape) != (B, T) or u_resample.dtype != torch.float32 or u_resample.device != dev:
            msg = f"noise['u_resample'] must be a float32 tensor of shape {(B, T)} on {dev}, got {u_resample.dtype} {tuple(u_resample.shape)}"
            raise ValueError(msg)
        segments = pf.segments(T)
        audio, vision = "audio" in pf.score, "vision" in pf.score
        planes = torch.empty(len(PARTICLE_PLANES), B, T, device=dev, dtype=torch.float32)
        carry = ParticleFilter.new_carry(B, S, dev)
        ancestor = torch.empty(B, S, device=dev, dtype=torch.int32)
        kept_ancestors = torch.empty(B, S, len(segments), device=dev, dtype=torch.int32) if keep_states else None
        kept: dict[str, Tensor | None] = {"se_audio": None, "se_vision": None, "ratio": None}
        state, wide_noise, logw_all = inp["state0"], inp["noise"], inp["logw"]
        for j, (t0, t1) in enumerate(segments):
            c, last = t1 - t0, t1 == T
            cut = (lambda x: x) if c == T else (lambda x: x[:, t0:t1].contiguous())  # noqa: B023
            seg_noise = {k: (cut(u) if k in self._POST_KEYS and u is not None else u) for k, u in wide_noise.items()}
            out = self._rollout_embedded(cut(inp["actions"]), cut(inp["audio_embed"]), cut(inp["vision_embed"]), state, seg_noise,
                                         sample_prior=False, modality=cut(inp["codes"]), expert_log_weights=None if logw_all is None else cut(logw_all))
            ratio = None
            if pf.latent:
                for suffix, factory in self._latent_levels():
                    ratio = LikelihoodBound.log_ratio(out[f"post_logits{suffix}"], out[f"prior_logits{suffix}"], out[f"post_stoch{suffix}"],
                                                      factory.category_size, factory.class_size, out=ratio, accumulate=ratio is not None)
                ratio = ratio.reshape(B, S, c)
            seg_valid = None if valid is None else (valid - t0).clamp_(min=0)  # the scorer counts frames from the segment's first
            feature = self._feature_of(out) if pf.score else None
            for r0, r1 in _row_chunks(B, S * c, pf.max_frames if pf.score else B * S * c):  # (nothing to decode: one chunk)
                n = r1 - r0
                se, events = [None, None], [0, 0]
                if pf.score:
                    preds, acts = self._decode_for_score(feature[r0 * S : r1 * S], audio=audio, vision=vision)
                    for m, (pred, key) in enumerate(zip(preds, ("recon/audio", "recon/vision"), strict=True)):
                        if pred is None:
                            continue
                        pred = pred.reshape(n, S, c, -1)  # noqa: PLW2901
                        events[m] = pred.shape[-1]
                        se[m] = ForecastSkill.score(pred, targets[key][r0:r1, t0:t1].reshape(n, c, -1), None if seg_valid is None else seg_valid[r0:r1],
                                                    acts[m], se_samples=True).se_samples
                part, _ = ParticleFilter.fold(se[0], se[1], None if ratio is None else ratio[r0:r1], None if valid is None else valid[r0:r1],
                                              None if last else u_resample[r0:r1, t1 - 1], t0, pf.threshold, last, carry[r0:r1], events[0], events[1],
                                              ancestor=ancestor[r0:r1])
                planes[:, r0:r1, t0:t1] = part
                if keep_states:
                    for name, x in (("se_audio", se[0]), ("se_vision", se[1]), ("ratio", None if ratio is None else ratio[r0:r1])):
                        if x is not None:
                            if kept[name] is None:
                                kept[name] = torch.zeros(B, S, T, device=dev, dtype=torch.float32)
                            kept[name][r0:r1, :, t0:t1] = x
            if keep_states:
                kept_ancestors[:, :, j] = ancestor
            if not last:
                moved = ParticleFilter.gather([out[self._LAST_KEYS[k]] for k in self._FRESH_KEYS], ancestor)
                state = self._state_like(state, dict(zip(self._FRESH_KEYS, moved, strict=True)))
        if table is None:
            table = ParticleTable(T, dev)
        table.fold(planes, valid)
        table.planes = planes if keep_states else None
        table.ancestors = kept_ancestors
        table.inputs = kept if keep_states else None
        return table

    # -- latent probes --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def probe_features(self, batch: tuple[Tensor, ...], probe: LatentProbe, noise: Noise | None = None, lengths: Tensor | None = None, *,
                       expert_log_weights: Tensor | None = None) -> tuple[Tensor, Tensor | None]:
        """The features a linear probe reads: ``x [G, B, T, Ffull]`` and the rows' lengths ``valid`` (int32 ``[B]``, or
        None).  Both encoders run once, then ONE masked posterior rollout over ``B * G`` rows (row ``b * G + g``): copy ``g`` of a row
        observes ``probe.observe[g]`` on every live step and at frame 0, nothing at or past the row's end, and the copies share the
        row's uniforms (``probe.noise_shapes``).  ``x[g]`` is the feature the decoders would read of that posterior; ``probe.columns(self)``
        names the part to probe in place.  No masked (7-tuple) batch, no ``state_carry``; a weighted model runs its gate once per row."""
        self._check_evaluation_step(batch, "probe", probe, LatentProbe)
        B, T = batch[0].shape[:2]  # noqa: N806
        out, valid = self._evaluation_rollout(batch, probe.plan(), noise, lengths, expert_log_weights)
        feature = self._feature_of(out)  # [B * G, T, Ffull]
        return feature.reshape(B, probe.groups, T, -1).permute(1, 0, 2, 3).contiguous(), valid

    @torch.no_grad()
    def probe_evaluate(self, batch: tuple[Tensor, ...], labels: Tensor, probe: LatentProbe, linear: LinearProbe,  # noqa: PLR0913
                       table: ProbeTable | None = None, noise: Noise | None = None, lengths: Tensor | None = None, *,
                       expert_log_weights: Tensor | None = None) -> ProbeTable:
        """One evaluation step of a fitted probe: ``probe_features``, ONE evaluation-only ``linear.step`` with planes on
        ``probe.columns(self)`` and the fold of ``hit`` / ``nll`` by frame position into ``table`` (a new one when None), which is
        returned; ``table.stats`` keeps the step's ``ProbeStats`` (planes ``[G, B * T]``).  ``labels``: int ``[B, T]`` on the device,
        -1 = silence; a frame at or past its row's end is dead whatever its label."""
        self._check_evaluation_step(batch, "probe", probe, LatentProbe, table, ProbeTable)
        _must_be("linear", linear, LinearProbe)
        actions = batch[0]
        B, T = actions.shape[:2]  # noqa: N806
        G, dev = probe.groups, actions.device  # noqa: N806
        col0, width = probe.columns(self)
        if linear.groups != G or linear.features != width:
            msg = f"{probe!r} on {type(self).__name__} needs a LinearProbe of {G} groups and {width} features, got {linear.groups} and {linear.features}"
            raise ValueError(msg)
        _check_labels(labels, batch)
        x, valid = self.probe_features(batch, probe, noise, lengths, expert_log_weights=expert_log_weights)
        flat = frame_labels(labels, valid)
        stats = linear.step(x.reshape(G, B * T, -1), flat, col0=col0, grad=False, planes=True)
        if table is None:
            table = ProbeTable(G, T, dev, probe.observe)
        live = ((flat >= 0) & (flat < linear.classes)).reshape(B, T)
        table.fold(stats.hit.reshape(G, B, T), stats.nll.reshape(G, B, T), live)
        table.stats = stats
        return table

    # -- latent census --------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def latent_census(self, batch: tuple[Tensor, ...], census: LatentCensus, noise: Noise | None = None, lengths: Tensor | None = None,  # noqa: PLR0913
                      table: CensusTable | None = None, *, keep_states: bool = False, expert_log_weights: Tensor | None = None) -> CensusTable:
        """One census step (``census.py`` states the quantity): both encoders once, then ONE masked posterior
        rollout over ``B * G`` rows (row ``b * G + g``; copy ``g`` observes ``census.observe[g]`` on every live step and nothing after a
        row's end; the copies share the row's uniforms, ``census.noise_shapes``) and one ``LatentCensus.fold`` per latent level
        (``mtrssm_latent_census``), added into ``table`` (a new one when None), which is returned.  No decoder runs and nothing is read
        back.  ``lengths`` (or a batch that carries ``valid_global``) as in ``likelihood_bound``.  ``keep_states``: ``table.planes`` is
        the step's planes per level (fp32 ``[5, B * G, T]`` each), ``table.inputs`` what each level's fold read (``post_logits``,
        ``prior_logits``, ``post_stoch``: the scan's raw outputs ``[B * G, T, K * C]``), ``table.valid`` the rows' lengths (or None) and
        ``table.states`` the posterior state sequence ``[B * G, T, .]``, whose distributions hold normalised logits.
        No masked (7-tuple) batch, no ``state_carry``; a weighted model runs its gate once per row."""
        self._check_evaluation_step(batch, "census", census, LatentCensus, table, CensusTable)
        (B, T), dev = batch[0].shape[:2], batch[0].device  # noqa: N806
        levels = tuple((suffix.lstrip("_"), factory.category_size, factory.class_size) for suffix, factory in self._latent_levels())
        if table is not None and table.levels != levels:
            msg = f"table must be a CensusTable of the levels {levels}, got {table.levels}"
            raise ValueError(msg)
        out, valid = self._evaluation_rollout(batch, census.plan(), noise, lengths, expert_log_weights)
        if table is None:
            table = CensusTable(levels, census.groups, T, dev, census.observe)
        table.active_nats = census.active_nats
        planes, inputs = [], []
        for level, (suffix, factory) in enumerate(self._latent_levels()):
            read = tuple(out[f"{name}{suffix}"].float() for name in ("post_logits", "prior_logits", "post_stoch"))
            got, _ = LatentCensus.fold(*read, census.groups, factory.category_size, factory.class_size, valid, table=table.level_view(level),
                                       planes=keep_states)
            planes.append(got)
            inputs.append(read)
        table.planes = planes if keep_states else None
        table.inputs = inputs if keep_states else None
        table.states = self._posterior_from_rollout(out) if keep_states else None
        table.valid = valid if keep_states else None
        return table

    # -- Frechet distance on reader / encoder features ------------------------------------------------------------------------
    @staticmethod
    def _reader_features(classifier: DigitClassifier, frames: Tensor, act: int) -> Tensor:
        """``[>= N, 128]`` fp32: ``classifier.hidden(classifier.features(frames, act))`` of ``N`` 32 x 32 frames -- the trunk writes into a
        buffer padded to whole 128-row tiles when ``fc1`` is large enough for the tile GEMM (as ``DigitClassifier.read`` does; the pad
        rows are zeros and rows do not mix); the first ``N`` rows are the frames'.  Non-GPU tensors take the torch rule."""
        n = frames.numel() // digits.PIXELS
        if not frames.is_cuda:
            f = classifier.reference_features(frames, act)
            return torch.relu(torch.nn.functional.linear(f, classifier.fc1.weight, classifier.fc1.bias))
        rows = n
        if 2.0 * n * digits.HIDDEN * digits.FEATURES >= linear.SPLIT_MIN_FLOPS:
            rows = -(-n // 128) * 128
        buf = torch.empty(rows, digits.FEATURES, device=frames.device, dtype=torch.float32)
        if rows > n:
            buf[n:].zero_()
        classifier.features(frames, act, out=buf)
        return classifier.hidden(buf)

    def _check_frechet(self, fd: FrechetDistance, classifier: DigitClassifier | None) -> int:
        """The refusals of a Frechet step beyond the shared ones; returns ``D``."""
        if fd.features == "reader":
            _must_be("classifier", classifier, DigitClassifier)
            return digits.HIDDEN
        embed = int(self.audio_representation.obs_embed_size)
        if embed > frechet.MAX_DIM:
            msg = f"features='encoder' keeps a full {embed} x {embed} second moment per bin: the embedding may have at most {frechet.MAX_DIM} features"
            raise ValueError(msg)
        return embed

    @torch.no_grad()
    def frechet_distance(self, batch: tuple[Tensor, ...], fd: FrechetDistance, classifier: DigitClassifier | None = None,  # noqa: PLR0913, PLR0914
                         noise: Noise | None = None, lengths: Tensor | None = None, table: FrechetTable | None = None, *,
                         keep_states: bool = False, expert_log_weights: Tensor | None = None) -> FrechetTable:
        """One Frechet step (``frechet.py`` states the quantity): ``forecast_skill``'s rollout (the same plan and
        noise: ``fd.samples`` futures per row after ``fd.context`` observed frames, scan row ``b * S + s``), the decoders over chunks of
        whole rows, the frames embedded -- ``fd.features == "reader"``: the vision frames through ``classifier.features`` and
        ``classifier.hidden`` (the decoder must give 1 x 32 x 32 frames; only vision is decoded); ``"encoder"``: both modalities'
        activated frames through the model's own encoders -- and one ``FrechetDistance.fold`` (``mtrssm_feature_moments``) per chunk
        and stream into the generated side of ``table`` (a new one when None), which is returned.  The real side takes the TARGET frames
        of the batch through the same feature path, once per ``(b, t)``, with the same bins.  A frame's bin is its horizon's
        (``fd.edges``); a dead frame (``lengths``, or a batch that carries ``valid_global``) has bin -1.  Nothing is read back.
        ``keep_states``: ``table.features[stream] = (real [B * T, D], generated [B * S * T, D])``, ``table.bins = (real, generated)``
        and ``table.states``.  No masked (7-tuple) batch, no ``state_carry``; a weighted model runs its gate as in ``forecast_skill``."""
        self._check_evaluation_step(batch, "fd", fd, FrechetDistance)
        dim = self._check_frechet(fd, classifier)
        (B, T), dev = batch[0].shape[:2], batch[0].device  # noqa: N806
        S, names, reader = fd.samples, fd.bin_names, fd.features == "reader"  # noqa: N806
        J = len(names)  # noqa: N806
        if table is not None and (not isinstance(table, FrechetTable) or not table.matches(fd.streams, dim, names) or table.buffer.device != dev):
            msg = f"table must be a FrechetTable of the streams {fd.streams}, {dim} features and the bins {names} on {dev}"
            raise ValueError(msg)
        targets = self.get_targets_from_batch(batch)
        if reader and targets["recon/vision"][0, 0].numel() != digits.PIXELS:
            msg = f"the digit classifier reads 1 x 32 x 32 vision frames, the batch holds {tuple(targets['recon/vision'].shape[2:])}"
            raise ValueError(msg)
        out, valid = self._evaluation_rollout(batch, fd.plan(), noise, lengths, expert_log_weights)
        feature = self._feature_of(out)
        if table is None:
            table = FrechetTable(fd.streams, dim, names, dev)
        bins_real = fd.bins(B, T, valid, dev)  # [B, T]
        bins_gen = bins_real[:, None, :].expand(B, S, T).contiguous()  # row (b, s, t)
        kept: dict[str, tuple[list[Tensor], list[Tensor]]] = {name: ([], []) for name in fd.streams}
        for r0, r1 in _row_chunks(B, S * T, fd.max_frames):
            n = r1 - r0
            preds, acts = self._decode_for_score(feature[r0 * S : r1 * S], audio=not reader)
            if reader:
                pred = preds[1]
                if pred.numel() != n * S * T * digits.PIXELS:
                    msg = f"the digit classifier reads 1 x 32 x 32 vision frames, the decoder gives {tuple(pred.shape[2:])}"
                    raise ValueError(msg)
                sides = {"vision": (self._reader_features(classifier, targets["recon/vision"][r0:r1], 0),
                                    self._reader_features(classifier, pred, acts[1]))}
            else:
                ya, yv = (torch.tanh(p) if a == 3 else p for p, a in zip(preds, acts, strict=True))  # noqa: PLR2004
                ea_g, ev_g = self._encode_both(ya.to(torch.float32), yv.to(torch.float32))
                ea_r, ev_r = self._encode_both(targets["recon/audio"][r0:r1], targets["recon/vision"][r0:r1])
                sides = {"audio": (ea_r.reshape(n * T, -1), ea_g.reshape(n * S * T, -1)),
                         "vision": (ev_r.reshape(n * T, -1), ev_g.reshape(n * S * T, -1))}
            for name, (real, gen) in sides.items():
                real, gen = real[: n * T].to(torch.float32), gen[: n * S * T].to(torch.float32)  # noqa: PLW2901  (views: the pad rows stay behind)
                FrechetDistance.fold(real, bins_real[r0:r1].reshape(-1), J, table.block(name, 0))
                FrechetDistance.fold(gen, bins_gen[r0:r1].reshape(-1), J, table.block(name, 1))
                if keep_states:
                    kept[name][0].append(real)
                    kept[name][1].append(gen)
        table.features = {name: (torch.cat(r), torch.cat(g)) for name, (r, g) in kept.items()} if keep_states else None
        table.bins = (bins_real.reshape(-1), bins_gen.reshape(-1)) if keep_states else None
        table.states = self._posterior_from_rollout(out) if keep_states else None
        return table

    # -- generation coherence -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generation_coherence(self, batch: tuple[Tensor, ...], labels: Tensor, gc: GenerationCoherence, readers: dict[str, DigitClassifier],  # noqa: PLR0913, PLR0914
                             noise: Noise | None = None, lengths: Tensor | None = None, table: CoherenceTable | None = None, *,
                             keep_states: bool = False, expert_log_weights: Tensor | None = None) -> CoherenceTable:
        """One coherence step (``coherence.py`` states the quantity): both encoders once, then ONE masked posterior
        rollout over ``B * G * S`` rows (copy ``g * S + s`` of row ``b`` is scan row ``b * G * S + g * S + s``: it observes
        ``gc.observe[g]`` on ``gc.context`` frames and runs open loop after them; with ``observe[0] == "both"`` the first ``S`` copies are
        ``forecast_skill``'s rollout under the same noise), both decoders over chunks of whole rows (paired when they pair), every
        decoded frame read by ``readers["vision"]`` / ``readers["audio"]`` (each a ``DigitClassifier`` for 1 x 32 x 32 frames; the
        decoder's raw output goes to the reader, which applies the output activation itself) and ONE ``GenerationCoherence.fold``
        (``mtrssm_coherence_fold``) of the two ``[B * G * S, T, 10]`` logit buffers into ``table`` (a new one when None), which is
        returned.  Nothing is read back.  ``labels``: int ``[B, T]`` on the device, the digit shown and spoken at each frame (-1 =
        silence; anything outside 0 .. 9 is dead).  ``lengths`` (or a batch that carries ``valid_global``): nothing is observed or scored
        at or past a row's end.  ``keep_states``: ``table.planes`` fp32 ``[5, B * G, T]``, ``table.logits = (vision, audio)`` and
        ``table.states``, the posterior state sequence ``[B * G * S, T, .]``.  No masked (7-tuple) batch, no ``state_carry``; a weighted
        model runs its gate as in ``forecast_skill``."""
        self._check_evaluation_step(batch, "gc", gc, GenerationCoherence, table, CoherenceTable)
        names = ("audio", "vision")
        if not isinstance(readers, dict) or any(not isinstance(readers.get(name), DigitClassifier) for name in names):
            msg = "readers must be {'vision': DigitClassifier, 'audio': DigitClassifier}: generation coherence reads both decodes"
            raise ValueError(msg)
        _check_labels(labels, batch)
        targets = self.get_targets_from_batch(batch)
        for name in names:
            if targets[f"recon/{name}"][0, 0].numel() != digits.PIXELS:
                msg = f"the digit classifier reads 1 x 32 x 32 {name} frames, the batch holds {tuple(targets[f'recon/{name}'].shape[2:])}"
                raise ValueError(msg)
        (B, T), dev = batch[0].shape[:2], batch[0].device  # noqa: N806
        G, S = gc.groups, gc.samples  # noqa: N806
        copies = G * S
        out, valid = self._evaluation_rollout(batch, gc.plan(), noise, lengths, expert_log_weights)
        feature = self._feature_of(out)
        logits = {name: torch.empty(B * copies, T, digits.CLASSES, device=dev, dtype=torch.float32) for name in names}
        for r0, r1 in _row_chunks(B, copies * T, gc.max_frames):
            rows = (r1 - r0) * copies
            preds, acts = self._decode_for_score(feature[r0 * copies : r1 * copies])
            for name, pred, act in zip(names, preds, acts, strict=True):
                if pred.numel() != rows * T * digits.PIXELS:
                    msg = f"the digit classifier reads 1 x 32 x 32 {name} frames, the decoder gives {tuple(pred.shape[2:])}"
                    raise ValueError(msg)
                logits[name][r0 * copies : r1 * copies] = readers[name].read(pred, act)[1].reshape(rows, T, digits.CLASSES)
        if table is None:
            table = CoherenceTable(G, T, dev, gc.observe)
        got = GenerationCoherence.fold(logits["vision"], logits["audio"], labels.to(torch.int32), G, S, gc.context, valid, table=table.buffer,
                                       planes=keep_states)
        table.planes = got[0] if keep_states else None
        table.logits = (logits["vision"], logits["audio"]) if keep_states else None
        table.states = self._posterior_from_rollout(out) if keep_states else None
        return table

    # -- word transitions -----------------------------------------------------------------------------------------------------
    def _read_vision(self, feature: Tensor, classifier: DigitClassifier) -> Tensor:
        """The digits (int32, ``feature``'s leading shape) the classifier reads off the vision frames decoded from ``feature``; the
        decoder's raw output goes to the reader, which applies the output activation itself."""
        dv = self.vision_decoder
        fused = isinstance(dv, cnn.Decoder) and dv.out_act_id is not None
        pred = dv(feature, raw=True) if fused else dv(feature)
        if pred.numel() != feature[..., 0].numel() * 32 * 32:
            msg = f"the digit classifier reads 1 x 32 x 32 vision frames, the decoder gives {tuple(pred.shape[feature.dim() - 1 :])}"
            raise ValueError(msg)
        return classifier.digits(pred, dv.out_act_id if fused else 0).reshape(feature.shape[:-1])

    @torch.no_grad()
    def word_transitions(self, batch: tuple[Tensor, ...], labels: Tensor, wt: WordTransitions, classifier: DigitClassifier,  # noqa: PLR0913, PLR0914
                         noise: Noise | None = None, table: TransitionTable | None = None, *,
                         expert_log_weights: Tensor | None = None) -> TransitionTable:
        """One transition step (``words.py``): sample ``wt.samples`` futures per row, read the predicted vision
        frame of each with ``classifier`` and add ``q_counts[word][digit] += 1`` into ``table`` (a new one when None), which is
        returned.  ``labels``: int ``[B, T]`` on the device, -1 = silence; row b's current word is ``labels[b, wt.query - 1]`` and a
        silent row is skipped.  ``protocol="context"``: ``forecast_skill``'s masked rollout (the same noise: ``u_post`` / ``u_tail``),
        frame ``wt.query - 1 + wt.read_at`` is read; only that frame is decoded, or -- ``wt.by_horizon`` -- chunks of whole rows of at
        most ``wt.max_frames`` frames, every frame read and the ``hit`` / ``any`` planes folded by horizon.  ``protocol="reference"``:
        the initial state of frame 0, then a prior-only step with the interval's last action ``batch[0][:, wt.query - 1]``
        (``noise["u_prior"]``: ``[B, S, 1, K]``), whose frame is read.  No masked (7-tuple) batch, no ``state_carry``.  A weighted model
        runs its gate as in ``forecast_skill``."""
        self._check_evaluation_step(batch, "wt", wt, WordTransitions, table, TransitionTable)
        _must_be("classifier", classifier, DigitClassifier)
        actions = batch[0]
        B, T = actions.shape[:2]  # noqa: N806
        S, dev, q = wt.samples, actions.device, wt.query  # noqa: N806
        _check_labels(labels, batch)
        if q > T:
            msg = f"a batch of {T} frames has no context of {q}"
            raise ValueError(msg)
        labels = labels.to(torch.int32)
        plan = wt.plan()
        word = plan.spread(labels[:, q - 1]).contiguous()
        if table is None:
            table = TransitionTable(T, dev)
        if wt.protocol == "reference":
            noise = dict(noise or {})
            audio_obs, vision_obs = self.get_observations_from_batch(batch)
            conv.begin_step(dev)
            state0 = self._spread_state(self.initial_state((audio_obs[:, 0], vision_obs[:, 0]), noise), plan.spread)
            prior_noise = {}
            for key in self._POST_KEYS:
                prior_key, k = key.replace("post", "prior"), self._category_size_of(key)
                u = noise.get(prior_key)
                prior_noise[prior_key] = _rand(actions, B * S, 1, k) if u is None else plan.uniforms(prior_key, u, "copy", B, 1, k)
            prior = self.rollout_transition(actions=plan.spread(actions[:, q - 1 : q]).contiguous(), prev_state=state0, noise=prior_noise)
            digits = self._read_vision(prior.feature, classifier)[:, 0]
            word_counts(word, digits.contiguous(), table.q_counts)
            return table
        t_read = wt.read_frame(T)
        out, _ = self._evaluation_rollout(batch, plan, noise, None, expert_log_weights)
        feature = self._feature_of(out)
        if not wt.by_horizon:
            digits = self._read_vision(feature[:, t_read : t_read + 1].contiguous(), classifier)[:, 0]
            word_counts(word, digits.contiguous(), table.q_counts)
            return table
        planes = torch.empty(3, B, T, device=dev, dtype=torch.float32)
        read = torch.empty(B * S, device=dev, dtype=torch.int32)
        for r0, r1 in _row_chunks(B, S * T, wt.max_frames):
            d = self._read_vision(feature[r0 * S : r1 * S], classifier).reshape(r1 - r0, S, T)
            read[r0 * S : r1 * S] = d[:, :, t_read].reshape(-1)
            lab = labels[r0:r1]
            live = lab >= 0
            same = (d == lab[:, None]).sum(1).to(torch.float32)  # copies that read the frame's label
            zero = torch.zeros((), device=dev)
            planes[0, r0:r1] = torch.where(live, same / float(S), zero)
            planes[1, r0:r1] = torch.where(live, (same > 0).to(torch.float32), zero)
            planes[2, r0:r1] = live.to(torch.float32)
        word_counts(word, read, table.q_counts)
        context = torch.full((B,), q, dtype=torch.int32, device=dev)
        frames = torch.zeros(T, device=dev)  # (the kernel's own count of all frames per bin: the table keeps the labelled ones)
        ForecastSkill.table_add(planes, context, None, table.horizon, frames)
        return table


__all__ = ["CopyPlan"]
