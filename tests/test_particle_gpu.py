"""GPU (MI355X): the particle-filter likelihood, kernels and end to end.

What is pinned here.  ``mtrssm_particle_fold`` computes in double and rounds once, so chained over the segments of a batch it is the
float64 rule on the same fp32 inputs: every plane within ``|got - ref| <= 1e-6 * max(1, |ref|)`` (the bound of section 6k), the carried
doubles within 1e-12 relative, the ancestors exactly -- the test asserts on its own inputs that no decision between two ancestors is
closer than ``margin >= 1e-9`` of the weights' sum, far above what ``exp`` may differ by between host and device.  It is bitwise
repeatable, a row's result does not depend on the batch around it, dead frames are exactly 0, ``1 <= ess <= S``, and at
``threshold = 0`` it is ``mtrssm_iw_bound`` on the same tensors.  ``mtrssm_particle_gather`` is ``index_select``, exactly.  A
particle-filter step is the rule on the inputs it kept (``table.inputs``), and those inputs are the composition of the public pieces
(``initial_state``, ``rollout_representation`` per segment from the states gathered by the step's ancestors, ``decode_state``): ``se``
to the project's loss-term tolerance, rtol 2e-5, the ratio within the kernels' bound.  At ``threshold = 0`` the step is
``likelihood_bound`` under the same noise.  ``validation_step`` keeps its ``val/*`` values bit for bit (at frame counts whose NLL sums
fit one workgroup, as in ``tests/test_likelihood_gpu.py``) and the epoch end logs ``val/smc/*``.
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd import LikelihoodBound, ParticleFilter, ParticleTable, StateCarry, _lib
from tests.test_likelihood_gpu import DEV, LENGTHS, B, T, _close, _levels, _setup
from tests.test_likelihood_host import HOST_B, HOST_EVENTS, HOST_T, HOST_VALID, bound_inputs
from tests.test_particle_host import check_particle_refusals, uniforms

pytestmark = pytest.mark.gpu
MARGIN = 1e-9


def _chain(inputs, valid, u, c: int, threshold: float, events=HOST_EVENTS):  # noqa: ANN001, ANN202
    """The fold chained over the segments of ``[B, S, T]`` inputs, on the inputs' device: planes ``[8, B, T]``, ancestors ``[B, S, J]``,
    the carry after every segment and the smallest margin (host route only)."""
    ref = next(x for x in inputs if x is not None)
    b, s, t = ref.shape
    carry = ParticleFilter.new_carry(b, s, ref.device)
    planes = torch.empty(8, b, t, device=ref.device, dtype=torch.float32 if ref.is_cuda else torch.float64)
    ancestors, carries, margin = [], [], math.inf
    for t0 in range(0, t, c):
        t1 = min(t, t0 + c)
        last = t1 == t
        cut = [None if x is None else x[:, :, t0:t1].contiguous() for x in inputs]
        col = None if last else u[:, t1 - 1]
        if ref.is_cuda:
            part, anc = ParticleFilter.fold(*cut, valid, col, t0, threshold, last, carry, *events)
        else:
            part, anc, gap = ParticleFilter.segment_reference(*cut, valid, col, t0, threshold, last, carry, *events)
            margin = min(margin, gap)
        planes[:, :, t0:t1] = part
        ancestors.append(anc.clone())
        carries.append(carry.clone())
    return planes, torch.stack(ancestors, dim=2), carries, margin


# a. the fold kernel is the rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["normal", "wide", "equal"])
@pytest.mark.parametrize("s", [1, 2, 5, 16])
def test_fold_kernel_equals_the_float64_rule(s: int, kind: str) -> None:
    inputs = bound_inputs(s, kind)
    dev = [x.to(DEV) for x in inputs]
    u = uniforms(HOST_B, HOST_T, seed=7 + s)
    du = u.to(DEV)
    resampled = 0
    for lengths in (torch.tensor(HOST_VALID, dtype=torch.int32), None):
        dvalid = None if lengths is None else lengths.to(DEV)
        for off in (None, 0, 1, 2):  # every term on, then each of the three inputs nulled in turn
            host, args = list(inputs), list(dev)
            if off is not None:
                host[off] = args[off] = None
            iw = LikelihoodBound.bound(*args, dvalid, *HOST_EVENTS)
            for c in (1, 2, HOST_T):
                for threshold in (0.0, 0.5, 1.0):
                    what = f"fold S {s} {kind} valid {None if lengths is None else lengths.tolist()} off {off} c {c} threshold {threshold}"
                    want, want_anc, want_carries, margin = _chain(host, lengths, u, c, threshold)
                    assert margin >= MARGIN, (what, margin)
                    if off is None:  # (the chain of segments is ParticleFilter.reference: it only adds the carries to compare)
                        full = ParticleFilter.reference(*host, lengths, *HOST_EVENTS, resample_every=c, threshold=threshold, u_resample=u)
                        assert torch.equal(full[0], want) and torch.equal(full[1], want_anc) and full[2] == margin, what
                    got, anc, carries, _ = _chain(args, dvalid, du, c, threshold)
                    again, anc2, carries2, _ = _chain(args, dvalid, du, c, threshold)
                    torch.cuda.synchronize()
                    assert got.dtype == torch.float32 and anc.dtype == torch.int32 and tuple(anc.shape) == (HOST_B, s, -(-HOST_T // c))
                    _close(got, want, what)  # every plane
                    assert torch.equal(anc.cpu(), want_anc), what
                    for have, ref in zip(carries, want_carries, strict=True):
                        err = (have.cpu() - ref).abs()
                        assert bool((err <= 1e-12 * ref.abs()).all()), f"{what}: carry off by {float(err.max())}"
                    assert torch.equal(got, again) and torch.equal(anc, anc2), what  # two calls agree bitwise
                    assert all(torch.equal(x, y) for x, y in zip(carries, carries2, strict=True)), what
                    resampled += int(got[6].sum())
                    if off is not None:
                        assert not bool(got[2 + off].any()), what
                    if lengths is not None:
                        dead = ~(torch.arange(HOST_T) < lengths[:, None]).to(DEV)
                        assert not bool(got[:, dead].any()), what  # exactly 0 on dead frames
                    live = got[5] != 0
                    assert bool((got[5][live] >= 1.0).all()) and bool((got[5] <= float(s)).all()), what
                    if threshold == 0.0:  # the importance-weighted bound's kernel on the same tensors
                        assert not bool(got[6].any()), what
                        _close(got[[0, 1, 2, 3, 4, 5, 7]], iw[[0, 1, 2, 3, 4, 5, 6]].cpu().double(), what + " vs iw_bound")
    assert resampled > 0, (s, kind)


# b. a row's result depends on that row only -------------------------------------------------------------------------------------------------
def test_fold_kernel_row_independence() -> None:
    """The same row in a different batch gives the same bits: alone, and as row 17 of 20 (a second workgroup, another DPP row)."""
    s, t, c = 5, 9, 3
    inputs = [x.to(DEV) for x in bound_inputs(s, "normal", b=20, t=t, seed=3)]
    valid = torch.randint(0, 11, (20,), generator=torch.Generator().manual_seed(4)).to(torch.int32)
    valid[17] = 7
    u = uniforms(20, t, seed=9)
    want, want_anc, _, margin = _chain([x.cpu() for x in inputs], valid, u, c, 1.0)
    assert margin >= MARGIN
    valid, u = valid.to(DEV), u.to(DEV)
    full, anc, carries, _ = _chain(inputs, valid, u, c, 1.0)
    _close(full, want, "fold B 20")
    assert torch.equal(anc.cpu(), want_anc) and bool(full[6].any())
    for row in (0, 15, 16, 17, 19):
        r = slice(row, row + 1)
        one, one_anc, one_carries, _ = _chain([x[r] for x in inputs], valid[r], u[r], c, 1.0)
        assert torch.equal(one[:, 0], full[:, row]) and torch.equal(one_anc[0], anc[row]), row
        assert all(torch.equal(x[0], y[row]) for x, y in zip(one_carries, carries, strict=True)), row
    r = slice(15, 19)
    moved, moved_anc, _, _ = _chain([x[r].contiguous() for x in inputs], valid[r].contiguous(), u[r], c, 1.0)
    assert torch.equal(moved, full[:, r]) and torch.equal(moved_anc, anc[r])


# c. the gather is index_select --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entries", [1, 2, 6])
@pytest.mark.parametrize("s", [1, 5, 16])
def test_gather_kernel_is_index_select(s: int, entries: int) -> None:
    widths = (1, 3, 4, 30, 200, 4)
    b = 7
    g = torch.Generator().manual_seed(10 * s + entries)
    for steps in (1, 3):
        for first in range(0, len(widths), entries):
            ws = [widths[(first + k) % len(widths)] for k in range(entries)]
            last = [torch.randn(b * s, steps, w, generator=g).to(DEV) for w in ws]
            anc = torch.randint(0, s, (b, s), generator=g).to(torch.int32)
            anc[0] = s - 1  # repeats: a whole row from one slot
            if s > 1:
                anc[1, : s // 2] = 0
            rows = (torch.arange(b)[:, None] * s + anc.long()).reshape(-1).to(DEV)
            got = ParticleFilter.gather(last, anc.to(DEV))
            torch.cuda.synchronize()
            for w, x, y in zip(ws, last, got, strict=True):
                assert tuple(y.shape) == (b * s, w) and torch.equal(y, x[:, -1].index_select(0, rows)), (s, entries, steps, w)


def test_gather_kernel_takes_a_misaligned_row_base() -> None:
    """``W = 4`` and ``W = 200`` rows that begin 4 bytes past a 16-byte boundary (source, destination, both): the scalar path."""
    b, s, steps = 3, 5, 2
    g = torch.Generator().manual_seed(3)
    anc = torch.randint(0, s, (b, s), generator=g).to(torch.int32).to(DEV)
    rows = (torch.arange(b, device=DEV)[:, None] * s + anc.long()).reshape(-1)
    for w in (4, 200):
        flat = torch.randn(1 + b * s * steps * w, generator=g).to(DEV)
        for src_off, dst_off in ((1, 0), (0, 1), (1, 1)):
            src = flat[src_off : src_off + b * s * steps * w].view(b * s, steps, w)
            room = torch.full((1 + b * s * w,), -7.0, device=DEV)
            dst = room[dst_off : dst_off + b * s * w].view(b * s, w)
            assert src.is_contiguous() and dst.is_contiguous() and (src.data_ptr() % 16 != 0 or dst.data_ptr() % 16 != 0)
            got = ParticleFilter.gather([src], anc, out=[dst])
            torch.cuda.synchronize()
            assert got[0] is dst and torch.equal(dst, src[:, -1].index_select(0, rows)), (w, src_off, dst_off)
            assert float(room[0]) == (-7.0 if dst_off else float(dst[0, 0])) and (dst_off == 1 or float(room[-1]) == -7.0)  # noqa: PLR2004
    same = torch.zeros(b * s, 1, 4, device=DEV)
    with pytest.raises(_lib.MtrssmLibraryError, match="in place"):
        ParticleFilter.gather([same], anc, out=[same.view(b * s, 4)])


# d. the C entries ---------------------------------------------------------------------------------------------------------------------------
def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_particle_refusals(_lib.load())


# e. a particle-filter step is the rule on its inputs, and its inputs are the public pieces --------------------------------------------------
def _noise(model, pf: ParticleFilter, b: int, t: int, seed: int = 11) -> dict[str, torch.Tensor]:  # noqa: ANN001
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(shape, generator=g).to(DEV) for k, shape in pf.noise_shapes(model, b, t).items()}


def _replayed(case, model, batch, pf: ParticleFilter, noise, lengths, ancestors: torch.Tensor):  # noqa: ANN001, ANN202, PLR0913, PLR0914
    """``se_audio``, ``se_vision`` and ``ratio`` ``[B, S, T]`` in float64 from public pieces: ``initial_state`` on the ``B * S`` repeated
    rows, then per segment ``rollout_representation`` from the previous segment's last posterior states taken by ``ancestors`` and
    ``decode_state``, all under the step's uniforms."""
    b, t = batch[0].shape[:2]
    s = pf.samples
    wide = tuple(x.repeat_interleave(s, dim=0) for x in batch)
    wide_noise = {k: v.reshape(b * s, *v.shape[2:]).contiguous() for k, v in noise.items() if k != "u_resample"}
    live = torch.ones(b, t, dtype=torch.bool) if lengths is None else torch.arange(t) < lengths.cpu()[:, None]
    mask = (live[:, :, None] & torch.tensor([bool(pf.bits & 1), bool(pf.bits & 2)])).repeat_interleave(s, dim=0).to(DEV)
    out = {"se_audio": torch.zeros(b, s, t, dtype=torch.float64), "se_vision": torch.zeros(b, s, t, dtype=torch.float64),
           "ratio": torch.zeros(b, s, t, dtype=torch.float64)}
    with torch.no_grad():
        state = model.initial_state((wide[1][:, 0], wide[2][:, 0]), wide_noise, modality_mask=mask[:, 0])
        for j, (t0, t1) in enumerate(pf.segments(t)):
            seg_noise = {k: (v[:, t0:t1].contiguous() if k.startswith("u_post") else v) for k, v in wide_noise.items()}
            post, prior = model.rollout_representation(actions=wide[0][:, t0:t1].contiguous(),
                                                       observations=(wide[1][:, t0:t1].contiguous(), wide[2][:, t0:t1].contiguous()),
                                                       prev_state=state, noise=seg_noise, modality_mask=mask[:, t0:t1].contiguous())
            dec = model.decode_state(post)
            for key, name, tgt in (("recon/audio", "se_audio", batch[4]), ("recon/vision", "se_vision", batch[5])):
                y = dec[key].flatten(2).double().cpu().reshape(b, s, t1 - t0, -1)
                out[name][:, :, t0:t1] = (0.5 * (tgt[:, t0:t1].flatten(2).double().cpu()[:, None] - y) ** 2).sum(-1)
            ratio = torch.zeros(b * s, t1 - t0, dtype=torch.float64)
            for suffix, cats, classes in _levels(case):
                q, p, z = (getattr(post, f"distribution{suffix}").logits, getattr(prior, f"distribution{suffix}").logits, getattr(post, f"stoch{suffix}"))
                ratio = ratio + LikelihoodBound.reference_ratio(q.flatten(-2).cpu(), p.flatten(-2).cpu(), z.cpu(), cats, classes)
            out["ratio"][:, :, t0:t1] = ratio.reshape(b, s, t1 - t0)
            rows = (torch.arange(b)[:, None] * s + ancestors[:, :, j].cpu().long()).reshape(-1).to(DEV)
            state = post[:, -1][rows]
    return out, live


STEP_CASES = [(name, ragged, c, "both") for name in ("mrssm_default", "mmtrssm_default") for ragged in (True, False) for c in (1, 2)]
STEP_CASES += [("mrssm_default", True, 2, "audio"), ("weighted", True, 2, "both")]


@pytest.mark.parametrize(("name", "ragged", "c", "observe"), STEP_CASES)
def test_particle_step_is_the_rule_on_the_composition_of_the_public_pieces(name: str, ragged: bool, c: int, observe: str) -> None:  # noqa: FBT001, PLR0914
    s = 4
    case, model, batch = _setup(name)
    pf = ParticleFilter(samples=s, resample_every=c, threshold=1.0, observe=observe)
    noise = _noise(model, pf, B, T)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV) if ragged else None
    what = f"{name} lengths {LENGTHS if ragged else None} c {c} {observe}"
    table = model.particle_filter(batch, pf, noise, lengths=lengths, keep_states=True)
    torch.cuda.synchronize()
    segments = pf.segments(T)
    assert isinstance(table, ParticleTable) and tuple(table.buffer.shape) == (8, T) and tuple(table.planes.shape) == (8, B, T)
    assert table.ancestors.dtype == torch.int32 and tuple(table.ancestors.shape) == (B, s, len(segments))
    assert set(table.inputs) == {"se_audio", "se_vision", "ratio"} and all(tuple(x.shape) == (B, s, T) and x.dtype == torch.float32 for x in table.inputs.values())
    # 1. the rule on the inputs the fold saw
    host = {k: v.cpu() for k, v in table.inputs.items()}
    events = (int(np.prod(batch[4].shape[2:])), int(np.prod(batch[5].shape[2:])))
    want, want_anc, margin = ParticleFilter.reference(host["se_audio"], host["se_vision"], host["ratio"], None if lengths is None else lengths.cpu(),
                                                      *events, resample_every=c, threshold=1.0, u_resample=noise["u_resample"].cpu())
    print(what, "margin", margin)
    assert margin >= MARGIN, what
    assert torch.equal(table.ancestors.cpu(), want_anc), what
    _close(table.planes, want, what)
    live = torch.ones(B, T, dtype=torch.bool) if lengths is None else torch.arange(T) < lengths.cpu()[:, None]
    flags = table.planes[6].cpu()
    for b in range(B):  # threshold 1: resampled after every segment end that has a live frame behind it
        for t0, t1 in segments:
            n = T if lengths is None else LENGTHS[b]
            assert float(flags[b, t1 - 1]) == float(t1 < T and t1 < n), (what, b, t1)
    assert bool((want_anc != torch.arange(s, dtype=torch.int32).reshape(1, s, 1)).any()), what  # something moved
    assert not bool(table.planes.cpu()[:, ~live].any()), what
    assert torch.equal(table.counts.cpu(), live.sum(0).float()), what
    np.testing.assert_allclose(table.sums.cpu().numpy(), table.planes[:7].sum(1).cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=what)
    # 2. the inputs are the public pieces, replayed with the step's ancestors
    replay, _ = _replayed(case, model, batch, pf, noise, lengths, table.ancestors)
    wide_live = live[:, None, :].expand(B, s, T)
    for key in ("se_audio", "se_vision"):
        np.testing.assert_allclose(host[key].double()[wide_live].numpy(), replay[key][wide_live].numpy(), rtol=2e-5, atol=0, err_msg=f"{what} {key}")
    _close(torch.where(wide_live, host["ratio"].double(), 0.0), torch.where(wide_live, replay["ratio"], 0.0), f"{what} ratio")
    if observe == "audio":  # (the proposal never saw vision: still scored)
        assert bool(table.planes[3].any())
    if name == "weighted":
        assert model.weights_timeseries is not None
    # a second step adds into the same table; chunks of one row at a time change nothing but the decoders' last bits
    small = ParticleFilter(samples=s, resample_every=c, threshold=1.0, observe=observe)
    small.max_frames = 1
    first = table.buffer.clone()
    again = model.particle_filter(batch, small, noise, lengths=lengths, table=table)
    assert again is table and table.planes is None and table.ancestors is None and table.inputs is None
    assert torch.equal(table.counts, 2.0 * first[7]) and torch.equal(table.sums[6], 2.0 * first[6])
    np.testing.assert_allclose(table.sums[1:4].cpu().numpy(), 2.0 * first[1:4].cpu().numpy(), rtol=2e-5, atol=0)


# f. threshold = 0 is the likelihood step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_threshold_zero_is_the_likelihood_step_under_the_same_noise(name: str) -> None:
    s = 4
    _, model, batch = _setup(name)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    live = torch.arange(T) < lengths.cpu()[:, None]
    for c in (T, 2):
        pf = ParticleFilter(samples=s, resample_every=c, threshold=0.0)
        noise = _noise(model, pf, B, T, seed=17)
        mine = model.particle_filter(batch, pf, noise, lengths=lengths, keep_states=True)
        theirs = model.likelihood_bound(batch, LikelihoodBound(samples=s), {k: v for k, v in noise.items() if k != "u_resample"}, lengths=lengths,
                                        keep_states=True)
        torch.cuda.synchronize()
        got, want = mine.planes.cpu().double(), theirs.planes.cpu().double()
        what = f"{name} c {c}"
        assert not bool(got[6].any()) and torch.equal(mine.ancestors.cpu(), torch.arange(s, dtype=torch.int32).reshape(1, s, 1).expand(B, s, -(-T // c)))
        for p, q in ((2, 2), (3, 3), (7, 6), (1, 1)):  # the data planes, the prefix, and mean against elbo: the loss-term tolerance
            np.testing.assert_allclose(got[p].numpy(), want[q].numpy(), rtol=2e-5, atol=0, err_msg=f"{what} plane {p}")
        _close(got[4], want[4], f"{what} plane 4")
        run = torch.where(live, got[0].cumsum(1), torch.zeros(()).double())  # plane 0 through its running sum (T + 1 roundings)
        np.testing.assert_allclose(run.numpy(), got[7].numpy(), rtol=1e-6, atol=0, err_msg=f"{what} plane 0 vs 7")
        ess = mine.planes[5].cpu()
        assert bool((ess[live] >= 1.0).all()) and bool((ess[live] <= float(s)).all()) and not bool(got[:, ~live].any()), what


# g. validation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_cfg3dims"])
def test_validation_step_keeps_its_values_and_the_epoch_end_logs_the_particle_filter(name: str) -> None:
    """B = 2, T = 4 frames of 16 x 8 audio and 8 x 8 vision: one NLL workgroup per modality (``tests/test_likelihood_gpu.py``)."""
    _, model, batch = _setup(name, (2, 4))
    pf = ParticleFilter(samples=3, resample_every=2, threshold=1.0)
    try:
        torch.manual_seed(5)
        plain = model.validation_step(batch)
        direct = model.particle_filter(batch, pf)
        model.validation_step(batch)
        model.particle_filter(batch, pf, table=direct)
        assert model.particle_table is None and model.on_validation_epoch_end() == {}
        model.val_particle = pf
        torch.manual_seed(5)
        both = model.validation_step(batch)
        assert set(both) == set(plain)
        for k, v in plain.items():
            assert torch.equal(both[k], v), (k, float(both[k]), float(v))  # bitwise: the particle step runs after everything else
        model.validation_step(batch)
        assert isinstance(model.particle_table, ParticleTable) and model.particle_table.counts.tolist() == [4.0] * 4
        logged = model.on_validation_epoch_end()
        assert model.particle_table is None and model.on_validation_epoch_end() == {}
        want = direct.scalars("val/smc")
        assert set(logged) == set(want) == {f"val/smc/{k}" for k in ("smc", "mean", "audio", "vision", "latent", "ess", "resampled")}
        for k, v in want.items():
            assert torch.equal(logged[k], v), (k, float(logged[k]), float(v))
        assert float(logged["val/smc/resampled"]) == 0.25 and 1.0 <= float(logged["val/smc/ess"]) <= 3.0  # noqa: PLR2004  (after frame 1 of 4)
        np.testing.assert_allclose(float(logged["val/smc/mean"]),
                                   float(logged["val/smc/audio"] + logged["val/smc/vision"] + logged["val/smc/latent"]), rtol=1e-5)
    finally:
        model.val_particle = None
        model.particle_table = None


def test_particle_step_refuses_masked_batches_and_a_set_carry() -> None:
    _, model, batch = _setup("mrssm_default")
    pf = ParticleFilter(samples=2)
    with pytest.raises(ValueError, match="masked"):
        model.particle_filter((*batch, torch.ones(B, T, 2, dtype=torch.bool, device=DEV)), pf)
    model.state_carry = StateCarry.for_model(model, B)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.particle_filter(batch, pf)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="u_resample"):
        model.particle_filter(batch, pf, {"u_resample": torch.rand(B, T + 1, device=DEV)})
    drawn = model.particle_filter(batch, ParticleFilter(samples=3, resample_every=4))  # without noise the step draws its own
    assert bool(torch.isfinite(drawn.buffer).all()) and drawn.counts.tolist() == [float(B)] * T and drawn.planes is None
