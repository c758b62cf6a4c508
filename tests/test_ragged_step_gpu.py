"""GPU (MI355X): training on episodes of different lengths, end to end.

The property pinned here: a row with ``valid[b] = L`` in a padded batch of length T contributes the same sums and the same gradients
as that row alone at ``T = L``, combined by the rule -- every term is a sum over rows divided by the GLOBAL count of its frames.
Tolerances are the project's: loss terms 2e-5 relative, posterior probabilities and deter 1e-5, samples exact,
every gradient 2e-4 of its tensor's largest entry; captured against eager: losses rtol 1e-4, parameters max 2e-4 / mean 2e-7 at
lr 1e-5.  The noise is screened (``oracle.cases.screened_noise``, margin 1e-4) so that no draw sits at a CDF edge.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import ModalityDropout, StateCarry, dropout, scan
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.optim import FlatParameters
from oracle.cases import CASES, build_batch, build_model, screened_noise, with_sizes
from oracle.ref_model import cat_probs
from tests.conftest import product_from_case
from tests.test_modality_mask_oracle import oracle_step, screened
from tests.test_state_carry_gpu import _oracle_chunk_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, T = 3, 6
VALID = (6, 4, 1)
# (case, one-CU scan forced): the default scan and the one-CU scan of both models
FAMILIES = [("mrssm_default", False), ("mrssm_default", True), ("mmtrssm_default", False), ("mmtrssm_default", True)]
IDS = [f"{c}{'-onecu' if f else ''}" for c, f in FAMILIES]
LOSS_KEYS = {"mrssm": ("loss", "recon", "recon/audio", "recon/vision", "kl"), "mmtrssm": ("loss", "recon", "recon/audio", "recon/vision", "kl", "kl_h")}


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _dev(batch: tuple, noise: dict) -> tuple[tuple, dict]:
    return tuple(x.to(DEV) for x in batch), {k: v.to(DEV) for k, v in noise.items()}


def _rows(batch: tuple, noise: dict, rows: slice, steps: int) -> tuple[tuple, dict]:
    """Rows ``rows`` and the first ``steps`` frames of a batch and of its noise tape."""
    return tuple(x[rows, :steps] for x in batch), {k: (v[rows, :steps] if v.dim() == 3 else v[rows]) for k, v in noise.items()}  # noqa: PLR2004


def _padded(batch: tuple, valid: tuple[int, ...], fill: float = 0.0) -> tuple:
    """The batch with every frame at or past a row's length set to ``fill`` (0: what the ragged gather writes)."""
    out = tuple(x.clone() for x in batch)
    for x in out:
        for b, n in enumerate(valid):
            x[b, n:] = fill
    return out


def _model(name: str, onecu: bool, oracle: torch.nn.Module, sizes: tuple[int, int] = (B, T)):  # noqa: ANN202, FBT001
    model = product_from_case(with_sizes(CASES[name], *sizes), oracle, DEV)
    if onecu:
        model.scan_rows_per_block = 1
    return model


def _train(model, batch, noise, **kw):  # noqa: ANN001, ANN003, ANN202
    model.zero_grad(set_to_none=True)
    out = model.shared_step(batch, noise, **kw)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in out.items()}, grads


def _check_grads(got: dict[str, torch.Tensor], want: dict[str, torch.Tensor], least: int = 40) -> None:
    seen = 0
    for k, g in want.items():
        scale = float(g.abs().max())
        mine = got.get(k)
        if scale == 0.0:
            assert mine is None or float(mine.abs().max()) == 0.0, f"grad {k} must be zero"
            continue
        assert mine is not None, k
        np.testing.assert_allclose(_np(mine), _np(g), rtol=0, atol=2e-4 * scale, err_msg=f"grad {k}")
        seen += 1
    assert seen > least


@functools.lru_cache(maxsize=None)
def _reference(name: str, valid: tuple[int, ...] = VALID) -> dict:
    """Computed once per model and shared: the oracle run PER ROW on the row's first ``valid[b]`` frames with that row's noise, combined
    by the rule -- each term's sum over rows divided by its count (without dropout all three counts are ``sum(valid)``)."""
    case = with_sizes(CASES[name], len(valid), T)
    oracle = build_model(case)
    batch = build_batch(case)
    noise, margin, _ = screened_noise(case, oracle, batch, margin=1e-4)
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    total = float(sum(valid))
    rows, terms = [], dict.fromkeys(LOSS_KEYS[case.kind], 0.0)
    loss = 0.0
    for b, n in enumerate(valid):
        out = oracle.shared_step(*_rows(batch, noise, slice(b, b + 1), n))
        loss = loss + (n / total) * out["loss"]
        for k in terms:
            terms[k] += n / total * float(out[k].detach())
        rows.append({k: v.detach() for k, v in out.items() if k.startswith("_")})
    oracle.zero_grad(set_to_none=True)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    return {"case": case, "oracle": oracle, "batch": batch, "noise": noise, "terms": terms, "grads": grads, "rows": rows}


# 1. against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_ragged_step_matches_the_oracle_per_row(name: str, onecu: bool) -> None:  # noqa: FBT001
    ref = _reference(name)
    case, d = ref["case"], ref["case"].dims
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _dev(_padded(ref["batch"], VALID), ref["noise"])
    valid = torch.tensor(VALID, dtype=torch.int32, device=DEV)
    out, grads = _train(model, batch, noise, lengths=valid)
    assert set(out) == set(ref["terms"])
    for k, want in ref["terms"].items():
        print(name, onecu, k, float(out[k]), want)
        np.testing.assert_allclose(float(out[k]), want, rtol=2e-5, err_msg=k)
    _check_grads(grads, ref["grads"])
    # the posterior on live steps is the per-row run's
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise, lengths=valid)
    if case.kind == "mrssm":
        levels = [(post.distribution.probs, post.stoch, "", d.cats, d.classes)]
        deters = [(post.deter, "deter")]
        kls = [post.kl_per_step]
    else:
        levels = [(post.distribution_l.probs, post.stoch_l, "_l", d.ls_cats, d.ls_classes), (post.distribution_h.probs, post.stoch_h, "_h", d.hs_cats, d.hs_classes)]
        deters = [(post.deter_l, "deter_l"), (post.deter_h, "deter_h")]
        kls = [post.kl_per_step, post.kl_h_per_step]
    for b, n in enumerate(VALID):
        row = ref["rows"][b]
        for probs, stoch, sfx, cats, classes in levels:
            want = cat_probs(row[f"_post_logits{sfx}"], cats, classes)[1]
            np.testing.assert_allclose(_np(probs[b, :n]), want[0].numpy(), rtol=0, atol=1e-5, err_msg=f"post probs{sfx} row {b}")
            assert torch.equal(stoch[b, :n].cpu(), row[f"_post_stoch{sfx}"][0]), f"post samples{sfx} row {b}"
        for deter, key in deters:
            np.testing.assert_allclose(_np(deter[b, :n]), row[f"_{key}"][0].numpy(), rtol=0, atol=1e-5, err_msg=f"{key} row {b}")
        for kl in kls:  # a dead step: posterior = prior, KL exactly 0
            assert not bool(kl[b, n:].any()) and bool(kl[b, :n].any())
    # lengths and a modality mask together are refused
    with pytest.raises(ValueError, match="not both"):
        model.shared_step(batch, noise, lengths=valid, modality_mask=torch.ones(B, T, 2, dtype=torch.bool, device=DEV))


# 2. against itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_ragged_step_equals_its_rows_run_alone(name: str, onecu: bool) -> None:  # noqa: FBT001
    ref = _reference(name)
    model = _model(name, onecu, ref["oracle"])
    batch, noise = _dev(_padded(ref["batch"], VALID), ref["noise"])
    out, grads = _train(model, batch, noise, lengths=torch.tensor(VALID, dtype=torch.int32, device=DEV))
    total = float(sum(VALID))
    terms = dict.fromkeys(out, 0.0)
    want: dict[str, torch.Tensor] = {}
    for b, n in enumerate(VALID):  # three separate steps at B = 1, T = 6 / 4 / 1, the plain path without lengths
        o, g = _train(model, *_rows(batch, noise, slice(b, b + 1), n))
        for k in terms:
            terms[k] += n / total * float(o[k])
        for k, v in g.items():
            want[k] = want.get(k, 0) + (n / total) * v
    for k in terms:
        np.testing.assert_allclose(float(out[k]), terms[k], rtol=2e-5, err_msg=k)
    _check_grads(grads, want)


# 3. nothing leaks from behind an episode's end ------------------------------------------------------------------------------------
def _loader(stores: list[torch.Tensor], steps: int, lengths: torch.Tensor, bs: int) -> ds.DeviceEpisodeLoader:
    chain = tr.Compose([tr.TakeFirstN(steps)])  # input = target: no noise is drawn inside the loader
    streams = tuple(ds._Stream(s.to(DEV), chain, chain) for s in stores)  # noqa: SLF001
    return ds.DeviceEpisodeLoader(streams, bs, shuffle=False, window="sequential", lengths=lengths)


def _stores(ref: dict, fill: float) -> list[torch.Tensor]:
    """Three ``[B, T, *event]`` stores (actions, audio, vision targets) with ``fill`` behind each episode's end."""
    return list(_padded(ref["batch"][3:], VALID, fill))


def _one_of_the_clean_runs_or_within_their_spread(got: torch.Tensor, clean: list[torch.Tensor], what: str) -> None:
    """For a quantity that is NOT deterministic run to run (its sums pass through split reductions that meet in fp32 atomics: the
    encoders' output Linear, the NLL sums, every weight gradient, and everything downstream of them): the run on the dirty store is
    the same computation on the same bits as the runs on the clean one, so it must be bit for bit one of them, or differ from the
    first no more than they may differ among themselves -- four times their spread, floored at 2e-5 of the scale (the yardstick of
    ``test_modality_mask_gpu._same_up_to_reruns``).  A leak of a 1e30 behind ``len`` passes neither."""
    if any(torch.equal(got, c) for c in clean):
        return
    ref = clean[0]
    scale = float(ref.abs().max()) + 1e-12
    spread = max(float((c - ref).abs().max()) for c in clean[1:])
    err = float((got - ref).abs().max())
    print(f"{what}: differs from every clean run: err {err:.3e}, their spread {spread:.3e}, scale {scale:.3e}")
    assert err <= max(4 * spread, 2e-5 * scale), what


def _rollout_outputs(model, batch, noise) -> dict[str, torch.Tensor]:  # noqa: ANN001
    """What ``rollout_representation(lengths=)`` gives for a batch that carries its lengths: deter, probabilities, samples, per-step KL."""
    with torch.no_grad():
        s0 = model.initial_state((batch[1][:, 0], batch[2][:, 0]), noise)
        post, _ = model.rollout_representation(actions=batch[0], observations=(batch[1], batch[2]), prev_state=s0, noise=noise,
                                               lengths=batch.valid)
    if hasattr(post, "deter_l"):
        return {"deter_l": post.deter_l, "deter_h": post.deter_h, "probs_l": post.distribution_l.probs, "probs_h": post.distribution_h.probs,
                "stoch_l": post.stoch_l, "stoch_h": post.stoch_h, "kl_l": post.kl_per_step, "kl_h": post.kl_h_per_step}
    return {"deter": post.deter, "probs": post.distribution.probs, "stoch": post.stoch, "kl": post.kl_per_step}


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_what_lies_behind_the_length_changes_nothing(name: str, onecu: bool) -> None:  # noqa: FBT001
    """The same episodes in a zero-padded store and in one with garbage (1e30) behind ``len``.  Deterministic by construction, so
    asserted bit for bit: every tensor the step reads (the gather issues no load behind ``len``), the loader's ``valid*``, every field
    of the ``StepMask``, and the posterior samples (the noise is screened).  From there on both runs are the same computation on the
    same bits; what it yields is not bitwise reproducible run to run, so the rollout's deter, probabilities and per-step KL, the loss
    terms and the gradients are held to ``_one_of_the_clean_runs_or_within_their_spread`` against three runs on the clean store."""
    ref = _reference(name)
    model = _model(name, onecu, ref["oracle"])
    noise = {k: v.to(DEV) for k, v in ref["noise"].items()}
    lens = torch.tensor(VALID)
    clean, dirty = (list(_loader(_stores(ref, fill), T, lens, B)) for fill in (0.0, 1e30))
    assert len(clean) == len(dirty) == 1
    clean, dirty = clean[0], dirty[0]
    for x, y in zip(clean, dirty, strict=True):
        assert torch.equal(x, y)
    for key in ("valid", "valid_host", "valid_global", "reset", "start"):
        assert torch.equal(getattr(clean, key), getattr(dirty, key)), key
    assert clean.valid.tolist() == list(VALID) and clean.valid_host.tolist() == list(VALID)
    for x, want in zip(clean, _padded(ref["batch"][3:] * 2, VALID), strict=True):
        assert torch.equal(x.cpu(), want)
    masks = [dropout.ragged_step_mask(b.valid_global, None, T) for b in (clean, dirty)]
    for key in ("codes", "present_audio", "present_vision", "mask0", "count_audio", "count_vision", "live", "count_live", "last"):
        assert torch.equal(getattr(masks[0], key), getattr(masks[1], key)), key
    rolls = [_rollout_outputs(model, clean, noise) for _ in range(3)]
    got = _rollout_outputs(model, dirty, noise)
    for k, v in got.items():
        if k.startswith("stoch"):
            assert torch.equal(v, rolls[0][k]), k
        else:
            _one_of_the_clean_runs_or_within_their_spread(v, [r[k] for r in rolls], k)
    steps = [_train(model, clean, noise) for _ in range(3)]  # (the batch carries its lengths: no lengths= here)
    b, gb = _train(model, dirty, noise)
    for k in b:
        _one_of_the_clean_runs_or_within_their_spread(b[k], [s[0][k] for s in steps], k)
    for k in gb:
        assert bool(torch.isfinite(gb[k]).all()), k
        _one_of_the_clean_runs_or_within_their_spread(gb[k], [s[1][k] for s in steps], f"grad {k}")


# 4. with dropout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_ragged_step_with_dropout_matches_the_masked_oracle(name: str, onecu: bool) -> None:  # noqa: FBT001
    """``modality_dropout`` with injected ``u_mask``: the step is the oracle's masked step (``tests/test_modality_mask_oracle``) fed
    ``ragged_reference``'s mask.  That helper averages the KL over all B * T steps; a dead step's KL is exactly 0, so the rule's
    KL -- the sum over live steps / count_live -- is its value times ``B * T / count_live``."""
    ref = _reference(name)
    case, oracle = ref["case"], ref["oracle"]
    md = ModalityDropout(0.4, 0.3, span=2)
    u = torch.rand(md.noise_shape(B, T), generator=torch.Generator().manual_seed(6))
    u[1, 0] = torch.tensor([0.1, 0.2])  # row 1 takes the t = 0 fix-up (vision)
    valid = torch.tensor(VALID, dtype=torch.int32)
    rule = dropout.ragged_reference(valid, u, T, md)
    assert rule.mask[1, 0].tolist() == [False, True] and not bool(rule.mask.all(dim=-1)[rule.live].all())  # something live is dropped
    batch = _padded(ref["batch"], VALID)
    noise, margin = screened(case, oracle, batch, rule.codes.long())
    assert margin >= 1e-5, f"no noise seed keeps the draws away from the CDF edges (best {margin})"
    want = oracle_step(case, oracle, batch, noise, rule.codes.long())
    scale = B * T / float(rule.counts[2])
    terms = {k: float(want[k]) for k in ("recon", "recon/audio", "recon/vision")}
    terms["kl"] = float(want["kl"]) * scale
    loss = want["recon"] + want["kl"] * scale
    if case.kind == "mmtrssm":
        terms["kl_h"] = float(want["kl_h"]) * scale
        loss = loss + want["kl_h"] * scale
    terms["loss"] = float(loss)
    oracle.zero_grad(set_to_none=True)
    loss.backward()
    want_grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    model = _model(name, onecu, oracle)
    dbatch, dnoise = _dev(batch, noise)
    out, grads = _train(model, dbatch, {**dnoise, "u_mask": u.to(DEV)}, modality_dropout=md, lengths=valid.to(DEV))
    assert set(out) == set(terms)
    for k, v in terms.items():
        print(name, onecu, k, float(out[k]), v)
        np.testing.assert_allclose(float(out[k]), v, rtol=2e-5, err_msg=k)
    _check_grads(grads, want_grads, least=10)


# 5. with the carry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_ragged_chunks_carry_the_last_valid_state(name: str, onecu: bool) -> None:  # noqa: FBT001, PLR0914
    """Lengths (6, 4, 2) walked in two chunks of T = 3: valid (3, 3, 2) then (3, 1, 0).  After chunk 2 the carry holds the posterior at
    frames 5 and 3 and, for row 2, chunk 1's frame 1; chunk 2's loss is the oracle's with the carried state injected, rows combined by
    the counts; ``init_proj`` gets exactly zero gradient in chunk 2 (no row resets)."""
    lens = (6, 4, 2)
    ref = _reference(name)
    case, oracle = ref["case"], ref["oracle"]
    stores = list(_padded(ref["batch"][3:], lens))
    batches = list(_loader(stores, 3, torch.tensor(lens), B))
    assert [b.valid_host.tolist() for b in batches] == [[3, 3, 2], [3, 1, 0]] and [bool(b.reset_host.all()) for b in batches] == [True, False]
    assert torch.equal(batches[1].valid.cpu(), batches[1].valid_host) and torch.equal(batches[1].valid_global, batches[1].valid)
    model = _model(name, onecu, oracle, (B, 3))
    sc = StateCarry.for_model(model, B)
    noise = ref["noise"]
    chunk = lambda a: {k: (v[:, a: a + 3] if v.dim() == 3 else v).to(DEV) for k, v in noise.items()}  # noqa: E731, PLR2004
    # the oracle, row by row: chunk 1 from the fresh state, chunk 2 from what chunk 1 left
    full = tuple(x for x in ref["batch"][3:]) * 2  # (input = target in this loader)
    carried, want_loss, live2 = [], 0.0, float(sum(batches[1].valid_host.tolist()))
    oracle.zero_grad(set_to_none=True)
    for b, n in enumerate(lens):
        one = slice(b, b + 1)
        n1, n2 = min(n, 3), max(n - 3, 0)
        rb, rn = _rows(full, noise, one, n1)
        with torch.no_grad():
            if case.kind == "mrssm":
                s0 = oracle.initial_state(rb[1][:, 0], rb[2][:, 0], rn["u_init"])
            else:
                s0 = oracle.initial_state(rb[1][:, 0], rb[2][:, 0], rn["u_init_h"], rn["u_init_l"])
            _, last = _oracle_chunk_loss(oracle, case, rb, rn, s0)
        if n2:
            cb = tuple(x[one, 3: 3 + n2] for x in full)
            cn = {k: (v[one, 3: 3 + n2] if v.dim() == 3 else v[one]) for k, v in noise.items()}  # noqa: PLR2004
            loss_b, last = _oracle_chunk_loss(oracle, case, cb, cn, last)
            want_loss = want_loss + (n2 / live2) * loss_b
        carried.append(last)
    want_loss.backward()
    want_grads = {k: p.grad.clone() for k, p in oracle.named_parameters() if p.grad is not None}
    _train(model, batches[0], chunk(0), state_carry=sc)
    after1 = {k: v.clone() for k, v in sc.buffers["train"].items()}
    out, grads = _train(model, batches[1], chunk(3), state_carry=sc)
    np.testing.assert_allclose(float(out["loss"]), float(want_loss), rtol=2e-5)
    for k, v in sc.buffers["train"].items():
        assert torch.equal(v[2], after1[k][2]), k  # row 2 had no live step in chunk 2: its carry is chunk 1's, untouched
        for b in range(B):
            want = carried[b][k][0]
            if k.startswith("stoch"):
                assert torch.equal(v[b].cpu(), want), (k, b)
            else:
                np.testing.assert_allclose(_np(v[b]), want.numpy(), rtol=0, atol=1e-5, err_msg=f"{k} row {b}")
    _check_grads(grads, want_grads)
    inits = [k for k, _ in model.named_parameters() if k.startswith("init_proj.")]
    assert inits and all(k not in want_grads for k in inits)
    for k in inits:
        assert k not in grads or float(grads[k].abs().max()) == 0.0, k
    # a row that resets with no valid frame is refused on the host, before anything is launched
    bad = ds.EpisodeBatch(tuple(batches[1]), batches[1].start, batches[1].reset, batches[1].start_host, torch.tensor([False, False, True]),
                          valid=batches[1].valid, valid_host=batches[1].valid_host, valid_global=batches[1].valid_global)
    with pytest.raises(ValueError, match="no valid frame"):
        model.shared_step(bad, chunk(3), state_carry=sc)


# 6. data parallel -----------------------------------------------------------------------------------------------------------------
def _episode_batch(items: tuple, valid: list[int], valid_global: list[int], row0: int, reset: list[bool] | None = None) -> ds.EpisodeBatch:
    n = len(valid)
    reset_host = torch.ones(n, dtype=torch.bool) if reset is None else torch.tensor(reset)
    start = torch.zeros(n, dtype=torch.int32)
    return ds.EpisodeBatch(items, start.to(DEV), reset_host.to(DEV), start, reset_host, valid=torch.tensor(valid, dtype=torch.int32, device=DEV),
                           valid_host=torch.tensor(valid, dtype=torch.int32), valid_global=torch.tensor(valid_global, dtype=torch.int32, device=DEV),
                           row0=row0)


@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_ragged_loss_is_exact_under_data_parallel_sharding(name: str, onecu: bool) -> None:  # noqa: FBT001
    lens = [6, 1, 3, 5]
    ref = _reference(name, tuple(lens))
    model = _model(name, onecu, ref["oracle"], (4, T))
    batch, noise = _dev(_padded(ref["batch"], lens), ref["noise"])
    one, g_one = _train(model, _episode_batch(batch, lens, lens, 0), noise)
    for k, want in ref["terms"].items():  # (and the one-rank step is the oracle's)
        np.testing.assert_allclose(float(one[k]), want, rtol=2e-5, err_msg=k)
    halves = []
    for r in range(2):
        rows = slice(2 * r, 2 * r + 2)
        sub, sub_noise = _rows(batch, noise, rows, T)
        halves.append(_train(model, _episode_batch(sub, lens[rows], lens, 2 * r), sub_noise))
    for k in one:
        np.testing.assert_allclose(0.5 * (float(halves[0][0][k]) + float(halves[1][0][k])), float(one[k]), rtol=2e-5, err_msg=k)
    mean = {k: 0.5 * (halves[0][1].get(k, 0) + halves[1][1].get(k, 0)) for k in g_one}  # the all-reduced sum scaled by 1 / world
    _check_grads(mean, g_one)


# 7. captured ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("name", "onecu"), FAMILIES, ids=IDS)
def test_captured_ragged_step_matches_eager(name: str, onecu: bool) -> None:  # noqa: FBT001
    ref = _reference(name)
    oracle = ref["oracle"]
    valids = [[6, 4, 1], [2, 6, 5]]
    batches = [_episode_batch(_dev(_padded(ref["batch"], v), {})[0], v, v, 0) for v in valids]
    results = {}
    for mode in ("eager", "graph"):
        model = _model(name, onecu, oracle)
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(B, T)
        losses = []
        if mode == "eager":
            for eb in batches:
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(eb, noise)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append({k: float(v) for k, v in out.items()})
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, batches[0], source, warmup=2, ragged=True)
            for eb in batches:
                losses.append({k: float(v) for k, v in cap.step(eb).items()})
            assert float(opt.state[1]) == 2.0 and opt.steps == 2
            before = flat.param.clone()
            with pytest.raises(ValueError, match="no valid frame"):  # a reset row with valid = 0: refused, nothing replayed
                cap.step(_episode_batch(tuple(batches[0]), [6, 0, 1], [6, 0, 1], 0))
            with pytest.raises(ValueError, match="ragged=True"):  # a batch without lengths: refused too
                cap.step(tuple(batches[0]))
            torch.cuda.synchronize()
            assert float(opt.state[1]) == 2.0 and torch.equal(flat.param, before) and cap.valid_global.tolist() == valids[1]
            cap.close()
        scan.check_cluster_status()
        results[mode] = (losses, flat.param.clone())
    for k in results["eager"][0][0]:
        got, want = [s[k] for s in results["graph"][0]], [s[k] for s in results["eager"][0]]
        print(name, onecu, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    assert results["eager"][0][0]["kl"] != results["eager"][0][1]["kl"]  # the replay read the second batch's lengths
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_captured_ragged_step_with_carry_and_dropout_matches_eager(name: str) -> None:
    """``ragged=True`` with ``state_carry=`` and ``modality_dropout=`` in ONE graph against the eager steps: chunk 1 resets every row,
    chunks 2 and 3 continue with an empty row each, whose carry must survive the replay untouched (save-at reads ``last`` on the device)."""
    ref = _reference(name)
    oracle = ref["oracle"]
    valids, resets = [[6, 4, 1], [2, 0, 5], [0, 3, 6]], [[True] * 3, [False] * 3, [False] * 3]
    batches = [_episode_batch(_dev(_padded(ref["batch"], v), {})[0], v, v, 0, r) for v, r in zip(valids, resets, strict=True)]
    md = ModalityDropout(0.3, 0.3, span=2)
    results = {}
    for mode in ("eager", "graph"):
        model = _model(name, False, oracle)
        model.modality_dropout = md  # (noise_shapes gains "u_mask")
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(B, T)
        assert "u_mask" in shapes
        sc = StateCarry.for_model(model, B)
        losses, carries = [], []
        cap = CapturedTrainStep(model, flat, opt, dp, batches[0], source, warmup=2, ragged=True, state_carry=sc, modality_dropout=md) \
            if mode == "graph" else None
        for eb in batches:
            if cap is None:
                noise = source.draw(shapes)
                opt.zero_grad()
                out = model.shared_step(eb, noise, modality_dropout=md, state_carry=sc)
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
            else:
                out = cap.step(eb)
            losses.append({k: float(v) for k, v in out.items()})
            carries.append({k: v.clone() for k, v in sc.buffers["train"].items()})
        for k in carries[0]:  # an empty row keeps its carry: row 1 through chunk 2, row 0 through chunk 3
            assert torch.equal(carries[1][k][1], carries[0][k][1]) and torch.equal(carries[2][k][0], carries[1][k][0]), (mode, k)
            assert not torch.equal(carries[1][k][2], carries[0][k][2]) or k.startswith("stoch")
        if cap is not None:
            assert float(opt.state[1]) == 3.0 and sc.filled["train"]
            with pytest.raises(ValueError, match="no valid frame"):  # row 1 resets with nothing at t = 0
                cap.step(_episode_batch(tuple(batches[1]), valids[1], valids[1], 0, [False, True, False]))
            assert float(opt.state[1]) == 3.0
            cap.close()
        scan.check_cluster_status()
        results[mode] = (losses, flat.param.clone(), carries[-1])
    for k in results["eager"][0][0]:
        got, want = [s[k] for s in results["graph"][0]], [s[k] for s in results["eager"][0]]
        print(name, k, got, want)
        np.testing.assert_allclose(got, want, rtol=1e-4, err_msg=k)
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))
    for k, v in results["graph"][2].items():
        np.testing.assert_allclose(_np(v), _np(results["eager"][2][k]), atol=1e-5, err_msg=k)
