"""GPU (MI355X): the fit loop -- ``mtrssm_fit_fold`` against ``fit.fold_reference``, the ``Trainer`` against
the loop of INTEGRATION.md section 5 written out here, a mid-epoch resume that restores every piece of training state bit for bit, and
a checkpoint taken between the two chunks of a carried episode.

Tolerances.  The fold: squares of fp32 values are exact in double and a sum of n < 2^24 of them is off by at most n 2^-53 < 2e-9
relative, whatever the order: 1e-8; the weighted scalar sums are a handful of double operations: 1e-12.  Two training runs on the same
uniforms: the project's recorded bound for five steps (``test_captured_train_step_matches_eager``: losses rtol 1e-4, parameters max
2e-4 and mean 2e-7 at lr 1e-5); these runs take four.  The step itself is not bitwise reproducible run to run, so parameters after
further steps are compared with that bound, never bit for bit; what depends on seeds and counters only (batches, uniforms) and what a
checkpoint restores IS compared bit for bit."""

from __future__ import annotations

import json
import types
from pathlib import Path

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import fit
from multimodal_mtrssm_amd import transform as tr
from multimodal_mtrssm_amd.optim import FlatParameters
from oracle.cases import CASES, build_model, with_sizes
from tests.conftest import product_from_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, T, N = 6, 8, 12
SEED = 11


# ---------------------------------------------------------------------------------------------
# 1. the fold against fold_reference
# ---------------------------------------------------------------------------------------------
def _chunk_floats() -> int:
    import ctypes as C

    chunk = C.c_int64(0)
    assert mt._lib.load().mtrssm_fit_fold_workspace_bytes(64, 1, C.byref(chunk)) > 0  # noqa: SLF001
    return int(chunk.value)


def _tables() -> dict[str, list[int]]:
    """Segment sizes in floats.  "five": 4 floats; 8 floats holding a 5-element parameter plus 3 zero pads; exactly one chunk; one
    chunk plus 4; three chunks minus 4.  "one": the same buffer as ONE segment.  "max": 32 segments, small ones and two that cross
    chunk borders."""
    c = _chunk_floats()
    five = [4, 8, c, c + 4, 3 * c - 4]
    return {"five": five, "one": [sum(five)], "max": [4 * (i % 5 + 1) for i in range(30)] + [c + 8, 2 * c]}


def _flat(sizes: list[int], seed: int) -> types.SimpleNamespace:
    """What ``EpochMetrics`` reads of a ``FlatParameters``: buffers of random values with the pads of a 5-element parameter zeroed."""
    g = torch.Generator().manual_seed(seed)
    numel = sum(sizes)
    grad, param = torch.randn(numel, generator=g) * 3.0, torch.randn(numel, generator=g)
    offsets = [sum(sizes[:i]) for i in range(len(sizes))]
    if len(sizes) > 1:
        grad[offsets[1] + 5: offsets[1] + 8] = 0.0
        param[offsets[1] + 5: offsets[1] + 8] = 0.0
    full = torch.cat([grad, torch.zeros(8)]).to(DEV)
    return types.SimpleNamespace(numel=numel, offsets=offsets, param=param.to(DEV), grad_full=full, grad=full[:numel], tail=full[numel:],
                                 params=[None] * len(sizes))


def _reference(flat: types.SimpleNamespace, m: mt.EpochMetrics, steps: list[tuple[list[float], float]], step0: int) -> tuple[torch.Tensor, ...]:
    acc, flags = torch.zeros(fit.ACC_DOUBLES, dtype=torch.float64), torch.zeros(fit.FLAG_INTS, dtype=torch.int32)
    flags[fit.FLAG_FIRST_BAD], flags[fit.FLAG_STEP] = -1, step0
    sums = None
    for scalars, w in steps:
        sums = fit.fold_reference(flat.grad.cpu(), flat.param.cpu(), m.offsets, m.group, torch.tensor(scalars), m.scalar_scale, m.grad_scale,
                                  m.clip_norm, w, acc, flags)
    return sums, acc, flags


@pytest.mark.parametrize("table", ["five", "one", "max"])
def test_fold_matches_the_float64_reference(table: str) -> None:
    sizes = _tables()[table]
    flat = _flat(sizes, seed=len(sizes))
    keys = ["loss", "recon", "kl"]
    m = mt.EpochMetrics(flat, [f"m{i}" for i in range(len(sizes))], keys, scalar_scale=0.5, grad_scale=0.5, clip_norm=10.0)
    assert m.chunk == _chunk_floats() and len(m.offsets) - 1 == len(sizes) and m.offsets[-1] == flat.numel
    steps = [([1.25, 0.75, 0.5], 2.0), ([2.5, 1.5, 1.0], 2.0), ([3.0, 2.875, 0.125], 1.0)]  # weights 2, 2, 1
    m.reset(40)
    for k, (scalars, w) in enumerate(steps):
        flat.tail[:3].copy_(torch.tensor(scalars))
        m.fold(flat.tail, w, 40 + k)
    sums, acc, flags = m.sums(), m.acc[0].cpu(), m.flags[0].cpu()
    ref_sums, ref_acc, ref_flags = _reference(flat, m, steps, 40)
    print(f"{table}: G={len(sizes)} numel={flat.numel} max rel err of the sums "
          f"{float(((sums[:2] - ref_sums[:2]).abs() / ref_sums[:2]).max()):.3e}, of acc {float(((acc - ref_acc).abs() / ref_acc.abs().clamp(min=1e-300)).max()):.3e}")
    torch.testing.assert_close(sums, ref_sums, rtol=1e-8, atol=0.0)
    torch.testing.assert_close(acc, ref_acc, rtol=1e-8, atol=0.0)
    assert torch.equal(flags, ref_flags) and flags.tolist() == [0, -1, 0, 0, 43, 0, 0, 0]
    # the fold sequence: weights 2, 2, 1 give the float64 weighted mean
    got = m.compute()
    for i, key in enumerate(keys):
        want = sum(w * (float(np.float32(s[i])) * 0.5) for s, w in steps) / 5.0
        assert got[f"train/{key}"] == pytest.approx(want, rel=1e-12), key
    assert got["grad_norm"] == pytest.approx(float(np.sqrt(float(ref_sums[0].sum()))) * 0.5, rel=1e-8) and got["bad_steps"] == 0.0
    assert got["clipped"] == (3.0 if float(np.sqrt(float(ref_sums[0].sum()))) * 0.5 > 10.0 else 0.0)  # noqa: PLR2004
    assert got[f"param_norm/m{len(sizes) - 1}"] == pytest.approx(float(np.sqrt(float(ref_sums[1, -1]))), rel=1e-8)
    # determinism: the same calls from the same state are bitwise equal, sums and accumulator
    block = m.block.clone()
    m.reset(40)
    for k, (scalars, w) in enumerate(steps):
        flat.tail[:3].copy_(torch.tensor(scalars))
        m.fold(flat.tail, w, 40 + k)
    assert torch.equal(m.sums(), sums) and torch.equal(m.block, block)


@pytest.mark.parametrize("table", ["five", "max"])
def test_fold_flags_exactly_the_non_finite_segments_and_leaves_the_sums_alone(table: str) -> None:
    """A NaN at the first float of one segment and an Inf at the last float of the segment before it (the two sides of a chunk
    border in "five", segments 30 and 31 -- bit 31 of the mask -- in "max")."""
    sizes = _tables()[table]
    flat = _flat(sizes, seed=7)
    m = mt.EpochMetrics(flat, [f"m{i}" for i in range(len(sizes))], ["loss", "kl"], clip_norm=10.0)
    flat.tail[:2].copy_(torch.tensor([1.5, 0.5]))
    m.reset(5)
    m.fold(flat.tail, 3.0, 5)
    before = m.acc.clone()
    hi = 3 if table == "five" else 31
    saved = flat.grad[m.offsets[hi] - 1: m.offsets[hi] + 1].clone()
    flat.grad[m.offsets[hi]] = float("nan")
    flat.grad[m.offsets[hi] - 1] = float("inf")
    m.fold(flat.tail, 3.0, 6)
    assert torch.equal(m.acc, before)  # bitwise
    flags = m.flags[0].cpu().tolist()
    mask = (1 << hi) | (1 << (hi - 1))
    assert flags[:5] == [1, 6, mask - (1 << 32) if hi == 31 else mask, 0, 7]  # noqa: PLR2004
    assert m.sums()[2].tolist() == [1.0 if s in (hi - 1, hi) else 0.0 for s in range(len(sizes))]
    assert m.bad_steps() == {"count": 1, "first": 6, "scalars": [], "modules": [f"m{hi - 1}", f"m{hi}"]}
    # a non-finite scalar on finite gradients: its bit, a second bad step, the first one stays recorded
    flat.grad[m.offsets[hi] - 1: m.offsets[hi] + 1] = saved
    flat.tail[1] = float("-inf")
    m.fold(flat.tail, 3.0, 7)
    assert torch.equal(m.acc, before) and m.flags[0].cpu().tolist()[:5] == [2, 6, flags[2], 0b10, 8]
    with pytest.raises(FloatingPointError, match=r"2 step\(s\).*first at step 6: scalars \['train/kl'\]"):
        m.check()
    flat.tail[1] = 0.5
    m.fold(flat.tail, 1.0, 8)  # finite again: folded
    assert float(m.acc[0, fit.ACC_WEIGHT]) == 4.0 and float(m.acc[0, fit.ACC_STEPS]) == 2.0  # noqa: PLR2004
    assert m.compute()["train/loss"] == 1.5 and m.compute()["bad_steps"] == 2.0  # noqa: PLR2004


# ---------------------------------------------------------------------------------------------
# 2. - 4. the Trainer
# ---------------------------------------------------------------------------------------------
CASE = with_sizes(CASES["mrssm_default"], B, T)
_ORACLE: list = []


def _chain(n: int, std: float | None) -> tr.Compose:
    return tr.Compose([tr.TakeFirstN(n)] + ([tr.GaussianNoise(std)] if std is not None else []))


def _loader(t_full: int, window: str, *, val: bool = False) -> ds.DeviceEpisodeLoader:
    """12 episodes in HBM, batches of 6, seeded feed noise on the two observation streams (the six action floats do not go through
    the gather kernel: no noise there)."""
    g = torch.Generator().manual_seed(CASE.data_seed)
    stores = [torch.randn(N, t_full, CASE.dims.action, generator=g), torch.rand(N, t_full, *CASE.audio_shape, generator=g) * 2 - 1,
              torch.rand(N, t_full, *CASE.vision_shape, generator=g) * 2 - 1]
    streams = tuple(ds._Stream(s.to(DEV), _chain(T, None if k == 0 else 0.1), _chain(T, None)) for k, s in enumerate(stores))  # noqa: SLF001
    if val:  # (as EpisodeDataModule.val_dataloader: the same batches and the same feed noise every epoch)
        return ds.DeviceEpisodeLoader(streams, B, shuffle=False, window=window, noise_seed=2 ** 40 + 9, noise_epoch="fixed")
    return ds.DeviceEpisodeLoader(streams, B, shuffle=True, seed=4, window=window, noise_seed=2 ** 40 + 9)


def _parts():  # noqa: ANN202
    if not _ORACLE:
        _ORACLE.append(build_model(CASE))
    model = product_from_case(CASE, _ORACLE[0], DEV)
    flat = FlatParameters(model, extra=8)
    return model, flat, mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0), mt.FlatDataParallel(flat)


def _record(model) -> list:  # noqa: ANN001
    """Every training ``shared_step`` of ``model`` (the ones handed uniforms; validation draws its own) leaves (batch, uniforms, loss,
    reset) here."""
    log: list = []
    inner = model.shared_step

    def shared_step(batch, noise=None, **kw):  # noqa: ANN001, ANN003, ANN202
        out = inner(batch, noise, **kw)
        if noise is not None:
            log.append({"batch": tuple(x.clone() for x in batch), "noise": {k: v.clone() for k, v in noise.items()}, "loss": out["loss"].detach().clone(),
                        "reset": getattr(batch, "reset_host", None)})
        return out

    model.shared_step = shared_step
    return log


def _lines(directory: Path) -> list[dict]:
    return [json.loads(x) for x in (directory / "metrics.jsonl").read_text().splitlines()]


@pytest.fixture(scope="module")
def run_a(tmp_path_factory: pytest.TempPathFactory) -> dict:
    """Run A: the Trainer, two epochs of two batches, uninterrupted.  Made once, read by the tests below."""
    directory = tmp_path_factory.mktemp("run_a")
    model, flat, opt, dp = _parts()
    log = _record(model)
    start = flat.param.clone()
    trainer = mt.Trainer(model, flat, opt, dp, seed=SEED, max_epochs=2, directory=directory)
    lines = trainer.fit(_loader(T, "first"), _loader(T, "first", val=True))
    torch.cuda.synchronize()
    assert trainer.global_step == 4 and float(opt.state[1]) == 4.0 and float((flat.param - start).abs().max()) > 2e-5  # noqa: PLR2004
    return {"log": log, "param": flat.param.clone(), "lines": lines, "dir": directory, "losses": [float(e["loss"]) for e in log]}


def _assert_same_run(param: torch.Tensor, losses: list[float], a: dict) -> None:
    np.testing.assert_allclose(losses, a["losses"], rtol=1e-4)
    diff = (param - a["param"]).abs()
    print(f"parameters: max diff {float(diff.max()):.3e}, mean {float(diff.mean()):.3e}; losses {losses} vs {a['losses']}")
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))  # noqa: PLR2004


def test_trainer_matches_the_hand_written_loop(run_a: dict) -> None:
    model, flat, opt, dp = _parts()
    loader = _loader(T, "first")
    source = dp.noise_source(SEED)
    losses = []
    for epoch in range(2):
        loader.set_epoch(epoch)
        for batch in loader:
            noise = source.draw(model.noise_shapes(B, T))
            opt.zero_grad()
            out = model.shared_step(batch, noise)
            out["loss"].backward()
            dp.sync({k: out[k] for k in out})
            opt.step(grad_scale=dp.grad_scale)
            losses.append(float(out["loss"].detach()))
    assert len(losses) == 4  # noqa: PLR2004
    _assert_same_run(flat.param, losses, run_a)
    # the logged train/loss of an epoch is the row-weighted mean of its steps' losses (every batch has 6 rows)
    lines = run_a["lines"]
    assert lines == _lines(run_a["dir"]) and [ln["epoch"] for ln in lines] == [0, 1] and [ln["global_step"] for ln in lines] == [2, 4]
    for e, ln in enumerate(lines):
        want = float(np.mean(np.asarray(run_a["losses"][2 * e: 2 * e + 2], dtype=np.float64)))
        print(f"epoch {e}: train/loss {ln['train/loss']!r} vs the mean of the steps {want!r}")
        assert ln["train/loss"] == pytest.approx(want, rel=1e-6) and ln["lr"] == 1e-5 and ln["bad_steps"] == 0.0  # noqa: PLR2004
        assert ln["train/loss"] == pytest.approx(ln["train/recon"] + ln["train/kl"], rel=1e-5)
        assert 0.0 < ln["grad_norm"] <= ln["grad_norm/max"] and ln["param_norm/transition"] > 0.0
    ckpt = torch.load(run_a["dir"] / "best.ckpt", weights_only=True)
    twin = product_from_case(CASE, _ORACLE[0], DEV)
    rest = mt.load_reference_checkpoint(twin, str(run_a["dir"] / "last.ckpt"))  # what every tool's --checkpoint does
    assert not rest["missing_keys"] and not rest["unexpected_keys"] and ckpt["format"] == fit.FORMAT
    assert torch.equal(FlatParameters(twin).param, run_a["param"])  # the file holds run A's final weights, bit for bit
    # validation ran after both epochs (run A has a validation loader, the loop above has none): it left the training streams alone,
    # saw the same draws and the same batches both times, and is what the best checkpoint was chosen by
    assert all(np.isfinite(ln["val/loss"]) and ln["val/loss"] == pytest.approx(ln["val/recon"] + ln["val/kl"], rel=1e-5) for ln in lines)
    assert ckpt["best"]["value"] == min(ln["val/loss"] for ln in lines) and ckpt["metrics"]["val"]["keys"][0] == "val/loss"
    assert lines[1]["val/loss"] == pytest.approx(lines[0]["val/loss"], rel=1e-3)  # (two steps at lr 1e-5 apart)


def test_resume_restores_every_piece_of_state_and_continues_run_a(run_a: dict, tmp_path: Path) -> None:
    # run B: stops after step 3, mid-epoch 1, and saves
    model, flat, opt, dp = _parts()
    log = _record(model)
    b = mt.Trainer(model, flat, opt, dp, seed=SEED, max_epochs=2, max_steps=3, directory=tmp_path)
    b.fit(_loader(T, "first"), _loader(T, "first", val=True))
    torch.cuda.synchronize()
    assert (b.epoch, b.global_step, b.batch_in_epoch) == (1, 3, 1) and len(_lines(tmp_path)) == 1
    held = {"param": flat.param.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(), "state": opt.state.clone(),
            "gen": b.noise.gen.get_state().clone(), "rng": torch.cuda.get_rng_state(DEV).clone(), "train": b.train_metrics.block.clone(),
            "val": b.val_metrics.block.clone()}
    # everything built anew, then the checkpoint
    model2, flat2, opt2, dp2 = _parts()
    log2 = _record(model2)
    c = mt.Trainer(model2, flat2, opt2, dp2, seed=SEED, max_epochs=2, directory=tmp_path)
    ckpt = c.load(tmp_path / "last.ckpt")
    assert torch.equal(flat2.param, held["param"]) and torch.equal(opt2.exp_avg, held["m"]) and torch.equal(opt2.exp_avg_sq, held["v"])
    assert torch.equal(opt2.state, held["state"]) and opt2.steps == 3 and float(opt2.state[1]) == 3.0  # noqa: PLR2004
    assert torch.equal(c.noise.gen.get_state(), held["gen"]) and torch.equal(torch.cuda.get_rng_state(DEV), held["rng"])
    assert torch.equal(c.train_metrics.block, held["train"]) and float(c.train_metrics.acc[0, fit.ACC_STEPS]) == 1.0
    # (the validation accumulator is empty between epochs: what is restored is its keys, its zeros and its flag block)
    assert torch.equal(c.val_metrics.block, held["val"]) and c.val_metrics.keys == b.val_metrics.keys and c.val_metrics.keys[0] == "val/loss"
    assert ckpt["state_carry"] is None and (c.epoch, c.global_step, c.batch_in_epoch) == (1, 3, 1)
    c.fit(_loader(T, "first"), _loader(T, "first", val=True))
    torch.cuda.synchronize()
    # step 4: the batch and the uniforms depend on seeds and counters only -- bit for bit run A's
    assert len(log) == 3 and len(log2) == 1 and c.global_step == 4  # noqa: PLR2004
    for k, entry in enumerate(log + log2):
        ref = run_a["log"][k]
        assert all(torch.equal(x, y) for x, y in zip(entry["batch"], ref["batch"], strict=True)), k
        assert entry["noise"].keys() == ref["noise"].keys() and all(torch.equal(v, ref["noise"][key]) for key, v in entry["noise"].items()), k
    _assert_same_run(flat2.param, [float(e["loss"]) for e in log + log2], run_a)
    lines, lines_a = _lines(tmp_path), run_a["lines"]
    assert [(ln["epoch"], ln["global_step"], ln["lr"]) for ln in lines] == [(ln["epoch"], ln["global_step"], ln["lr"]) for ln in lines_a]
    print(f"epoch 1 train/loss: resumed {lines[1]['train/loss']!r}, uninterrupted {lines_a[1]['train/loss']!r}")
    assert lines[1]["train/loss"] == pytest.approx(lines_a[1]["train/loss"], rel=1e-4)
    want = float(np.mean(np.asarray([float(log[2]["loss"]), float(log2[0]["loss"])], dtype=np.float64)))  # one step before the save, one after
    assert lines[1]["train/loss"] == pytest.approx(want, rel=1e-6)


def test_checkpoint_between_two_chunks_restores_a_filled_carry(tmp_path: Path) -> None:
    """``window="sequential"``, T_full = 2 T: a group of six episodes comes twice in a row.  The run stops after the group's first
    chunk; the resumed step is the second chunk, which continues the carried state of every row."""
    model, flat, opt, dp = _parts()
    model.state_carry = mt.StateCarry.for_model(model, B)
    b = mt.Trainer(model, flat, opt, dp, seed=SEED, max_epochs=1, max_steps=1, directory=tmp_path)
    b.fit(_loader(2 * T, "sequential"))
    torch.cuda.synchronize()
    assert (b.global_step, b.batch_in_epoch) == (1, 1) and model.state_carry.filled == {"train": True, "val": False}
    held = {k: v.clone() for k, v in model.state_carry.buffers["train"].items()}
    assert all(float(v.abs().sum()) > 0.0 for v in held.values())
    model2, flat2, opt2, dp2 = _parts()
    model2.state_carry = mt.StateCarry.for_model(model2, B)
    log2 = _record(model2)
    c = mt.Trainer(model2, flat2, opt2, dp2, seed=SEED, max_epochs=1, max_steps=2, directory=tmp_path)
    c.load(tmp_path / "last.ckpt")
    assert model2.state_carry.filled == {"train": True, "val": False}
    assert all(torch.equal(model2.state_carry.buffers["train"][k], v) for k, v in held.items())
    c.fit(_loader(2 * T, "sequential"))  # (StateCarry.check raises on a partial reset into an empty carry)
    torch.cuda.synchronize()
    assert c.global_step == 2 and len(log2) == 1 and not bool(log2[0]["reset"].any())  # no row was reset  # noqa: PLR2004
    assert torch.isfinite(log2[0]["loss"]) and not torch.equal(model2.state_carry.buffers["train"]["deter"], held["deter"])
    with pytest.raises(ValueError, match="set model.state_carry"):
        model3, flat3, opt3, dp3 = _parts()
        mt.Trainer(model3, flat3, opt3, dp3, seed=SEED, max_epochs=1, directory=tmp_path).load(tmp_path / "last.ckpt")


def test_resume_after_the_scheduler_lowered_the_rate_trains_with_the_new_rate(tmp_path: Path) -> None:
    """The plateau scheduler changes the host's rate at an epoch's end; the kernels read the DEVICE word ``opt.state[0]``.  A checkpoint
    written at that epoch end holds the new rate in both places, and the first resumed step runs with it.  (``threshold=0.5``: only a
    halved loss would count as an improvement, so epoch 1 is a bad epoch and, with patience 0, halves the rate.)"""
    def parts():  # noqa: ANN202
        model, flat, opt, dp = _parts()
        sched = mt.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=0, threshold=0.5)
        return model, flat, opt, sched, dp

    model, flat, opt, sched, dp = parts()
    b = mt.Trainer(model, flat, opt, dp, seed=SEED, max_epochs=2, scheduler=sched, monitor="train/loss", directory=tmp_path)
    lines = b.fit(_loader(T, "first"))
    torch.cuda.synchronize()
    new = float(np.float32(5e-6))
    assert [ln["lr"] for ln in lines] == [1e-5, 1e-5] and opt.param_groups[0]["lr"] == 5e-6 and float(opt.state[0]) == new  # noqa: PLR2004
    ckpt = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert ckpt["optimizer"]["lr"] == 5e-6 and float(ckpt["optimizer"]["state"][0]) == new and ckpt["scheduler"]["num_bad_epochs"] == 0  # noqa: PLR2004
    model2, flat2, opt2, sched2, dp2 = parts()
    c = mt.Trainer(model2, flat2, opt2, dp2, seed=SEED, max_epochs=3, max_steps=5, scheduler=sched2, monitor="train/loss", directory=tmp_path)
    c.fit(_loader(T, "first"), resume=tmp_path / "last.ckpt")
    torch.cuda.synchronize()
    assert c.global_step == 5 and float(opt2.state[1]) == 5.0 and float(opt2.state[0]) == new  # noqa: PLR2004
    # a file whose device word still holds the old rate (written between the scheduler and the next step): the first step uploads
    ckpt["optimizer"]["state"][0] = 1e-5
    torch.save(ckpt, tmp_path / "stale.ckpt")
    model3, flat3, opt3, sched3, dp3 = parts()
    d = mt.Trainer(model3, flat3, opt3, dp3, seed=SEED, max_epochs=3, max_steps=5, scheduler=sched3, monitor="train/loss", directory=tmp_path)
    d.load(tmp_path / "stale.ckpt")
    assert float(opt3.state[0]) == float(np.float32(1e-5)) and opt3.param_groups[0]["lr"] == 5e-6  # noqa: PLR2004
    d.fit(_loader(T, "first"))
    torch.cuda.synchronize()
    assert d.global_step == 5 and float(opt3.state[0]) == new  # noqa: PLR2004
