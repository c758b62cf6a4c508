"""CPU: the fit loop's rules -- the fold in float64 against values written out by hand, the segment table of
the default model, the Trainer's decisions driven by a stub step and stub loaders against a hand-written trace, the checkpoint file,
and a mid-epoch resume that skips exactly the batches already trained on."""

from __future__ import annotations

import json
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import multimodal_mtrssm_amd as mt  # noqa: E402
from multimodal_mtrssm_amd import dataset as ds  # noqa: E402
from multimodal_mtrssm_amd import fit  # noqa: E402
from multimodal_mtrssm_amd import transform as tr  # noqa: E402
from multimodal_mtrssm_amd.optim import FlatParameters  # noqa: E402

OFFSETS = [0, 4, 8, 12]
GRAD = torch.tensor([3.0, 4.0, 0.0, 0.0, 1.0, 2.0, 2.0, 0.0, 6.0, 8.0, 0.0, 0.0])   # norms 5, 3, 10; all: sqrt(134)
PARAM = torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 2.0, 2.0, 2.0, 2.0])  # norms 1, 2, 4; all: sqrt(21)


def _blocks() -> tuple[torch.Tensor, torch.Tensor]:
    flags = torch.zeros(fit.FLAG_INTS, dtype=torch.int32)
    flags[fit.FLAG_FIRST_BAD] = -1
    flags[fit.FLAG_STEP] = 10
    return torch.zeros(fit.ACC_DOUBLES, dtype=torch.float64), flags


def test_fold_reference_matches_values_written_out_by_hand() -> None:
    acc, flags = _blocks()
    losses, weights = [1.0, 2.0, 4.0], [2.0, 2.0, 1.0]
    for loss, w in zip(losses, weights, strict=True):
        sums = fit.fold_reference(GRAD, PARAM, OFFSETS, None, torch.tensor([2.0 * loss, 6.0]), 0.5, 0.5, 3.0, w, acc, flags)
    assert sums.tolist() == [[25.0, 9.0, 100.0], [1.0, 4.0, 16.0], [0.0, 0.0, 0.0]]
    assert float(acc[fit.ACC_WEIGHT]) == 5.0 and float(acc[fit.ACC_STEPS]) == 3.0
    assert float(acc[fit.ACC_SCALARS]) / 5.0 == (2 * 1.0 + 2 * 2.0 + 1 * 4.0) / 5.0 == 2.0  # the mean weighted by rows
    assert float(acc[fit.ACC_SCALARS + 1]) / 5.0 == 3.0
    norm = math.sqrt(134.0) * 0.5
    assert float(acc[fit.ACC_GRAD_SUM]) == pytest.approx(3 * norm, rel=1e-15) and float(acc[fit.ACC_GRAD_MAX]) == norm
    assert float(acc[fit.ACC_CLIPPED]) == 3.0 and float(acc[fit.ACC_PARAM]) == math.sqrt(21.0)  # 5.79 > 3 on every step
    seg = acc[fit.ACC_SEGMENTS: fit.ACC_SEGMENTS + 9].reshape(3, 3)
    assert seg[:, 0].tolist() == [7.5, 4.5, 15.0] and seg[:, 1].tolist() == [2.5, 1.5, 5.0] and seg[:, 2].tolist() == [1.0, 2.0, 4.0]
    assert flags.tolist() == [0, -1, 0, 0, 13, 0, 0, 0]
    # a NaN scalar: the sums stay exactly as they were, the masks and the first bad step are set
    before = acc.clone()
    fit.fold_reference(GRAD, PARAM, OFFSETS, None, torch.tensor([1.0, float("nan")]), 0.5, 0.5, 3.0, 2.0, acc, flags)
    assert torch.equal(acc, before) and flags.tolist() == [1, 13, 0, 0b10, 14, 0, 0, 0]
    bad = GRAD.clone()
    bad[4], bad[11] = float("inf"), float("nan")
    sums = fit.fold_reference(bad, PARAM, OFFSETS, None, torch.tensor([1.0, 1.0]), 0.5, 0.5, 3.0, 2.0, acc, flags)
    assert torch.equal(acc, before) and flags.tolist() == [2, 13, 0b110, 0b10, 15, 0, 0, 0] and sums[2].tolist() == [0.0, 1.0, 1.0]
    # a name with two runs (segments 0 and 2): the root of the summed squares, kept at its first segment
    acc, flags = _blocks()
    fit.fold_reference(GRAD, PARAM, OFFSETS, [0, 1, 0], torch.tensor([1.0]), 1.0, 1.0, 0.0, 1.0, acc, flags)
    seg = acc[fit.ACC_SEGMENTS: fit.ACC_SEGMENTS + 9].reshape(3, 3)
    assert seg[0].tolist() == [math.sqrt(125.0), math.sqrt(125.0), math.sqrt(17.0)] and seg[1].tolist() == [3.0, 3.0, 2.0] and seg[2].tolist() == [0.0] * 3
    assert float(acc[fit.ACC_CLIPPED]) == 0.0  # clip_norm 0: no clipping, nothing counted


def test_segment_table_of_the_default_model_covers_the_flat_buffer() -> None:
    sys.path.insert(0, str(ROOT / "tools"))
    from word_transitions import build_model

    model = build_model("mrssm", (32, 32, 4, 4, 64), "cpu")
    flat = FlatParameters(model)
    metrics = mt.EpochMetrics(flat, model, ["loss"])
    print("segments:", list(zip(metrics.names, metrics.offsets, strict=False)))
    assert metrics.offsets[0] == 0 and metrics.offsets[-1] == flat.numel and all(o % 4 == 0 for o in metrics.offsets)
    assert all(a < b for a, b in zip(metrics.offsets, metrics.offsets[1:], strict=False)) and 1 <= len(metrics.names) <= fit.MAX_SEGMENTS
    children = [name for name, _ in model.named_children()]
    assert set(metrics.names) <= set(children) and {"transition", "audio_encoder", "vision_decoder", "init_proj"} <= set(metrics.names)
    assert metrics.group == [metrics.names.index(n) for n in metrics.names]
    # runs: a name that comes back after another one is a second segment of the same group
    names, offsets, group = fit.segment_runs(["a", "a", "b", "a"], [0, 4, 12, 20], 24)
    assert (names, offsets, group) == (["a", "b", "a"], [0, 12, 20, 24], [0, 1, 0])
    with pytest.raises(ValueError, match="runs of top-level names"):
        fit.segment_runs([str(i) for i in range(33)], list(range(0, 132, 4)), 132)


class _Net(torch.nn.Module):
    """A model the host can step: ``validation_step`` reports the losses a test hands it, epoch by epoch."""

    def __init__(self, val_losses: list[float]) -> None:
        super().__init__()
        self.body = torch.nn.Linear(3, 2)
        self.head = torch.nn.Linear(2, 1)
        self.val_losses, self.val_epochs = val_losses, 0

    def validation_step(self, batch: tuple[torch.Tensor, ...], _k: int = 0) -> dict[str, torch.Tensor]:
        return {"val/loss": torch.tensor(self.val_losses[min(self.val_epochs, len(self.val_losses) - 1)]), "val/rows": torch.tensor(float(batch[0].shape[0]))}

    def on_validation_epoch_end(self) -> dict[str, torch.Tensor]:
        self.val_epochs += 1
        return {"val/extra": torch.tensor(7.0)}


def _parts(val_losses: list[float], lr: float = 1e-3):  # noqa: ANN202
    torch.manual_seed(0)
    net = _Net(val_losses)
    flat = FlatParameters(net)
    return net, flat, mt.FlatAdamW(flat, lr=lr), mt.FlatDataParallel(flat)


def test_trainer_decisions_match_a_hand_written_trace(tmp_path: Path) -> None:
    """Plateau (patience 1, factor 0.5), early stopping (patience 3) and the best checkpoint over val/loss 1.0, 0.9, 0.95, 0.97, 0.98:
    epochs 0 and 1 improve; epochs 2 and 3 are two bad epochs > patience 1, so the rate halves after epoch 3; epoch 4 is the third epoch
    without improvement, so training stops there although max_epochs is 9."""
    net, flat, opt, dp = _parts([1.0, 0.9, 0.95, 0.97, 0.98, 0.99])
    train = [(torch.full((4, 3), float(i)),) for i in range(2)] + [(torch.full((2, 3), 2.0),)]  # rows 4, 4, 2
    val = [(torch.zeros(3, 3),), (torch.zeros(1, 3),)]
    seen = []

    def step(batch: tuple[torch.Tensor, ...]) -> dict[str, torch.Tensor]:
        seen.append(float(batch[0][0, 0]))
        flat.grad.fill_(0.5)
        return {"loss": torch.tensor(1.0 + float(batch[0][0, 0])), "kl": torch.tensor(0.25)}

    trainer = mt.Trainer(net, flat, opt, dp, seed=3, max_epochs=9, scheduler=mt.ReduceLROnPlateau(opt, factor=0.5, patience=1),
                         early_stopping=mt.EarlyStopping("val/loss", patience=3), directory=tmp_path, train_step=step)
    lines = trainer.fit(train, val)
    assert [ln["epoch"] for ln in lines] == [0, 1, 2, 3, 4] and [ln["global_step"] for ln in lines] == [3, 6, 9, 12, 15]
    assert [ln["lr"] for ln in lines] == [1e-3, 1e-3, 1e-3, 1e-3, 5e-4] and opt.param_groups[0]["lr"] == 5e-4
    assert [ln["val/loss"] for ln in lines] == pytest.approx([1.0, 0.9, 0.95, 0.97, 0.98], rel=1e-6)
    assert trainer.should_stop and trainer.early_stopping.stopped_epoch == 4 and trainer.best["epoch"] == 1
    assert trainer.best["value"] == pytest.approx(0.9, rel=1e-6) and seen == [0.0, 1.0, 2.0] * 5
    for ln in lines:  # rows 4, 4, 2 with losses 1, 2, 3: (4 + 8 + 6) / 10; the validation rows 3 and 1
        assert ln["train/loss"] == pytest.approx(1.8, rel=1e-12) and ln["train/kl"] == 0.25 and ln["val/rows"] == pytest.approx(2.5)
        assert ln["val/extra"] == 7.0 and ln["bad_steps"] == 0.0 and ln["grad_norm"] == pytest.approx(0.5 * math.sqrt(flat.numel), rel=1e-12)  # (the stub fills pads too)
        assert {"grad_norm/body", "grad_norm/max/head", "param_norm/body", "clipped", "train_time", "wall_time"} <= set(ln)
    on_disk = [json.loads(x) for x in (tmp_path / "metrics.jsonl").read_text().splitlines()]
    assert on_disk == lines  # one line per epoch
    best = torch.load(tmp_path / "best.ckpt", weights_only=True)
    last = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert best["format"] == last["format"] == fit.FORMAT and best["epoch"] == 2 and best["best"]["epoch"] == 1 and last["epoch"] == 5
    assert last["early_stopping"] == {"best": pytest.approx(0.9, rel=1e-6), "wait": 3, "stopped_epoch": 4} and last["scheduler"]["num_bad_epochs"] == 1
    assert set(best["state_dict"]) == set(net.state_dict()) and last["optimizer"]["lr"] == 5e-4 and last["batch_in_epoch"] == 0
    # every tool's --checkpoint reads the file as it is
    twin = _Net([0.0])
    rest = mt.load_reference_checkpoint(twin, str(tmp_path / "best.ckpt"))
    assert not rest["missing_keys"] and not rest["unexpected_keys"] and torch.equal(twin.body.weight, net.body.weight)


def test_a_non_finite_step_raises_and_names_step_and_key(tmp_path: Path) -> None:
    net, flat, opt, dp = _parts([1.0])

    def step(_batch: tuple[torch.Tensor, ...]) -> dict[str, torch.Tensor]:
        k = step.calls = getattr(step, "calls", -1) + 1
        flat.grad.fill_(0.0)
        if k == 3:
            flat.grad[flat.offsets[2]] = float("inf")  # the head's weight
        return {"loss": torch.tensor(float("nan") if k == 3 else 1.0), "kl": torch.tensor(0.0)}

    trainer = mt.Trainer(net, flat, opt, dp, seed=0, max_epochs=3, directory=tmp_path, train_step=step, check_every_n_steps=2)
    with pytest.raises(FloatingPointError, match=r"first at step 3: scalars \['train/loss'\], gradients of \['head'\]"):
        trainer.fit([(torch.zeros(2, 3),)] * 6)
    assert trainer.global_step == 4 and opt.param_groups[0]["lr"] == 1e-3  # found at the next check; the optimizer is as it was
    acc = trainer.train_metrics.acc[0]
    assert float(acc[fit.ACC_SCALARS]) / float(acc[fit.ACC_WEIGHT]) == 1.0 and float(acc[fit.ACC_STEPS]) == 3.0  # the bad step is not in the sums
    got = trainer.train_metrics.compute()  # ... and a key that was non-finite on a step does not report the finite steps' mean as the epoch's
    assert math.isnan(got["train/loss"]) and got["train/kl"] == 0.0 and got["bad_steps"] == 1.0


def _loader(seed: int = 5, **kw) -> ds.DeviceEpisodeLoader:  # noqa: ANN003
    """12 episodes whose every value is the episode's number; an event of 3 floats keeps the host's per-episode path."""
    ident = tr.Compose([])
    store = torch.arange(12, dtype=torch.float32).reshape(12, 1, 1).expand(12, 4, 3).contiguous()
    streams = tuple(ds._Stream(store.clone(), ident, ident) for _ in range(3))  # noqa: SLF001
    return ds.DeviceEpisodeLoader(streams, 4, shuffle=True, seed=seed, **kw)


def test_batches_zero_is_iter_and_skip_walks_the_schedule_only() -> None:
    a, b, c = _loader(), _loader(), _loader()
    for epoch in range(2):
        whole = [x[0][:, 0, 0].tolist() for x in a]
        assert whole == [x[0][:, 0, 0].tolist() for x in b.batches(0)] and len(whole) == 3
        c.set_epoch(epoch)
        assert [x[0][:, 0, 0].tolist() for x in c.batches(2)] == whole[2:]
    assert sorted(sum(whole, [])) == list(range(12))
    with pytest.raises(ValueError, match="skip"):
        list(a.batches(-1))


def test_mid_epoch_resume_skips_exactly_the_batches_already_trained_on(tmp_path: Path, monkeypatch: pytest.MonkeyPatch) -> None:
    """Run A: two epochs of three batches.  Run B: stopped after step 4 (mid-epoch 1), saved, everything built anew and resumed.  The
    index batches of B's steps are A's, the skipped batch is never gathered, and the epoch's metrics are those of the whole epoch."""
    plain = _loader()
    order = [rows.tolist() for _ in range(2) for rows in plain.index_batches()]

    def run(directory: Path, *, max_steps: int | None, resume: Path | None, seen: list) -> mt.Trainer:
        net, flat, opt, dp = _parts([1.0])

        def step(batch: tuple[torch.Tensor, ...]) -> dict[str, torch.Tensor]:
            seen.append(batch[0][:, 0, 0].to(torch.int64).tolist())
            flat.grad.fill_(float(len(seen)))
            return {"loss": batch[0].mean()}

        trainer = mt.Trainer(net, flat, opt, dp, seed=1, max_epochs=2, max_steps=max_steps, directory=directory, train_step=step)
        trainer.fit(_loader(), None, resume=resume)
        return trainer

    seen_a: list = []
    a = run(tmp_path / "a", max_steps=None, resume=None, seen=seen_a)
    assert seen_a == order and a.global_step == 6
    seen_b: list = []
    b = run(tmp_path / "b", max_steps=4, resume=None, seen=seen_b)
    assert b.global_step == 4 and (b.epoch, b.batch_in_epoch) == (1, 1) and len(b.history) == 1
    ckpt = torch.load(tmp_path / "b" / "last.ckpt", weights_only=True)  # tensors and plain values only
    assert (ckpt["epoch"], ckpt["global_step"], ckpt["batch_in_epoch"]) == (1, 4, 1) and ckpt["loader"]["seed"] == 5
    assert ckpt["metrics"]["train"]["keys"] == ["loss"] and float(ckpt["metrics"]["train"]["acc"][0, fit.ACC_STEPS]) == 1.0
    gathered = []
    real = ds.DeviceEpisodeLoader.batch
    monkeypatch.setattr(ds.DeviceEpisodeLoader, "batch", lambda self, idx, *a_, **k: (gathered.append(idx.tolist()), real(self, idx, *a_, **k))[1])
    c = run(tmp_path / "b", max_steps=None, resume=tmp_path / "b" / "last.ckpt", seen=seen_b)
    assert seen_b == order and gathered == order[4:]  # batch 0 of epoch 1 was skipped on the host, not gathered
    assert c.global_step == 6 and c.epoch == 2
    lines_a = [json.loads(x) for x in (tmp_path / "a" / "metrics.jsonl").read_text().splitlines()]
    lines_b = [json.loads(x) for x in (tmp_path / "b" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines_a) == len(lines_b) == 2
    for la, lb in zip(lines_a, lines_b, strict=True):
        assert {k: v for k, v in la.items() if not k.endswith("_time")} == {k: v for k, v in lb.items() if not k.endswith("_time")}
    # a loader that would walk another schedule is refused
    with pytest.raises(ValueError, match="schedule would differ"):
        net, flat, opt, dp = _parts([1.0])
        mt.Trainer(net, flat, opt, dp, seed=1, max_epochs=2, directory=tmp_path / "b", train_step=lambda _b: {"loss": torch.tensor(0.0)}).fit(
            _loader(seed=6), None, resume=tmp_path / "b" / "last.ckpt")


def test_early_stopping_and_metrics_state_round_trip() -> None:
    stop = mt.EarlyStopping("val/loss", patience=2, mode="max")
    assert [stop.step(v, e) for e, v in enumerate([1.0, 2.0, 2.0, 1.5])] == [False, False, False, True] and stop.stopped_epoch == 3
    twin = mt.EarlyStopping("val/loss", patience=2, mode="max")
    twin.load_state_dict(stop.state_dict())
    assert (twin.best, twin.wait, twin.stopped_epoch) == (2.0, 2, 3)
    assert mt.EarlyStopping(patience=5).step(float("nan"), 0) is True  # a non-finite monitor stops at once
    with pytest.raises(ValueError, match="mode"):
        mt.EarlyStopping(mode="best")
    # ten scalars take two banks of the accumulator; the state restores both
    keys = [f"k{i}" for i in range(10)]
    m = mt.EpochMetrics(None, None, keys, prefix="val/")
    m.fold({k: torch.tensor(float(i)) for i, k in enumerate(keys)}, 3.0, 0)
    m.fold({k: torch.tensor(float(2 * i)) for i, k in enumerate(keys)}, 1.0, 1)
    got = m.compute()
    assert [got[f"val/k{i}"] for i in range(10)] == [pytest.approx(i * 5.0 / 4.0, rel=1e-15) for i in range(10)] and m.banks == 2
    twin_m = mt.EpochMetrics(None, None, keys, prefix="val/")
    twin_m.load_state(m.state())
    assert torch.equal(twin_m.block, m.block) and twin_m.compute() == got
    with pytest.raises(ValueError, match="saved metrics"):
        mt.EpochMetrics(None, None, keys[:3]).load_state(m.state())


def test_resume_across_a_rate_change_uploads_the_new_rate(tmp_path: Path) -> None:
    """The scheduler lowers ``param_groups[0]["lr"]`` at an epoch's end; the kernels read ``opt.state[0]``.  The checkpoint written at
    that epoch end holds the new rate in both, and a file whose device word is still the old one is repaired by the first ``sync_lr``."""
    def run(directory: Path, resume: Path | None, max_epochs: int):  # noqa: ANN202
        net, flat, opt, dp = _parts([1.0, 2.0, 3.0, 4.0])
        trainer = mt.Trainer(net, flat, opt, dp, seed=0, max_epochs=max_epochs, scheduler=mt.ReduceLROnPlateau(opt, factor=0.5, patience=0),
                             directory=directory, train_step=lambda _b: {"loss": torch.tensor(1.0)})
        if resume is not None:
            trainer.load(resume)
        return trainer, opt

    trainer, opt = run(tmp_path, None, 2)
    trainer.fit([(torch.zeros(2, 3),)], [(torch.zeros(2, 3),)])  # val/loss 1.0, then 2.0: a bad epoch, patience 0
    assert opt.param_groups[0]["lr"] == 5e-4 and float(opt.state[0]) == float(torch.tensor(5e-4))
    ckpt = torch.load(tmp_path / "last.ckpt", weights_only=True)
    assert ckpt["optimizer"]["lr"] == 5e-4 and float(ckpt["optimizer"]["state"][0]) == float(torch.tensor(5e-4))
    assert set(ckpt["optimizer"]) == set(opt.state_dict()) | {"state", "touched"}  # FlatAdamW.state_dict() plus the device vector
    ckpt["optimizer"]["state"][0] = 1e-3  # what a file written between the scheduler and the next step would hold
    torch.save(ckpt, tmp_path / "stale.ckpt")
    _, opt2 = run(tmp_path, tmp_path / "stale.ckpt", 3)
    assert float(opt2.state[0]) == float(torch.tensor(1e-3)) and opt2.param_groups[0]["lr"] == 5e-4
    opt2.sync_lr()  # (what the next opt.step does first)
    assert float(opt2.state[0]) == float(torch.tensor(5e-4))


def test_a_non_finite_validation_loss_is_null_in_the_file_and_stops_training(tmp_path: Path) -> None:
    net, flat, opt, dp = _parts([1.0, float("nan"), 0.5])
    trainer = mt.Trainer(net, flat, opt, dp, seed=0, max_epochs=3, early_stopping=mt.EarlyStopping("val/loss", patience=5), directory=tmp_path,
                         train_step=lambda _b: {"loss": torch.tensor(1.0)})
    lines = trainer.fit([(torch.zeros(2, 3),)], [(torch.zeros(2, 3),), (torch.zeros(2, 3),)])
    assert len(lines) == 2 and math.isnan(lines[1]["val/loss"]) and lines[1]["val/bad_steps"] == 2.0 and math.isnan(lines[1]["val/rows"])  # (no finite step: no mean)
    assert trainer.should_stop and trainer.best["epoch"] == 0  # a non-finite monitor stops at once and is no improvement
    on_disk = [json.loads(x, parse_constant=lambda c: pytest.fail(f"{c} is no JSON")) for x in (tmp_path / "metrics.jsonl").read_text().splitlines()]
    assert on_disk[1]["val/loss"] is None and on_disk[0]["val/loss"] == 1.0
    with pytest.raises(ValueError, match="takes 8 scalars"):
        mt.EpochMetrics(flat, net, [f"k{i}" for i in range(9)])
