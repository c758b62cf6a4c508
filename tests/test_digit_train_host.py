"""CPU: training the digit reader -- the float64 rule against plain torch autograd, the dropout masks against the
Philox words, the trainer's life cycle, the checkpoint it leaves, memorisation of a small set and the share of units whose tape entry a
kernel within the feature bound may choose differently.  Also the inputs the GPU tests share (``memorise_set``, ``literal_step``,
``MEMORISE_STEPS``)."""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from multimodal_mtrssm_amd import DigitTrainer, dropout_mask_reference, tape_reference
from multimodal_mtrssm_amd.dataset import philox4x32_10, stream_key
from multimodal_mtrssm_amd.digit_train import DEAD, PARAMETERS, TAPE, TAPE_CONV1
from multimodal_mtrssm_amd.digits import DigitClassifier
from tests.test_digits_host import EXEMPT_CAP, LOGIT_BOUND, digit_set, seeded_classifier, seeded_frames

TAPE_FRAMES = 300
MEMORISE_STEPS = 11  # recorded: the host path below reaches 100 % within this many steps (the GPU test gets twice as many)


def literal_step(clf: DigitClassifier, images: torch.Tensor, labels: torch.Tensor, keep: torch.Tensor, p: float) -> tuple[torch.Tensor, list[torch.Tensor]]:
    """The network written out with torch's own functions, in float64: the mean cross-entropy of ``images [N, 1, 32, 32]`` and its eight
    gradients by autograd."""
    params = [dict(clf.named_parameters())[k].detach().double().requires_grad_(True) for k in PARAMETERS]
    w1, b1, w2, b2, wf1, bf1, wf2, bf2 = params
    x = F.max_pool2d(F.relu(F.conv2d(images, w1, b1, padding=1)), 2, 2)
    x = F.max_pool2d(F.relu(F.conv2d(x, w2, b2, padding=1)), 2, 2)
    x = F.relu(F.linear(x.view(-1, 64 * 8 * 8), wf1, bf1))
    x = x * keep.double() / (1.0 - p)
    loss = F.cross_entropy(F.linear(x, wf2, bf2), labels.long())
    return loss.detach(), list(torch.autograd.grad(loss, params))


@functools.lru_cache(maxsize=None)
def memorise_set() -> tuple[torch.Tensor, torch.Tensor]:
    """40 frames: 10 prototypes (``2 N(0, 1)`` on 4 x 4, bilinearly upsampled as ``seeded_frames`` does) x 4 copies with ``0.5 N(0, 1)``
    noise; the label is the prototype."""
    g = torch.Generator().manual_seed(4040)
    proto = F.interpolate(2.0 * torch.randn(10, 1, 4, 4, generator=g, dtype=torch.float64), size=(32, 32), mode="bilinear", align_corners=False)
    idx = torch.arange(10).repeat_interleave(4)
    raw = proto[idx].reshape(40, 1024) + 0.5 * torch.randn(40, 1024, generator=g, dtype=torch.float64)
    return raw.float(), idx.to(torch.int32)


def memorise(device: str, max_steps: int) -> int:
    """Full-batch steps without dropout on the set until every frame is read right; returns the steps taken (``max_steps + 1``: never)."""
    raw, labels = (t.to(device) for t in memorise_set())
    clf = DigitClassifier()
    clf.load_state_dict(seeded_classifier(5).state_dict())
    clf.to(device)
    with DigitTrainer(clf, lr=1e-3, dropout=0.0, seed=0) as trainer:
        for step in range(1, max_steps + 1):
            trainer.fit(raw, labels, epochs=1, batch_size=40, act=3)
            stats = trainer.evaluate(raw, labels, act=3)
            if int(stats.hits) == 40:  # noqa: PLR2004
                return step
    return max_steps + 1


def _relative(got: torch.Tensor, want: torch.Tensor) -> float:
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


@pytest.mark.parametrize("p", [0.0, 0.5])
def test_rule_equals_autograd_on_the_literal_network_with_and_without_its_own_tape(p: float) -> None:
    clf = seeded_classifier(11)
    raw = seeded_frames(11, 12).double()
    labels = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8], dtype=torch.int32)
    keep = dropout_mask_reference(7, 2, 12, 128, p)
    for act in (3, 0):
        images = clf.images(raw, act)
        loss, grads = literal_step(clf, images, labels, keep, p)
        ref = tape_reference(clf, raw, act)
        for tape in (None, ref.tape):
            got_loss, stats, got = DigitTrainer.rule(clf, raw, labels, keep, p, act, None, tape)
            assert abs(float(got_loss - loss)) <= 1e-12 * abs(float(loss))
            assert float(stats.count) == 12.0 and abs(float(stats.nll_sum) - 12.0 * float(loss)) <= 1e-11 * abs(float(loss))  # noqa: PLR2004
            for name, g, w in zip(PARAMETERS, got, grads, strict=True):
                assert _relative(g, w) <= 1e-12, (name, act, tape is not None)


def test_rule_skips_dead_rows_and_follows_select() -> None:
    clf = seeded_classifier(12)
    raw = seeded_frames(12, 9).double()
    labels = torch.tensor([3, -1, 4, -1, 5, 9, -1, 6, 5], dtype=torch.int32)
    live = labels >= 0
    poisoned = raw.clone()
    poisoned[~live] = float("nan")
    full = DigitTrainer.rule(clf, poisoned, labels, None, 0.0, 3)
    part = DigitTrainer.rule(clf, raw[live], labels[live], None, 0.0, 3)
    assert float(full[1].count) == float(live.sum()) and float(full[0]) == pytest.approx(float(part[0]), rel=1e-13)
    for g, w in zip(full[2], part[2], strict=True):
        assert _relative(g, w) <= 1e-12
    select = torch.tensor([4, 4, 0, 8], dtype=torch.int32)
    picked = DigitTrainer.rule(clf, raw, labels[select.long()], None, 0.0, 3, select)
    copied = DigitTrainer.rule(clf, raw[select.long()], labels[select.long()], None, 0.0, 3)
    for g, w in zip(picked[2], copied[2], strict=True):
        assert torch.equal(g, w)
    none = DigitTrainer.rule(clf, raw, torch.full((9,), -1, dtype=torch.int32), None, 0.0, 3)
    assert float(none[0]) == 0.0 and float(none[1].count) == 0.0 and all(not bool(g.any()) for g in none[2])


def test_tape_reference_names_the_first_maximum_and_the_dead_units() -> None:
    clf = DigitClassifier()
    clf.conv1.weight.fill_(0.0)
    clf.conv1.bias.fill_(1.0)       # conv1 is 1 everywhere: every window ties, member 0
    clf.conv2.weight.fill_(0.0)
    clf.conv2.bias.fill_(0.0)       # conv2 is 0 everywhere: max + bias <= 0, dead
    ref = tape_reference(clf, torch.zeros(2, 1024), 0)
    assert ref.tape.dtype == torch.uint8 and tuple(ref.tape.shape) == (2, TAPE)
    assert not bool(ref.tape[:, :TAPE_CONV1].any()) and bool((ref.tape[:, TAPE_CONV1:] == DEAD).all())
    clf.conv1.weight[:, 0, 1, 1] = 1.0  # conv1 = 1 + x: a single bright pixel at (5, 8) wins member (1, 0) of window (2, 4)
    raw = torch.full((1, 32, 32), -1.0)
    raw[0, 5, 8] = 1.0
    ref = tape_reference(clf, raw.reshape(1, 1024), 0)
    t1 = ref.tape[0, :TAPE_CONV1].reshape(32, 16, 16)
    assert bool((t1[:, 2, 4] == 2).all()) and int((t1 != 0).sum()) == 32  # noqa: PLR2004


def test_dropout_masks_are_the_philox_words() -> None:
    seed, step = (5 << 32) | 77, 9
    rows = torch.tensor([0, 1, 2, 1000, 2**31 + 5], dtype=torch.int64)
    mask = dropout_mask_reference(seed, step, rows, 128, 0.5)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (5, 128)
    key = stream_key(seed, 3)
    for i, r in enumerate(rows.tolist()):
        for j in (0, 1, 2, 3, 4, 63, 64, 127):
            w = int(philox4x32_10((j >> 2, r & 0xFFFFFFFF, step, 0), key)[j & 3])
            assert bool(mask[i, j]) == ((w >> 8) * 2.0 ** -24 >= 0.5), (r, j)  # noqa: PLR2004
    big = dropout_mask_reference(seed, step, 512, 128, 0.5)  # 2^16 units
    share = float(big.double().mean())
    print("keep share at p = 0.5 over 2^16 units", share)
    assert abs(share - 0.5) <= 4.0 * 0.5 / 2 ** 8  # 4 sigma of a fair coin over 2^16 draws
    assert torch.equal(big[:3], mask[:3])  # a count names rows 0 .. n - 1
    assert bool(dropout_mask_reference(seed, step, 7, 128, 0.0).all())
    assert not torch.equal(dropout_mask_reference(seed, step + 1, 512, 128, 0.5), big)
    assert not torch.equal(big[0], big[1]) and not torch.equal(dropout_mask_reference(seed + 1, step, 512, 128, 0.5), big)
    quarter = float(dropout_mask_reference(seed, step, 512, 128, 0.25).double().mean())
    assert abs(quarter - 0.75) <= 4.0 * (0.25 * 0.75) ** 0.5 / 2 ** 8
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        dropout_mask_reference(seed, step, 4, 128, 1.0)


def test_trainer_life_cycle_and_the_checkpoint_it_leaves(tmp_path) -> None:  # noqa: ANN001
    clf = DigitClassifier()
    clf.load_state_dict(seeded_classifier(3).state_dict())
    before = {k: v.clone() for k, v in clf.state_dict().items()}
    assert not any(p.requires_grad for p in clf.parameters()) and not clf.training
    raw, labels = memorise_set()
    with DigitTrainer(clf, dropout=0.5, seed=1) as trainer:
        assert all(p.requires_grad for p in clf.parameters()) and clf.training
        assert all(p.data_ptr() == trainer.flat.param.data_ptr() + 4 * off for p, off in zip(trainer.flat.params, trainer.flat.offsets, strict=True))
        stats = trainer.step(raw, labels, act=3)
        assert float(stats.count) == 40.0 and float(stats.nll_sum) > 0.0 and trainer.steps == 1  # noqa: PLR2004
        again = trainer.step(raw, labels, act=3, select=torch.arange(0, 40, 3, dtype=torch.int32))
        assert float(again.count) == 14.0  # noqa: PLR2004
    assert not any(p.requires_grad for p in clf.parameters()) and not clf.training and all(p.grad is None for p in clf.parameters())
    assert any(not torch.equal(v, before[k]) for k, v in clf.state_dict().items())
    with pytest.raises(RuntimeError, match="closed"):
        trainer.step(raw, labels, act=3)
    digits = clf.digits(raw, 3)  # the frozen classifier reads as before
    assert digits.dtype == torch.int32 and tuple(digits.shape) == (40,)
    path = tmp_path / "mnist_cnn.pt"
    torch.save(clf.state_dict(), path)
    fresh = DigitClassifier()
    result = fresh.load_state_dict(torch.load(path, weights_only=True), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(fresh.digits(raw, 3), digits)
    with pytest.raises(TypeError, match="DigitClassifier"):
        DigitTrainer(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        DigitTrainer(DigitClassifier(), dropout=1.0)


def test_host_step_is_adam_on_the_rule() -> None:
    clf = DigitClassifier()
    clf.load_state_dict(seeded_classifier(3).state_dict())
    twin = seeded_classifier(3).double().requires_grad_(True)
    raw, labels = memorise_set()
    opt = torch.optim.Adam(twin.parameters(), lr=1e-3)
    with DigitTrainer(clf, dropout=0.5, seed=9) as trainer:
        for step in range(2):
            keep = dropout_mask_reference(9, step, 40, 128, 0.5)
            _, _, grads = DigitTrainer.rule(twin, raw, labels, keep, 0.5, 3)
            for p, g in zip((dict(twin.named_parameters())[k] for k in PARAMETERS), grads, strict=True):
                p.grad = g
            opt.step()
            trainer.step(raw, labels, act=3)
    for k, v in clf.state_dict().items():
        np.testing.assert_allclose(v.numpy(), twin.state_dict()[k].numpy(), rtol=0, atol=2e-6, err_msg=k)


def test_the_host_path_memorises_forty_frames() -> None:
    steps = memorise("cpu", MEMORISE_STEPS)
    print("steps to 100 % training accuracy on the host", steps)
    assert steps <= MEMORISE_STEPS


@pytest.mark.parametrize("seed", [100, 101])
def test_few_tape_entries_are_within_the_feature_bound_of_another_choice(seed: int) -> None:
    ref = digit_set(seed)
    tape = tape_reference(ref["clf"], ref["raw"][:TAPE_FRAMES], 3)
    unsure = tape.uncertain(LOGIT_BOUND)
    share1, share2 = float(unsure[:, :TAPE_CONV1].double().mean()), float(unsure[:, TAPE_CONV1:].double().mean())
    print("seed", seed, "uncertain share conv1", share1, "conv2", share2, "scales", tape.scales)
    assert share1 <= EXEMPT_CAP and share2 <= EXEMPT_CAP
    assert 0.05 < float((tape.tape == DEAD).double().mean()) < 0.95  # noqa: PLR2004  (both kinds of unit occur)


def test_the_training_tool_writes_a_checkpoint_the_evaluation_loads(tmp_path, monkeypatch, capsys) -> None:  # noqa: ANN001
    import importlib.util
    import sys
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("train_digit_classifier", Path(__file__).resolve().parents[1] / "tools" / "train_digit_classifier.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    raw, labels = memorise_set()
    images = ((torch.tanh(raw.double()) + 1.0) * 127.5).round().reshape(40, 1, 32, 32).numpy().astype(np.uint8)
    lab = labels.numpy().astype(np.int64)
    for i in range(2):  # two episodes of 24 frames: 20 labelled, 4 silent
        silent = np.full(4, -1, dtype=np.int64)
        np.savez(tmp_path / f"ep{i}.npz", image=np.concatenate([images[20 * i : 20 * i + 20], images[:4]]), label=np.concatenate([lab[20 * i : 20 * i + 20], silent]))
    frames, got = tool.load_labelled_frames(tmp_path)
    assert tuple(frames.shape) == (40, 1024) and torch.equal(got, labels) and float(frames.min()) >= -1.0 and float(frames.max()) <= 1.0
    out = tmp_path / "out" / "mnist_cnn.pt"
    monkeypatch.setattr(sys, "argv", ["train_digit_classifier.py", "--data-dir", str(tmp_path), "--output", str(out), "--epochs", "2", "--batch-size", "12",
                                      "--holdout", "0.1", "--seed", "3", "--device", "cpu"])
    tool.main()
    text = capsys.readouterr().out
    assert "36 to fit on, 4 held out" in text and "epoch 2:" in text and "held-out loss" in text and "strict=True" in text
    clf = DigitClassifier()
    result = clf.load_state_dict(torch.load(out, weights_only=True), strict=True)
    assert not result.missing_keys and not result.unexpected_keys and all(bool(torch.isfinite(v).all()) for v in clf.state_dict().values())


def test_bad_arguments_of_the_new_entry_points_are_rejected_without_a_launch() -> None:
    from multimodal_mtrssm_amd import _lib

    lib = _lib.load()
    keep = torch.zeros(64)
    buf = (keep.data_ptr() + 15) // 16 * 16  # a 16-byte aligned host address: every call returns before a launch

    def features(**kw) -> int:  # noqa: ANN003
        a = {"pred": buf, "frames": 4, "select": None, "N": 4, "act": 3, "w1": buf, "b1": buf, "w2": buf, "b2": buf, "out": buf, "tape": buf} | kw
        return lib.mtrssm_digit_features_train(a["pred"], a["frames"], a["select"], a["N"], a["act"], a["w1"], a["b1"], a["w2"], a["b2"], a["out"], a["tape"], None)

    for name, bad in (("tape", None), ("pred", None), ("N", 5), ("act", 1), ("out", buf + 8)):
        assert features(**{name: bad}) == -1 and b"digit_features" in lib.mtrssm_last_error(), (name, bad)

    def trunk(**kw) -> int:  # noqa: ANN003
        a = {"pred": buf, "frames": 4, "select": None, "N": 4, "act": 0, "tape": buf, "g": buf, "labels": buf, "w1": buf, "b1": buf, "w2": buf, "gw1": buf,
             "gb1": buf, "gw2": buf, "gb2": buf, "acc": 0, "ws": buf, "bytes": 1 << 30} | kw
        return lib.mtrssm_digit_trunk_bwd(a["pred"], a["frames"], a["select"], a["N"], a["act"], a["tape"], a["g"], a["labels"], a["w1"], a["b1"], a["w2"],
                                          a["gw1"], a["gb1"], a["gw2"], a["gb2"], a["acc"], a["ws"], a["bytes"], None)

    for name, bad in (("pred", None), ("tape", None), ("g", None), ("labels", None), ("w1", None), ("b1", None), ("w2", None), ("gw1", None), ("gb2", None),
                      ("ws", None), ("frames", 0), ("N", 0), ("N", 5), ("N", 1 << 31), ("act", 2), ("acc", 2), ("tape", buf + 4), ("g", buf + 8),
                      ("labels", buf + 2), ("bytes", 16)):
        assert trunk(**{name: bad}) == -1 and b"digit_trunk_bwd" in lib.mtrssm_last_error(), (name, bad)
    assert lib.mtrssm_digit_trunk_bwd_workspace_bytes(0) == -1 and lib.mtrssm_digit_trunk_bwd_workspace_bytes(1) == 21056 * 4
    assert lib.mtrssm_digit_head_train_workspace_bytes(0) == -1 and lib.mtrssm_digit_head_train_workspace_bytes(4) == 1293 * 4

    def head(**kw) -> int:  # noqa: ANN003
        a = {"h": buf, "w": buf, "b": buf, "labels": buf, "rows": None, "N": 4, "row0": 0, "step": 0, "p": 0.5, "norm": 1, "stats": buf, "gh": buf, "gw": buf,
             "gb": buf, "acc": 0, "ws": buf, "bytes": 1 << 30} | kw
        return lib.mtrssm_digit_head_train(a["h"], a["w"], a["b"], a["labels"], a["rows"], a["N"], a["row0"], a["step"], 1, 2, a["p"], a["norm"], None, None,
                                           a["stats"], a["gh"], a["gw"], a["gb"], a["acc"], a["ws"], a["bytes"], None)

    for name, bad in (("h", None), ("w", None), ("labels", None), ("stats", None), ("gh", None), ("gw", None), ("ws", None), ("N", 0), ("N", 1 << 31),
                      ("row0", -1), ("row0", 1 << 32), ("step", -1), ("step", 1 << 32), ("p", 1.0), ("p", -0.1), ("p", float("nan")), ("norm", 2), ("acc", -1),
                      ("rows", buf + 2), ("bytes", 16)):
        assert head(**{name: bad}) == -1 and b"digit_head_train" in lib.mtrssm_last_error(), (name, bad)
