"""GPU (MI355X): the kernels that train the digit reader against the float64 rule.

Bounds.  Gradients: ``2e-4`` of the tensor's largest entry, the project's gradient tolerance; the rule is given the
kernel's OWN tape, so near a pool tie or a ReLU zero both sides route the same way and the comparison is one of arithmetic only.  Tape:
equal to the float64 choice on every unit that two members each within the feature bound (``1e-4`` of the layer's scale) cannot flip;
at most 2 % of a layer's units may be exempt (asserted).  Whole-number weights and frames: everything is exact, ties included.  Losses:
``1e-5`` relative (fp32 ``expf`` / ``logf`` on ten logits).
"""

from __future__ import annotations

import pytest
import torch

from multimodal_mtrssm_amd import DigitTrainer, dropout_mask_reference, tape_reference
from multimodal_mtrssm_amd.dataset import stream_key
from multimodal_mtrssm_amd.digit_train import (
    DEAD,
    PARAMETERS,
    TAPE,
    TAPE_CONV1,
    features_train,
    head_rule,
    head_train,
    trunk_backward,
    trunk_rule,
)
from multimodal_mtrssm_amd.digits import FEATURES, DigitClassifier
from tests.test_digit_train_host import MEMORISE_STEPS, TAPE_FRAMES, memorise
from tests.test_digits_host import EXEMPT_CAP, LOGIT_BOUND, digit_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAD_BOUND = 2e-4
TRUNK = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")


def _on_device(clf: DigitClassifier) -> DigitClassifier:
    copy = DigitClassifier()
    copy.load_state_dict(clf.state_dict())
    return copy.to(DEV)


def _cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_grads(got, want, names, what: str) -> None:  # noqa: ANN001
    for name, g, w in zip(names, got, want, strict=True):
        scale = float(w.abs().max())
        err = float((g.detach().cpu().double().reshape(w.shape) - w).abs().max())
        print(what, name, "worst error / largest entry", err / max(scale, 1e-300), "bound", GRAD_BOUND)
        assert err <= GRAD_BOUND * scale, f"{what} {name}: {err} > {GRAD_BOUND * scale}"


def _graded() -> DigitClassifier:
    """``test_digits_gpu``'s small whole numbers that tell channels and taps apart."""
    clf = DigitClassifier()
    c1, c2 = torch.arange(32.0), torch.arange(64.0)
    taps = torch.arange(9.0).reshape(3, 3)
    clf.conv1.weight.copy_(((c1[:, None, None] + taps) % 4.0).reshape(32, 1, 3, 3))
    clf.conv1.bias.copy_(c1 % 3.0)
    clf.conv2.weight.copy_(((c2[:, None, None, None] + 2.0 * c1[None, :, None, None] + taps) % 5.0) - 1.0)
    clf.conv2.bias.copy_(c2 % 7.0 - 3.0)
    return clf


def test_training_forward_features_are_the_inference_features_and_the_tape_is_the_float64_choice() -> None:
    ref = digit_set(100)
    clf = _on_device(ref["clf"])
    raw = ref["raw"][:TAPE_FRAMES].to(DEV)
    full = clf.features(raw, 3)
    feats, tape = features_train(clf, raw, 3)
    feats2, tape2 = features_train(clf, raw, 3)
    torch.cuda.synchronize()
    assert tape.dtype == torch.uint8 and tuple(tape.shape) == (TAPE_FRAMES, TAPE) and tuple(feats.shape) == (TAPE_FRAMES, FEATURES)
    assert torch.equal(feats, full) and torch.equal(feats, feats2) and torch.equal(tape, tape2)
    assert _cus() + 1 <= TAPE_FRAMES
    for n in (1, 3, _cus() + 1):
        f, t = features_train(clf, raw[:n], 3)
        assert torch.equal(f, full[:n]) and torch.equal(t, tape[:n]), n
    select = torch.tensor([TAPE_FRAMES - 1, 0, TAPE_FRAMES - 1, 17, 5, 17, 250], dtype=torch.int32, device=DEV)
    f, t = features_train(clf, raw, 3, select)
    assert torch.equal(f, full[select.long()]) and torch.equal(t, tape[select.long()]) and torch.equal(f, clf.features(raw, 3, select))
    want = tape_reference(ref["clf"], ref["raw"][:TAPE_FRAMES], 3)
    unsure = want.uncertain(LOGIT_BOUND)
    share1, share2 = float(unsure[:, :TAPE_CONV1].double().mean()), float(unsure[:, TAPE_CONV1:].double().mean())
    differ = tape.cpu() != want.tape
    print("uncertain share conv1", share1, "conv2", share2, "entries that differ from float64 (all uncertain)", int(differ.sum()))
    assert share1 <= EXEMPT_CAP and share2 <= EXEMPT_CAP
    assert not bool((differ & ~unsure).any())
    assert int(tape.max()) <= DEAD
    for act in (0,):  # Identity: the clamp makes exact ties; the features stay the inference features
        f, _ = features_train(clf, raw, act)
        assert torch.equal(f, clf.features(raw, act))


def _exact_frames() -> torch.Tensor:
    spots = [(0, 0), (0, 31), (31, 0), (31, 31), (15, 15), (16, 16), (7, 22)]
    raw = torch.full((3 + len(spots), 32, 32), -1.0)
    raw[1] = 1.0
    raw[2] = 0.0  # x = 0, 1 and 0.5 everywhere: every interior window ties
    for i, (y, x) in enumerate(spots):
        raw[3 + i, y, x] = 1.0
    return raw.reshape(-1, 1024)


def test_ties_and_dead_units_on_exact_arithmetic() -> None:
    host = _graded()
    raw = _exact_frames()
    n = raw.shape[0]
    want_tape = tape_reference(host, raw, 0)
    interior = want_tape.tape[:3, :TAPE_CONV1].reshape(3, 32, 16, 16)[:, :, 1:15, 1:15]
    assert bool(((interior == 0) | (interior == DEAD)).all()) and float(want_tape.margin[:3, :TAPE_CONV1].reshape(3, 32, 16, 16)[:, :, 1:15, 1:15].max()) == 0.0
    clf = _on_device(host)
    feats, tape = features_train(clf, raw.to(DEV), 0)
    assert torch.equal(feats.cpu(), host.reference_features(raw, 0))
    assert torch.equal(tape.cpu(), want_tape.tape)  # exact ties included: the first member in row-major order
    g = torch.randint(-3, 4, (n, FEATURES), generator=torch.Generator().manual_seed(2)).float()
    labels = torch.zeros(n, dtype=torch.int32)
    want = trunk_rule(host, raw, labels, g, 0)  # torch's own max_pool2d / relu backward, float64
    assert all(float(w.abs().max()) < 1 << 24 for w in want)
    got = trunk_backward(clf, raw.to(DEV), tape, g.to(DEV), labels.to(DEV), 0)
    for name, a, w in zip(TRUNK, got, want, strict=True):
        assert torch.equal(a.cpu().double(), w), name
    with_tape = trunk_rule(host, raw, labels, g, 0, None, want_tape.tape)
    for a, w in zip(with_tape, want, strict=True):
        assert torch.equal(a, w)


@pytest.mark.parametrize("act", [3, 0])
@pytest.mark.parametrize("seed", [100, 101])
def test_trunk_backward_equals_the_rule_with_the_kernels_own_tape(seed: int, act: int) -> None:
    ref = digit_set(seed)
    clf = _on_device(ref["clf"])
    n = _cus() + 1  # one workgroup walks two frames
    raw_host = ref["raw"][:n]
    raw = raw_host.to(DEV)
    g_host = torch.randn(n, FEATURES, generator=torch.Generator().manual_seed(seed + act))
    g = g_host.to(DEV)
    labels_host = torch.zeros(n, dtype=torch.int32)
    labels = labels_host.to(DEV)
    _, tape = features_train(clf, raw, act)
    got = trunk_backward(clf, raw, tape, g, labels, act)
    again = trunk_backward(clf, raw, tape, g, labels, act)
    torch.cuda.synchronize()
    for a, b in zip(got, again, strict=True):
        assert torch.equal(a, b)  # two calls agree bitwise
    want = trunk_rule(ref["clf"], raw_host, labels_host, g_host, act, None, tape.cpu())
    _assert_grads(got, want, TRUNK, f"seed {seed} act {act} N {n}")
    for few in (1, 3):  # fewer frames than workgroups
        part = trunk_backward(clf, raw[:few], tape[:few].contiguous(), g[:few].contiguous(), labels[:few], act)
        _assert_grads(part, trunk_rule(ref["clf"], raw_host[:few], labels_host[:few], g_host[:few], act, None, tape[:few].cpu()), TRUNK, f"N {few}")
    if (seed, act) != (100, 3):
        return
    # select with repeats: rows of a larger decode, no copy
    select_host = torch.tensor([n - 1, 0, n - 1, 9, 200, 9, 31, 31, 31, 77], dtype=torch.int32)
    select = select_host.to(DEV)
    m = select_host.numel()
    _, tape_s = features_train(clf, raw, act, select)
    picked = trunk_backward(clf, raw, tape_s, g[:m].contiguous(), labels[:m], act, select)
    _assert_grads(picked, trunk_rule(ref["clf"], raw_host, labels_host[:m], g_host[:m], act, select_host, tape_s.cpu()), TRUNK, "select")
    # a third of the rows dead: the same call on the live frames alone (at most one frame per workgroup, and an absent frame's partial
    # set is zeros: the sums meet in the same order), NaN pixels in the dead frames change nothing
    m = 48
    dead = torch.arange(m) % 3 == 1
    lab = torch.where(dead, torch.tensor(-1), torch.arange(m) % 10).to(torch.int32)
    frames, gm, tm = raw[:m].clone(), g[:m].contiguous(), tape[:m].contiguous()
    mixed = trunk_backward(clf, frames, tm, gm, lab.to(DEV), act)
    live = (~dead).to(DEV)
    alone = trunk_backward(clf, frames[live], tm[live], gm[live], lab[~dead].to(DEV), act)
    frames[dead.to(DEV)] = float("nan")
    poisoned = trunk_backward(clf, frames, tm, torch.where(live[:, None], gm, torch.full_like(gm, float("nan"))), lab.to(DEV), act)
    for a, b, c in zip(mixed, alone, poisoned, strict=True):
        assert torch.equal(a, b) and torch.equal(a, c) and bool(torch.isfinite(a).all())
    _assert_grads(mixed, trunk_rule(ref["clf"], raw_host[:m], lab, g_host[:m], act, None, tm.cpu()), TRUNK, "a third dead")
    none = trunk_backward(clf, frames, tm, gm, torch.full((m,), -1, dtype=torch.int32, device=DEV), act)
    assert all(not bool(a.any()) for a in none)
    # accumulate adds onto what the buffers hold
    filled = tuple(torch.full_like(a, 1.5) for a in mixed)
    trunk_backward(clf, raw[:m], tm, gm, lab.to(DEV), act, grads=filled, accumulate=True)
    fresh = trunk_backward(clf, raw[:m], tm, gm, lab.to(DEV), act)
    for a, b in zip(filled, fresh, strict=True):
        assert torch.equal(a, b + 1.5)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("n", [1, 7, 1100])
def test_head_in_training_mode_equals_the_rule(n: int, p: float) -> None:
    ref = digit_set(100)
    gen = torch.Generator().manual_seed(n)
    hidden = torch.randn(n, 128, generator=gen).abs() + 0.1  # every unit is active: g_hidden vanishes only where the mask does
    labels = torch.randint(0, 10, (n,), generator=gen).to(torch.int32)
    if n > 1:
        labels[1::5] = -1
    live = labels >= 0
    rows = (torch.arange(n) * 3 + 7).to(torch.int32)
    seed, step = (3 << 32) | 12345, 6
    keep = dropout_mask_reference(seed, step, rows, 128, p)
    w, b = ref["clf"].fc2.weight, ref["clf"].fc2.bias
    for normalize in (True, False):
        want = head_rule(hidden, w, b, labels, keep, p, normalize)
        got = head_train(hidden.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV), rows=rows.to(DEV), step=step, key=stream_key(seed, 3), p=p,
                         normalize=normalize, planes=True)
        again = head_train(hidden.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV), rows=rows.to(DEV), step=step, key=stream_key(seed, 3), p=p,
                           normalize=normalize, planes=True)
        torch.cuda.synchronize()
        assert all(torch.equal(a, c) for a, c in zip(got, again, strict=True))
        scale = max(float(want.nll.abs().max()), 1.0)
        assert float((got.nll.cpu().double() - want.nll).abs().max()) <= 1e-5 * scale
        assert float(got.stats[2]) == float(live.sum()) and abs(float(got.stats[0]) - float(want.stats[0])) <= 1e-5 * max(float(want.stats[0]), 1.0)
        # pred: the first maximum; equal to float64's wherever its top-2 margin exceeds the logit bound
        z = (hidden.double() * keep.double() / (1.0 - p)) @ w.double().T + b.double()
        top2 = z.topk(2, dim=1).values
        sure = live & ((top2[:, 0] - top2[:, 1]) > LOGIT_BOUND * float(z.abs().max()))
        assert torch.equal(got.pred.cpu()[sure], want.pred[sure]) and bool((got.pred.cpu()[~live] == -1).all())
        if bool(sure[live].all()):
            assert float(got.stats[1]) == float(want.stats[1])
        _assert_grads((got.g_hidden, got.g_weight, got.g_bias), (want.g_hidden, want.g_weight, want.g_bias), ("g_hidden", "g_fc2.weight", "g_fc2.bias"),
                      f"head N {n} p {p} normalize {normalize}")
        assert torch.equal((got.g_hidden.cpu() != 0)[live], keep[live])  # the kernel's keep-mask, bit for bit
        assert not bool(got.g_hidden.cpu()[~live].any()) and not bool(got.nll.cpu()[~live].any())  # dead rows are exactly zero
    none = head_train(hidden.to(DEV), w.to(DEV), b.to(DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV), p=p, key=stream_key(seed, 3))
    assert not bool(none.stats.any()) and not bool(none.g_weight.any()) and not bool(none.g_bias.any()) and not bool(none.g_hidden.any())
    filled = (torch.full((10, 128), 2.0, device=DEV), torch.full((10,), 2.0, device=DEV))
    head_train(hidden.to(DEV), w.to(DEV), b.to(DEV), labels.to(DEV), rows=rows.to(DEV), step=step, key=stream_key(seed, 3), p=p, normalize=False,
               g_weight=filled[0], g_bias=filled[1], accumulate=True)
    assert torch.equal(filled[0], got.g_weight + 2.0) and torch.equal(filled[1], got.g_bias + 2.0)


def test_one_whole_step_leaves_the_rules_gradients_and_is_reproducible() -> None:
    ref = digit_set(100)
    n = _cus() + 1
    raw_host = ref["raw"][:n]
    labels_host = ref["digits"][:n].clone()
    labels_host[2::7] = -1
    seed = 21
    outcomes = []
    for _ in range(2):
        clf = _on_device(ref["clf"])
        with DigitTrainer(clf, dropout=0.5, seed=seed) as trainer:
            stats = trainer.step(raw_host.to(DEV), labels_host.to(DEV), act=3)
            torch.cuda.synchronize()
            grads = [dict(clf.named_parameters())[k].grad.clone() for k in PARAMETERS]
            tape = trainer._work["tape"].cpu()  # noqa: SLF001
            outcomes.append((grads, trainer.flat.param.clone(), [float(s) for s in stats]))
    for a, b in zip(outcomes[0][0], outcomes[1][0], strict=True):
        assert torch.equal(a, b)
    assert torch.equal(outcomes[0][1], outcomes[1][1]) and outcomes[0][2] == outcomes[1][2]  # bitwise, from the same state
    keep = dropout_mask_reference(seed, 0, n, 128, 0.5)
    loss, want_stats, want = DigitTrainer.rule(ref["clf"], raw_host, labels_host, keep, 0.5, 3, None, tape)
    _assert_grads(outcomes[0][0], want, PARAMETERS, "whole step")
    nll_sum, hits, count = outcomes[0][2]
    assert count == float(want_stats.count) and abs(nll_sum - float(want_stats.nll_sum)) <= 1e-4 * float(want_stats.nll_sum)
    assert 0.0 <= hits <= count and float(loss) == pytest.approx(float(want_stats.nll_sum) / count, rel=1e-12)
    moved = outcomes[0][1].cpu()
    assert bool(torch.isfinite(moved).all()) and not torch.equal(moved[:288], ref["clf"].conv1.weight.reshape(-1))


def test_the_gpu_path_memorises_forty_frames() -> None:
    steps = memorise(DEV, 2 * MEMORISE_STEPS)
    print("steps to 100 % training accuracy on the GPU", steps, "budget", 2 * MEMORISE_STEPS)
    assert steps <= 2 * MEMORISE_STEPS


def test_close_leaves_the_reader_as_it_was() -> None:
    ref = digit_set(100)
    clf = _on_device(ref["clf"])
    raw = ref["raw"][:300].to(DEV)
    digit, logits = clf.read(raw, 3)
    with DigitTrainer(clf, dropout=0.5) as trainer:
        inside = trainer.evaluate(raw, ref["digits"][:300].to(DEV), act=3)
        assert all(p.requires_grad for p in clf.parameters()) and clf.training
    assert not any(p.requires_grad for p in clf.parameters()) and not clf.training
    digit2, logits2 = clf.read(raw, 3)
    assert torch.equal(digit, digit2) and torch.equal(logits, logits2)
    assert float(inside.count) == 300.0 and float(inside.hits) >= 0.97 * 300.0  # noqa: PLR2004  (the labels are the set's own digits)
