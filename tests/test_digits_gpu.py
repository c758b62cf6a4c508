"""GPU (MI355X): the digit reader's kernels against the float64 rule.

Bounds.  Logits: ``1e-4 * max |logit|`` of the set, the project's north-star tolerance; conv2 and the large
fc1 multiply two bf16 pieces per operand (relative product error about 2^-16 before the fp32 sums average it down), fp32 torch on the
host sits at about 1e-6 of the scale on these inputs.  Digits: equal to the float64 arg-max on every frame whose float64 top-2 margin is at least
``1e-3 * max |logit|`` -- two logits each off by 1e-4 of the scale cannot flip such a frame; at most 2 % of a set may be exempt (the test
asserts the cap).  Features of integer-valued inputs and weights are exact: every product and sum is a small whole number.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd.digits import CLASSES, FEATURES, DigitClassifier, word_counts
from tests.test_digits_host import EXEMPT_CAP, LOGIT_BOUND, SET_FRAMES, SET_SEEDS, digit_set

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _on_device(ref: dict) -> DigitClassifier:
    """A copy of the set's classifier on the GPU (the shared one stays on the host, where the float64 rule runs)."""
    clf = DigitClassifier()
    clf.load_state_dict(ref["clf"].state_dict())
    return clf.to(DEV)


def _assert_logits(got: torch.Tensor, want: torch.Tensor, scale: float, what: str) -> float:
    err = float((got.cpu().double() - want).abs().max())
    print(what, "worst |logit error| / max |logit|", err / scale, "bound", LOGIT_BOUND)
    assert err <= LOGIT_BOUND * scale, f"{what}: {err} > {LOGIT_BOUND * scale}"
    return err


@pytest.mark.parametrize("seed", SET_SEEDS)
def test_logits_and_digits_equal_the_float64_rule(seed: int) -> None:
    ref = digit_set(seed)
    clf = _on_device(ref)
    raw = ref["raw"].to(DEV)
    digit, logits = clf.read(raw, 3)
    digit2, logits2 = clf.read(raw, 3)
    torch.cuda.synchronize()
    assert logits.dtype == torch.float32 and tuple(logits.shape) == (SET_FRAMES, CLASSES) and digit.dtype == torch.int32
    _assert_logits(logits, ref["logits"], ref["scale"], f"seed {seed}")
    certain = ref["certain"]
    exempt = 1.0 - float(certain.double().mean())
    counts = torch.bincount(ref["digits"].long(), minlength=CLASSES)
    print("seed", seed, "digits", counts.tolist(), "exempt share", exempt)
    assert exempt <= EXEMPT_CAP and int(counts.min()) > 0
    assert torch.equal(digit.cpu()[certain], ref["digits"][certain])
    assert torch.equal(digit.cpu(), DigitClassifier.first_max(logits.cpu()))  # the head's arg-max is its own logits' first maximum
    assert torch.equal(digit, digit2) and torch.equal(logits, logits2)  # two back-to-back calls agree bitwise
    assert torch.equal(clf.digits(raw, 3), digit) and torch.equal(clf.logits(raw.reshape(4, SET_FRAMES // 4, 1, 32, 32), 3), logits)


def test_frame_loop_tails_and_select() -> None:
    ref = digit_set(SET_SEEDS[0])
    clf = _on_device(ref)
    raw = ref["raw"].to(DEV)
    full = clf.features(raw, 3)
    again = clf.features(raw, 3)
    want = ref["clf"].reference_features(ref["raw"].double(), 3)
    torch.cuda.synchronize()
    assert torch.equal(full, again)
    fscale = float(want.abs().max())
    ferr = float((full.cpu().double() - want).abs().max())
    print("features worst error / max", ferr / fscale)
    assert ferr <= LOGIT_BOUND * fscale
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for n in (1, 3, cus + 1):  # one workgroup, fewer frames than workgroups, one workgroup with a second frame
        assert n <= SET_FRAMES
        part = clf.features(raw[:n], 3)
        assert torch.equal(part, full[:n]), n  # a frame's features depend on that frame only
        digit, logits = clf.read(raw[:n], 3)
        _assert_logits(logits, ref["logits"][:n], ref["scale"], f"N = {n}")
        keep = ref["certain"][:n]
        assert torch.equal(digit.cpu()[keep], ref["digits"][:n][keep]), n
    # forward(): already denormalised images in [0, 1] through the same launch
    images = ref["clf"].images(ref["raw"][:300], 3)
    _assert_logits(clf(images.to(DEV)), ref["logits"][:300], ref["scale"], "forward(images)")
    # select: a draw with repeats, out of a [B * S, T] decode's frames
    g = torch.Generator().manual_seed(1)
    select = torch.randint(0, SET_FRAMES, (700,), generator=g).to(torch.int32)
    select[:3] = torch.tensor([SET_FRAMES - 1, 0, SET_FRAMES - 1], dtype=torch.int32)
    assert select.unique().numel() < select.numel()
    picked = clf.features(raw.reshape(32, 64, 1, 32, 32), 3, select.to(DEV))
    assert torch.equal(picked, full[select.long().to(DEV)])
    digit, logits = clf.read(raw, 3, select.to(DEV))
    _assert_logits(logits, ref["logits"][select.long()], ref["scale"], "select")
    keep = ref["certain"][select.long()]
    assert torch.equal(digit.cpu()[keep], ref["digits"][select.long()][keep])
    # an index outside the decode reads nothing: NaN features, the failure bin
    bad = torch.tensor([3, SET_FRAMES, -1, 5], dtype=torch.int32, device=DEV)
    feats = clf.features(raw, 3, bad)
    digit, logits = clf.read(raw, 3, bad)
    assert bool(feats[1:3].isnan().all()) and torch.equal(feats[[0, 3]], full[[3, 5]])
    assert digit.tolist()[1:3] == [CLASSES, CLASSES] and bool(logits[1:3].isnan().all()) and bool(torch.isfinite(logits[[0, 3]]).all())


def test_saturated_frames_take_the_halo_and_bias_only_paths() -> None:
    ref = digit_set(SET_SEEDS[0])
    clf = _on_device(ref)
    raw = torch.stack([torch.full((1024,), -40.0), torch.full((1024,), 40.0), torch.full((1024,), -1e30), torch.full((1024,), 1e30)])
    for act in (3, 0):  # Tanh's flat ends; Identity: the clamp
        want_f = ref["clf"].reference_features(raw.double(), act)
        want = ref["clf"].reference_logits(raw.double(), act)
        got_f = clf.features(raw.to(DEV), act)
        _, got = clf.read(raw.to(DEV), act)
        assert bool(torch.isfinite(got).all())
        images = clf.images(raw.to(DEV), act)
        assert not bool(images[0].any()) and bool((images[1] == 1.0).all())  # x = 0 and x = 1 everywhere
        np.testing.assert_allclose(got_f.cpu().double().numpy(), want_f.numpy(), rtol=0, atol=LOGIT_BOUND * float(want_f.abs().max()), err_msg=str(act))
        _assert_logits(got, want, max(ref["scale"], float(want.abs().max())), f"saturated act {act}")
        # x = 0 everywhere: conv1 is its bias, the same at every pixel; the pooled image's halo shows at conv2's border only
        f0 = got_f[0].reshape(64, 8, 8)
        assert torch.equal(f0[:, 1:7, 1:7], f0[:, 1:2, 1:2].expand(64, 6, 6))


@pytest.mark.parametrize("weights", ["ones", "graded"])
def test_one_hot_pixels_pin_the_pool_windows_the_halo_and_the_view_order(weights: str) -> None:
    clf = DigitClassifier()
    if weights == "ones":
        for p in (clf.conv1.weight, clf.conv1.bias, clf.conv2.weight, clf.conv2.bias):
            p.fill_(1.0)
    else:  # small whole numbers that tell channels and taps apart (every product and sum stays a whole number below 2^16)
        c1, c2 = torch.arange(32.0), torch.arange(64.0)
        taps = torch.arange(9.0).reshape(3, 3)
        clf.conv1.weight.copy_(((c1[:, None, None] + taps) % 4.0).reshape(32, 1, 3, 3))
        clf.conv1.bias.copy_(c1 % 3.0)
        clf.conv2.weight.copy_(((c2[:, None, None, None] + 2.0 * c1[None, :, None, None] + taps) % 5.0) - 1.0)
        clf.conv2.bias.copy_(c2 % 7.0 - 3.0)
    spots = [(0, 0), (0, 31), (31, 0), (31, 31), (15, 15), (16, 16), (7, 22)]
    raw = torch.full((len(spots), 32, 32), -1.0)
    for i, (y, x) in enumerate(spots):
        raw[i, y, x] = 1.0
    raw = raw.reshape(len(spots), 1024)
    want = clf.reference_features(raw, 0)  # fp32 torch on whole numbers: exact
    assert torch.equal(want, clf.reference_features(raw.double(), 0).float()) and float(want.abs().max()) < 1 << 16
    got = clf.to(DEV).features(raw.to(DEV), 0)
    assert tuple(got.shape) == (len(spots), FEATURES) and torch.equal(got.cpu(), want)
    if weights == "graded":
        assert len({tuple(r.tolist()) for r in want}) == len(spots)  # the spots are told apart


def test_head_ties_take_the_lowest_index_and_the_logits_are_optional() -> None:
    ref = digit_set(SET_SEEDS[0])
    clf = DigitClassifier()
    clf.load_state_dict(ref["clf"].state_dict())
    clf.fc2.weight[7] = clf.fc2.weight[2]
    clf.fc2.bias[7] = clf.fc2.bias[2]
    clf.fc2.weight[9] = clf.fc2.weight[0]
    clf.fc2.bias[9] = clf.fc2.bias[0]
    clf.to(DEV)
    raw = ref["raw"][:512].to(DEV)
    digit, logits = clf.read(raw, 3)
    bare, none = clf.read(raw, 3, want_logits=False)
    assert none is None and torch.equal(bare, digit)
    assert torch.equal(logits[:, 7], logits[:, 2]) and torch.equal(logits[:, 9], logits[:, 0])
    assert not bool(((digit == 7) | (digit == 9)).any()) and bool(((digit == 2) | (digit == 0)).any())  # noqa: PLR2004
    assert torch.equal(digit.cpu().long(), torch.max(logits.cpu(), 1).indices)


@pytest.mark.parametrize("n", [1, 70000])
def test_word_counts_equal_bincount(n: int) -> None:
    g = torch.Generator().manual_seed(n)
    word = torch.randint(-1, 10, (n,), generator=g).to(torch.int32)
    digit = torch.randint(0, 11, (n,), generator=g).to(torch.int32)
    if n == 1:
        word[0] = 4
    keep = word >= 0
    want = torch.bincount(word[keep].long() * 11 + digit[keep].long(), minlength=110).reshape(10, 11).float()
    got, again = torch.zeros(10, 11, device=DEV), torch.zeros(10, 11, device=DEV)
    word_counts(word.to(DEV), digit.to(DEV), got)
    word_counts(word.to(DEV), digit.to(DEV), again)
    assert torch.equal(got.cpu(), want) and torch.equal(got, again) and float(got.sum()) == float(keep.sum())
    word_counts(word.to(DEV), digit.to(DEV), got)  # IN/OUT: a second batch adds onto the first
    assert torch.equal(got.cpu(), 2 * want)
    silent = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    word_counts(silent, digit.to(DEV), got)
    assert torch.equal(got.cpu(), 2 * want)  # silence adds nothing
