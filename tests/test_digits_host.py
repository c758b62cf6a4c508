"""CPU: the digit reader's torch rule, its checkpoint format, the count table's host path and the argument checks of the three entry
points.  Also the seeded inputs the GPU tests share (``digit_set``): random weights collapse onto one digit, so
the frames are noisy copies of 16 smooth prototypes and ``fc2.bias`` is centred on the set's mean logits -- all ten digits then occur
and well under 2 % of the frames have a float64 top-2 margin below ``1e-3 * max |logit|``.
"""

from __future__ import annotations

import functools

import pytest
import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.digits import CLASSES, FEATURES, DigitClassifier, word_counts

SET_FRAMES = 2048
SET_SEEDS = (100, 101, 102, 103)
LOGIT_BOUND = 1e-4   # x max |logit|: the north-star tolerance
MARGIN = 1e-3        # x max |logit|: a frame whose float64 top-2 margin is below this may read either digit
EXEMPT_CAP = 0.02


def seeded_classifier(seed: int) -> DigitClassifier:
    """Weights ``N(0, 2 / fan_in)``, biases ``N(0, 0.01)`` (variances) from a seeded generator."""
    g = torch.Generator().manual_seed(seed)
    clf = DigitClassifier()
    for layer in (clf.conv1, clf.conv2, clf.fc1, clf.fc2):
        fan_in = layer.weight[0].numel()
        layer.weight.copy_(torch.randn(layer.weight.shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5)
        layer.bias.copy_(torch.randn(layer.bias.shape, generator=g, dtype=torch.float64) * 0.1)
    return clf


def seeded_frames(seed: int, n: int) -> torch.Tensor:
    """``raw = proto[idx] + 0.5 N(0, 1)``, 16 prototypes ``2 N(0, 1)`` on 4 x 4 bilinearly upsampled to 32 x 32: fp32 ``[n, 1024]``."""
    g = torch.Generator().manual_seed(seed + 1000)
    proto = F.interpolate(2.0 * torch.randn(16, 1, 4, 4, generator=g, dtype=torch.float64), size=(32, 32), mode="bilinear", align_corners=False)
    idx = torch.randint(0, 16, (n,), generator=g)
    raw = proto[idx].reshape(n, 1024) + 0.5 * torch.randn(n, 1024, generator=g, dtype=torch.float64)
    return raw.float()


@functools.lru_cache(maxsize=None)
def digit_set(seed: int, n: int = SET_FRAMES) -> dict:
    """The shared inputs and their float64 reference (computed once): classifier, raw frames (``act = 3``), logits, digits, the
    scale ``max |logit|`` and the frames whose margin makes their digit certain."""
    clf = seeded_classifier(seed)
    raw = seeded_frames(seed, n)
    clf.fc2.bias -= clf.reference_logits(raw.double(), 3).mean(0).float()
    logits = clf.reference_logits(raw.double(), 3)
    scale = float(logits.abs().max())
    top2 = logits.topk(2, dim=1).values
    return {"clf": clf, "raw": raw, "logits": logits, "digits": DigitClassifier.first_max(logits), "scale": scale,
            "certain": (top2[:, 0] - top2[:, 1]) >= MARGIN * scale}


class _Literal(nn.Module):
    """The network written out with torch's own layers."""

    def __init__(self) -> None:
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, kernel_size=3, padding=1)
        self.conv2 = nn.Conv2d(32, 64, kernel_size=3, padding=1)
        self.pool = nn.MaxPool2d(2, 2)
        self.fc1 = nn.Linear(64 * 8 * 8, 128)
        self.fc2 = nn.Linear(128, 10)
        self.relu = nn.ReLU()
        self.dropout = nn.Dropout(0.5)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.pool(self.relu(self.conv1(x)))
        x = self.pool(self.relu(self.conv2(x)))
        x = self.relu(self.fc1(x.view(-1, 64 * 8 * 8)))
        return self.fc2(self.dropout(x))


def test_a_checkpoint_of_the_evaluations_classifier_loads_strictly() -> None:
    state = _Literal().state_dict()
    assert {k: tuple(v.shape) for k, v in state.items()} == {
        "conv1.weight": (32, 1, 3, 3), "conv1.bias": (32,), "conv2.weight": (64, 32, 3, 3), "conv2.bias": (64,),
        "fc1.weight": (128, 4096), "fc1.bias": (128,), "fc2.weight": (10, 128), "fc2.bias": (10,)}
    clf = DigitClassifier()
    result = clf.load_state_dict(state, strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert set(clf.state_dict()) == set(state) and not any(p.requires_grad for p in clf.parameters()) and not clf.training
    bad = dict(state)
    bad["pool.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="pool.weight"):
        DigitClassifier().load_state_dict(bad, strict=True)


def test_reference_logits_is_the_literal_module_in_float64() -> None:
    clf = seeded_classifier(7)
    literal = _Literal().double().eval()
    literal.load_state_dict({k: v.double() for k, v in clf.state_dict().items()})
    raw = seeded_frames(7, 24).double() * 1.5
    select = torch.tensor([5, 0, 23, 5, 11], dtype=torch.int32)
    for act in (0, 3):
        for sel in (None, select):
            x = raw if sel is None else raw[sel.long()]
            y = torch.tanh(x) if act == 3 else x  # noqa: PLR2004
            images = ((y + 1.0) / 2.0).clamp(0.0, 1.0).reshape(-1, 1, 32, 32)
            if act == 0:  # (Identity: the clamp works on both sides)
                assert float(images.min()) == 0.0 and float(images.max()) == 1.0
            with torch.no_grad():
                want = literal(images)
            got = clf.reference_logits(raw, act, sel)
            assert got.dtype == torch.float64 and tuple(got.shape) == (x.shape[0], 10)
            assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), (act, sel)
            assert torch.equal(clf.images(raw, act, sel), images)
            # non-GPU tensors take the rule: logits / digits / forward
            assert torch.equal(clf.logits(raw, act, sel), got) and torch.equal(clf.digits(raw, act, sel), DigitClassifier.first_max(got))
    assert torch.allclose(clf(images), want, rtol=0, atol=1e-12)
    assert clf.reference_logits(raw.float(), 3).dtype == torch.float32 and clf.reference_logits(raw.reshape(2, 12, 1, 32, 32), 3).shape == (24, 10)
    assert tuple(clf.features(raw, 3).shape) == (24, FEATURES)


def test_first_max_takes_the_lowest_index_among_the_maxima() -> None:
    logits = torch.tensor([[0.0, 3.0, 3.0, 1.0], [2.0, 2.0, 2.0, 2.0], [-1.0, -5.0, -1.0, -1.0], [0.0, 0.0, 0.0, 9.0]])
    assert DigitClassifier.first_max(logits).tolist() == [1, 0, 0, 3] and DigitClassifier.first_max(logits).dtype == torch.int32
    assert torch.equal(DigitClassifier.first_max(logits).long(), torch.max(logits, 1).indices)


def test_the_shared_inputs_meet_the_conditions_the_gpu_tests_rely_on() -> None:
    ref = digit_set(SET_SEEDS[0])
    counts = torch.bincount(ref["digits"].long(), minlength=CLASSES)
    exempt = 1.0 - float(ref["certain"].double().mean())
    flat = float((torch.tanh(ref["raw"].double()).abs() > 0.999).double().mean())  # noqa: PLR2004
    print("digits", counts.tolist(), "exempt share", exempt, "pixels in tanh's flat ends", flat, "scale", ref["scale"])
    assert int(counts.min()) > 0 and exempt <= EXEMPT_CAP and flat > 0.01  # noqa: PLR2004


def test_messages() -> None:
    clf = DigitClassifier()
    with pytest.raises(ValueError, match="act must be 0"):
        clf.reference_logits(torch.zeros(1, 1024), 1)
    with pytest.raises(ValueError, match="whole 32 x 32 frames"):
        clf.reference_logits(torch.zeros(3, 1000))
    with pytest.raises(ValueError, match="int32 vector"):
        clf.reference_logits(torch.zeros(3, 1024), 0, torch.tensor([0, 1]))
    with pytest.raises(ValueError, match=r"\[N, 1, 32, 32\]"):
        clf(torch.zeros(3, 32, 32))
    table = torch.zeros(10, 11)
    with pytest.raises(ValueError, match="int32 vectors of one length"):
        word_counts(torch.zeros(3, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), table)
    with pytest.raises(ValueError, match="int32 vectors of one length"):
        word_counts(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), table)
    with pytest.raises(ValueError, match=r"fp32 \[10, 11\] table"):
        word_counts(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.zeros(10, 10))
    with pytest.raises(ValueError, match="exact below 2\\^24"):
        word_counts(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), table)


def test_word_counts_host_path_counts_pairs_and_skips_silence() -> None:
    g = torch.Generator().manual_seed(3)
    word = torch.randint(-1, 10, (500,), generator=g).to(torch.int32)
    digit = torch.randint(0, 11, (500,), generator=g).to(torch.int32)
    table = torch.zeros(10, 11)
    word_counts(word, digit, table)
    want = torch.zeros(10, 11)
    for w, d in zip(word.tolist(), digit.tolist(), strict=True):
        if w >= 0:
            want[w, d] += 1
    assert torch.equal(table, want) and float(table.sum()) == float((word >= 0).sum())
    word_counts(word, digit, table)  # IN/OUT
    assert torch.equal(table, 2 * want)


def test_bad_arguments_are_rejected_without_a_launch() -> None:
    lib = _lib.load()
    keep = torch.zeros(64)
    buf = (keep.data_ptr() + 15) // 16 * 16  # a 16-byte aligned host address: every call returns before a launch

    def features(**kw) -> int:  # noqa: ANN003
        a = {"pred": buf, "frames": 4, "select": None, "N": 4, "act": 3, "w1": buf, "b1": buf, "w2": buf, "b2": buf, "out": buf} | kw
        return lib.mtrssm_digit_features(a["pred"], a["frames"], a["select"], a["N"], a["act"], a["w1"], a["b1"], a["w2"], a["b2"], a["out"], None)

    for name, bad in (("pred", None), ("w1", None), ("b1", None), ("w2", None), ("b2", None), ("out", None), ("frames", 0), ("N", 0), ("N", 5),
                      ("N", 1 << 31), ("frames", 1 << 31), ("act", 1), ("act", 2), ("pred", buf + 4), ("out", buf + 8), ("w2", buf + 2)):
        assert features(**{name: bad}) == -1 and b"digit_features" in lib.mtrssm_last_error(), (name, bad)
    assert lib.mtrssm_digit_head(None, buf, buf, 4, None, 0, buf, None, None) == -1 and b"digit_head" in lib.mtrssm_last_error()
    assert lib.mtrssm_digit_head(buf, buf, buf, 4, None, 0, None, None, None) == -1
    assert lib.mtrssm_digit_head(buf, buf, buf, 0, None, 0, buf, None, None) == -1
    assert lib.mtrssm_digit_head(buf, buf + 2, buf, 4, None, 0, buf, None, None) == -1
    assert lib.mtrssm_digit_head(buf, buf, buf, 4, buf, 0, buf, None, None) == -1  # select without the frame count it indexes
    assert lib.mtrssm_word_counts(None, buf, 4, buf, None) == -1 and b"word_counts" in lib.mtrssm_last_error()
    assert lib.mtrssm_word_counts(buf, buf, 0, buf, None) == -1
    assert lib.mtrssm_word_counts(buf, buf, 1 << 24, buf, None) == -1 and b"2^24" in lib.mtrssm_last_error()
    assert lib.mtrssm_word_counts(buf, buf, 4, None, None) == -1
