"""``mt.likelihood`` (``mtrssm_gaussian_nll_*`` of csrc/train_ops.hip) at the depth its loops are written for, against the reference
formula in float64 on the CPU: ``-Independent(Normal(act(pred), scale), k).log_prob(target)`` averaged over the present frames (or
divided by the given count), gradients from autograd on that formula.

Sizes.  ``(545, 3851)``: 2 098 795 elements = 524 698 quads + 3.  The sums run 512 workgroups of 256 threads, four quads in flight:
the unrolled loop needs more than 3 * 131 072 quads (one trip here), the remainder loop takes the rest, the last three elements are
the tail; the backward's 2048 * 256 quads make a second lap; the event is odd, so every quad after the first frame straddles or
sits askew of the frame borders (the non-``EV4`` instances).  ``(545, 3852)``: the ``EV4`` instances at the same depth.  ``(2, 7, 15)``
and ``(1, 1, 3)``: one workgroup, and the tail alone.

Bounds, all from ``test_gaussian_nll_kernel``: value ``rtol = 2e-6`` (non-negative terms: a tree sum's relative error does not grow
with its length); Identity gradient ``rtol = 1e-6, atol = 1e-8``; Tanh gradient ``rtol = 2e-5, atol = 1e-7``.  Saturated and absent
positions: exact zeros.

Measured on the MI355X (profiles/stream_kernel_tests_notes.md): value at most 6.1e-7 off (relative); gradient error / (atol + rtol |ref|) at
most 0.14 (Identity) and 0.34 (Tanh); all-present against plain: 0 differing gradient words.
"""

from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEEP = [(545, 3851), (545, 3852)]
SHAPES = [*DEEP, (2, 7, 15), (1, 1, 3)]
ACTS = [0, 3]
VALUE_RTOL = 2e-6
GRAD_TOL = {0: {"rtol": 1e-6, "atol": 1e-8}, 3: {"rtol": 2e-5, "atol": 1e-7}}


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


def _ids(shape: tuple[int, ...]) -> str:
    return "x".join(map(str, shape))


@functools.cache
def _data(shape: tuple[int, ...]) -> tuple[torch.Tensor, torch.Tensor]:
    """Prediction and target of a shape, made once and never written to."""
    gen = torch.Generator().manual_seed(17 + math.prod(shape))
    return torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)


def _frames(shape: tuple[int, ...]) -> int:
    return math.prod(shape[:-1])


@functools.cache
def _mask(shape: tuple[int, ...]) -> torch.Tensor:
    """A random mask over the frames with the first and the last frame absent (and at least one present where there are three)."""
    gen = torch.Generator().manual_seed(23)
    m = torch.rand(shape[:-1], generator=gen) < 0.6  # noqa: PLR2004
    flat = m.reshape(-1)
    flat[0] = flat[-1] = False
    if flat.numel() > 2:  # noqa: PLR2004
        flat[1] = True
    return m


def reference(pred: torch.Tensor, tgt: torch.Tensor, *, act: int, scale: float = 1.0, mask: torch.Tensor | None = None,  # noqa: PLR0913
              count: float | None = None) -> tuple[float, torch.Tensor]:
    """Value and gradient of the formula in float64.  ``mask``: bool over the frames; ``count``: the divisor when it is not the
    number of present frames.  Absent frames are taken out with a select, so that whatever they hold does not reach the result."""
    p = pred.double().requires_grad_()
    if mask is not None:
        keep = mask.unsqueeze(-1).expand_as(p)
        clean = torch.where(keep, p, torch.zeros((), dtype=torch.float64))
    else:
        clean = p
    mean = torch.tanh(clean) if act == 3 else clean  # noqa: PLR2004
    dist = torch.distributions.Independent(torch.distributions.Normal(mean, torch.tensor(scale, dtype=torch.float64)), 1)
    nll = -dist.log_prob(tgt.double())  # per frame
    if mask is None:
        value = nll.mean()
    else:
        n = float(mask.sum()) if count is None else count
        value = torch.where(mask, nll, torch.zeros((), dtype=torch.float64)).sum() / n if n > 0 else (nll * 0.0).sum()
    value.backward()
    return float(value), p.grad


def ours(pred: torch.Tensor, tgt: torch.Tensor, *, act: int, scale: float = 1.0, **kw: object) -> tuple[float, torch.Tensor]:
    import multimodal_mtrssm_amd as mt

    p = pred.to(DEV).requires_grad_()
    value = mt.likelihood(prediction=p, target=tgt.to(DEV), event_ndims=1, scale=scale, out_act=act, **kw)
    (value * 1.0).backward()
    return float(value), p.grad.cpu()


def compare(tag: str, got: tuple[float, torch.Tensor], want: tuple[float, torch.Tensor], act: int) -> None:
    rel = abs(got[0] - want[0]) / abs(want[0]) if want[0] else abs(got[0])
    tol = GRAD_TOL[act]
    err = (got[1].double() - want[1]).abs()
    ratio = float((err / (tol["atol"] + tol["rtol"] * want[1].abs())).max())
    print(f"{tag}: value {got[0]:.9e} vs float64 {want[0]:.9e}, relative {rel:.2e} (bound {VALUE_RTOL:.0e}); gradient worst |err| {float(err.max()):.2e}, "
          f"worst err / (atol + rtol |ref|) {ratio:.3f}")
    np.testing.assert_allclose(got[0], want[0], rtol=VALUE_RTOL, err_msg=tag)
    np.testing.assert_allclose(got[1].numpy(), want[1].numpy(), err_msg=tag, **tol)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_plain(shape: tuple[int, ...], act: int, lib_loaded: None) -> None:
    pred, tgt = _data(shape)
    compare(f"plain {shape} act {act}", ours(pred, tgt, act=act), reference(pred, tgt, act=act), act)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_masked(shape: tuple[int, ...], act: int, lib_loaded: None) -> None:
    """A random mask with the first and the last frame absent; gradients of absent frames are exact zeros."""
    pred, tgt = _data(shape)
    mask = _mask(shape)
    got = ours(pred, tgt, act=act, frame_mask=mask.to(DEV))
    compare(f"masked {shape} act {act} ({int(mask.sum())} of {mask.numel()} frames)", got, reference(pred, tgt, act=act, mask=mask), act)
    assert not bool(got[1][~mask].any())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_all_present_is_plain(shape: tuple[int, ...], act: int, lib_loaded: None) -> None:
    """Every frame present: the plain result within the value bound (the order of the workgroups' atomics is free), and the plain
    gradient bit for bit (the header's claim: the same arithmetic)."""
    pred, tgt = _data(shape)
    full = torch.ones(shape[:-1], dtype=torch.bool)
    got, plain = ours(pred, tgt, act=act, frame_mask=full.to(DEV)), ours(pred, tgt, act=act)
    compare(f"all present {shape} act {act}", got, reference(pred, tgt, act=act), act)
    np.testing.assert_allclose(got[0], plain[0], rtol=VALUE_RTOL)
    assert torch.equal(got[1].view(torch.int32), plain[1].view(torch.int32))


@pytest.mark.parametrize("scale", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(545, 3851), (2, 7, 15)], ids=_ids)
def test_none_present(shape: tuple[int, ...], act: int, scale: float, lib_loaded: None) -> None:
    """No frame present: the value is 0 and the gradient all zeros, at any scale."""
    pred, tgt = _data(shape)
    value, grad = ours(pred, tgt, act=act, scale=scale, frame_mask=torch.zeros(shape[:-1], dtype=torch.bool, device=DEV))
    assert value == 0.0 and not bool(grad.any())


@pytest.mark.parametrize("scale", [1.0, 2.0])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_given_count(shape: tuple[int, ...], act: int, scale: float, lib_loaded: None) -> None:
    """``frame_present = (present, count)`` with ``count = present.sum() / 2``: what a data-parallel rank of two passes.  The whole
    per-frame term is divided by the count, ``0.5 E log 2pi`` and ``E log(scale)`` included: until this test the forward added
    the constant once whatever the count (3538.83 = 3851 * 0.5 log 2pi short of 14777.38 at ``(545, 3851)``)."""
    pred, tgt = _data(shape)
    mask = _mask(shape) if _frames(shape) > 1 else torch.ones(shape[:-1], dtype=torch.bool)
    present = mask.reshape(-1).float().to(DEV)
    count = present.sum() / 2
    got = ours(pred, tgt, act=act, scale=scale, frame_present=(present, count))
    compare(f"given count {shape} act {act} scale {scale}", got, reference(pred, tgt, act=act, scale=scale, mask=mask, count=float(count)), act)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("scale", [0.5, 2.0])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(545, 3851), (545, 3852), (2, 7, 15)], ids=_ids)
def test_scale(shape: tuple[int, ...], act: int, scale: float, masked: bool, lib_loaded: None) -> None:  # noqa: FBT001
    """``scale != 1``: the unit-scale kernel on ``pred / scale, target / scale`` plus ``event log(scale)`` (on present counts only)."""
    pred, tgt = _data(shape)
    mask = _mask(shape) if masked else None
    kw = {"frame_mask": mask.to(DEV)} if masked else {}
    compare(f"scale {scale} {shape} act {act} masked {masked}", ours(pred, tgt, act=act, scale=scale, **kw),
            reference(pred, tgt, act=act, scale=scale, mask=mask), act)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("shape", [(545, 3851), (545, 3852), (1, 1, 3)], ids=_ids)
def test_saturated_tanh(shape: tuple[int, ...], masked: bool, lib_loaded: None) -> None:  # noqa: FBT001
    """Raw predictions of +-20 and +-100 under Tanh, in the quad part and in the last elements: a finite value, and a gradient of
    exactly 0 there (``1 - tanh^2`` is 0 in float32 from |x| ~ 9 on; the float64 gradient there is below 1e-16)."""
    pred, tgt = _data(shape)
    pred = pred.clone()
    flat = pred.view(-1)
    n = flat.numel()
    where = torch.tensor(sorted({0, n - 1, n - 2, n // 2, n // 3, 4 * 131072 * 3 + 5, 4 * 524288 + 1} & set(range(n))))
    values = torch.tensor([20.0, -20.0, 100.0, -100.0]).repeat(2)[: where.numel()]
    flat[where] = values
    mask = torch.ones(shape[:-1], dtype=torch.bool)
    if masked and _frames(shape) > 2:  # noqa: PLR2004
        mask = _mask(shape).clone()
        mask.view(-1)[0] = mask.view(-1)[-1] = True  # the saturated ends are present
    kw = {"frame_mask": mask.to(DEV)} if masked else {}
    got = ours(pred, tgt, act=3, **kw)
    assert math.isfinite(got[0]) and bool(torch.isfinite(got[1]).all())
    compare(f"saturated {shape} masked {masked}", got, reference(pred, tgt, act=3, mask=mask if masked else None), 3)
    assert not bool(got[1].view(-1)[where].any())


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_misaligned_slices(masked: bool, act: int, lib_loaded: None) -> None:  # noqa: FBT001
    """Prediction and target as contiguous slices at a storage offset of 60 bytes (``full[1:]`` at event 15): value and gradient
    are those of the same data in a fresh tensor, bit for bit (one workgroup: no free order).  Before the copy in
    ``objective._aligned`` this raised ``MtrssmLibraryError`` (``pred/target must be 16-byte aligned``)."""
    import multimodal_mtrssm_amd as mt

    gen = torch.Generator().manual_seed(41)
    full_p, full_t = torch.randn(8, 15, generator=gen).to(DEV), torch.randn(8, 15, generator=gen).to(DEV)
    mask = torch.tensor([False, True, True, False, True, True, False], device=DEV)
    kw = {"frame_mask": mask} if masked else {}

    def run(leaf: torch.Tensor, pred: torch.Tensor, tgt: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        value = mt.likelihood(prediction=pred, target=tgt, event_ndims=1, out_act=act, **kw)
        (value * 1.0).backward()
        return value.detach().cpu(), leaf.grad.cpu()

    fresh = full_p[1:].clone().requires_grad_()
    assert fresh.data_ptr() % 16 == 0
    want_v, want_g = run(fresh, fresh, full_t[1:].clone())
    ref = reference(full_p[1:].cpu(), full_t[1:].cpu(), act=act, mask=mask.cpu() if masked else None)
    compare(f"fresh copy of the slices, act {act} masked {masked}", (float(want_v), want_g), ref, act)
    for slice_p, slice_t in ((True, True), (True, False), (False, True)):
        leaf = full_p.clone().requires_grad_()
        pred = leaf[1:] if slice_p else fresh.detach().clone().requires_grad_()
        tgt = full_t[1:] if slice_t else full_t[1:].clone()
        assert (pred.data_ptr() % 16 == 12) == slice_p and (tgt.data_ptr() % 16 == 12) == slice_t and pred.is_contiguous()  # noqa: PLR2004
        value, grad = run(leaf if slice_p else pred, pred, tgt)
        assert torch.equal(value.view(torch.int32), want_v.view(torch.int32)), (slice_p, slice_t)
        g = grad[1:] if slice_p else grad
        assert torch.equal(g.view(torch.int32), want_g.view(torch.int32)), (slice_p, slice_t)
        if slice_p:
            assert not bool(grad[0].any())


def test_raw_entry_points_refuse_misaligned_pointers(lib_loaded: None) -> None:
    """The C entry points keep their contract: a pointer off a 16-byte boundary returns -1 and launches nothing (a host check).
    The buffers hold sentinels that a launch would overwrite."""
    import multimodal_mtrssm_amd as mt

    lib, L = mt._lib.load(), mt._lib  # noqa: SLF001, N806
    buf_p, buf_t, buf_g = (torch.full((64,), 3.0, device=DEV) for _ in range(3))
    out, one = torch.full((1,), 7.0, device=DEV), torch.ones(1, device=DEV)
    present, count = torch.ones(4, device=DEV), torch.full((1,), 4.0, device=DEV)
    stream = L.stream_ptr(buf_p.device)
    good = (L.ptr(buf_p), L.ptr(buf_t), L.ptr(buf_g))
    assert all(a % 16 == 0 for a in good)
    for off_p, off_t, off_g in ((4, 0, 0), (0, 4, 0), (0, 0, 4), (12, 12, 12), (8, 0, 0)):
        p, t, g = good[0] + off_p, good[1] + off_t, good[2] + off_g
        for act in ACTS:
            if off_p or off_t:
                assert lib.mtrssm_gaussian_nll_fwd(p, t, 4, 15, act, L.ptr(out), stream) == -1
                assert lib.mtrssm_gaussian_nll_masked_fwd(p, t, L.ptr(present), L.ptr(count), 4, 15, act, L.ptr(out), stream) == -1
            assert lib.mtrssm_gaussian_nll_bwd(p, t, L.ptr(one), 4, 15, act, g, stream) == -1
            assert lib.mtrssm_gaussian_nll_masked_bwd(p, t, L.ptr(present), L.ptr(count), L.ptr(one), 4, 15, act, g, stream) == -1
    assert b"aligned" in lib.mtrssm_last_error()
    torch.cuda.synchronize()
    assert float(out) == 7.0 and bool((buf_g == 3.0).all())  # noqa: PLR2004
    # and aligned pointers pass
    assert lib.mtrssm_gaussian_nll_fwd(good[0], good[1], 4, 15, 0, L.ptr(out), stream) == 0
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(out), 15 * 0.5 * math.log(2 * math.pi), rtol=VALUE_RTOL)  # pred == target


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape", [(545, 3851), (545, 3852), (2, 7, 15)], ids=_ids)
def test_absent_frames_may_hold_anything(shape: tuple[int, ...], act: int, poison: str, lib_loaded: None) -> None:
    """Absent frames whose predictions are NaN, or +-Inf: the value is that of the clean data and the gradient is exactly 0 on
    those frames, in the quad part and in the last ``n % 4`` elements (the last frame is absent).  Before the select in
    ``nll_masked_bwd_kernel`` the Tanh instances wrote NaN (``0 * (1 - tanh(NaN)^2)``) on the quads of NaN frames."""
    pred, tgt = _data(shape)
    mask = _mask(shape)
    absent = (~mask).unsqueeze(-1).expand_as(pred)
    if poison == "nan":
        bad = torch.full_like(pred, float("nan"))
    else:
        bad = torch.where(torch.arange(pred.numel()).reshape(pred.shape) % 2 == 0, float("inf"), float("-inf"))
    dirty = torch.where(absent, bad, pred)
    assert not bool(torch.isfinite(dirty[absent]).any()) and bool(torch.isfinite(dirty[~absent]).all())
    got = ours(dirty, tgt, act=act, frame_mask=mask.to(DEV))
    bad_words = int((~torch.isfinite(got[1])).sum())
    print(f"absent frames hold {poison}, {shape} act {act}: {bad_words} non-finite gradient words, "
          f"{int((got[1][absent] != 0).sum())} non-zero words on absent frames")
    assert not bool(got[1][absent].view(torch.int32).any())  # +0.0 words
    compare(f"absent {poison} {shape} act {act}", got, reference(pred, tgt, act=act, mask=mask), act)
