"""CPU: latent overshooting -- the rule against values written out by hand and against a plain-Python loop, the
starts and the refusals, the rule's backward formulas against autograd on the float64 rule, dead terms, an empty count, the scatter
rule as the gather rule's autograd, the table, the model's noise shapes and the new C-ABI entries (declared, bound, rejecting bad
arguments without a launch).  Nothing here launches a kernel."""

from __future__ import annotations

import ctypes as C
import math
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import Forecast, LatentOvershoot, OvershootTable, _lib
from multimodal_mtrssm_amd.distributions import KL_BALANCE_ALPHA
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.parallel import FlatDataParallel, GlobalRowNoise
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


def _two(p: float) -> list[float]:
    """Logits of a two-class categorical with probabilities ``(1 - p, p)``."""
    return [0.0, math.log(p / (1.0 - p))]


# -- the rule ---------------------------------------------------------------------------------------------------------------------
def test_the_rule_against_values_written_out_by_hand() -> None:
    """B = 1, T = 4, K = 1, C = 2, D = 2, s = 1: starts 0, 1, 2; row i, distance k targets frame i + k."""
    lo = LatentOvershoot(2)
    assert lo.starts(4) == [0, 1, 2] and lo.rows(4) == 3
    post = torch.tensor([[_two(0.6), _two(0.75), _two(0.5), _two(0.875)]])  # q at frames 0 .. 3 (frame 0 is no target)
    os_logits = torch.tensor([[_two(0.5), _two(0.75)], [_two(0.5), _two(0.5)], [_two(0.75), _two(0.9)]])  # p of (row, k)
    kl_01 = 0.25 * math.log(0.25 / 0.5) + 0.75 * math.log(0.75 / 0.5)      # row 0, k = 1: q of frame 1 against (1/2, 1/2)
    kl_02 = 0.5 * math.log(0.5 / 0.25) + 0.5 * math.log(0.5 / 0.75)        # row 0, k = 2: q of frame 2 against (1/4, 3/4)
    kl_11 = 0.0                                                              # row 1, k = 1: q of frame 2 against itself
    kl_12 = 0.125 * math.log(0.125 / 0.5) + 0.875 * math.log(0.875 / 0.5)  # row 1, k = 2: q of frame 3 against (1/2, 1/2)
    kl_21 = 0.125 * math.log(0.125 / 0.25) + 0.875 * math.log(0.875 / 0.75)  # row 2, k = 1: q of frame 3 against (1/4, 3/4)
    got = lo.reference(post, os_logits, 1)
    want = torch.tensor([[kl_01, kl_02], [kl_11, kl_12], [kl_21, 0.0]], dtype=torch.float64)  # (row 2, k = 2) targets frame 4: dead
    torch.testing.assert_close(got.plane, want, rtol=1e-6, atol=1e-9)
    assert float(got.plane[2, 1]) == 0.0 and float(got.count) == 2.0  # noqa: PLR2004
    torch.testing.assert_close(got.table, torch.tensor([[kl_01 + kl_11 + kl_21, kl_02 + kl_12], [3.0, 2.0]], dtype=torch.float64), rtol=1e-6, atol=1e-9)
    assert float(got.term) == pytest.approx((kl_02 + kl_12) / 2.0, rel=1e-6)
    # with lengths: valid = 3 kills frame 3 -- (1, 2) and (2, 1) -- and leaves one trained term
    short = lo.reference(post, os_logits, 1, torch.tensor([3], dtype=torch.int32))
    torch.testing.assert_close(short.plane, torch.tensor([[kl_01, kl_02], [kl_11, 0.0], [0.0, 0.0]], dtype=torch.float64), rtol=1e-6, atol=1e-9)
    assert float(short.count) == 1.0 and float(short.term) == pytest.approx(kl_02, rel=1e-6)
    assert short.table[1].tolist() == [2.0, 1.0]


def _loop_rule(lo: LatentOvershoot, post, os_logits, cats: int, valid, row0: int, b_global: int):  # noqa: ANN001, ANN202, PLR0913
    """The rule as a plain-Python loop over rows, starts, distances, categoricals and classes."""
    b, t, width = post.shape
    classes = width // cats
    n, d = lo.rows(t), lo.depth

    def length(g: int) -> int:
        return t if valid is None else max(0, min(t, int(valid[g])))

    count = sum(1 for g in range(b_global) for i in range(n) for k in range(2, d + 1) if lo.offset + i * lo.stride + k < length(g))
    plane = [[0.0] * d for _ in range(b * n)]
    table = [[0.0] * d, [0.0] * d]
    total = 0.0
    for bl in range(b):
        for i in range(n):
            for k in range(1, d + 1):
                frame = lo.offset + i * lo.stride + k
                if frame >= length(row0 + bl):
                    continue
                kl = 0.0
                for c0 in range(cats):
                    q = [float(x) for x in post[bl, frame, c0 * classes : (c0 + 1) * classes]]
                    p = [float(x) for x in os_logits[bl * n + i, k - 1, c0 * classes : (c0 + 1) * classes]]
                    lq = [x - max(q) - math.log(sum(math.exp(y - max(q)) for y in q)) for x in q]
                    lp = [x - max(p) - math.log(sum(math.exp(y - max(p)) for y in p)) for x in p]
                    kl += sum(math.exp(a) * (a - bb) for a, bb in zip(lq, lp, strict=True) if math.exp(a) > 0.0)
                plane[bl * n + i][k - 1] = kl
                table[0][k - 1] += kl
                table[1][k - 1] += 1.0
                if k >= 2:  # noqa: PLR2004
                    total += kl
    return plane, table, float(count), total / max(count, 1)


@pytest.mark.parametrize("ragged", [False, True], ids=["full", "lengths"])
def test_the_rule_against_a_plain_python_loop(ragged: bool) -> None:  # noqa: FBT001
    g = torch.Generator().manual_seed(1)
    lo = LatentOvershoot(3, stride=2, offset=1)
    b, t, cats, classes = 2, 7, 3, 4
    n = lo.rows(t)
    assert lo.starts(t) == [1, 3, 5] and n == 3  # noqa: PLR2004
    post = torch.randn(b, t, cats * classes, generator=g, dtype=torch.float64) * 3.0
    os_logits = torch.randn(b * n, 3, cats * classes, generator=g, dtype=torch.float64) * 3.0
    valid = torch.tensor([7, 5, 9, 0], dtype=torch.int32) if ragged else None  # four global rows, the rank holds rows 1 .. 2
    bound = lo if ragged else lo.for_rank(2, 0)
    row0 = 1 if ragged else 0
    got = bound.reference(post, os_logits, cats, valid, row0)
    plane, table, count, term = _loop_rule(lo, post, os_logits, cats, valid, row0, 4)
    torch.testing.assert_close(got.plane, torch.tensor(plane, dtype=torch.float64), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(got.table, torch.tensor(table, dtype=torch.float64), rtol=1e-12, atol=1e-14)
    assert float(got.count) == count
    assert float(got.term) == pytest.approx(bound.world * term, rel=1e-12)


def test_starts_rows_noise_shape_and_the_argument_refusals() -> None:
    lo = LatentOvershoot(5, stride=4)
    assert lo.starts(6) == [0, 4] and lo.rows(6) == 2 and lo.noise_shape(3, 6, 7) == (3, 2, 5, 7)  # noqa: PLR2004
    assert LatentOvershoot(2, stride=3, offset=4).starts(6) == [4]  # the last start is T - 2
    assert LatentOvershoot(7).starts(2) == [0]
    assert repr(lo) == "LatentOvershoot(depth=5, stride=4, offset=0, weight=1.0, balanced=False, detach_state=False)"
    with pytest.raises(ValueError, match="offset"):
        LatentOvershoot(2, offset=5).rows(6)
    for bad in ({"depth": 1}, {"depth": 2.0}, {"depth": True}, {"depth": 2, "stride": 0}, {"depth": 2, "stride": 1.5}, {"depth": 2, "offset": -1},
                {"depth": 2, "weight": -0.5}, {"depth": 2, "weight": float("nan")}, {"depth": 2, "weight": "1"}, {"depth": 2, "balanced": 1},
                {"depth": 2, "detach_state": 0}):
        with pytest.raises(ValueError, match="depth|stride|offset|weight|balanced"):
            LatentOvershoot(**bad)
    with pytest.raises(ValueError, match="rank"):
        lo.for_rank(2, 2)
    bound = lo.for_rank(4, 3)
    assert (bound.world, bound.rank, lo.world, lo.rank) == (4, 3, 1, 0)
    # the gradient weights
    assert lo.kl_weights(True) == (1.0, 0.0) and lo.kl_weights(False) == (1.0, 0.0)
    both = LatentOvershoot(2, balanced=True)
    assert both.kl_weights(True) == (KL_BALANCE_ALPHA, 1.0 - KL_BALANCE_ALPHA) and both.kl_weights(False) == (1.0, 1.0)
    # shapes
    post, os_logits = torch.zeros(2, 6, 8), torch.zeros(4, 5, 8)
    lo.reference(post, os_logits, 4)
    with pytest.raises(ValueError, match="os_logits"):
        lo.reference(post, os_logits[:3], 4)
    with pytest.raises(ValueError, match="categoricals"):
        lo.reference(post, os_logits, 3)
    with pytest.raises(ValueError, match="valid"):
        lo.reference(post, os_logits, 4, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="global rows"):
        lo.reference(post, os_logits, 4, torch.tensor([6, 6], dtype=torch.int32), 1)


@pytest.mark.parametrize("weights", [(1.0, 0.0), (KL_BALANCE_ALPHA, 1.0 - KL_BALANCE_ALPHA), (1.0, 1.0)])
def test_backward_formulas_against_autograd_on_the_rule(weights: tuple[float, float]) -> None:
    g = torch.Generator().manual_seed(2)
    lo = LatentOvershoot(3, stride=1)
    b, t, cats, classes = 2, 5, 2, 3
    n, d = lo.rows(t), 3
    valid = torch.tensor([5, 3], dtype=torch.int32)
    post = torch.randn(b, t, cats * classes, generator=g, dtype=torch.float64, requires_grad=True)
    os_logits = torch.randn(b * n, d, cats * classes, generator=g, dtype=torch.float64, requires_grad=True)
    got = lo.reference(post, os_logits, cats, valid, 0, weights)
    got.term.backward()
    plain = lo.reference(post.detach(), os_logits.detach(), cats, valid, 0, (1.0, 1.0))
    assert float(plain.term) == float(got.term.detach())  # the value is the KL whatever the weights
    w_prior, w_post = weights
    count = float(got.count)
    want_os, want_post = torch.zeros_like(os_logits), torch.zeros_like(post)
    for bl in range(b):
        for i in range(n):
            for k in range(2, d + 1):
                frame = i + k
                if frame >= int(valid[bl]):
                    continue
                lq = torch.log_softmax(post.detach()[bl, frame].reshape(cats, classes), dim=-1)
                lp = torch.log_softmax(os_logits.detach()[bl * n + i, k - 1].reshape(cats, classes), dim=-1)
                q, p = lq.exp(), lp.exp()
                kl_cat = (q * (lq - lp)).sum(dim=-1, keepdim=True)
                want_os[bl * n + i, k - 1] = (w_prior * (p - q) / count).reshape(-1)
                want_post[bl, frame] += (w_post * q * ((lq - lp) - kl_cat) / count).reshape(-1)
    torch.testing.assert_close(os_logits.grad, want_os.detach(), rtol=1e-10, atol=1e-13)
    torch.testing.assert_close(post.grad, want_post.detach(), rtol=1e-10, atol=1e-13)
    assert not bool(os_logits.grad[:, 0].any())  # k = 1 is reported, never trained
    if w_post == 0.0:
        assert not bool(post.grad.any())  # the posterior is a fixed target


def test_dead_terms_are_exactly_zero_and_an_empty_count_gives_zero_loss_and_gradients() -> None:
    g = torch.Generator().manual_seed(3)
    lo = LatentOvershoot(4, stride=2)
    b, t, cats, classes = 3, 6, 2, 4
    n = lo.rows(t)
    post = torch.randn(b, t, cats * classes, generator=g, dtype=torch.float64, requires_grad=True)
    os_logits = torch.randn(b * n, 4, cats * classes, generator=g, dtype=torch.float64, requires_grad=True)
    valid = torch.tensor([6, 4, 1], dtype=torch.int32)
    got = lo.reference(post, os_logits, cats, valid, 0, (1.0, 1.0))
    for bl in range(b):
        for i, t0 in enumerate(lo.starts(t)):
            for k in range(1, 5):
                live = t0 + k < int(valid[bl])
                assert (float(got.plane[bl * n + i, k - 1]) != 0.0) == live, (bl, i, k)
    # every row has valid <= 2: no k >= 2 term is live anywhere
    none = lo.reference(post, os_logits, cats, torch.tensor([2, 1, 0], dtype=torch.int32), 0, (1.0, 1.0))
    assert float(none.count) == 0.0 and float(none.term) == 0.0
    none.term.backward()
    assert not bool(post.grad.any()) and not bool(os_logits.grad.any())
    assert none.table[1].tolist() == [1.0, 0.0, 0.0, 0.0]  # (row 0's k = 1 term at frame 1 is still reported)
    fp32 = lo.kl(post.detach().float(), os_logits.detach().float(), cats, torch.tensor([2, 1, 0], dtype=torch.int32))  # the CPU route
    assert float(fp32.term) == 0.0 and fp32.plane.dtype == torch.float32 and fp32.table.dtype == torch.float64


def test_the_scatter_rule_is_the_autograd_of_the_gather_rule() -> None:
    g = torch.Generator().manual_seed(4)
    for depth, stride, offset in ((2, 1, 0), (3, 2, 1), (5, 4, 0), (7, 1, 0)):
        lo = LatentOvershoot(depth, stride=stride, offset=offset)
        b, t, a = 3, 6, 5
        n = lo.rows(t)
        states = [torch.randn(b, t, w, generator=g, requires_grad=True) for w in (7, 4)]
        actions = torch.randn(b, t, a, generator=g)
        picked, windows = lo.gather(states, actions)  # (the CPU route is the rule)
        for x, got in zip(states, picked, strict=True):
            for bl in range(b):
                for i, t0 in enumerate(lo.starts(t)):
                    assert torch.equal(got[bl * n + i], x[bl, t0])
        for bl in range(b):
            for i, t0 in enumerate(lo.starts(t)):
                for j in range(depth):
                    want = actions[bl, t0 + 1 + j] if t0 + 1 + j < t else torch.zeros(a)
                    assert torch.equal(windows[bl * n + i, j], want)
        grads = [torch.randn(x.shape, generator=g) for x in picked]
        torch.autograd.backward(picked, grads)
        for x, full in zip(states, lo.scatter_reference(grads, b, t), strict=True):
            assert torch.equal(x.grad, full)
        detached, _ = LatentOvershoot(depth, stride=stride, offset=offset, detach_state=True).gather(states, actions)
        assert not any(x.requires_grad for x in detached)


def test_table_fold_curves_and_scalars() -> None:
    table = OvershootTable(2, 3)
    assert tuple(table.buffer.shape) == (2, 2, 3) and table.buffer.dtype == torch.float64 and table.levels == 2  # noqa: PLR2004
    assert all(bool(torch.isnan(v).all()) for v in table.curves().values())  # nothing counted yet
    one = torch.tensor([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0]], dtype=torch.float64)
    two = torch.tensor([[3.0, 0.5, 0.0], [1.0, 1.0, 0.0]], dtype=torch.float64)
    table.fold([one, two]).fold([one, one])
    curves = table.curves()
    assert list(curves) == ["kl", "kl_h"]
    assert curves["kl"][:2].tolist() == [0.5, 2.0] and bool(torch.isnan(curves["kl"][2]))
    assert curves["kl_h"][:2].tolist() == [4.0 / 3.0, 1.25]
    scalars = table.scalars("val/overshoot")
    assert list(scalars) == [f"val/overshoot/{name}_d{k}" for name in ("kl", "kl_h") for k in (1, 2, 3)]
    assert float(scalars["val/overshoot/kl_d2"]) == 2.0 and scalars["val/overshoot/kl_d2"].dtype == torch.float32  # noqa: PLR2004
    other = OvershootTable(2, 3).fold([two, two])
    assert table.add(other).buffer[1, 0].tolist() == [7.0, 3.0, 0.0]
    assert table.all_reduce() is table  # no process group: a no-op
    with pytest.raises(ValueError, match="tables"):
        table.fold([one])
    with pytest.raises(ValueError, match="depth"):
        OvershootTable(1, 1)
    assert list(OvershootTable(1, 2).curves()) == ["kl"]


# -- model surface ----------------------------------------------------------------------------------------------------------------
def test_noise_shapes_gain_the_overshoot_uniforms_only_with_the_attribute(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    assert model.overshoot is None and model.val_overshoot is None and model.overshoot_table is None
    shapes = dict(model.noise_shapes(6, 9))
    assert not any(k.startswith("u_overshoot") for k in shapes)
    model.overshoot = LatentOvershoot(3, stride=2)  # N = 4 starts in 9 frames
    try:
        with_os = model.noise_shapes(6, 9)
    finally:
        model.overshoot = None
    d = case.dims
    new = {"u_overshoot": (6, 4, 3, d.cats)} if case.kind == "mrssm" else {"u_overshoot_l": (6, 4, 3, d.ls_cats), "u_overshoot_h": (6, 4, 3, d.hs_cats)}
    assert with_os == {**shapes, **new} and list(with_os)[: len(shapes)] == list(shapes)
    assert model.noise_shapes(6, 9) == shapes
    model.val_overshoot = LatentOvershoot(3)  # validation only: the training step's uniforms are unchanged
    try:
        assert model.noise_shapes(6, 9) == shapes
    finally:
        model.val_overshoot = None
    # batch row first: GlobalRowNoise slices the key, and two ranks' rows are the one-rank draw
    ranks = [GlobalRowNoise(5, 2, r, "cpu").draw({k: (3, *s[1:]) for k, s in with_os.items()}) for r in (0, 1)]
    whole = GlobalRowNoise(5, 1, 0, "cpu").draw(with_os)
    for k in new:
        assert torch.equal(torch.cat([ranks[0][k], ranks[1][k]]), whole[k]), k


def test_step_and_capture_refusals(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    lo = LatentOvershoot(2)
    with pytest.raises(ValueError, match="not posteriors"):
        model.shared_step(batch, forecast=Forecast(2), overshoot=lo)
    with pytest.raises(ValueError, match="LatentOvershoot"):
        model.shared_step(batch, overshoot=2)
    with pytest.raises(ValueError, match="offset"):
        model.shared_step(batch, overshoot=LatentOvershoot(2, offset=case.steps - 1))
    with pytest.raises(ValueError, match="valid_global"):  # lengths= is one rank's own rows
        model.shared_step(batch, overshoot=lo.for_rank(2, 0), lengths=torch.full((case.batch,), case.steps, dtype=torch.int32))
    with pytest.raises(ValueError, match="not posteriors"):
        CapturedTrainStep(model, None, None, None, batch, None, forecast=Forecast(2), overshoot=lo)
    with pytest.raises(ValueError, match="LatentOvershoot"):
        CapturedTrainStep(model, None, None, None, batch, None, overshoot=(2, 1))
    dp = FlatDataParallel.__new__(FlatDataParallel)
    dp.world, dp.rank, dp.group = 4, 1, None
    bound = dp.overshoot(lo)
    assert (bound.world, bound.rank, lo.world) == (4, 1, 1)


def test_training_step_passes_the_overshoot_on(cpu_model, monkeypatch: pytest.MonkeyPatch) -> None:  # noqa: ANN001
    case, model = cpu_model
    seen = {}

    def fake(batch, noise=None, **kw):  # noqa: ANN001, ANN003, ANN202, ARG001
        seen.update(kw)
        return {"loss": torch.zeros(()), "overshoot": torch.ones(())}

    monkeypatch.setattr(model, "shared_step", fake)
    monkeypatch.setattr(model, "log_dict", lambda *a, **k: None)
    lo = LatentOvershoot(2)
    model.overshoot = lo
    try:
        logged = model.training_step(build_batch(case))
    finally:
        model.overshoot = None
    assert seen["overshoot"] is lo and float(logged["train/overshoot"]) == 1.0
    seen.clear()
    model.training_step(build_batch(case))
    assert seen["overshoot"] is None


# -- the C entries ----------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_refuse_bad_arguments_without_a_launch() -> None:
    names = ("mtrssm_overshoot_gather", "mtrssm_overshoot_scatter", "mtrssm_overshoot_kl_workspace_bytes", "mtrssm_overshoot_kl_fwd",
             "mtrssm_overshoot_kl_bwd")
    lib = _lib.load()
    for name in names:
        assert re.search(r"^\s*(?:int|int64_t)\s+" + name + r"\s*\(", HEADER, flags=re.MULTILINE), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    table = _lib.StateTable()
    geom = (3, 6, 2, 4, 0)  # B, T, N, s, o with N = (6 - 2 - 0) // 4 + 1
    assert lib.mtrssm_overshoot_gather(None, None, None, *geom, 5, 6, None) == -1 and b"overshoot_gather" in lib.mtrssm_last_error()
    assert lib.mtrssm_overshoot_gather(C.byref(table), None, None, *geom, 5, 6, None) == -1  # null actions
    assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *geom, 5, 6, None) == -1 and b"count" in lib.mtrssm_last_error()
    table.count = 1
    table.width[0] = 8
    assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *geom, 5, 6, None) == -1 and b"entry 0" in lib.mtrssm_last_error()
    table.src[0], table.dst[0] = 1024, 2048
    for bad in ((0, 6, 2, 4, 0), (3, 1, 2, 4, 0), (3, 6, 3, 4, 0), (3, 6, 2, 0, 0), (3, 6, 2, 4, 5), (3, 6, 2, 4, -1)):  # B, T, N, s, o
        assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *bad, 5, 6, None) == -1, bad
        assert lib.mtrssm_overshoot_scatter(C.byref(table), *bad, None) == -1, bad
    assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *geom, 1, 6, None) == -1  # D < 2
    assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *geom, 5, 0, None) == -1  # A <= 0
    assert lib.mtrssm_overshoot_gather(C.byref(table), 258, 512, *geom, 5, 6, None) == -1  # misaligned actions
    table.dst[0] = 1024
    assert lib.mtrssm_overshoot_gather(C.byref(table), 256, 512, *geom, 5, 6, None) == -1 and b"in place" in lib.mtrssm_last_error()
    assert lib.mtrssm_overshoot_scatter(C.byref(table), *geom, None) == -1
    table.dst[0] = 2050
    assert lib.mtrssm_overshoot_scatter(C.byref(table), *geom, None) == -1 and b"aligned" in lib.mtrssm_last_error()
    assert lib.mtrssm_overshoot_scatter(None, *geom, None) == -1
    # the KL pair: (b_global, row0, b_local, T, N, s, o, D, K, C)
    assert lib.mtrssm_overshoot_kl_workspace_bytes(3, 2, 5) == 3 * 2 * 5 * 8
    assert lib.mtrssm_overshoot_kl_workspace_bytes(0, 2, 5) == -1 and lib.mtrssm_overshoot_kl_workspace_bytes(3, 2, 1) == -1
    assert lib.mtrssm_overshoot_kl_workspace_bytes(1 << 20, 1 << 20, 2) == -1
    ok = (5, 1, 3, 6, 2, 4, 0, 5, 6, 5)
    fwd = lambda g, ptrs=(256, 512, None), outs=(1024, 2048, 4096, 8192, 16384), nbytes=240: lib.mtrssm_overshoot_kl_fwd(  # noqa: E731
        *ptrs, *g, *outs, nbytes, None)
    bwd = lambda g, ptrs=(256, 512, None, 1024, 2048), w=(1.0, 0.0), outs=(4096, None): lib.mtrssm_overshoot_kl_bwd(*ptrs, *g, *w, *outs, None)  # noqa: E731
    assert fwd(ok, ptrs=(None, 512, None)) == -1 and b"overshoot_kl_fwd" in lib.mtrssm_last_error()
    assert fwd(ok, outs=(1024, None, 4096, 8192, 16384)) == -1
    assert bwd(ok, ptrs=(256, 512, None, None, 2048)) == -1 and b"overshoot_kl_bwd" in lib.mtrssm_last_error()
    for bad in ((5, 3, 3, 6, 2, 4, 0, 5, 6, 5), (5, -1, 3, 6, 2, 4, 0, 5, 6, 5), (0, 0, 3, 6, 2, 4, 0, 5, 6, 5), (5, 1, 0, 6, 2, 4, 0, 5, 6, 5),
                (5, 1, 3, 6, 1, 4, 0, 5, 6, 5), (5, 1, 3, 6, 2, 4, 0, 1, 6, 5), (5, 1, 3, 6, 2, 4, 0, 5, 0, 5), (5, 1, 3, 6, 2, 4, 0, 5, 6, 0),
                (5, 1, 3, 6, 2, 4, 0, 5, 1 << 20, 1 << 20)):
        assert fwd(bad) == -1, bad
        assert bwd(bad) == -1, bad
    assert fwd(ok, nbytes=232) == -1 and b"workspace" in lib.mtrssm_last_error()
    assert fwd(ok, outs=(1024, 2052, 4096, 8192, 16384)) == -1 and b"aligned" in lib.mtrssm_last_error()  # the table is a double
    assert fwd(ok, ptrs=(258, 512, None)) == -1
    assert bwd(ok, w=(1.0, 0.5)) == -1 and b"w_post" in lib.mtrssm_last_error()  # a weight without its buffer
    assert bwd(ok, outs=(4096, 8192)) == -1  # a buffer without its weight
    assert bwd(ok, w=(-1.0, 0.0)) == -1
    assert bwd(ok, outs=(512, None)) == -1 and b"aliases" in lib.mtrssm_last_error()
    assert bwd(ok, w=(1.0, 1.0), outs=(4096, 4096)) == -1
