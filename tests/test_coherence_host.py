"""CPU: generation coherence on the host -- the config's refusals and plan, the float64 rule on hand-built logits
whose answers are known by hand (a tie, a non-finite row, dead labels, a short row, every split of context against ``T``), the table's
rules (``add``, exact doubling, the scalar keys and bins, kappa on a diagonal and on an outer-product histogram, NaN on empty) and the
audio route of the reader training tool's loader.  ``coherence_inputs`` also makes the synthetic logits of ``tests/test_coherence_gpu.py``."""

from __future__ import annotations

import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd import CoherenceTable, ForecastSkill, GenerationCoherence
from multimodal_mtrssm_amd.coherence import PLANES, group_cells, table_views
from multimodal_mtrssm_amd.evaluation import CopyPlan

NAN = float("nan")


def coherence_inputs(b: int, g: int, s: int, t: int, seed: int = 0) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """fp32 logits of both readers ``[B * G * S, T, 10]`` and int32 labels ``[B, T]``.  The audio reader agrees with the vision reader on
    about half of the copy-frames; about half of the labels are what copy 0 of the first group reads off the vision decode, a fifth
    what it hears; planted: exact ties of the two largest logits, a NaN row, a +inf row, a -inf entry, silence (-1) and a label past 9."""
    gen = torch.Generator().manual_seed(100 + seed)
    rows = b * g * s
    lv = torch.randn(rows, t, 10, generator=gen) * 2.0
    la = torch.randn(rows, t, 10, generator=gen) * 2.0
    same = torch.rand(rows, t, generator=gen) < 0.5  # noqa: PLR2004
    la = torch.where(same[..., None], lv + 0.25 * torch.randn(rows, t, 10, generator=gen), la)
    tie = torch.rand(rows, t, generator=gen) < 0.15  # noqa: PLR2004
    top = lv.max(-1).values + 1.0
    lv[..., 3] = torch.where(tie, top, lv[..., 3])
    lv[..., 7] = torch.where(tie, top, lv[..., 7])
    dv = lv.reshape(b, g * s, t, 10)[:, 0].argmax(-1)
    da = la.reshape(b, g * s, t, 10)[:, 0].argmax(-1)
    labels = torch.randint(0, 10, (b, t), generator=gen)
    pick = torch.rand(b, t, generator=gen)
    labels = torch.where(pick < 0.5, dv, labels)  # noqa: PLR2004
    labels = torch.where((pick >= 0.5) & (pick < 0.7), da, labels)  # noqa: PLR2004
    labels = torch.where(pick > 0.9, torch.full_like(labels, -1), labels)  # noqa: PLR2004
    labels[-1, t - 1] = 12
    if t > 2:  # noqa: PLR2004  (dead labels inside the rows as well)
        labels[0, 1], labels[min(1, b - 1), 2] = -1, 12
    labels[0, 0], labels[0, t - 1] = int(dv[0, 0]), int(da[0, t - 1])  # (live frames at both ends of the first row)
    lv[0, 0, 4] = NAN                      # copy 0 of row 0 at frame 0: the vision reader fails
    la[min(1, rows - 1), t - 1] = math.inf  # the audio reader fails at the last frame
    lv[rows - 1, t // 2, 9] = -math.inf    # not finite either
    return lv, la, labels.to(torch.int32)


def mixed_valid(b: int, t: int) -> torch.Tensor:
    """int32 ``[B]``: whole rows, then rows that end early (down to one frame)."""
    return torch.tensor([max(t - 2 * i, 1) if i else t for i in range(b)], dtype=torch.int32)


# -- the config ------------------------------------------------------------------------------------------------------------------------------
def test_config_refusals() -> None:
    for bad in (0, -1, True, 1.5, "3", 1 << 31):
        with pytest.raises(ValueError, match="context"):
            GenerationCoherence(bad)
    for bad in (0, 17, True, 2.0):
        with pytest.raises(ValueError, match="samples"):
            GenerationCoherence(3, samples=bad)
    for bad in ((), "both", ("both", "both"), ("both", "sound"), ("both", "audio", "vision", "both", "audio"), None, (3,)):
        with pytest.raises(ValueError, match="observe"):
            GenerationCoherence(3, observe=bad)
    gc = GenerationCoherence(30, samples=10)
    assert gc.observe == ("both", "audio", "vision") and gc.groups == 3 and gc.copies == 30 and gc.max_frames == 4096 and gc.group is None  # noqa: PLR2004
    assert repr(gc) == "GenerationCoherence(30, samples=10, observe=('both', 'audio', 'vision'))"
    bound = gc.for_group("a group")
    assert bound is not gc and bound.group == "a group" and gc.group is None and bound.observe == gc.observe
    assert GenerationCoherence((1 << 31) - 1, samples=16, observe=["vision"]).observe == ("vision",)


class _Model:
    _INIT_KEYS = ("u_init",)
    _POST_KEYS = ("u_post",)

    @staticmethod
    def _category_size_of(key: str) -> int:
        return 3


def test_plan_is_the_documented_copy_plan_and_its_first_copies_are_the_skills() -> None:
    b, t, s, c = 2, 6, 3, 4
    gc = GenerationCoherence(c, samples=s, observe=("both", "audio", "vision"))
    plan = gc.plan()
    assert plan == CopyPlan(9, (3, 3, 3, 1, 1, 1, 2, 2, 2), c, init="row", post="tail")
    assert gc.noise_shapes(_Model, b, t) == {"u_init": (b, 3), "u_post": (b, t, 3), "u_tail": (b, 9, t, 3)}
    skill = ForecastSkill(c, samples=s).plan()
    assert ForecastSkill(c, samples=s).noise_shapes(_Model, b, t) == {"u_init": (b, 3), "u_post": (b, t, 3), "u_tail": (b, s, t, 3)}
    gen = torch.Generator().manual_seed(0)
    codes = ((torch.arange(t) < c).to(torch.int32) * 3).expand(b, t).contiguous()
    base = {c: (codes, torch.ones(b, 2, dtype=torch.bool))}
    noise = {"u_init": torch.rand(b, 3, generator=gen), "u_post": torch.rand(b, t, 3, generator=gen), "u_tail": torch.rand(b, 9, t, 3, generator=gen)}
    wide_codes, mask0, wide, spread = plan.expand(base, noise, {"u_init": 3, "u_post": 3})
    want_codes, want_mask0, want, _ = skill.expand(base, {**noise, "u_tail": noise["u_tail"][:, :s].contiguous()}, {"u_init": 3, "u_post": 3})
    assert tuple(wide_codes.shape) == (b * 9, t) and tuple(wide["u_post"].shape) == (b * 9, t, 3)
    first = lambda x: x.reshape(b, 9, *x.shape[1:])[:, :s].reshape(b * s, *x.shape[1:])  # noqa: E731
    assert torch.equal(first(wide_codes), want_codes) and torch.equal(first(mask0), want_mask0)
    for key in ("u_init", "u_post"):
        assert torch.equal(first(wide[key]), want[key]), key
    per_copy = wide_codes.reshape(b, 9, t)
    assert per_copy[0, :, 0].tolist() == [3, 3, 3, 1, 1, 1, 2, 2, 2] and not bool(per_copy[:, :, c:].any())
    assert torch.equal(wide["u_post"].reshape(b, 9, t, 3)[:, 5, c:], noise["u_tail"][:, 5, c:])  # copy (g = 1, s = 2) reads u_tail[b, 1 * S + 2]
    assert torch.equal(spread(torch.arange(b)), torch.arange(b).repeat_interleave(9))
    one = GenerationCoherence(c, samples=2, observe=("audio",)).plan()
    assert one == CopyPlan(2, (1, 1), c, init="row", post="tail")


# -- the rule on hand-built logits -------------------------------------------------------------------------------------------------------------
def _hot(*digits: int, scale: float = 4.0) -> torch.Tensor:
    z = torch.zeros(10)
    for d in digits:
        z[d] = scale
    return z


E4 = math.exp(4.0)
P_HOT, P_OFF = E4 / (E4 + 9.0), 1.0 / (E4 + 9.0)          # softmax of one logit at 4, nine at 0
P_TIE, P_TIE_OFF = E4 / (2.0 * E4 + 8.0), 1.0 / (2.0 * E4 + 8.0)  # two logits at 4, eight at 0
SOFT_SAME = P_HOT * P_HOT + 9.0 * P_OFF * P_OFF
SOFT_TIE_OTHER = 2.0 * P_TIE * P_OFF + P_TIE_OFF * P_HOT + 7.0 * P_TIE_OFF * P_OFF  # vision tie (3, 7), audio hot at 5


def _hand_case() -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """B = 1, G = 1, S = 2, T = 4.  Frame 0 (label 3): copy 0 reads (3, 3); copy 1 has a vision tie of 3 and 7 (reads 3) and hears 5.
    Frame 1 (label 5): copy 0's vision row holds a NaN (bin 10) and it hears 5; copy 1 reads (5, 5).  Frame 2 is silence, frame 3 has
    label 12: both dead, whatever their logits."""
    lv, la = torch.zeros(2, 4, 10), torch.zeros(2, 4, 10)
    lv[0, 0], la[0, 0] = _hot(3), _hot(3)
    lv[1, 0], la[1, 0] = _hot(3, 7), _hot(5)
    lv[0, 1], la[0, 1] = _hot(5), _hot(5)
    lv[0, 1, 8] = NAN
    lv[1, 1], la[1, 1] = _hot(5), _hot(5)
    lv[:, 2:], la[:, 2:] = _hot(1), _hot(1)
    lv[1, 3, 0] = NAN
    return lv, la, torch.tensor([[3, 5, -1, 12]], dtype=torch.int32)


def _pairs_of(entries: dict[tuple[int, int, int], float]) -> torch.Tensor:
    want = torch.zeros(2, 11, 11, dtype=torch.float64)
    for key, n in entries.items():
        want[key] = n
    return want


def test_reference_on_hand_built_logits() -> None:
    lv, la, labels = _hand_case()
    planes, table = GenerationCoherence.reference(lv, la, labels, 1, 2, 2)
    assert planes.dtype == torch.float64 and tuple(planes.shape) == (5, 1, 4) and tuple(table.shape) == (1, group_cells(4)) and group_cells(4) == 6 * 4 + 242  # noqa: PLR2004
    v = table_views(table, 4)
    # the tie reads 3 (the first maximum); the NaN row reads bin 10: no hit, no agreement, soft 0
    assert planes[:4, 0].tolist() == [[1.0, 0.5, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0], [0.5, 0.5, 0.0, 0.0]]
    assert float(planes[4, 0, 0]) == pytest.approx((SOFT_SAME + SOFT_TIE_OTHER) / 2.0, rel=1e-12)
    assert float(planes[4, 0, 1]) == pytest.approx(SOFT_SAME / 2.0, rel=1e-12) and planes[4, 0, 2:].tolist() == [0.0, 0.0]
    assert v["sums"][0, :4].tolist() == [[3.0, 0.0, 0.0, 0.0], [3.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]]
    assert float(v["sums"][0, 4, 0]) == pytest.approx(2.0 * SOFT_SAME + SOFT_TIE_OTHER, rel=1e-12) and not bool(v["sums"][0, 4, 1:].any())
    assert v["counts"][0].tolist() == [4.0, 0.0, 0.0, 0.0]
    assert torch.equal(v["pairs"][0], _pairs_of({(0, 3, 3): 1.0, (0, 3, 5): 1.0, (0, 10, 5): 1.0, (0, 5, 5): 1.0}))
    # context = 1: frame 1 is the first open-loop frame (h = 1, phase 1)
    _, table = GenerationCoherence.reference(lv, la, labels, 1, 2, 1)
    v = table_views(table, 4)
    assert v["sums"][0, :4].tolist() == [[2.0, 1.0, 0.0, 0.0], [1.0, 2.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]
    assert float(v["sums"][0, 4, 1]) == pytest.approx(SOFT_SAME, rel=1e-12) and v["counts"][0].tolist() == [2.0, 2.0, 0.0, 0.0]
    assert torch.equal(v["pairs"][0], _pairs_of({(0, 3, 3): 1.0, (0, 3, 5): 1.0, (1, 10, 5): 1.0, (1, 5, 5): 1.0}))
    # context >= T: everything is phase 0, whatever the context beyond T is
    for context in (4, 5, (1 << 31) - 1):
        _, wide = GenerationCoherence.reference(lv, la, labels, 1, 2, context)
        w = table_views(wide, 4)
        assert w["counts"][0].tolist() == [4.0, 0.0, 0.0, 0.0] and not bool(w["pairs"][0, 1].any()) and float(w["pairs"][0, 0].sum()) == 4.0  # noqa: PLR2004
        assert w["sums"][0, :4, 0].tolist() == [3.0, 3.0, 2.0, 2.0]
    # valid shorter than the context: frame 1 is past the row's end
    planes, table = GenerationCoherence.reference(lv, la, labels, 1, 2, 2, torch.tensor([1], dtype=torch.int32))
    v = table_views(table, 4)
    assert v["counts"][0].tolist() == [2.0, 0.0, 0.0, 0.0] and v["sums"][0, :4, 0].tolist() == [2.0, 1.0, 1.0, 1.0] and not bool(planes[:, :, 1:].any())
    assert torch.equal(v["pairs"][0], _pairs_of({(0, 3, 3): 1.0, (0, 3, 5): 1.0}))
    # valid outside [0, T] is clamped; a row of length 0 adds nothing
    _, none = GenerationCoherence.reference(lv, la, labels, 1, 2, 2, torch.tensor([-3], dtype=torch.int32))
    assert not bool(none.any())
    _, whole = GenerationCoherence.reference(lv, la, labels, 1, 2, 2, torch.tensor([9], dtype=torch.int32))
    assert table_views(whole, 4)["counts"][0].tolist() == [4.0, 0.0, 0.0, 0.0]


def test_groups_rows_and_the_fold_order() -> None:
    """Two rows of two groups: group g of row b reads the scan rows (b * G + g) * S ..; a table's cell is the left fold over b, then t."""
    b, g, s, t, c = 4, 2, 3, 7, 3
    lv, la, labels = coherence_inputs(b, g, s, t)
    valid = mixed_valid(b, t)
    planes, table, u = GenerationCoherence._rule(lv, la, labels, g, s, c, valid, None)  # noqa: SLF001
    assert tuple(u.shape) == (5, b * g, t) and torch.equal(planes, u / 3.0)
    v = table_views(table, t)
    want = torch.zeros(g, 5, t, dtype=torch.float64)
    rows = u.reshape(5, b, g, t)
    for row in range(b):
        for i in range(t):
            want[:, :, 0 if i < c else i - c + 1] += rows[:, row, :, i].T
    assert torch.equal(v["sums"], want)
    # a group's planes are the one-group rule on that group's scan rows
    for group in range(g):
        pick = torch.arange(b * g * s).reshape(b, g, s)[:, group].reshape(-1)
        alone, alone_table = GenerationCoherence.reference(lv[pick], la[pick], labels, 1, s, c, valid)
        assert torch.equal(alone, planes.reshape(5, b, g, t)[:, :, group]) and torch.equal(alone_table[0], table[group])
    live = (torch.arange(t) < valid[:, None]) & (labels >= 0) & (labels <= 9)  # noqa: PLR2004
    assert float(v["counts"].sum()) == float(live.sum()) * g * s and float(v["pairs"].sum()) == float(live.sum()) * g * s
    assert not bool(planes.reshape(5, b, g, t)[:, ~live.unsqueeze(1).expand(b, g, t)].any())
    fold_planes, fold_table = GenerationCoherence.fold(lv, la, labels, g, s, c, valid)  # (non-GPU tensors take the rule)
    assert fold_planes.dtype == torch.float32 and torch.equal(fold_planes, planes.float()) and torch.equal(fold_table, table)
    assert GenerationCoherence.fold(lv, la, labels, g, s, c, valid, planes=False)[0] is None


def test_fold_refusals() -> None:
    lv, la, labels = coherence_inputs(2, 2, 2, 5)
    for kw, match in (({"groups": 0}, "1 <= G"), ({"groups": 5}, "1 <= G"), ({"samples": 17}, "1 <= S"), ({"context": 0}, "context"),
                      ({"groups": 3}, "the logits must be")):
        args = {"groups": 2, "samples": 2, "context": 3, **kw}
        with pytest.raises(ValueError, match=match):
            GenerationCoherence.reference(lv, la, labels, args["groups"], args["samples"], args["context"])
    with pytest.raises(ValueError, match="both readers"):
        GenerationCoherence.reference(lv, la[:, :4], labels, 2, 2, 3)
    with pytest.raises(ValueError, match="both readers"):
        GenerationCoherence.reference(lv, la.double(), labels, 2, 2, 3)
    with pytest.raises(ValueError, match="labels must be"):
        GenerationCoherence.reference(lv, la, labels.long(), 2, 2, 3)
    with pytest.raises(ValueError, match="valid must be"):
        GenerationCoherence.reference(lv, la, labels, 2, 2, 3, torch.tensor([5, 5, 5], dtype=torch.int32))
    with pytest.raises(ValueError, match="table must be"):
        GenerationCoherence.reference(lv, la, labels, 2, 2, 3, table=torch.zeros(2, group_cells(6), dtype=torch.float64))
    with pytest.raises(ValueError, match="2\\^24"):
        GenerationCoherence.reference(torch.zeros(1 << 12, 1 << 12, 10), torch.zeros(1 << 12, 1 << 12, 10), torch.zeros(1 << 12, 1 << 12, dtype=torch.int32), 1, 1, 3)


# -- the table -------------------------------------------------------------------------------------------------------------------------------
def _table_of(rows: slice, t: int = 12, c: int = 3):  # noqa: ANN202
    b, g, s = 6, 3, 2
    lv, la, labels = coherence_inputs(b, g, s, t, seed=3)
    table = CoherenceTable(g, t)
    pick = slice(rows.start * g * s, rows.stop * g * s)
    GenerationCoherence.fold(lv[pick], la[pick], labels[rows], g, s, c, mixed_valid(b, t)[rows], table=table.buffer, planes=False)
    return table


def test_table_add_doubling_and_refusals() -> None:
    whole, a, b = _table_of(slice(0, 6)), _table_of(slice(0, 2)), _table_of(slice(2, 6))
    assert whole.buffer.dtype == torch.float64 and tuple(whole.buffer.shape) == (3, group_cells(12)) and whole.steps == 12 and whole.groups == 3  # noqa: PLR2004
    assert whole.observe == ("both", "audio", "vision") and whole.planes is None and whole.logits is None and whole.states is None
    both = _table_of(slice(0, 2))
    assert both.add(b) is both
    v, w = both.views(), whole.views()
    assert torch.equal(v["counts"], w["counts"]) and torch.equal(v["pairs"], w["pairs"]) and torch.equal(v["sums"][:, :4], w["sums"][:, :4])
    torch.testing.assert_close(v["sums"][:, 4], w["sums"][:, 4], rtol=1e-12, atol=0.0)
    assert bool((w["sums"][:, :4] == w["sums"][:, :4].round()).all()) and float(w["counts"].sum()) > 0
    # a second fold of the same step doubles the table exactly; two steps into one table are the add of two tables
    twice = _table_of(slice(0, 6))
    lv, la, labels = coherence_inputs(6, 3, 2, 12, seed=3)
    GenerationCoherence.fold(lv, la, labels, 3, 2, 3, mixed_valid(6, 12), table=twice.buffer, planes=False)
    assert torch.equal(twice.buffer, 2.0 * whole.buffer)
    assert torch.equal(_table_of(slice(0, 6)).add(whole).buffer, twice.buffer)
    assert a.all_reduce() is a  # (no process group: a no-op)
    for other in (CoherenceTable(3, 11), CoherenceTable(2, 12)):
        with pytest.raises(ValueError, match="do not add"):
            whole.add(other)
    for kw in ({"groups": 0}, {"groups": 5}, {"steps": 0}, {"observe": ("both",)}):
        with pytest.raises(ValueError):
            CoherenceTable(**{"groups": 3, "steps": 4, **kw})
    assert CoherenceTable(4, 2).observe == ("g0", "g1", "g2", "g3") and CoherenceTable(2, 2, observe=("vision", "audio")).observe == ("vision", "audio")


def test_rates_failed_scalars_and_bins() -> None:
    t = 12
    table = _table_of(slice(0, 6), t, 3)
    v = table.views()
    rates = table.rates(1)
    assert set(rates) == set(PLANES)
    for i, plane in enumerate(PLANES):
        have = v["counts"][1] > 0
        assert torch.equal(rates[plane][have], (v["sums"][1, i] / v["counts"][1])[have]) and bool(torch.isnan(rates[plane][~have]).all())
        assert bool(((rates[plane][have] >= 0) & (rates[plane][have] <= 1)).all())
    assert bool((rates["joint"][have] <= rates["agree"][have]).all()) and bool((rates["joint"][have] <= rates["vision"][have]).all())
    failed = table.failed(0)
    pairs = v["pairs"][0]
    assert float(failed["vision"][0]) == float(pairs[0, 10].sum() / pairs[0].sum()) and float(failed["audio"][1]) == float(pairs[1, :, 10].sum() / pairs[1].sum())
    assert float(pairs[0, 10].sum()) >= 1.0  # (the planted NaN row of group 0, frame 0)
    scalars = table.scalars("val/coherence")
    bins = ("obs", "h1", "h2", "h4", "h8")
    want = {f"val/coherence/{o}/{p}/{n}" for o in table.observe for p in PLANES for n in bins}
    want |= {f"val/coherence/{o}/kappa/{n}" for o in table.observe for n in ("obs", "open")}
    want |= {f"val/coherence/{o}/failed/{m}" for o in table.observe for m in ("vision", "audio")} | {"val/coherence/reads"}
    assert set(scalars) == want and all(x.dtype == torch.float32 for x in scalars.values())
    assert float(scalars["val/coherence/reads"]) == float(v["counts"].sum())
    # bins: obs is horizon 0, h2 the horizons [2, 4), h8 the horizons [8, T)
    assert float(scalars["val/coherence/audio/vision/obs"]) == pytest.approx(float(v["sums"][1, 0, 0] / v["counts"][1, 0]), rel=1e-6)
    assert float(scalars["val/coherence/audio/agree/h2"]) == pytest.approx(float(v["sums"][1, 2, 2:4].sum() / v["counts"][1, 2:4].sum()), rel=1e-6)
    assert float(scalars["val/coherence/vision/soft/h8"]) == pytest.approx(float(v["sums"][2, 4, 8:].sum() / v["counts"][2, 8:].sum()), rel=1e-6)
    other = table.scalars("x", edges=(1, 3))
    assert {k.rsplit("/", 1)[1] for k in other if "/joint/" in k} == {"obs", "h1", "h3"}
    with pytest.raises(ValueError, match="edges"):
        table.scalars("x", edges=(0, 2))


def test_kappa_and_nan_on_empty() -> None:
    table = CoherenceTable(2, 5)
    pairs = table.views()["pairs"]
    pairs[0, 0, :10, :10] = torch.diag(torch.arange(1.0, 11.0, dtype=torch.float64))  # the readers always agree: kappa 1
    row, col = torch.tensor([3.0, 1.0, 2.0] + [0.0] * 7, dtype=torch.float64), torch.tensor([1.0, 4.0] + [0.0] * 8, dtype=torch.float64)
    pairs[0, 1, :10, :10] = torch.outer(row, col)  # independent readers: agreement is what chance gives, kappa 0
    pairs[0, 1, 10, 2], pairs[0, 1, 4, 10] = 7.0, 5.0  # failed reads stay out of kappa ...
    assert float(table.kappa(0, 0)) == pytest.approx(1.0, abs=1e-15) and float(table.kappa(0, 1)) == pytest.approx(0.0, abs=1e-15)
    assert float(table.failed(0)["vision"][1]) == 7.0 / 42.0 and float(table.failed(0)["audio"][1]) == 5.0 / 42.0  # ... and are counted here  # noqa: PLR2004
    pairs[1, 0, 2, 2] = 9.0  # one digit only: pe = 1
    assert math.isnan(float(table.kappa(1, 0))) and math.isnan(float(table.kappa(1, 1)))
    empty = CoherenceTable(1, 3)
    assert all(bool(torch.isnan(x).all()) for x in empty.rates(0).values()) and all(bool(torch.isnan(x).all()) for x in empty.failed(0).values())
    scalars = empty.scalars("c")
    assert float(scalars["c/reads"]) == 0.0 and all(math.isnan(float(x)) for k, x in scalars.items() if k != "c/reads")


def _tool(name: str):  # noqa: ANN202
    spec = importlib.util.spec_from_file_location(name, Path(__file__).resolve().parents[1] / "tools" / f"{name}.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_the_report_of_the_cli_and_the_benchs_torch_scoring() -> None:
    cli = _tool("generation_coherence")
    assert cli.windows([10, 3, 8], 4, 3) == [(0, 0), (0, 3), (0, 6), (2, 0), (2, 3)] and cli.windows([10], 4, 4) == [(0, 0), (0, 4)]
    table = _table_of(slice(0, 6))
    text, tree = cli.report(table, "MoPoE-MRSSM", 3, 2, 6)
    assert set(tree["groups"]) == {"both", "audio", "vision"} and tree["reads"] == float(table.views()["counts"].sum())
    both = tree["groups"]["both"]
    assert set(both["rates"]) == set(PLANES) and list(both["rates"]["soft"]) == ["obs", "h1", "h2", "h4", "h8"]
    assert both["rates"]["agree"]["h2"] == float(table.binned(0)["agree"][2]) and both["kappa"]["open"] == float(table.kappa(0, 1))
    assert np.asarray(both["open_loop_pairs"]).shape == (10, 10) and len(both["by_horizon"]["joint"]) == 12  # noqa: PLR2004
    for line in ("## Observed: audio", "| rate | obs | h1 | h2 | h4 | h8 |", "Cohen's kappa of the two readers", "| | 0 | 1 | 2 |"):
        assert line in text, line
    empty_text, empty = cli.report(CoherenceTable(1, 4, observe=("vision",)), "x", 2, 1, 0)
    assert empty["groups"]["vision"]["kappa"] == {"obs": None, "open": None} and "n/a" in empty_text
    # the bench's yardstick: the same table from vectorised torch ops (whole numbers exactly, soft within addition order)
    bench = _tool("coherence_bench")
    lv, la, labels = coherence_inputs(4, 3, 2, 9, seed=1)
    for context in (4, 9, 20):
        _, want = GenerationCoherence.reference(lv, la, labels, 3, 2, context)
        a, b = table_views(bench.torch_scoring(lv, la, labels, 3, 2, context), 9), table_views(want, 9)
        assert torch.equal(a["counts"], b["counts"]) and torch.equal(a["pairs"], b["pairs"]) and torch.equal(a["sums"][:, :4], b["sums"][:, :4])
        torch.testing.assert_close(a["sums"][:, 4], b["sums"][:, 4], rtol=1e-12, atol=0.0)


# -- the audio reader's training data ----------------------------------------------------------------------------------------------------------
def test_the_training_tools_loader_reads_both_modalities(tmp_path: Path) -> None:
    spec = importlib.util.spec_from_file_location("train_digit_classifier", Path(__file__).resolve().parents[1] / "tools" / "train_digit_classifier.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    rng = np.random.default_rng(0)
    label = np.array([3, -1, 7, 7, 12, 0], dtype=np.int64)
    audio = rng.uniform(-80.0, 0.0, size=(6, 32, 32)).astype(np.float32)
    image = rng.integers(0, 256, size=(6, 1, 32, 32)).astype(np.float32)
    np.savez(tmp_path / "ep0.npz", audio=audio, image=image, label=label)
    keep = [0, 2, 3, 5]
    frames, got = tool.load_labelled_frames(tmp_path, "audio")
    assert got.dtype == torch.int32 and got.tolist() == [3, 7, 7, 0] and frames.dtype == torch.float32 and tuple(frames.shape) == (4, 1024)
    want = (torch.from_numpy(audio[keep]).reshape(4, 1024) + 80.0) / 80.0 * 2.0 - 1.0
    torch.testing.assert_close(frames, want, rtol=0.0, atol=1e-6)
    assert float(frames.min()) >= -1.0 and float(frames.max()) <= 1.0
    wide, _ = tool.load_labelled_frames(tmp_path, "audio", -100.0, 20.0)
    torch.testing.assert_close(wide, (torch.from_numpy(audio[keep]).reshape(4, 1024) + 100.0) / 120.0 * 2.0 - 1.0, rtol=0.0, atol=1e-6)
    vision, got_v = tool.load_labelled_frames(tmp_path)  # (the default is the vision route, as before)
    same, _ = tool.load_labelled_frames(tmp_path, "vision")
    assert got_v.tolist() == [3, 7, 7, 0] and tuple(vision.shape) == (4, 1024) and torch.equal(vision, same) and not torch.equal(vision, frames)
    np.savez(tmp_path / "ep1.npz", audio=audio.reshape(6, 1, 32, 32)[:, :, :16], image=image, label=label)
    with pytest.raises(ValueError, match="ep1.npz"):
        tool.load_labelled_frames(tmp_path, "audio")
    assert tool.load_labelled_frames(tmp_path)[1].numel() == 8  # noqa: PLR2004  (its images are fine)
    with pytest.raises(ValueError, match="modality"):
        tool.load_labelled_frames(tmp_path, "speaker")
