"""GPU (MI355X): the latent census, kernel and end to end.

What is pinned here.  ``mtrssm_latent_census`` is the float64 rule on the same fp32 inputs: the planes to the project's loss-term
tolerance (rtol 2e-5, atol 2e-6: at gain 8 some entropies lie below the atol and are held to it alone), the double accumulators to rtol
1e-12, ``n``, ``frames``, ``pairs`` and the position counts exactly, the planes' zero pattern the rule's.  Two calls agree bitwise and
a second call doubles the table exactly; ``planes = NULL`` gives the same table; the position sums are the host's float64 left fold of
the returned planes bit for bit; a row's planes depend on that row (and its first copy) only.  The shapes are the smallest at which the
kernel takes another path: one wave per scan row with the row's partial in LDS (K <= 64 and K * C <= 512), the partial in the
workspace on either side of both limits, staged spans up to C = 512 and in-place reads from C = 513, more scan rows than the grid has
workgroups.  A census step of either model class and of a weighted model is the rule on what its rollout returned, ``lengths`` equals a
batch that carries ``valid_global``, and ``validation_step`` keeps its ``val/*`` values bit for bit (at frame counts whose NLL sums fit
one workgroup, as in ``tests/test_likelihood_gpu.py``)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from multimodal_mtrssm_amd import CensusTable, LatentCensus, _lib
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd.census import PLANES, group_cells, table_views
from tests.test_census_capi import check_c_refusals
from tests.test_census_host import census_inputs, mixed_valid
from tests.test_likelihood_gpu import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

B, T = 3, 6
LENGTHS = (6, 4, 1)
OBSERVE = ("both", "audio", "vision")

SHAPES = [  # (B, G, T, K, C)
    (1, 1, 1, 1, 1),      # the smallest possible shape
    (3, 1, 5, 3, 5),
    (2, 3, 7, 8, 2),
    (4, 2, 6, 4, 4),
    (2, 2, 4, 2, 9),      # the general path above 8 classes
    (2, 2, 3, 64, 8),     # K = 64, K * C = 512: the last row partial that stays in LDS
    (2, 2, 3, 65, 3),     # K = 65: two spans of categoricals, the partial in the workspace
    (2, 2, 3, 33, 16),    # K * C = 528 > 512: spans of 32 categoricals, the partial in the workspace
    (2, 2, 3, 2, 512),    # C = 512: the widest staged categorical, one per span
    (2, 2, 3, 2, 513),    # C = 513: read in place
    (40, 3, 4, 3, 5),     # 40 partials per group for the second pass
    (1400, 3, 2, 2, 3),   # 4200 scan rows: more than the first pass has workgroups
]


def _assert_against_rule(got_planes, got_table, want_planes, want_table, k: int, c: int, t: int, what: str) -> None:  # noqa: ANN001, PLR0913
    planes = got_planes.cpu()
    assert planes.dtype == torch.float32 and bool(torch.isfinite(planes).all()), what
    err = (planes.double() - want_planes).abs()
    print(what, "planes: worst abs", float(err.max()), "worst err / (2e-6 + 2e-5 |ref|)", float((err / (2e-6 + 2e-5 * want_planes.abs())).max()))
    np.testing.assert_allclose(planes.double().numpy(), want_planes.numpy(), rtol=2e-5, atol=2e-6, err_msg=f"{what} planes")
    assert torch.equal(planes == 0, want_planes.float() == 0), f"{what}: zero pattern"
    got, want = table_views(got_table.cpu(), k, c, t), table_views(want_table, k, c, t)
    for name in ("n", "frames", "pairs", "counts"):
        assert torch.equal(got[name], want[name]), f"{what} {name}"
    for name in ("qsum", "psum", *PLANES):
        rel = ((got[name] - want[name]).abs() / want[name].abs().clamp_min(1e-300)).max()
        print(what, name, "worst rel", float(rel))
        torch.testing.assert_close(got[name], want[name], rtol=1e-12, atol=0.0, msg=f"{what} {name}")
    # the position sums: the float64 left fold of the returned planes, bit for bit
    g = got_table.shape[0]
    rows = planes.double().reshape(len(PLANES), -1, g, t)
    fold = torch.zeros(g, len(PLANES), t, dtype=torch.float64)
    for row in range(rows.shape[1]):
        fold += rows[:, row].permute(1, 0, 2)
    assert torch.equal(got["positions"], fold), f"{what} positions"


# 1. the kernel is the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("b", "g", "t", "k", "c"), SHAPES)
def test_census_kernel_equals_the_float64_rule(b: int, g: int, t: int, k: int, c: int) -> None:  # noqa: PLR0914
    for i, gain in enumerate((0.1, 1.0, 8.0)):
        post, prior, stoch = census_inputs(b, g, t, k, c, gain, seed=i)
        dev = [x.to(DEV) for x in (post, prior, stoch)]
        for valid in (mixed_valid(b, t), None):
            what = f"census {(b, g, t, k, c)} gain {gain} valid {'mixed' if valid is not None else None}"
            dvalid = None if valid is None else valid.to(DEV)
            want_planes, want_table = LatentCensus.reference(post, prior, stoch, g, k, c, valid)
            planes, table = LatentCensus.fold(*dev, g, k, c, dvalid)
            torch.cuda.synchronize()
            assert tuple(planes.shape) == (5, b * g, t) and tuple(table.shape) == (g, group_cells(k, c, t)) and table.dtype == torch.float64
            _assert_against_rule(planes, table, want_planes, want_table, k, c, t, what)
            if valid is not None:
                dead = ~(torch.arange(t) < valid.clamp(0, t)[:, None]).repeat_interleave(g, dim=0)
                assert not bool(planes.cpu()[:, dead].any()), what  # exactly 0 on dead frames
            assert not bool(planes[3, 0::g].any()), what  # cross of the first copy: exactly 0
            # two calls agree bitwise; a second call into the same table doubles it exactly; planes = NULL gives the same table
            planes2, table2 = LatentCensus.fold(*dev, g, k, c, dvalid)
            assert torch.equal(planes, planes2) and torch.equal(table, table2), what
            none, table3 = LatentCensus.fold(*dev, g, k, c, dvalid, planes=False)
            assert none is None and torch.equal(table, table3), what
            _, twice = LatentCensus.fold(*dev, g, k, c, dvalid, table=table2)
            assert twice is table2 and torch.equal(twice, 2.0 * table), what
        same, same_table = LatentCensus.fold(dev[0], dev[0].clone(), dev[2], g, k, c)
        assert not bool(same[2].any()) and not bool(table_views(same_table, k, c, t)["kl"].any()), (b, g, t, k, c, gain)  # equal logits: exactly 0


def test_a_rows_planes_depend_on_that_row_only() -> None:
    b, g, t, k, c = 5, 3, 6, 4, 5
    post, prior, stoch = (x.to(DEV) for x in census_inputs(b, g, t, k, c, 1.0))
    valid = torch.tensor([6, 6, 5, 6, 3], dtype=torch.int32, device=DEV)
    planes, _ = LatentCensus.fold(post, prior, stoch, g, k, c, valid)
    moved = 2 * g + 1  # row 2's second copy: no other row's cross reads it
    other = [x.clone() for x in census_inputs(b, g, t, k, c, 1.0, seed=9)]
    changed = [x.clone() for x in (post, prior, stoch)]
    for x, y in zip(changed, other, strict=True):
        x[moved] = y[moved].to(DEV)
    planes2, _ = LatentCensus.fold(*changed, g, k, c, valid)
    keep = torch.ones(b * g, dtype=torch.bool, device=DEV)
    keep[moved] = False
    assert torch.equal(planes[:, keep], planes2[:, keep]) and not torch.equal(planes[:3, moved], planes2[:3, moved])
    first = 2 * g  # row 2's first copy: its own planes and the cross of its copies move, nothing else
    changed = [x.clone() for x in (post, prior, stoch)]
    for x, y in zip(changed, other, strict=True):
        x[first] = y[first].to(DEV)
    planes3, _ = LatentCensus.fold(*changed, g, k, c, valid)
    keep[moved] = True
    keep[first : first + g] = False
    assert torch.equal(planes[:, keep], planes3[:, keep])
    assert torch.equal(planes[[0, 1, 2, 4], first + 1 : first + g], planes3[[0, 1, 2, 4], first + 1 : first + g])
    assert not torch.equal(planes[3, first + 1 : first + g], planes3[3, first + 1 : first + g])


def test_c_entry_rejects_bad_arguments_without_a_launch_on_the_device() -> None:
    check_c_refusals(_lib.load())
    post, prior, stoch = (x.to(DEV) for x in census_inputs(2, 2, 3, 3, 4))
    with pytest.raises(ValueError, match="table must be"):
        LatentCensus.fold(post, prior, stoch, 2, 3, 4, table=torch.zeros(2, group_cells(3, 4, 3), device=DEV))  # (fp32)
    with pytest.raises(ValueError, match="valid"):
        LatentCensus.fold(post, prior, stoch, 2, 3, 4, torch.tensor([3, 3], dtype=torch.int32))  # (on the host)


# 2. a census step is the rule on what its rollout returned ------------------------------------------------------------------------------------
def _levels(model) -> tuple[tuple[str, int, int], ...]:  # noqa: ANN001
    return tuple((s.lstrip("_"), f.category_size, f.class_size) for s, f in model._latent_levels())  # noqa: SLF001


def _noise(model, census: LatentCensus, seed: int = 11) -> dict[str, torch.Tensor]:  # noqa: ANN001
    gen = torch.Generator().manual_seed(seed)
    return {key: torch.rand(shape, generator=gen).to(DEV) for key, shape in census.noise_shapes(model, B, T).items()}


def _assert_same_step(got: torch.Tensor, want: torch.Tensor, like: CensusTable, what: str) -> None:
    """Two runs of one step under the same uniforms: the rollout in front of the fold (encoders, gate, scans) is repeatable to the
    project's loss-term tolerance only (rtol 2e-5 with its atol 2e-6 per frame), so the census of the second run is the first's within
    that -- the frames, pairs and position counts exactly, and the class counts ``n`` wherever no sample sat on a bin's edge."""
    a, b = CensusTable(like.levels, like.groups, like.steps), CensusTable(like.levels, like.groups, like.steps)
    a.buffer.copy_(got.cpu())
    b.buffer.copy_(want.cpu())
    print(what, "bitwise equal:", torch.equal(a.buffer, b.buffer), "worst abs", float((a.buffer - b.buffer).abs().max()))
    for level in range(len(like.levels)):
        va, vb = a.views(level), b.views(level)
        frames = float(vb["frames"][0])
        for key in ("frames", "pairs", "counts"):
            assert torch.equal(va[key], vb[key]), f"{what} {key}"
        for key in ("n", "qsum", "psum", "positions", *PLANES):
            torch.testing.assert_close(va[key], vb[key], rtol=2e-5, atol=2e-6 * frames, msg=f"{what} level {level} {key}")


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default", "weighted"])
def test_census_step_is_the_rule_on_its_rollout(name: str) -> None:  # noqa: PLR0914
    case, model, batch = _setup(name)
    census = LatentCensus(OBSERVE, active_nats=0.05)
    noise = _noise(model, census)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    table = model.latent_census(batch, census, noise, lengths=lengths, keep_states=True)
    torch.cuda.synchronize()
    levels = _levels(model)
    assert isinstance(table, CensusTable) and table.levels == levels and table.groups == 3 and table.steps == T and table.observe == OBSERVE  # noqa: PLR2004
    assert table.active_nats == 0.05 and len(table.planes) == len(table.inputs) == len(levels) and torch.equal(table.valid, lengths)  # noqa: PLR2004
    stoch = table.states.stoch if case.kind == "mrssm" else table.states.stoch_l
    assert torch.equal(stoch.reshape(B * 3, T, -1), table.inputs[0][2])
    for level, (label, k, c) in enumerate(levels):
        host = [x.cpu() for x in table.inputs[level]]
        assert tuple(host[0].shape) == (B * 3, T, k * c)
        want_planes, want_table = LatentCensus.reference(*host, 3, k, c, lengths.cpu())
        _assert_against_rule(table.planes[level], table.level_view(level), want_planes, want_table, k, c, T, f"{name} level {label!r}")
        views = table.views(level)
        assert views["frames"].tolist() == [11.0] * 3 and views["pairs"].tolist() == [8.0] * 3 and views["counts"][0].tolist() == [3.0, 2.0, 2.0, 2.0, 1.0, 1.0]
        # the copies of a row share its uniforms and differ in what they observe: the subsets' posteriors part ways
        assert bool((views["cross"][1:].sum(-1) > 0).all()) and not bool(views["cross"][0].any())
    logged = table.scalars("val/latent")
    assert all(bool(torch.isfinite(x)) for x in logged.values()) and len(logged) == len(levels) * (3 * 9 + 2)
    # a second step adds into the same table and keeps nothing of the batch
    first = table.buffer.clone()
    again = model.latent_census(batch, census, noise, lengths=lengths, table=table)
    assert again is table and table.planes is None and table.inputs is None and table.states is None and table.valid is None
    _assert_same_step(table.buffer - first, first, table, f"{name} second step")
    # lengths= equals the batch that carries valid_global
    start, reset = torch.zeros(B, dtype=torch.int32), torch.ones(B, dtype=torch.bool)
    ragged = ds.EpisodeBatch(tuple(batch), start.to(DEV), reset.to(DEV), start, reset, valid=lengths, valid_host=lengths.cpu(), valid_global=lengths, row0=0)
    carried = model.latent_census(ragged, census, noise)
    _assert_same_step(carried.buffer, first, table, f"{name} valid_global")
    drawn = model.latent_census(batch, LatentCensus())  # without noise the step draws its own; one group, every frame live
    assert bool(torch.isfinite(drawn.buffer).all()) and drawn.views(0)["frames"].tolist() == [float(B * T)]
    if name == "weighted":
        assert model.weights_timeseries is not None


# 3. validation ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_cfg3dims"])
def test_validation_step_keeps_its_values_and_the_epoch_end_logs_the_census(name: str) -> None:
    """B = 2, T = 4 frames of 16 x 8 audio and 8 x 8 vision: one NLL workgroup per modality (see ``tests/test_likelihood_gpu.py``)."""
    _, model, batch = _setup(name, (2, 4))
    census = LatentCensus(("both", "vision"))
    try:
        torch.manual_seed(5)
        plain = model.validation_step(batch)
        direct = model.latent_census(batch, census)
        model.validation_step(batch)
        model.latent_census(batch, census, table=direct)
        assert model.census_table is None and model.on_validation_epoch_end() == {}
        model.val_census = census
        torch.manual_seed(5)
        both = model.validation_step(batch)
        assert set(both) == set(plain)
        for key, value in plain.items():
            assert torch.equal(both[key], value), (key, float(both[key]), float(value))  # bitwise: the census step runs after everything else
        model.validation_step(batch)
        assert isinstance(model.census_table, CensusTable) and model.census_table.views(0)["frames"].tolist() == [16.0, 16.0]
        logged = model.on_validation_epoch_end()
        assert model.census_table is None and model.on_validation_epoch_end() == {}
        want = direct.scalars("val/latent")
        assert set(logged) == set(want) and all(key.startswith("val/latent/") for key in logged)
        for key, value in want.items():
            assert torch.equal(logged[key], value), (key, float(logged[key]), float(value))
    finally:
        model.val_census = None
        model.census_table = None
