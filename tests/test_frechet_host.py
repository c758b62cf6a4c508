"""CPU: the Frechet distance on reader features -- the config's refusals, its plan and bins, the float64 rule of
the moments against a per-bin loop, the table's algebra, ``compute()`` against closed forms, and the model-level refusals.  Nothing here
launches a kernel: the models of this package run on the GPU only, so the evaluator's counts, the validation hook and the model-level
equality with the rule are pinned in ``tests/test_frechet_gpu.py``.  ``moment_bound``, ``integer_features`` and ``hand_counts`` are
shared with it.

Bounds.  Moments: the products are exact and both sides add at most ``n_j`` terms in double, so a second-moment cell may differ by
``2 n_j 2^-53 sum_n |x_ni x_nj|`` and a sum by ``2 n_j 2^-53 sum_n |x_ni|``; counts are equal.  ``compute()``: for covariances
``Q diag(a) Q^T`` and ``Q diag(b) Q^T`` with ``a, b`` in ``[0.5, 2]`` the closed form is ``cov = sum (sqrt a_i - sqrt b_i)^2`` and
``mean = |d mu|^2``; ``eigh`` is backward stable and ``sqrt`` Lipschitz on ``lambda >= 0.25``, so ``|got - want| <= 1e-9 (tr r + tr g)``
has orders of margin.  A singular covariance (``n < D``) is held to "finite and >= 0" only."""

from __future__ import annotations

import math

import pytest
import torch

from multimodal_mtrssm_amd import DigitClassifier, ForecastSkill, FrechetDistance, FrechetTable, StateCarry
from multimodal_mtrssm_amd.frechet import bin_names, cells
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

B, T, S, Q = 3, 8, 2, 3
LENGTHS = (8, 5, 2)
EDGES = (1, 2, 4)


def moment_bound(x: torch.Tensor, bins: torch.Tensor, j: int) -> torch.Tensor:
    """``[J, 1 + D + D * D]`` float64: the largest ``|kernel - rule|`` per cell (0 for the counts)."""
    d = x.shape[1]
    ax = x.detach().cpu().double().abs()
    bins = bins.cpu()
    out = torch.zeros(j, cells(d), dtype=torch.float64)
    for k in range(j):
        mine = ax[bins == k]
        n = float(mine.shape[0])
        out[k, 1 : 1 + d] = 2.0 * n * 2.0**-53 * mine.sum(0)
        out[k, 1 + d :] = (2.0 * n * 2.0**-53 * (mine.t() @ mine)).reshape(-1) * (1.0 + 2.0**-40)  # (the bound's own rounding)
    return out


def integer_features(n: int, d: int) -> torch.Tensor:
    """``x[n][i] = ((3 n + 5 i + n i) mod 17) - 8``: integers in [-8, 8], asymmetric in ``i``; every partial sum is exact."""
    r, c = torch.arange(n).unsqueeze(1), torch.arange(d).unsqueeze(0)
    return (((3 * r + 5 * c + r * c) % 17) - 8).to(torch.float32)


def hand_counts(lengths: tuple[int, ...], steps: int, q: int, edges: tuple[int, ...]) -> list[float]:
    """The live frames per bin, counted frame by frame."""
    names = bin_names(edges)
    counts = [0.0] * len(names)
    for n in lengths:
        c = max(1, min(q, steps))
        for t in range(min(n, steps)):
            h = 0 if t < c else t - c + 1
            if h == 0:
                counts[0] += 1
                continue
            for i, lo in enumerate(edges):
                hi = edges[i + 1] if i + 1 < len(edges) else steps
                if lo <= h < hi:
                    counts[i + 1] += 1
    return counts


def loop_moments(x: torch.Tensor, bins: torch.Tensor, j: int) -> torch.Tensor:
    """The statistic one row at a time."""
    d = x.shape[1]
    out = torch.zeros(j, cells(d), dtype=torch.float64)
    for n in range(x.shape[0]):
        k = int(bins[n])
        if 0 <= k < j:
            row = x[n].double()
            out[k, 0] += 1
            out[k, 1 : 1 + d] += row
            out[k, 1 + d :] += torch.outer(row, row).reshape(-1)
    return out


# -- 1. the config -------------------------------------------------------------------------------------------------------------------------
def test_config_validation_plan_and_bins() -> None:
    fd = FrechetDistance(Q, samples=S, edges=EDGES)
    assert (fd.context, fd.samples, fd.observe, fd.features, fd.edges, fd.group) == (Q, S, "both", "reader", EDGES, None)
    assert fd.bin_names == ("obs", "h1", "h2", "h4") and fd.streams == ("vision",) and fd.max_frames == ForecastSkill(Q).max_frames
    assert FrechetDistance(Q, features="encoder").streams == ("audio", "vision") and FrechetDistance(Q).edges == (1, 2, 4, 8)
    assert repr(fd) == "FrechetDistance(3, samples=2, observe='both', features='reader', edges=(1, 2, 4))"
    bound = fd.for_group("g")
    assert bound is not fd and bound.group == "g" and fd.group is None and bound.edges == EDGES
    for observe in ("both", "audio", "vision"):
        assert FrechetDistance(Q, S, observe).plan() == ForecastSkill(Q, S, observe).plan()
    for context in (0, -1, 1.5, True, None, 1 << 31):
        with pytest.raises(ValueError, match="context"):
            FrechetDistance(context)
    for samples in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="samples"):
            FrechetDistance(Q, samples=samples)
    with pytest.raises(ValueError, match="observe"):
        FrechetDistance(Q, observe="sound")
    for features in ("pixels", None, 3):
        with pytest.raises(ValueError, match="features"):
            FrechetDistance(Q, features=features)
    for edges in ((), (0, 1), (2, 2), (4, 2), (1.0, 2), "12", None, tuple(range(1, 17)), (True, 2)):
        with pytest.raises(ValueError, match="edges"):
            FrechetDistance(Q, edges=edges)
    valid = torch.tensor(LENGTHS, dtype=torch.int32)
    bins = fd.bins(B, T, valid, torch.device("cpu"))
    assert bins.dtype == torch.int32 and bins.tolist() == [[0, 0, 0, 1, 2, 2, 3, 3], [0, 0, 0, 1, 2, -1, -1, -1], [0, 0, -1, -1, -1, -1, -1, -1]]
    assert [float((bins == k).sum()) for k in range(4)] == hand_counts(LENGTHS, T, Q, EDGES) == [8.0, 2.0, 3.0, 2.0]
    assert FrechetDistance(2, edges=(2, 3)).bins(1, 6, None, torch.device("cpu")).tolist() == [[0, 0, -1, 1, 2, 2]]  # h = 1 is below the first edge
    assert FrechetDistance(9).bins(1, 4, None, torch.device("cpu")).tolist() == [[0, 0, 0, 0]]  # (a context past the end: all observed)


@pytest.fixture(scope="module", params=["mrssm_default", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


def test_noise_shapes_are_forecast_skills(cpu_model) -> None:  # noqa: ANN001
    _, model = cpu_model
    for observe in ("both", "audio"):
        assert FrechetDistance(Q, S, observe).noise_shapes(model, B, T) == ForecastSkill(Q, S, observe).noise_shapes(model, B, T)


# -- 2. the rule of the moments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize(("n", "d", "j"), [(1, 1, 1), (37, 10, 3), (70, 130, 2)])
def test_reference_moments_equal_the_loop_skip_foreign_bins_and_read_strided_rows(n: int, d: int, j: int) -> None:
    g = torch.Generator().manual_seed(100 * n + d)
    pad = torch.randn(n, d + 6, generator=g)
    x = pad[:, :d]  # a strided view: row stride d + 6
    assert n == 1 or d == 1 or not x.is_contiguous()
    bins = torch.randint(-1, j + 2, (n,), generator=g).to(torch.int32)  # -1, J and J + 1 skip the row
    if j > 1:
        bins[bins == j - 1] = -1  # one bin stays empty
    table = torch.full((j, cells(d)), 0.5, dtype=torch.float64)  # (the rule adds onto what is there)
    assert FrechetDistance.reference_moments(x, bins, j, table) is table
    want = loop_moments(x, bins, j)
    assert torch.equal(table[:, 0], want[:, 0] + 0.5)
    err, bound = (table - 0.5 - want).abs(), moment_bound(x, bins, j) + 2.0**-52 * (1.0 + want.abs())  # (+ the rounding of the 0.5)
    assert bool((err <= bound).all()), float((err - bound).max())
    kept = int(((bins >= 0) & (bins < j)).sum())
    assert float(want[:, 0].sum()) == kept and (j == 1 or float(want[j - 1].abs().sum()) == 0.0)
    # the same through fold (non-GPU tensors take the rule), and on integers exactly
    xi = integer_features(n, d + 6)[:, :d]
    got = FrechetDistance.fold(xi, bins, j, torch.zeros(j, cells(d), dtype=torch.float64))
    assert torch.equal(got, loop_moments(xi, bins, j))
    m = got[:, 1 + d :].reshape(j, d, d)
    assert torch.equal(m, m.transpose(1, 2))


def test_fold_refuses_bad_arguments() -> None:
    x, bins, table = torch.zeros(5, 4), torch.zeros(5, dtype=torch.int32), torch.zeros(2, cells(4), dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        FrechetDistance.fold(x.double(), bins, 2, table)
    with pytest.raises(ValueError, match="rows are contiguous"):
        FrechetDistance.fold(torch.zeros(4, 5).t(), bins, 2, table)
    with pytest.raises(ValueError, match="1 <= J <= 16"):
        FrechetDistance.fold(x, bins, 17, table)
    with pytest.raises(ValueError, match="1 <= D <= 256"):
        FrechetDistance.fold(torch.zeros(5, 257), bins, 2, table)
    with pytest.raises(ValueError, match="bins must be"):
        FrechetDistance.fold(x, bins.long(), 2, table)
    with pytest.raises(ValueError, match="bins must be"):
        FrechetDistance.fold(x, bins[:4], 2, table)
    with pytest.raises(ValueError, match="table must be"):
        FrechetDistance.fold(x, bins, 2, table.float())
    with pytest.raises(ValueError, match="table must be"):
        FrechetDistance.reference_moments(x, bins, 3, table)


# -- 3. the table ----------------------------------------------------------------------------------------------------------------------------
def _filled(streams: tuple[str, ...], d: int, names: tuple[str, ...], seed: int) -> FrechetTable:
    g = torch.Generator().manual_seed(seed)
    table = FrechetTable(streams, d, names)
    for s in range(len(streams)):
        for side in range(2):
            x = torch.randn(40, d, generator=g)
            FrechetDistance.fold(x, torch.randint(0, len(names), (40,), generator=g).to(torch.int32), len(names), table.block(s, side))
    return table


def test_table_add_save_load_and_refusals() -> None:
    names = ("obs", "h1", "h2")
    a, b = _filled(("audio", "vision"), 6, names, 1), _filled(("audio", "vision"), 6, names, 2)
    assert a.buffer.dtype == torch.float64 and tuple(a.buffer.shape) == (2, 2, 3, cells(6)) and a.features is None and a.bins is None and a.states is None
    assert a.block("vision", "generated").data_ptr() == a.buffer[1, 1].data_ptr() and a.block(0, 0).is_contiguous()
    want = a.buffer + b.buffer
    assert a.add(b) is a and torch.equal(a.buffer, want) and a.all_reduce() is a  # (no process group: a no-op)
    saved = a.state_dict()
    fresh = FrechetTable(("audio", "vision"), 6, names)
    fresh.load_state_dict(saved)
    assert torch.equal(fresh.buffer, a.buffer) and saved["buffer"].data_ptr() != a.buffer.data_ptr()
    for other in (FrechetTable(("vision",), 6, names), FrechetTable(("audio", "vision"), 7, names), FrechetTable(("audio", "vision"), 6, names[:2]),
                  FrechetTable(("audio", "vision"), 6, ("obs", "h1", "h3"))):
        with pytest.raises(ValueError, match="do not add"):
            a.add(other)
        with pytest.raises(ValueError, match="does not load"):
            other.load_state_dict(saved)
    for bad in (((), 6, names), (("a", "a"), 6, names), (("a",), 0, names), (("a",), 257, names), (("a",), 6, ()), (("a", "b"), (6, 7), names)):
        with pytest.raises(ValueError):
            FrechetTable(*bad)
    assert FrechetTable(("a", "b"), (6, 6), names).dim == 6  # noqa: PLR2004


def _moments_of(mu: torch.Tensor, cov: torch.Tensor, n: float) -> torch.Tensor:
    """The block ``[1 + D + D * D]`` of ``n`` rows with exactly this mean and (population) covariance."""
    return torch.cat([torch.tensor([n], dtype=torch.float64), n * mu, (n * (cov + torch.outer(mu, mu))).reshape(-1)])


@pytest.mark.parametrize("d", [10, 128, 256])
def test_compute_meets_the_closed_form(d: int) -> None:
    g = torch.Generator().manual_seed(d)
    q, _ = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    a, b = 0.5 + 1.5 * torch.rand(d, generator=g, dtype=torch.float64), 0.5 + 1.5 * torch.rand(d, generator=g, dtype=torch.float64)
    mu_r, mu_g = torch.randn(d, generator=g, dtype=torch.float64), torch.randn(d, generator=g, dtype=torch.float64)
    cov_r, cov_g = (q * a) @ q.t(), (q * b) @ q.t()
    table = FrechetTable(("vision",), d, ("obs", "h1", "h2", "h4"))
    table.block(0, 0)[0], table.block(0, 1)[0] = _moments_of(mu_r, cov_r, 1000.0), _moments_of(mu_g, cov_g, 3000.0)
    table.block(0, 0)[1], table.block(0, 1)[1] = _moments_of(mu_r, cov_r, 500.0), _moments_of(mu_r, cov_r, 700.0)  # identical sides
    table.block(0, 0)[2], table.block(0, 1)[2] = _moments_of(mu_r, cov_r, 500.0), _moments_of(0.5 * mu_r, 0.25 * cov_r, 500.0)  # scaled by 0.5
    table.block(0, 0)[3], table.block(0, 1)[3] = _moments_of(mu_r, cov_r, 1.0), _moments_of(mu_g, cov_g, 50.0)  # one real row
    got = table.compute()["vision"]
    trace = float(a.sum() + b.sum())
    want_cov, want_mean = float(((a.sqrt() - b.sqrt()) ** 2).sum()), float(((mu_r - mu_g) ** 2).sum())
    print(d, "cov err / trace", abs(float(got["cov"][0]) - want_cov) / trace, "mean err / trace", abs(float(got["mean"][0]) - want_mean) / trace,
          "self fd / trace", float(got["fd"][1]) / (2 * float(a.sum())))
    assert abs(float(got["cov"][0]) - want_cov) <= 1e-9 * trace and abs(float(got["mean"][0]) - want_mean) <= 1e-9 * trace
    assert abs(float(got["fd"][0]) - (want_cov + want_mean)) <= 1e-9 * trace
    assert abs(float(got["trace_ratio"][0]) - float(b.sum() / a.sum())) <= 1e-9 * float(b.sum() / a.sum())
    assert (float(got["n_real"][0]), float(got["n_generated"][0])) == (1000.0, 3000.0)
    assert 0.0 <= float(got["fd"][1]) <= 1e-9 * 2 * float(a.sum()) and abs(float(got["trace_ratio"][1]) - 1.0) <= 1e-9  # noqa: PLR2004
    assert abs(float(got["trace_ratio"][2]) - 0.25) <= 1e-9  # noqa: PLR2004
    assert abs(float(got["cov"][2]) - 0.25 * float(a.sum())) <= 1e-9 * 1.25 * float(a.sum())  # sum (sqrt a - sqrt(a / 4))^2
    for key in ("fd", "mean", "cov", "trace_ratio"):
        assert math.isnan(float(got[key][3])), key  # fewer than 2 rows on the real side
    assert (float(got["n_real"][3]), float(got["n_generated"][3])) == (1.0, 50.0)
    scalars = table.scalars("val/frechet")
    assert set(scalars) == {f"val/frechet/vision/{p}/{n}" for p in ("fd", "mean", "cov", "trace_ratio", "n") for n in ("obs", "h1", "h2", "h4")}
    assert all(v.dtype == torch.float32 for v in scalars.values()) and float(scalars["val/frechet/vision/n/h2"]) == 500.0  # noqa: PLR2004
    assert math.isnan(float(scalars["val/frechet/vision/fd/h4"])) and float(scalars["val/frechet/vision/n/h4"]) == 1.0


def test_a_singular_bin_is_finite_and_not_negative_and_an_empty_table_is_nan() -> None:
    d, n = 24, 7  # n < D: a singular covariance
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(3))
    table = FrechetTable(("vision",), d, ("obs", "h1"))
    zeros = torch.zeros(n, dtype=torch.int32)
    FrechetDistance.fold(x, zeros, 2, table.block(0, 0))
    FrechetDistance.fold(x, zeros, 2, table.block(0, 1))
    got = table.compute()["vision"]
    assert math.isfinite(float(got["fd"][0])) and float(got["fd"][0]) >= 0.0 and float(got["mean"][0]) == 0.0
    assert all(math.isnan(float(got[k][1])) for k in ("fd", "mean", "cov", "trace_ratio")) and float(got["n_real"][1]) == 0.0


# -- 4. the model-level refusals ---------------------------------------------------------------------------------------------------------------
def test_frechet_step_refusals(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    b, t = batch[0].shape[:2]
    fd, reader = FrechetDistance(Q, S), DigitClassifier()
    assert model.val_frechet is None and model.frechet_table is None and model.frechet_classifier is None
    assert model.on_validation_epoch_end() == {}  # without val_frechet an epoch logs what it logged
    keys = set(model.state_dict())
    model.frechet_classifier = reader
    try:
        assert set(model.state_dict()) == keys and model.frechet_classifier is reader  # a tool, not a submodule
    finally:
        model.frechet_classifier = None
    with pytest.raises(ValueError, match="masked"):
        model.frechet_distance((*batch, torch.ones(b, t, 2, dtype=torch.bool)), fd, reader)
    with pytest.raises(ValueError, match="FrechetDistance"):
        model.frechet_distance(batch, ForecastSkill(Q), reader)
    model.state_carry = StateCarry.for_model(model, b)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.frechet_distance(batch, fd, reader)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="classifier must be a DigitClassifier"):
        model.frechet_distance(batch, fd)
    with pytest.raises(ValueError, match="classifier must be a DigitClassifier"):
        model.frechet_distance(batch, fd, torch.nn.Linear(2, 2))
    embed = model.audio_representation.obs_embed_size
    for foreign in (FrechetTable(("audio", "vision"), 128, fd.bin_names), FrechetTable(("vision",), 64, fd.bin_names),
                    FrechetTable(("vision",), 128, ("obs", "h1")), ForecastSkill(Q)):
        with pytest.raises(ValueError, match="table must be a FrechetTable"):
            model.frechet_distance(batch, fd, reader, table=foreign)
    with pytest.raises(ValueError, match="table must be a FrechetTable"):
        model.frechet_distance(batch, FrechetDistance(Q, S, features="encoder"), table=FrechetTable(("vision",), embed, fd.bin_names))
    model.audio_representation.obs_embed_size = 257
    try:
        with pytest.raises(ValueError, match="at most 256"):
            model.frechet_distance(batch, FrechetDistance(Q, S, features="encoder"))
    finally:
        model.audio_representation.obs_embed_size = embed


def test_the_reader_refuses_frames_that_are_not_32_by_32() -> None:
    case = CASES["mrssm_nonsquare"]  # 8 x 8 vision frames
    model = product_from_case(case, build_model(case), "cpu")
    with pytest.raises(ValueError, match="the digit classifier reads 1 x 32 x 32 vision frames"):
        model.frechet_distance(build_batch(case), FrechetDistance(2, 2), DigitClassifier())
