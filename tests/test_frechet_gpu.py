"""GPU (MI355X): the Frechet distance on reader features, kernel and end to end.

What is pinned here.  ``mtrssm_feature_moments`` is the float64 rule on the same fp32 features: the counts exactly, every sum and
second-moment cell within ``2 n_j 2^-53 sum_n |x_ni x_nj|`` (``tests/test_frechet_host.moment_bound``: exact products, at most ``n_j``
double additions on either side), and bit for bit on the integer features ``((3 n + 5 i + n i) mod 17) - 8``, whose partial sums are
all exact and which are asymmetric in ``i`` (a transposed or mis-rowed MFMA tile shows).  Both triangles are bit-identical, the call
adds onto the table, two calls agree bitwise and two half-calls are one whole call within the bound.  The shapes: the smallest, one
MFMA, tails in N and D with an empty bin and skipped rows, a tile edge past 128 with strided rows, the widest D, the reader's shape
and one where every row slice is busy.  A Frechet step of either model class is the rule on the features it returned
(``keep_states``), its generated features are the reader's on the same decode, its counts are the hand count, and two steps add up.
The models of this package run on the GPU only, so the evaluator cases the host file cannot run are here.  No ``fd`` value is compared
across devices."""

from __future__ import annotations

import pytest
import torch

from multimodal_mtrssm_amd import DigitClassifier, FrechetDistance, FrechetTable, _lib
from multimodal_mtrssm_amd.frechet import cells
from tests.test_frechet_capi import check_c_refusals
from tests.test_frechet_host import B, EDGES, LENGTHS, Q, S, T, hand_counts, integer_features, moment_bound
from tests.test_likelihood_gpu import _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [  # (N, D, J, ldx)
    (1, 1, 1, 1),         # the smallest case
    (4, 16, 1, 16),       # one MFMA
    (37, 10, 3, 10),      # tails in both N and D; one bin empty; some rows -1
    (70, 130, 2, 136),    # a tile edge past 128; strided rows
    (33, 256, 2, 256),    # the widest D
    (300, 128, 5, 128),   # the reader's shape
    (5000, 32, 4, 32),    # every row slice busy
]


def _bins(n: int, j: int, seed: int) -> torch.Tensor:
    """int32 ``[N]`` in ``[-1, J)``; with three bins the last stays empty."""
    bins = torch.randint(-1, j, (n,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    if n == 1:
        bins[:] = 0
    if j == 3:  # noqa: PLR2004
        bins[bins == 2] = -1  # noqa: PLR2004
    return bins


def _strided(x: torch.Tensor, ldx: int) -> torch.Tensor:
    """``x`` as a view of a ``[N, ldx]`` device buffer whose pad columns hold NaN: they must never be read."""
    pad = torch.full((x.shape[0], ldx), float("nan"), device=DEV)
    pad[:, : x.shape[1]] = x.to(DEV)
    return pad[:, : x.shape[1]]


def _rule(x: torch.Tensor, bins: torch.Tensor, j: int) -> torch.Tensor:
    return FrechetDistance.reference_moments(x, bins, j, torch.zeros(j, cells(x.shape[1]), dtype=torch.float64))


def _assert_within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    got = got.cpu()
    assert torch.equal(got[:, 0], want[:, 0]), f"{what}: counts {got[:, 0].tolist()} != {want[:, 0].tolist()}"
    err = (got - want).abs()
    over = err / bound.clamp_min(1e-300)
    print(what, "worst |got - ref|", float(err.max()), "worst err / bound", float(torch.where(err > 0, over, torch.zeros_like(over)).max()))
    assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} cells above the bound, worst {float(err.max())}"


def _assert_symmetric(table: torch.Tensor, d: int, what: str) -> None:
    m = table[:, 1 + d :].reshape(table.shape[0], d, d)
    assert torch.equal(m, m.transpose(1, 2)), f"{what}: the triangles differ"


# 1. the kernel is the rule ------------------------------------------------------------------------------------------------------------------
def test_c_entry_rejects_bad_arguments_without_a_launch_on_the_device() -> None:
    check_c_refusals(_lib.load())
    x, table = torch.zeros(5, 4, device=DEV), torch.zeros(2, cells(4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="bins must be"):
        FrechetDistance.fold(x, torch.zeros(5, dtype=torch.int32), 2, table)  # (on the host)
    with pytest.raises(ValueError, match="table must be"):
        FrechetDistance.fold(x, torch.zeros(5, dtype=torch.int32, device=DEV), 2, table.cpu())


@pytest.mark.parametrize(("n", "d", "j", "ldx"), SHAPES)
def test_moment_kernel_equals_the_float64_rule(n: int, d: int, j: int, ldx: int) -> None:
    what = f"moments {(n, d, j, ldx)}"
    bins = _bins(n, j, 7 * n + d)
    dbins = bins.to(DEV)
    # random normals, by the bound, onto a zeroed table
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(n + 1000 * d))
    dx = _strided(x, ldx)
    assert dx.stride(0) == ldx or n == 1
    table = torch.zeros(j, cells(d), dtype=torch.float64, device=DEV)
    assert FrechetDistance.fold(dx, dbins, j, table) is table
    torch.cuda.synchronize()
    _assert_within(table, _rule(x, bins, j), moment_bound(x, bins, j), f"{what} normal")
    _assert_symmetric(table, d, what)
    # the same call on another zeroed table: bitwise equal
    again = FrechetDistance.fold(dx, dbins, j, torch.zeros_like(table))
    assert torch.equal(again, table), f"{what}: two calls differ"
    # two half-calls onto one table: one whole call within the bound (each side adds a bin's rows once, in double)
    if n >= 2:  # noqa: PLR2004
        half = n // 2
        halves = torch.zeros_like(table)
        FrechetDistance.fold(dx[:half], dbins[:half].contiguous(), j, halves)
        FrechetDistance.fold(dx[half:], dbins[half:].contiguous(), j, halves)
        _assert_within(halves, table.cpu(), moment_bound(x, bins, j), f"{what} halves")
    # integers: exact, onto a table that already holds something; the prior contents are kept
    xi = integer_features(n, d)
    prior = torch.full((j, cells(d)), 3.0, dtype=torch.float64, device=DEV)
    FrechetDistance.fold(_strided(xi, ldx), dbins, j, prior)
    want = _rule(xi, bins, j) + 3.0
    got = prior.cpu()
    assert torch.equal(got, want), f"{what} integers: {int((got != want).sum())} cells differ, first at {(got != want).nonzero()[:4].tolist()}"
    _assert_symmetric(prior, d, f"{what} integers")
    if j == 3:  # noqa: PLR2004
        assert bool((got[2] == 3.0).all()), f"{what}: the empty bin was written"  # noqa: PLR2004


# 2. a Frechet step is the rule on the features it returned ------------------------------------------------------------------------------------
def _reader(seed: int = 5) -> DigitClassifier:
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        return DigitClassifier().to(DEV)


def _noise(model, fd: FrechetDistance, seed: int) -> dict[str, torch.Tensor]:  # noqa: ANN001
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(shape, generator=g).to(DEV) for k, shape in fd.noise_shapes(model, B, T).items()}


def _rule_of_step(table: FrechetTable, stream: str, side: int, j: int) -> tuple[torch.Tensor, torch.Tensor]:
    x, bins = table.features[stream][side].cpu(), table.bins[side].cpu()
    return _rule(x, bins, j), moment_bound(x, bins, j)


@pytest.mark.parametrize("name", ["mrssm_default", "mmtrssm_default"])
def test_frechet_step_is_the_rule_on_its_features(name: str) -> None:  # noqa: PLR0914
    case, model, batch = _setup(name, (B, T))
    reader, fd = _reader(), FrechetDistance(Q, samples=S, edges=EDGES)
    j = len(fd.bin_names)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    table = model.frechet_distance(batch, fd, reader, _noise(model, fd, 11), lengths=lengths, keep_states=True)
    torch.cuda.synchronize()
    assert isinstance(table, FrechetTable) and table.streams == ("vision",) and table.dim == 128 and table.bin_names == ("obs", "h1", "h2", "h4")  # noqa: PLR2004
    real, gen = table.features["vision"]
    assert tuple(real.shape) == (B * T, 128) and tuple(gen.shape) == (B * S * T, 128) and real.dtype == gen.dtype == torch.float32
    bins_r, bins_g = table.bins
    want_bins = fd.bins(B, T, lengths.cpu(), torch.device("cpu"))
    assert torch.equal(bins_r.cpu().reshape(B, T), want_bins) and torch.equal(bins_g.cpu().reshape(B, S, T), want_bins[:, None].expand(B, S, T))
    assert want_bins[2].tolist() == [0, 0] + [-1] * (T - 2)  # a row shorter than the context adds nothing past its end
    counts = hand_counts(LENGTHS, T, Q, EDGES)
    assert table.block(0, 0)[:, 0].tolist() == counts and table.block(0, 1)[:, 0].tolist() == [S * c for c in counts]
    assert float(real.std()) > 0 and float(gen.std()) > 0 and bool((table.block(0, 1)[:, 1 + 128 :].abs().sum(1) > 0).all())  # (features, not zeros)
    firsts = {}
    for side in (0, 1):
        want, bound = _rule_of_step(table, "vision", side, j)
        _assert_within(table.block(0, side), want, bound, f"{name} side {side}")
        _assert_symmetric(table.block(0, side), 128, f"{name} side {side}")
        firsts[side] = (want, bound)
    # the generated features are the reader's on the same decode; the real ones the reader's on the targets
    st = table.states
    feature = torch.cat([st.deter, st.stoch], -1) if case.kind == "mrssm" else torch.cat([st.deter_h, st.stoch_h, st.deter_l, st.stoch_l], -1)
    dv = model.vision_decoder
    pred = dv(feature.reshape(B * S, T, -1), raw=True)
    assert torch.equal(gen, reader.hidden(reader.features(pred, dv.out_act_id)))
    assert torch.equal(real, reader.hidden(reader.features(model.get_targets_from_batch(batch)["recon/vision"], 0)))
    # a second step (other uniforms) adds onto the same table: the sum of the two steps' rules
    again = model.frechet_distance(batch, fd, reader, _noise(model, fd, 12), lengths=lengths, table=table, keep_states=True)
    assert again is table
    for side in (0, 1):
        want, bound = _rule_of_step(table, "vision", side, j)
        _assert_within(table.block(0, side), firsts[side][0] + want, firsts[side][1] + bound + 2.0**-52 * (firsts[side][0] + want).abs(),
                       f"{name} two steps side {side}")
    third = model.frechet_distance(batch, fd, reader, lengths=lengths, table=table)  # (draws its own uniforms; keeps nothing of the batch)
    assert third.features is None and third.bins is None and third.states is None
    assert table.block(0, 0)[:, 0].tolist() == [3 * c for c in counts]
    got = table.compute()["vision"]
    assert all(bool(torch.isfinite(got[k]).all()) and bool((got[k] >= 0).all()) for k in ("fd", "mean", "trace_ratio"))


def test_audio_context_and_encoder_features() -> None:
    _, model, batch = _setup("mrssm_default", (B, T))
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV)
    counts = hand_counts(LENGTHS, T, Q, EDGES)
    heard = model.frechet_distance(batch, FrechetDistance(Q, samples=S, observe="audio", edges=EDGES), _reader(), lengths=lengths)
    assert heard.block(0, 1)[:, 0].tolist() == [S * c for c in counts] and bool(torch.isfinite(heard.buffer).all())
    fd = FrechetDistance(Q, samples=S, features="encoder", edges=EDGES)
    table = model.frechet_distance(batch, fd, None, _noise(model, fd, 13), lengths=lengths, keep_states=True)
    embed = model.audio_representation.obs_embed_size
    assert table.streams == ("audio", "vision") and table.dim == embed and tuple(table.buffer.shape) == (2, 2, 4, cells(embed))
    for s, stream in enumerate(table.streams):
        assert tuple(table.features[stream][0].shape) == (B * T, embed) and tuple(table.features[stream][1].shape) == (B * S * T, embed)
        for side in (0, 1):
            want, bound = _rule_of_step(table, stream, side, 4)
            _assert_within(table.block(s, side), want, bound, f"encoder {stream} side {side}")
    assert set(table.scalars("x")) == {f"x/{m}/{p}/{n}" for m in ("audio", "vision") for p in ("fd", "mean", "cov", "trace_ratio", "n") for n in fd.bin_names}


# 3. validation ---------------------------------------------------------------------------------------------------------------------------------
def test_validation_step_keeps_its_values_and_the_epoch_end_logs_the_distances() -> None:
    """B = 2, T = 4 frames of 16 x 8 audio and 8 x 8 vision (one NLL workgroup per modality, see ``tests/test_likelihood_gpu.py``); the
    frames are not 32 x 32, so the model's own encoders give the features."""
    _, model, batch = _setup("mrssm_nonsquare", (2, 4))
    fd = FrechetDistance(2, samples=3, features="encoder", edges=(1, 2))
    try:
        torch.manual_seed(5)
        plain = model.validation_step(batch)
        assert model.frechet_table is None and model.on_validation_epoch_end() == {}
        model.val_frechet = fd
        torch.manual_seed(5)
        both = model.validation_step(batch)
        assert set(both) == set(plain)
        for key, value in plain.items():
            assert torch.equal(both[key], value), (key, float(both[key]), float(value))  # bitwise: the Frechet step runs after everything else
        model.validation_step(batch)
        assert isinstance(model.frechet_table, FrechetTable) and model.frechet_table.block("audio", 0)[:, 0].tolist() == [8.0, 4.0, 4.0]
        assert model.frechet_table.block("vision", 1)[:, 0].tolist() == [24.0, 12.0, 12.0]
        logged = model.on_validation_epoch_end()
        assert model.frechet_table is None and model.on_validation_epoch_end() == {}
        want = {f"val/frechet/{m}/{p}/{n}" for m in ("audio", "vision") for p in ("fd", "mean", "cov", "trace_ratio", "n") for n in ("obs", "h1", "h2")}
        assert set(logged) == want and all(bool(torch.isfinite(v)) for v in logged.values())
        assert float(logged["val/frechet/audio/n/obs"]) == 8.0  # noqa: PLR2004
    finally:
        model.val_frechet = None
        model.frechet_table = None
