"""CPU: forecast skill by horizon -- the scoring rule and the horizon fold in torch, the argument refusals of
the Python surface and of the two C-ABI entries (which return before any launch), the table's binning and naming, its all-reduce over
gloo, and the default surface, which stays what it was.  Nothing here launches a kernel."""

from __future__ import annotations

import math
import socket
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

from multimodal_mtrssm_amd import ForecastSkill, SkillTable, StateCarry, _lib
from multimodal_mtrssm_amd.parallel import FlatDataParallel
from oracle.cases import CASES, build_batch, build_model
from tests import skill_worker
from tests.conftest import product_from_case

# the hand-written fold: B = 5, T = 7; a context past T (row 3), a row with no live step (row 4), contexts at or past a row's end
# (rows 2 and 3: only bin 0), a row that ends inside its tail (row 1)
HOST_Q = (1, 3, 7, 9, 2)
HOST_VALID = (7, 5, 7, 7, 0)
HOST_COUNTS = [18.0, 2.0, 2.0, 1.0, 1.0, 1.0, 1.0]
HOST_SUMS = [[425.0, 14.0, 16.0, 3.0, 4.0, 5.0, 6.0], [2225.0, 214.0, 216.0, 103.0, 104.0, 105.0, 106.0]]


def host_planes() -> torch.Tensor:
    """``plane[p][b][t] = 100 p + 10 b + t``: every sum of the case is a whole number, exact in fp32."""
    p, b, t = torch.meshgrid(torch.arange(2), torch.arange(5), torch.arange(7), indexing="ij")
    return (100 * p + 10 * b + t).to(torch.float32)


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


# -- 1. the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 3], ids=["identity", "tanh"])
def test_mean_is_ens_plus_spread_and_best_is_the_lowest_sample(act: int) -> None:
    g = torch.Generator().manual_seed(2)
    pred = torch.randn(3, 5, 4, 24, generator=g, dtype=torch.float64)
    target = torch.randn(3, 4, 24, generator=g, dtype=torch.float64)
    got = ForecastSkill.reference(pred, target, None, act)
    assert got.mean.dtype == torch.float64 and tuple(got.mean.shape) == (3, 4) and tuple(got.se_samples.shape) == (3, 5, 4)
    torch.testing.assert_close(got.mean, got.ens + got.spread, rtol=1e-12, atol=1e-12)
    y = torch.tanh(pred) if act else pred
    se = (0.5 * (target[:, None] - y) ** 2).sum(-1)
    torch.testing.assert_close(got.se_samples, se, rtol=1e-12, atol=0)
    torch.testing.assert_close(got.mean, se.mean(1), rtol=1e-12, atol=0)
    assert torch.equal(got.best, got.se_samples.min(1).values)
    torch.testing.assert_close(got.ens, (0.5 * (target - y.mean(1)) ** 2).sum(-1), rtol=1e-12, atol=0)
    assert bool((got.spread > 0).all()) and bool((got.best <= got.mean).all()) and bool((got.ens <= got.mean).all())


def test_one_sample_has_no_spread_and_dead_frames_score_zero() -> None:
    g = torch.Generator().manual_seed(3)
    pred = torch.randn(4, 1, 5, 8, generator=g, dtype=torch.float64)
    target = torch.randn(4, 5, 8, generator=g, dtype=torch.float64)
    one = ForecastSkill.reference(pred, target, None, 3)
    assert not bool(one.spread.any()) and torch.equal(one.mean, one.ens) and torch.equal(one.mean, one.best)
    valid = torch.tensor([5, 2, 0, 9], dtype=torch.int32)
    pred3 = torch.randn(4, 3, 5, 8, generator=g, dtype=torch.float64)
    got, full = ForecastSkill.reference(pred3, target, valid, 0), ForecastSkill.reference(pred3, target, None, 0)
    live = torch.arange(5) < valid[:, None]
    for plane, whole in zip(got[:4], full[:4], strict=True):
        assert not bool(plane[~live].any()) and torch.equal(plane[live], whole[live])
    assert not bool(got.se_samples[~live[:, None].expand(4, 3, 5)].any())
    assert ForecastSkill.score(pred3, target, valid, 0).se_samples is None  # (CPU tensors: the rule; se_samples only when asked for)
    assert torch.equal(ForecastSkill.score(pred3, target, valid, 0, se_samples=True).se_samples, got.se_samples)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_horizon_fold_against_the_hand_written_table(dtype: torch.dtype) -> None:
    context, valid = torch.tensor(HOST_Q, dtype=torch.int32), torch.tensor(HOST_VALID, dtype=torch.int32)
    h, live = ForecastSkill.horizon(context, valid, 7)
    assert h[0].tolist() == [0, 1, 2, 3, 4, 5, 6] and h[1].tolist() == [0, 0, 0, 1, 2, 3, 4] and not bool(h[2:4].any())
    assert live.sum(1).tolist() == [7, 5, 7, 7, 0]
    sums, counts = torch.zeros(2, 7, dtype=dtype), torch.zeros(7, dtype=dtype)
    ForecastSkill.reference_table(host_planes(), context, valid, sums, counts)
    assert counts.tolist() == HOST_COUNTS and sums.tolist() == HOST_SUMS
    assert float(counts.sum()) == float(sum(HOST_VALID))  # counts are whole numbers: every live frame once
    ForecastSkill.table_add(host_planes(), context, valid, sums, counts)  # (CPU tensors: the same rule) batches add up in one buffer
    assert counts.tolist() == [2 * c for c in HOST_COUNTS] and sums.tolist() == [[2 * v for v in row] for row in HOST_SUMS]
    with pytest.raises(ValueError, match="2\\^24"):
        ForecastSkill.reference_table(torch.zeros(1, 1 << 12, 1 << 12, device="meta"), torch.zeros(1 << 12, dtype=torch.int32, device="meta"), None,
                                      torch.zeros(1, 1 << 12, device="meta"), torch.zeros(1 << 12, device="meta"))


# -- 2. refusals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [0, 17, -1, 2.0, True, None])
def test_bad_sample_counts_are_refused(samples) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="samples"):
        ForecastSkill(3, samples)


@pytest.mark.parametrize("observe", ["all", "Audio", "", None, 3])
def test_bad_observe_is_refused(observe) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="observe"):
        ForecastSkill(3, 2, observe)


@pytest.mark.parametrize("context", [0, -2, 1.5, True, (1, 3), None, 1 << 31])
def test_bad_context_is_refused(context) -> None:  # noqa: ANN001
    with pytest.raises(ValueError, match="context"):
        ForecastSkill(context)


def test_skill_surface() -> None:
    sk = ForecastSkill(3, samples=4, observe="vision")
    assert (sk.context, sk.samples, sk.observe, sk.bits, sk.max_frames, sk.group) == (3, 4, "vision", 2, 4096, None)
    assert ForecastSkill(1).samples == 1 and ForecastSkill(1).bits == 3 and ForecastSkill(1, observe="audio").bits == 1
    assert repr(sk) == "ForecastSkill(3, samples=4, observe='vision')"
    u_post, u_tail = torch.rand(2, 6, 5), torch.rand(2, 4, 6, 5)
    u = sk.compose_noise(u_post, u_tail)
    assert tuple(u.shape) == (8, 6, 5)
    for b in range(2):
        for s in range(4):
            assert torch.equal(u[b * 4 + s, :3], u_post[b, :3]) and torch.equal(u[b * 4 + s, 3:], u_tail[b, s, 3:])
    assert torch.equal(ForecastSkill(9, 4).compose_noise(u_post, u_tail), u_post.repeat_interleave(4, 0))  # a context past T: no tail
    with pytest.raises(ValueError, match="tail"):
        sk.compose_noise(u_post, u_tail[:, :3])


def test_skill_noise_shapes_put_the_batch_first(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    shapes = ForecastSkill(2, samples=3).noise_shapes(model, 4, 6)
    if case.kind == "mrssm":
        k = case.dims.cats
        assert shapes == {"u_init": (4, k), "u_post": (4, 6, k), "u_tail": (4, 3, 6, k)}
    else:
        kl, kh = case.dims.ls_cats, case.dims.hs_cats
        assert shapes == {"u_init_h": (4, kh), "u_init_l": (4, kl), "u_post_l": (4, 6, kl), "u_post_h": (4, 6, kh),
                          "u_tail_l": (4, 3, 6, kl), "u_tail_h": (4, 3, 6, kh)}
    assert all(s[0] == 4 for s in shapes.values())  # (GlobalRowNoise slices the first extent)


def test_skill_step_refuses_masked_batches_and_a_set_carry(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    b, t = batch[0].shape[:2]
    sk = ForecastSkill(2, samples=2)
    with pytest.raises(ValueError, match="masked"):
        model.forecast_skill((*batch, torch.ones(b, t, 2, dtype=torch.bool)), sk)
    with pytest.raises(ValueError, match="ForecastSkill"):
        model.forecast_skill(batch, 2)
    model.state_carry = StateCarry.for_model(model, b)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.forecast_skill(batch, sk)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="SkillTable"):
        model.forecast_skill(batch, sk, table=SkillTable(t + 1))


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    ok, odd = 0x10000, 0x10004  # never dereferenced: every call below returns before a launch
    good = {"pred": ok, "target": ok, "valid": None, "B": 2, "S": 4, "T": 3, "E": 8, "act": 3, "mean": ok, "ens": ok, "best": ok, "spread": ok,
            "se": None}

    def score(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_ensemble_score(a["pred"], a["target"], a["valid"], a["B"], a["S"], a["T"], a["E"], a["act"], a["mean"], a["ens"], a["best"],
                                         a["spread"], a["se"], None)

    for name in ("pred", "target", "mean", "ens", "best", "spread"):
        assert score(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
    for name in ("B", "T", "E"):
        assert score(**{name: 0}) == -1 and score(**{name: -3}) == -1, name
    for s in (0, 17, -1):
        assert score(S=s) == -1 and b"samples" in lib.mtrssm_last_error(), s
    for e in (1, 6, 1037):
        assert score(E=e) == -1 and b"multiple of 4" in lib.mtrssm_last_error(), e
    for act in (1, 2, 4, -1):
        assert score(act=act) == -1 and b"Identity or Tanh" in lib.mtrssm_last_error(), act
    assert score(pred=odd) == -1 and b"16-byte" in lib.mtrssm_last_error()
    assert score(target=ok + 8) == -1 and b"16-byte" in lib.mtrssm_last_error()
    assert score(mean=ok + 2) == -1 and score(se=ok + 1) == -1 and score(valid=ok + 3) == -1 and b"4-byte" in lib.mtrssm_last_error()
    assert score(B=1 << 20, T=1 << 11) == -1 and b"2^31" in lib.mtrssm_last_error()  # B * T = 2^31 frames
    assert score(B=1 << 40, T=1 << 40) == -1  # (the product overflows 64 bits)
    assert score(B=1 << 15, S=16, T=1 << 15, E=1 << 26) == -1 and b"2^60" in lib.mtrssm_last_error()

    tgood = {"planes": ok, "P": 8, "context": ok, "valid": None, "B": 5, "T": 7, "sums": ok, "counts": ok}

    def table(**kw) -> int:  # noqa: ANN003
        a = {**tgood, **kw}
        return lib.mtrssm_horizon_table(a["planes"], a["P"], a["context"], a["valid"], a["B"], a["T"], a["sums"], a["counts"], None)

    for name in ("planes", "context", "sums", "counts"):
        assert table(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
        assert table(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    assert table(valid=ok + 1) == -1
    for name, bad in (("P", 0), ("P", 65), ("B", 0), ("T", 0), ("B", -1), ("T", -1)):
        assert table(**{name: bad}) == -1 and b"horizon_table" in lib.mtrssm_last_error(), (name, bad)
    assert table(B=1 << 12, T=1 << 12) == -1 and b"2^24" in lib.mtrssm_last_error()
    assert table(B=1 << 40, T=1 << 40) == -1


# -- 3. binned and scalars --------------------------------------------------------------------------------------------------------
def test_binned_and_scalars_arithmetic_and_names() -> None:
    t = 12
    table = SkillTable(t)
    assert tuple(table.buffer.shape) == (9, t) and table.buffer.dtype == torch.float32 and table.steps == t
    counts = torch.tensor([20.0, 4, 4, 3, 3, 0, 0, 0, 2, 2, 1, 1])  # horizons 5 .. 7 are empty: the bin [4, 8) keeps horizon 4
    table.counts.copy_(counts)
    for r in range(8):
        table.sums[r] = counts * (r + 1) * torch.arange(1, t + 1)  # the mean score of bin h in row r is (r + 1) (h + 1)
    curves = table.curves()
    assert list(curves) == ["audio", "vision"] and list(curves["audio"]) == ["mean", "ens", "best", "spread"]
    assert torch.equal(curves["vision"]["ens"][:5], 6.0 * torch.arange(1, 6)) and bool(curves["vision"]["ens"][5:8].isnan().all())
    assert not bool(curves["vision"]["ens"][8:].isnan().any())  # an empty bin is NaN and poisons nothing else
    binned = table.binned((1, 2, 4, 8))
    row = binned["audio"]["best"]  # r = 2: per-frame mean 3 (h + 1)
    want = [3.0 * 1, 3.0 * 2, 3.0 * (4 * 3 + 3 * 4) / 7, 3.0 * 5, 3.0 * (2 * 9 + 2 * 10 + 11 + 12) / 6]
    assert tuple(row.shape) == (5,)
    torch.testing.assert_close(row, torch.tensor(want), rtol=1e-6, atol=0)
    empty = table.binned((1, 6, 8))  # [6, 8) has no frame
    assert math.isnan(float(empty["audio"]["mean"][2])) and not bool(empty["audio"]["mean"][[0, 1, 3]].isnan().any())
    scalars = table.scalars("val/skill", (1, 2, 4, 8))
    assert set(scalars) == {f"val/skill/{m}/{k}/{n}" for m in ("audio", "vision") for k in ("mean", "ens", "best", "spread")
                            for n in ("obs", "h1", "h2", "h4", "h8")}
    assert float(scalars["val/skill/audio/best/h4"]) == float(row[3]) and float(scalars["val/skill/vision/spread/obs"]) == 8.0  # noqa: PLR2004
    short = SkillTable(3)  # edges past T: bins without frames
    short.counts.fill_(1.0)
    got = short.scalars("s", (1, 2, 4, 8))
    assert math.isnan(float(got["s/audio/mean/h4"])) and math.isnan(float(got["s/audio/mean/h8"])) and float(got["s/audio/mean/h2"]) == 0.0
    with pytest.raises(ValueError, match="edges"):
        table.binned((2, 2))
    with pytest.raises(ValueError, match="edges"):
        table.binned((0, 2))
    other = SkillTable(t)
    other.buffer.fill_(1.0)
    assert table.add(other) is table and float(table.counts[0]) == 21.0  # noqa: PLR2004
    with pytest.raises(ValueError, match="do not add"):
        table.add(SkillTable(t + 1))
    assert table.all_reduce() is table and float(table.counts[0]) == 21.0  # noqa: PLR2004  (no process group: nothing happens)


# -- 4. all_reduce over gloo ------------------------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_all_reduce_equals_the_single_process_table(tmp_path: Path) -> None:
    mp.spawn(skill_worker.worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    assert torch.equal(r0, r1)
    planes, context, valid = skill_worker.planes_case()
    one = SkillTable(skill_worker.T)
    ForecastSkill.table_add(planes, context, valid, one.sums, one.counts)
    assert torch.equal(r0[8], one.counts) and float(one.counts.sum()) == float(valid.clamp(0, skill_worker.T).sum())
    assert int((one.counts > 1).sum()) >= 3  # noqa: PLR2004  (bins with several addends, split over the ranks)
    # every addend is non-negative: any summation order stays within (n - 1) 2^-24 relative of the exact sum
    for h in range(skill_worker.T):
        n = float(one.counts[h])
        torch.testing.assert_close(r0[:8, h], one.sums[:, h], rtol=2.0 * n * 2.0 ** -24, atol=0.0)


# -- 5. the default surface ---------------------------------------------------------------------------------------------------------
def test_without_val_skill_the_surface_is_what_it_was(cpu_model, monkeypatch: pytest.MonkeyPatch) -> None:  # noqa: ANN001
    case, model = cpu_model
    assert model.val_skill is None and model.skill_table is None
    if case.kind == "mrssm":
        k = case.dims.cats
        assert model.noise_shapes(4, 6) == {"u_init": (4, k), "u_post": (4, 6, k)}
    else:
        kl, kh = case.dims.ls_cats, case.dims.hs_cats
        assert model.noise_shapes(4, 6) == {"u_init_h": (4, kh), "u_init_l": (4, kl), "u_post_l": (4, 6, kl), "u_post_h": (4, 6, kh)}
    # validation_step over a stubbed shared_step (the kernels need a GPU): the keys of before, no skill step, nothing logged at the end
    terms = {"recon": torch.tensor(3.0), "recon/audio": torch.tensor(1.0), "recon/vision": torch.tensor(2.0), "kl": torch.tensor(0.5),
             "loss": torch.tensor(3.5)}
    calls = []
    monkeypatch.setattr(model, "shared_step", lambda *a, **k: dict(terms))
    monkeypatch.setattr(model, "forecast_skill", lambda *a, **k: calls.append(a) or SkillTable(6))
    batch = build_batch(case)
    assert set(model.validation_step(batch)) == {f"val/{k}" for k in terms} and not calls and model.skill_table is None
    assert model.on_validation_epoch_end() == {}
    # with val_skill set the step runs after the existing work and the epoch end logs and clears
    model.val_skill = ForecastSkill(2, samples=2)
    try:
        assert set(model.validation_step(batch)) == {f"val/{k}" for k in terms} and len(calls) == 1
        assert isinstance(model.skill_table, SkillTable)
        model.skill_table.buffer.fill_(2.0)
        logged = model.on_validation_epoch_end()
        assert len(logged) == 2 * 4 * 5 and all(k.startswith("val/skill/") for k in logged) and model.skill_table is None  # noqa: PLR2004
        assert float(logged["val/skill/audio/mean/obs"]) == 1.0
    finally:
        model.val_skill = None


def test_flat_data_parallel_binds_the_group() -> None:
    class _Flat:  # (FlatDataParallel reads nothing of it here)
        pass

    dp = FlatDataParallel(_Flat())
    sk = ForecastSkill(3, samples=2, observe="audio")
    bound = dp.skill(sk)
    assert bound is not sk and (bound.context, bound.samples, bound.observe) == (3, 2, "audio") and bound.group is dp.group
