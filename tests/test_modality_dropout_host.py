"""Modality dropout, host side (no GPU): the rule's torch restatement, argument checks, noise shapes, capture-mode refusals."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import ModalityDropout, _lib
from multimodal_mtrssm_amd.dropout import StepMask
from multimodal_mtrssm_amd.graph import CapturedTrainStep
from multimodal_mtrssm_amd.parallel import GlobalRowNoise
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()


@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


# -- ModalityDropout ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    {"p_audio": -0.1, "p_vision": 0.0}, {"p_audio": 1.0, "p_vision": 0.0}, {"p_audio": 0.0, "p_vision": 1.5},
    {"p_audio": 0.0, "p_vision": float("nan")}, {"p_audio": "0.3", "p_vision": 0.0}, {"p_audio": True, "p_vision": 0.0},
    {"p_audio": 0.1, "p_vision": 0.1, "span": 0}, {"p_audio": 0.1, "p_vision": 0.1, "span": -2}, {"p_audio": 0.1, "p_vision": 0.1, "span": 1.5},
])
def test_bad_arguments_raise(kw: dict) -> None:
    with pytest.raises(ValueError, match="p_audio|p_vision|span"):
        ModalityDropout(**kw)


def test_valid_arguments_and_noise_shape() -> None:
    md = ModalityDropout(0.0, 0.999, span=7)
    assert (md.p_audio, md.p_vision, md.span, md.world, md.rank) == (0.0, 0.999, 7, 1, 0)
    assert md.noise_shape(64, 50) == (64, 8, 2)  # ceil(50 / 7)
    assert ModalityDropout(0.3, 0.3).noise_shape(3, 6) == (3, 6, 2)
    assert ModalityDropout(0.3, 0.3, span=4).noise_shape(3, 8) == (3, 2, 2)
    bound = md.for_rank(4, 3)
    assert (bound.world, bound.rank, md.world, md.rank) == (4, 3, 1, 0)
    with pytest.raises(ValueError, match="rank"):
        md.for_rank(2, 2)


def test_reference_rejects_wrong_uniforms() -> None:
    md = ModalityDropout(0.3, 0.3, span=4)
    with pytest.raises(ValueError, match="float32"):
        md.reference(torch.zeros(2, 3, 2), 8)  # S must be 2
    with pytest.raises(ValueError, match="float32"):
        md.reference(torch.zeros(2, 2, 2, dtype=torch.float64), 8)
    with pytest.raises(ValueError, match="world"):
        md.sample(torch.zeros(3, 2, 2), 8, world=2, rank=0)  # 3 rows on 2 ranks (refused before the library is touched)


def test_reference_honours_the_rule_on_handwritten_cases() -> None:
    md = ModalityDropout(0.5, 0.25, span=2)
    # row 0: plain thresholds; row 1: t = 0 fix-up, vision larger; row 2: fix-up, audio larger; row 3: fix-up tie -> audio;
    # row 4: exactly at the threshold is PRESENT (>=)
    u = torch.tensor([
        [[0.6, 0.1], [0.4, 0.3], [0.1, 0.2]],
        [[0.1, 0.2], [0.9, 0.9], [0.0, 0.0]],
        [[0.3, 0.2], [0.0, 0.0], [0.9, 0.0]],
        [[0.2, 0.2], [0.0, 0.9], [0.5, 0.25]],
        [[0.5, 0.25], [0.49999997, 0.24999999], [0.0, 0.0]],
    ])
    mask = md.reference(u, 5)  # S = 3 blocks: t = 0,1 | 2,3 | 4
    assert mask.dtype == torch.bool and tuple(mask.shape) == (5, 5, 2)
    want = {
        0: [(1, 0), (1, 0), (0, 1), (0, 1), (0, 0)],
        1: [(0, 1), (0, 0), (1, 1), (1, 1), (0, 0)],  # the fix-up touches t = 0 ONLY: t = 1 (same block) stays empty
        2: [(1, 0), (0, 0), (0, 0), (0, 0), (1, 0)],
        3: [(1, 0), (0, 0), (0, 1), (0, 1), (1, 1)],
        4: [(1, 1), (1, 1), (0, 0), (0, 0), (0, 0)],
    }
    for b, rows in want.items():
        assert mask[b].tolist() == [[bool(a), bool(v)] for a, v in rows], b
    assert bool(mask[:, 0].any(dim=-1).all())
    # p = 0 keeps everything; the fix-up never fires
    assert bool(ModalityDropout(0.0, 0.0, span=3).reference(torch.rand(4, 2, 2), 6).all())
    # span that does not divide T: the last block is short
    m7 = ModalityDropout(0.5, 0.5, span=7).reference(torch.tensor([[[0.9, 0.9], [0.1, 0.9]]]), 9)
    assert m7[0, :, 0].tolist() == [True] * 7 + [False] * 2 and bool(m7[0, :, 1].all())


def test_step_mask_from_mask_matches_the_scan_codes() -> None:
    mask = torch.tensor([[[True, False], [False, True], [True, True], [False, False]]])
    sm = StepMask.from_mask(mask)
    assert sm.codes.dtype == torch.int32 and sm.codes.tolist() == [[1, 2, 3, 0]]
    assert sm.present_audio.tolist() == [1.0, 0.0, 1.0, 0.0] and sm.present_vision.tolist() == [0.0, 1.0, 1.0, 0.0]
    assert float(sm.count_audio) == 2.0 and float(sm.count_vision) == 2.0 and sm.mask0.tolist() == [[True, False]]


# -- model surface ----------------------------------------------------------------------------------------------------------
def test_noise_shapes_unchanged_without_dropout_and_gain_u_mask_with(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    assert model.modality_dropout is None
    shapes = model.noise_shapes(6, 9)
    if case.kind == "mrssm":
        k = model.transition.distribution_factory.category_size
        assert shapes == {"u_init": (6, k), "u_post": (6, 9, k)}
    else:
        kl, kh = model.l_dist.category_size, model.h_dist.category_size
        assert shapes == {"u_init_h": (6, kh), "u_init_l": (6, kl), "u_post_l": (6, 9, kl), "u_post_h": (6, 9, kh)}
    assert list(shapes) == list(model.noise_shapes(6, 9))
    model.modality_dropout = ModalityDropout(0.2, 0.2, span=4)
    try:
        with_md = model.noise_shapes(6, 9)
    finally:
        model.modality_dropout = None
    assert with_md == {**shapes, "u_mask": (6, 3, 2)}
    assert model.noise_shapes(6, 9) == shapes


def test_global_row_noise_keeps_u_mask_whole_and_other_draws_as_before() -> None:
    shapes = {"u_init": (2, 3), "u_post": (2, 4, 3)}
    plain = GlobalRowNoise(5, 2, 1, "cpu").draw(shapes)
    again = GlobalRowNoise(5, 2, 1, "cpu").draw(dict(reversed(shapes.items())))
    for k in shapes:
        assert torch.equal(plain[k], again[k])
    ranks = [GlobalRowNoise(5, 2, r, "cpu").draw({**shapes, "u_mask": (2, 2, 2)}) for r in (0, 1)]
    assert tuple(ranks[0]["u_mask"].shape) == (4, 2, 2) and torch.equal(ranks[0]["u_mask"], ranks[1]["u_mask"])
    assert tuple(ranks[0]["u_post"].shape) == (2, 4, 3) and not torch.equal(ranks[0]["u_post"], ranks[1]["u_post"])
    assert torch.equal(ranks[1]["u_init"], plain["u_init"])  # "u_init" sorts before "u_mask": same numbers as without it


def test_mask_and_dropout_together_raise(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool)
    md = ModalityDropout(0.3, 0.3)
    with pytest.raises(ValueError, match="not both"):
        model.shared_step(batch, modality_mask=mask, modality_dropout=md)
    with pytest.raises(ValueError, match="not both"):
        model.shared_step((*batch, mask), modality_dropout=md)
    with pytest.raises(ValueError, match="ModalityDropout"):
        model.shared_step(batch, modality_dropout=0.3)
    with pytest.raises(ValueError, match="u_mask"):  # more than one rank: the uniforms of the GLOBAL batch must be given
        model.shared_step(batch, modality_dropout=md.for_rank(2, 0))
    with pytest.raises(ValueError, match="rows"):
        model.shared_step(batch, {"u_mask": torch.rand(case.batch, case.steps, 2)}, modality_dropout=md.for_rank(2, 0))


def test_validation_step_never_samples_a_mask(cpu_model, monkeypatch: pytest.MonkeyPatch) -> None:  # noqa: ANN001
    case, model = cpu_model
    seen = []
    monkeypatch.setattr(model, "shared_step", lambda batch, **kw: seen.append(kw) or {"loss": torch.zeros(())})
    model.modality_dropout = ModalityDropout(0.3, 0.3)
    try:
        model.validation_step(build_batch(case))
        model.training_step(build_batch(case))
    finally:
        model.modality_dropout = None
    assert seen[0].get("modality_dropout") is None
    assert isinstance(seen[1].get("modality_dropout"), ModalityDropout)


# -- captured step ------------------------------------------------------------------------------------------------------------
def test_captured_step_modes_refuse_the_other_kind_of_batch(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool)
    with pytest.raises(ValueError, match="7-tuple"):
        CapturedTrainStep(model, None, None, None, batch, None, masked=True)
    with pytest.raises(ValueError, match="6-tuple"):
        CapturedTrainStep(model, None, None, None, (*batch, mask), None, modality_dropout=ModalityDropout(0.3, 0.3))
    with pytest.raises(ValueError, match="not both"):
        CapturedTrainStep(model, None, None, None, (*batch, mask), None, modality_dropout=ModalityDropout(0.3, 0.3), masked=True)
    with pytest.raises(ValueError, match="ModalityDropout"):
        CapturedTrainStep(model, None, None, None, batch, None, modality_dropout=0.3)
    with pytest.raises(NotImplementedError, match="modality mask"):  # without the keyword: as before
        CapturedTrainStep(model, None, None, None, (*batch, mask), None)
    with pytest.raises(ValueError, match="eager-only"):
        CapturedTrainStep(model, None, None, None, (batch[0], None, *batch[2:], mask), None, masked=True)
    bad = mask.clone()
    bad[1, 0] = False
    with pytest.raises(ValueError, match="t = 0"):
        CapturedTrainStep(model, None, None, None, (*batch, bad), None, masked=True)


# -- C-ABI ----------------------------------------------------------------------------------------------------------------------
def test_sampler_is_declared_exported_and_bound() -> None:
    lib = _lib.load()
    assert re.search(r"\bint mtrssm_modality_dropout\(", HEADER)
    assert "mtrssm_modality_dropout" in _lib.SYMBOLS
    assert lib.mtrssm_modality_dropout is not None
    nm = __import__("subprocess").run(["nm", "-D", "--defined-only", str(_lib.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT mtrssm_modality_dropout\b", nm)


def test_sampler_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    p = C.c_void_p(16)
    call = lib.mtrssm_modality_dropout
    assert call(None, 4, 5, 1, 0.3, 0.3, 0, 4, None, None, None, None, None, None) == -1
    assert b"modality_dropout" in lib.mtrssm_last_error()
    for args in [
        (p, 0, 5, 1, 0.3, 0.3, 0, 4),          # empty global batch
        (p, 4, 0, 1, 0.3, 0.3, 0, 4),          # no steps
        (p, 4, 5, 0, 0.3, 0.3, 0, 4),          # span 0
        (p, 4, 5, 1, 0.3, 0.3, 2, 4),          # the slice runs past the batch
        (p, 4, 5, 1, 0.3, 0.3, -1, 2),         # negative first row
        (p, 4, 5, 1, 1.0, 0.3, 0, 4),          # p = 1 would drop a modality everywhere
        (p, 4, 5, 1, 0.3, -0.5, 0, 4),
        (p, 4, 5, 1, float("nan"), 0.3, 0, 4),
        (p, 1 << 12, 1 << 12, 1, 0.3, 0.3, 0, 4),  # 2^24 frames: the fp32 counts would stop being exact
        (C.c_void_p(20), 4, 5, 1, 0.3, 0.3, 0, 4),  # u is read as float2
    ]:
        assert call(*args, p, p, p, p, p, None) == -1, args
        assert b"modality_dropout" in lib.mtrssm_last_error()
