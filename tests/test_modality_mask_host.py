"""Missing-modality API, host side (no GPU): C-ABI declarations, argument checks, mask validation."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import _lib
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()
MASKED_NLL = ("mtrssm_gaussian_nll_masked_fwd", "mtrssm_gaussian_nll_masked_bwd")


def test_masked_nll_is_declared_exported_and_bound() -> None:
    lib = _lib.load()
    for name in MASKED_NLL:
        assert re.search(r"\bint " + name + r"\(", HEADER), name
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("cls", [_lib.MrssmFwdIO, _lib.MrssmBwdIO, _lib.MmtrssmFwdIO, _lib.MmtrssmBwdIO])
def test_io_structs_carry_the_modality_codes_last(cls: type) -> None:
    body = re.search(r"typedef struct " + cls.__name__ + r" \{(.*?)\} " + cls.__name__ + ";", HEADER, flags=re.DOTALL).group(1)
    assert re.search(r"const int32_t\* modality;", body)
    assert cls._fields_[-1][0] == "modality"


def test_masked_nll_rejects_bad_arguments_without_a_launch() -> None:
    lib = _lib.load()
    assert lib.mtrssm_gaussian_nll_masked_fwd(None, None, None, None, 1, 1, 0, None, None) == -1
    assert b"gaussian_nll_masked_fwd" in lib.mtrssm_last_error()
    assert lib.mtrssm_gaussian_nll_masked_bwd(None, None, None, None, None, 1, 1, 0, None, None) == -1
    assert b"gaussian_nll_masked_bwd" in lib.mtrssm_last_error()
    # non-null but non-positive sizes: refused before the pointers are looked at
    p = C.c_void_p(16)
    assert lib.mtrssm_gaussian_nll_masked_fwd(p, p, p, p, 0, 4, 0, p, None) == -1
    assert lib.mtrssm_gaussian_nll_masked_bwd(p, p, p, p, p, 4, 0, 0, p, None) == -1


@pytest.fixture(scope="module")
def cpu_model():  # noqa: ANN201
    case = CASES["mrssm_nonsquare"]
    return case, product_from_case(case, build_model(case), "cpu")


def test_get_modality_mask_from_batch(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    assert model.get_modality_mask_from_batch(batch) is None
    mask = torch.ones(case.batch, case.steps, 2, dtype=torch.bool)
    assert model.get_modality_mask_from_batch((*batch, mask)) is mask


@pytest.mark.parametrize(("shape", "dtype", "fill", "what"), [
    ((None, None, 3), torch.bool, True, "shape"),
    ((None, None), torch.bool, True, "shape"),
    ((None, None, 2), torch.uint8, 1, "bool"),
    ((None, None, 2), torch.float32, 1.0, "bool"),
    ((None, None, 2), torch.bool, False, "t = 0"),
])
def test_bad_masks_raise_value_error_before_any_launch(cpu_model, shape, dtype, fill, what) -> None:  # noqa: ANN001, PLR0913
    case, model = cpu_model
    batch = build_batch(case)
    dims = [case.batch if i == 0 else (case.steps if i == 1 else s) for i, s in enumerate(shape)]
    mask = torch.full(dims, fill, dtype=dtype)
    if what == "t = 0":  # only the first step is empty: later ones are allowed to be
        mask[:, 1:] = True
        mask[0, 0] = False
    with pytest.raises(ValueError, match=re.escape(what)):
        model.shared_step((*batch, mask))
    with pytest.raises(ValueError, match=re.escape(what)):
        model.shared_step(batch, modality_mask=mask)


def test_initial_state_mask_is_validated(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    obs = (batch[1][:, 0], batch[2][:, 0])
    with pytest.raises(ValueError, match="t = 0"):
        model.initial_state(obs, modality_mask=torch.zeros(case.batch, 2, dtype=torch.bool))
    with pytest.raises(ValueError, match="shape"):
        model.initial_state(obs, modality_mask=torch.ones(case.batch, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="None"):
        model.initial_state((obs[0], None), modality_mask=torch.ones(case.batch, 2, dtype=torch.bool))


def test_captured_step_refuses_a_masked_batch(cpu_model) -> None:  # noqa: ANN001
    from multimodal_mtrssm_amd.graph import CapturedTrainStep  # noqa: PLC0415

    case, model = cpu_model
    batch = (*build_batch(case), torch.ones(case.batch, case.steps, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="modality mask"):
        CapturedTrainStep(model, None, None, None, batch, None)
