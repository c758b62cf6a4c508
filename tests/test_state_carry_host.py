"""CPU: the host rules of ``carry.StateCarry``, the torch restatements of ``mtrssm_state_select`` /
``mtrssm_state_save`` and of the select's backward, how ``shared_step`` / ``training_step`` / ``CapturedTrainStep`` take a carry, and
the argument checks of the two C-ABI entries.  Nothing is launched here."""

from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import StateCarry, _lib, carry
from multimodal_mtrssm_amd.dataset import EpisodeBatch
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()


def _mrssm_carry(batch: int = 3) -> StateCarry:
    return StateCarry({"deter": 8, "stoch": 6}, batch, "cpu", {"stoch": (3, 2)})


def test_empty_set_needs_a_full_reset_and_sets_are_independent() -> None:
    sc = _mrssm_carry()
    assert sc.filled == {"train": False, "val": False}
    partial, full = torch.tensor([True, False, True]), torch.ones(3, dtype=torch.bool)
    with pytest.raises(ValueError, match="empty"):
        sc.check("train", 3, partial)
    with pytest.raises(ValueError, match="empty"):  # a reset nobody saw on the host cannot vouch for an empty carry
        sc.check("train", 3, None)
    sc.check("train", 3, full)
    sc.filled["train"] = True  # (what save() does after its launch)
    sc.check("train", 3, partial)
    sc.check("train", 3, None)
    with pytest.raises(ValueError, match="empty"):  # the validation set knows nothing of the training set
        sc.check("val", 3, partial)
    sc.check("val", 3, full)
    with pytest.raises(ValueError, match="empty"):
        sc.last("val")
    assert sc.last("train").deter.shape == (3, 8)
    sc.clear("train")
    with pytest.raises(ValueError, match="empty"):
        sc.check("train", 3, partial)
    assert sc.buffers["train"]["deter"] is not sc.buffers["val"]["deter"]


def test_wrong_batch_size_prefix_and_widths_raise() -> None:
    sc = _mrssm_carry()
    full4 = torch.ones(4, dtype=torch.bool)
    with pytest.raises(ValueError, match="4 rows"):
        sc.check("train", 4, full4)
    with pytest.raises(ValueError, match="shape"):
        sc.check("train", 3, full4)
    with pytest.raises(ValueError, match="prefix"):
        sc.check("test", 3, torch.ones(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="widths"):
        StateCarry({"deter": 8}, 3, "cpu")
    with pytest.raises(ValueError, match="batch"):
        StateCarry({"deter": 8, "stoch": 6}, 0, "cpu")
    mt = StateCarry(dict.fromkeys(carry.MMTRSSM_FIELDS, 4), 2, "cpu")
    assert mt.fields == carry.MMTRSSM_FIELDS and set(mt.buffers["val"]) == set(carry.MMTRSSM_FIELDS)


def test_restatements_of_select_save_and_the_select_backward() -> None:
    g = torch.Generator().manual_seed(1)
    reset = torch.tensor([True, False, False, True])
    fresh = torch.randn(4, 5, generator=g, requires_grad=True)
    held = torch.randn(4, 5, generator=g, requires_grad=True)
    out = carry.select_reference(reset, fresh, held)
    assert torch.equal(out[0], fresh[0]) and torch.equal(out[1], held[1]) and torch.equal(out[3], fresh[3])
    gout = torch.randn(4, 5, generator=g)
    out.backward(gout)
    want = carry.select_backward_reference(reset, gout)
    assert torch.equal(fresh.grad, want)  # autograd of the restatement IS the stated backward
    assert torch.equal(want[1], torch.zeros(5)) and torch.equal(want[0], gout[0])
    last = torch.randn(4, 7, 5, generator=g, requires_grad=True)
    saved = carry.save_reference(last)
    assert torch.equal(saved, last[:, 6].detach()) and not saved.requires_grad


def test_last_returns_the_carried_state_with_point_mass_distributions() -> None:
    sc = _mrssm_carry(2)
    sc.buffers["train"]["deter"].copy_(torch.arange(16.0).reshape(2, 8))
    sc.buffers["train"]["stoch"].copy_(torch.tensor([[1, 0, 0, 1, 1, 0], [0, 1, 1, 0, 0, 1]], dtype=torch.float32))
    sc.filled["train"] = True
    st = sc.last("train")
    assert torch.equal(st.deter, sc.buffers["train"]["deter"]) and st.deter is not sc.buffers["train"]["deter"]
    assert st.distribution.probs.shape == (2, 3, 2) and torch.equal(st.distribution.probs.flatten(1), st.stoch)
    assert st.feature.shape == (2, 14)
    snap = sc.snapshot()
    sc.buffers["train"]["deter"].zero_()
    sc.clear()
    sc.restore(snap)
    assert sc.filled["train"] and float(sc.buffers["train"]["deter"][1, 7]) == 15.0


@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_default"])
def test_model_surface_of_the_carry(name: str, monkeypatch: pytest.MonkeyPatch) -> None:
    import multimodal_mtrssm_amd as mt

    case = CASES[name]
    model = product_from_case(case, build_model(case), "cpu")
    batch = build_batch(case)
    assert model.state_carry is None
    shapes = model.noise_shapes(case.batch, case.steps)
    sc = StateCarry.for_model(model, case.batch)
    d = case.dims
    if case.kind == "mrssm":
        assert sc.widths == {"deter": d.deter, "stoch": d.classes * d.cats}
    else:
        assert sc.widths == {"deter_l": d.ld, "deter_h": d.hd, "stoch_l": d.ls, "stoch_h": d.hs, "hidden_l": d.ld, "hidden_h": d.hd}
    with pytest.raises(ValueError, match="reset"):  # a plain tuple says nothing about where its rows start
        model.shared_step(batch, state_carry=sc)
    with pytest.raises(ValueError, match="bool"):
        model.shared_step(batch, state_carry=sc, reset=torch.ones(case.batch))
    with pytest.raises(ValueError, match="StateCarry"):
        model.shared_step(batch, state_carry=object(), reset=torch.ones(case.batch, dtype=torch.bool))
    partial = torch.ones(case.batch, dtype=torch.bool)
    partial[0] = False
    with pytest.raises(ValueError, match="empty"):
        model.shared_step(batch, state_carry=sc, reset=partial)
    eb = EpisodeBatch(batch, torch.zeros(case.batch, dtype=torch.int32), partial, torch.zeros(case.batch, dtype=torch.int32), partial)
    with pytest.raises(ValueError, match="empty"):  # reset defaults to the batch's
        model.shared_step(eb, state_carry=sc)
    with pytest.raises(ValueError, match="rows"):
        model.shared_step(batch, state_carry=StateCarry.for_model(model, case.batch + 1), reset=torch.ones(case.batch, dtype=torch.bool))
    # training_step uses the "train" set, validation_step the "val" set; unset, shared_step is called as before
    seen: list[dict] = []
    monkeypatch.setattr(type(model), "shared_step", lambda self, b, **kw: seen.append(kw) or {"loss": torch.zeros(())})
    model.training_step(batch)
    model.state_carry = sc
    model.training_step(batch)
    model.validation_step(batch)
    assert "state_carry" not in seen[0]
    assert seen[1]["state_carry"] is sc and seen[1]["carry_prefix"] == "train"
    assert seen[2]["state_carry"] is sc and seen[2]["carry_prefix"] == "val"
    assert model.noise_shapes(case.batch, case.steps) == shapes  # the carry draws nothing
    assert mt.StateCarry is StateCarry and mt.EpisodeBatch is EpisodeBatch


def test_captured_step_checks_its_carry_argument() -> None:
    from multimodal_mtrssm_amd.graph import CapturedTrainStep

    case = CASES["mrssm_nonsquare"]
    model = product_from_case(case, build_model(case), "cpu")
    batch = build_batch(case)
    with pytest.raises(ValueError, match="StateCarry"):
        CapturedTrainStep(model, None, None, None, batch, None, state_carry=object())
    with pytest.raises(ValueError, match="rows"):
        CapturedTrainStep(model, None, None, None, batch, None, state_carry=StateCarry.for_model(model, case.batch + 2))


def test_state_entries_are_declared_and_reject_bad_tables_without_a_launch() -> None:
    lib = _lib.load()
    for name in ("mtrssm_state_select", "mtrssm_state_save", "mtrssm_episode_gather_window"):
        assert re.search(r"\bint " + name + r"\(", HEADER) and name in _lib.SYMBOLS and hasattr(lib, name)
    assert int(re.search(r"#define MTRSSM_STATE_MAX (\d+)", HEADER).group(1)) == _lib.STATE_MAX
    body = re.search(r"typedef struct MtrssmStateTable \{(.*?)\} MtrssmStateTable;", HEADER, flags=re.DOTALL).group(1)
    assert re.findall(r"(\w+)\[MTRSSM_STATE_MAX\]", body) == [n for n, _ in _lib.StateTable._fields_[1:]]  # noqa: SLF001
    one = C.c_void_p(16)
    table = _lib.StateTable()
    assert lib.mtrssm_state_select(None, one, 4, None) == -1
    assert lib.mtrssm_state_select(C.byref(table), one, 4, None) == -1 and b"count" in lib.mtrssm_last_error()
    table.count = 7
    assert lib.mtrssm_state_save(C.byref(table), 4, 5, None) == -1 and b"count" in lib.mtrssm_last_error()
    table.count = 1
    assert lib.mtrssm_state_select(C.byref(table), one, 4, None) == -1 and b"entry 0" in lib.mtrssm_last_error()
    table.src[0], table.dst[0], table.width[0], table.src_stride[0] = 16, 32, 8, 4
    assert lib.mtrssm_state_select(C.byref(table), one, 4, None) == -1 and b"stride" in lib.mtrssm_last_error()
    table.src_stride[0] = 8
    assert lib.mtrssm_state_select(C.byref(table), None, 4, None) == -1 and b"reset" in lib.mtrssm_last_error()
    assert lib.mtrssm_state_select(C.byref(table), one, 0, None) == -1
    assert lib.mtrssm_state_save(C.byref(table), 4, 0, None) == -1 and b"steps" in lib.mtrssm_last_error()
    table.dst[0] = 34
    assert lib.mtrssm_state_save(C.byref(table), 4, 5, None) == -1 and b"aligned" in lib.mtrssm_last_error()
