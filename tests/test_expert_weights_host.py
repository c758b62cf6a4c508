"""Weighted MoPoE, host side (no GPU): the rule in torch, the gate module, the reported weights, state-dict keys, argument
checks."""

from __future__ import annotations

import io
import re
from pathlib import Path

import pytest
import torch

from multimodal_mtrssm_amd import _lib, scan
from multimodal_mtrssm_amd.experts import LOG_THIRD, ExpertWeights
from oracle.cases import CASES, build_model
from oracle.ref_model import mopoe_mix
from tests.conftest import product_from_case

HEADER = (Path(__file__).resolve().parents[1] / "include" / "mtrssm.h").read_text()
B, T, S = 3, 5, 12


def _logits(dtype: torch.dtype = torch.float32, seed: int = 0) -> tuple[torch.Tensor, ...]:
    g = torch.Generator().manual_seed(seed)
    return tuple(3.0 * torch.randn(B, T, S, generator=g).to(dtype) for _ in range(3))


def _all_codes() -> torch.Tensor:
    codes = torch.arange(B * T).reshape(B, T) % 4
    codes[:, 0] = 3
    return codes


def test_constant_third_is_the_stock_mixture_bit_for_bit() -> None:
    la, lv, lp = _logits()
    lw = torch.full((B, T, 3), LOG_THIRD, dtype=torch.float32)
    got = ExpertWeights.reference_mix(la, lv, lp, lw, torch.full((B, T), 3))
    assert torch.equal(got, mopoe_mix(la, lv))
    # the fp32 value is the one a zero-initialised gate produces
    assert torch.equal(lw[0, 0], torch.log_softmax(torch.zeros(3), dim=-1))


def test_one_or_no_modality_ignores_the_weights() -> None:
    la, lv, lp = _logits(seed=1)
    lw = torch.log_softmax(2.0 * torch.randn(B, T, 3, generator=torch.Generator().manual_seed(2)), dim=-1)
    for code, want in ((1, torch.log_softmax(la, dim=-1)), (2, torch.log_softmax(lv, dim=-1)), (0, lp)):
        got = ExpertWeights.reference_mix(la, lv, lp, lw, torch.full((B, T), code))
        assert torch.equal(got, want), code


def test_reference_mix_gradients() -> None:
    la, lv, lp = (x.requires_grad_() for x in _logits(torch.float64, seed=3))
    lw = torch.log_softmax(2.0 * torch.randn(B, T, 3, generator=torch.Generator().manual_seed(4), dtype=torch.float64), dim=-1).requires_grad_()
    codes = _all_codes()
    assert torch.autograd.gradcheck(lambda a, v, w: ExpertWeights.reference_mix(a, v, lp.detach(), w, codes), (la, lv, lw))
    out = ExpertWeights.reference_mix(la, lv, lp, lw, codes)
    (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)).sum().backward()
    assert torch.equal(lw.grad[codes != 3], torch.zeros_like(lw.grad[codes != 3]))  # noqa: PLR2004
    assert bool((lw.grad[codes == 3].abs() > 0).all())  # noqa: PLR2004
    # the stated gradient: g_i = sum_s dmx[s] r_i[s] and d_a = dmx (r_a + r_f) in front of the flat log-softmax
    a, v = torch.log_softmax(la.detach(), -1), torch.log_softmax(lv.detach(), -1)
    r_a = torch.exp(lw.detach()[..., 0:1] + a - out.detach())
    r_v = torch.exp(lw.detach()[..., 1:2] + v - out.detach())
    r_f = torch.exp(lw.detach()[..., 2:3] + a + v - out.detach())
    both = (codes == 3).unsqueeze(-1)  # noqa: PLR2004
    torch.testing.assert_close(torch.where(both, r_a + r_v + r_f, torch.ones_like(r_a)), torch.ones_like(r_a))


def test_table_follows_the_rule() -> None:
    codes = _all_codes()
    lw = 2.0 * torch.randn(B, T, 3, generator=torch.Generator().manual_seed(6))
    table = ExpertWeights.table(lw, codes)
    assert table.shape == (B, T, 3) and table.dtype == torch.float32 and not table.requires_grad
    assert torch.equal(table[codes == 3], torch.softmax(lw, dim=-1)[codes == 3])  # noqa: PLR2004
    assert torch.equal(table[codes == 1], torch.tensor([1.0, 0.0, 0.0]).expand(int((codes == 1).sum()), 3))
    assert torch.equal(table[codes == 2], torch.tensor([0.0, 1.0, 0.0]).expand(int((codes == 2).sum()), 3))  # noqa: PLR2004
    assert torch.equal(table[codes == 0], torch.zeros(int((codes == 0).sum()), 3))
    third = ExpertWeights.table(None, codes)
    assert torch.equal(third[codes == 3], torch.full((int((codes == 3).sum()), 3), 1.0 / 3.0))  # noqa: PLR2004
    assert torch.equal(third[codes != 3], table[codes != 3])  # noqa: PLR2004


@pytest.mark.parametrize("mode", ["static", "gated"])
def test_zero_initialised_gate_returns_log_third(mode: str) -> None:
    gate = ExpertWeights(mode, 7 if mode == "gated" else None)
    assert all(float(p.detach().abs().max()) == 0.0 for p in gate.parameters())
    g = torch.Generator().manual_seed(7)
    lw = gate(torch.randn(B, T, 7, generator=g), torch.randn(B, T, 7, generator=g))
    assert lw.shape == (B, T, 3) and lw.dtype == torch.float32 and lw.is_contiguous()
    assert torch.equal(lw, torch.full((B, T, 3), LOG_THIRD, dtype=torch.float32))


def test_gate_modes_and_parameters() -> None:
    assert [n for n, _ in ExpertWeights("static").named_parameters()] == ["logits"]
    assert {n: tuple(p.shape) for n, p in ExpertWeights("gated", 5).named_parameters()} == {"weight": (3, 10), "bias": (3,)}
    with pytest.raises(ValueError, match="mode"):
        ExpertWeights("learned")
    with pytest.raises(ValueError, match="embed_size"):
        ExpertWeights("gated")
    with pytest.raises(ValueError, match="embed_size"):
        ExpertWeights("static", 4)
    # the gate is per frame and its gradient reaches the embeddings
    gate = ExpertWeights("gated", 4)
    with torch.no_grad():
        gate.weight.copy_(torch.randn(3, 8, generator=torch.Generator().manual_seed(8)))
    ea, ev = torch.randn(B, T, 4, requires_grad=True), torch.randn(B, T, 4, requires_grad=True)
    lw = gate(ea, ev)
    torch.testing.assert_close(lw.exp().sum(-1), torch.ones(B, T))
    torch.testing.assert_close(gate(ea[:1, 2:3], ev[:1, 2:3]), lw[:1, 2:3])
    lw[..., 0].sum().backward()
    assert float(ea.grad.abs().max()) > 0.0 and float(ev.grad.abs().max()) > 0.0 and float(gate.weight.grad.abs().max()) > 0.0


@pytest.mark.parametrize("name", ["mrssm_nonsquare", "mmtrssm_cfg3dims"])
def test_state_dict_keys(name: str) -> None:
    case = CASES[name]
    oracle = build_model(case)
    model = product_from_case(case, oracle, "cpu")
    assert model.expert_weights is None and model.weights_timeseries is None
    assert list(model.state_dict()) == list(oracle.state_dict())
    model.expert_weights = ExpertWeights("gated", case.dims.embed)
    keys = set(model.state_dict()) - set(oracle.state_dict())
    assert keys == {"expert_weights.weight", "expert_weights.bias"}
    assert "expert_weights.weight" in dict(model.named_parameters())
    with torch.no_grad():
        model.expert_weights.weight.copy_(torch.randn(model.expert_weights.weight.shape, generator=torch.Generator().manual_seed(9)))
        model.expert_weights.bias.copy_(torch.tensor([0.5, -0.25, 0.125]))
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    other = product_from_case(case, oracle, "cpu")
    other.expert_weights = ExpertWeights("gated", case.dims.embed)
    result = other.load_state_dict(torch.load(buf), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert torch.equal(other.expert_weights.weight, model.expert_weights.weight)
    assert torch.equal(other.expert_weights.bias, model.expert_weights.bias)
    static = product_from_case(case, oracle, "cpu")
    static.expert_weights = ExpertWeights("static")
    assert set(static.state_dict()) - set(oracle.state_dict()) == {"expert_weights.logits"}
    # without the module the reference's checkpoint still loads strictly
    plain = product_from_case(case, oracle, "cpu")
    assert not plain.load_state_dict(oracle.state_dict(), strict=True).missing_keys


@pytest.mark.parametrize(("shape", "dtype"), [
    ((2, 4, 2), torch.float32),
    ((2, 4), torch.float32),
    ((2, 5, 3), torch.float32),
    ((3, 4, 3), torch.float32),
    ((2, 4, 3), torch.float64),
    ((2, 4, 3), torch.int32),
])
def test_wrong_shape_or_dtype_raises_value_error(shape: tuple[int, ...], dtype: torch.dtype) -> None:
    with pytest.raises(ValueError, match="expert log-weights"):
        scan.check_expert_logw(torch.zeros(shape, dtype=dtype), 2, 4)


def test_check_expert_logw_accepts_and_makes_contiguous() -> None:
    assert scan.check_expert_logw(None, 2, 4) is None
    lw = torch.zeros(2, 3, 4).transpose(1, 2)
    out = scan.check_expert_logw(lw, 2, 4)
    assert out.is_contiguous() and out.shape == (2, 4, 3)


def test_model_rejects_bad_weights_before_any_launch() -> None:
    case = CASES["mrssm_nonsquare"]
    model = product_from_case(case, build_model(case), "cpu")
    ea = torch.zeros(case.batch, case.steps, case.dims.embed)
    with pytest.raises(ValueError, match="expert log-weights"):
        model._expert_logw(ea, ea, torch.zeros(case.batch, case.steps, 2), case.batch, case.steps)  # noqa: SLF001
    # a modality absent at every step: no step has both, nothing is passed and the gate is not run
    model.expert_weights = ExpertWeights("static")
    assert model._expert_logw(ea, None, None, case.batch, case.steps) is None  # noqa: SLF001
    assert torch.equal(model._expert_logw(ea, ea, None, case.batch, case.steps),  # noqa: SLF001
                       torch.full((case.batch, case.steps, 3), LOG_THIRD, dtype=torch.float32))


@pytest.mark.parametrize(("cls", "new"), [(_lib.MrssmFwdIO, ["expert_logw"]), (_lib.MrssmBwdIO, ["expert_logw", "g_expert_logw"]),
                                          (_lib.MmtrssmFwdIO, ["expert_logw"]), (_lib.MmtrssmBwdIO, ["expert_logw", "g_expert_logw"])])
def test_io_structs_carry_the_weights(cls: type, new: list[str]) -> None:
    body = re.search(r"typedef struct " + cls.__name__ + r" \{(.*?)\} " + cls.__name__ + ";", HEADER, flags=re.DOTALL).group(1)
    assert re.search(r"const float\* expert_logw;", body)
    names = [n for n, _ in cls._fields_]  # noqa: SLF001
    assert names[-len(new) - 1 :] == [*new, "modality"]


def test_entry_points_refuse_weights_without_codes() -> None:
    import ctypes as C  # noqa: PLC0415

    lib = _lib.load()
    io_ = _lib.MrssmFwdIO()
    io_.expert_logw = 16
    dims = _lib.MrssmDims(1, 1, 8, 8, 2, 2, 0, 1, 1.0, 1.0, 0, 0)
    assert lib.mtrssm_mrssm_rollout_fwd(C.byref(dims), None, C.byref(io_), None) == -1
    assert b"expert_logw needs modality" in lib.mtrssm_last_error()
    bio = _lib.MmtrssmBwdIO()
    bio.g_expert_logw = 16
    bio.modality = 16
    assert lib.mtrssm_mmtrssm_rollout_bwd(None, None, C.byref(bio), None) == -1
    assert b"g_expert_logw needs expert_logw" in lib.mtrssm_last_error()


def test_factory_key_builds_the_weighted_classes() -> None:
    import multimodal_mtrssm_amd as mt  # noqa: PLC0415

    case = CASES["mrssm_nonsquare"]
    d = case.dims
    kw = dict(deter=d.deter, hidden=d.hidden, classes=d.classes, cats=d.cats, action=d.action, embed=d.embed, enc_audio=d.enc_audio,
              enc_vision=d.enc_vision, dec_audio=d.dec_audio, dec_vision=d.dec_vision, activation=d.activation, init_cells=d.init_cells)
    plain = mt.make_mrssm(**kw)
    assert type(plain) is mt.MoPoE_MRSSM and plain.expert_weights is None
    gated = mt.make_mrssm(**kw, expert_weights="gated")
    assert isinstance(gated, mt.WeightedMoPoE_MRSSM) and gated.expert_weights.mode == "gated"
    assert tuple(gated.expert_weights.weight.shape) == (3, 2 * d.embed)
    assert set(gated.state_dict()) - set(plain.state_dict()) == {"expert_weights.weight", "expert_weights.bias"}
    static = mt.make_mrssm(**kw, expert_weights="static")
    assert static.expert_weights.mode == "static"
    with pytest.raises(ValueError, match="mode"):
        mt.make_mrssm(**kw, expert_weights="both")
    c3 = CASES["mmtrssm_cfg3dims"].dims
    mm = mt.make_mmtrssm(hd=c3.hd, hs=(c3.hs_classes, c3.hs_cats), ld=c3.ld, ls=(c3.ls_classes, c3.ls_cats), hidden=c3.hidden, action=c3.action,
                         embed=c3.embed, enc_audio=c3.enc_audio, enc_vision=c3.enc_vision, dec_audio=c3.dec_audio, dec_vision=c3.dec_vision,
                         expert_weights="static")
    assert isinstance(mm, mt.WeightedMoPoE_MMTRSSM) and [n for n, _ in mm.expert_weights.named_parameters()] == ["logits"]
