"""The weight-resident 3x3 kernels' epilogue operands, staging variants and activation instances (``conv_resident.h``),
through the public functions in ``bf16x2``: ``conv.residual_block`` / ``conv.residual_block_pair`` (fused forward
``conv3x3_resident_kernel<64, 4 | 2, 1, true, ELU, false, true>``; backward-data with BOTH operands, act'(x) and the skip
gradient: ``<128, 2, 2, ...>`` / ``<64, 2, 1, ...>`` as ``<.., false, ELU, true, false>``) and ``conv.conv2d`` 32 -> 64 (forward
``<32, 2, 1, true, ELU, false, false>``, backward-data ``<64, 1, 2, false, ELU, true, false>``: act' only, K split over wave
pairs).  ELU runs the compile-time instances, ReLU and identity the run-time-select body (``ELU = false``).

Frame counts.  2 frames: one tile per workgroup, prologue and drain only.  38 / 50: fewer tiles than workgroups.  Multi-tile:
``tiles = 2 * W + W // 3`` for the ``W`` workgroups the problem gets (all CUs alone, half of them in a pair of equal tile
counts): a third of the workgroups walks 3 tiles (both image buffers and both operand sets go round), the others 2 (an even
number).  A tile is one frame for the 128-wide block and two frames for 64 -> 64 and for 32 <-> 64.

Reference: torch on the CPU in float64.  Tolerances: the forward as ``test_fused_residual_block_matches_two_launches_and_float64``
(``rtol=1e-4, atol=4e-5 * max|ref|``), the data gradient as ``test_conv2d_kernel`` (``rtol=1e-4, atol=max(1e-4, 1e-5 * max|g_x|)``).
A paired launch equals the two single launches bitwise (``test_paired_launches_change_nothing``).

ReLU: act'(h) of the block's intermediate is a step, and the GPU's ``h`` differs from the float64 one by its rounding
(held to 1e-4 by ``test_conv2d_kernel``): a value that close to 0 may switch its gradient.  The upstream gradient is therefore
zero at the pixels where some channel of the float64 ``h`` lies within 2e-4 of 0 (the 1x1 layer maps a pixel's upstream
gradient to that pixel's ``g_h`` only), for every activation alike.  act'(x) is taken from the input itself and has no such case.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENTITY, RELU, ELU = 0, 1, 2  # _lib.ACT_IDS
H_GUARD = 2e-4
KERNEL = "mtrssm::conv3x3_resident_kernel"


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001
    assert mt.conv.mfma_mode() == "bf16x2"


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _flag(b: bool) -> str:  # noqa: FBT001
    return "true" if b else "false"


def multi_tiles(workgroups: int) -> int:
    """More tiles than workgroups: a third of them walks three tiles, the others two."""
    return 2 * workgroups + max(1, workgroups // 3)


def frame_counts(kind: str, frames_per_tile: int) -> tuple[int, int, int]:
    """(frames of the first problem alone, its frames in the pair, frames of the second problem)."""
    if kind == "two":
        return 2, 2, 2
    if kind == "few":
        return 38, 38, 50
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return multi_tiles(cus) * frames_per_tile, multi_tiles(cus // 2) * frames_per_tile, multi_tiles(cus // 2) * frames_per_tile


def _act64(x: torch.Tensor, act: int) -> torch.Tensor:
    import torch.nn.functional as F  # noqa: N812

    return F.elu(x) if act == ELU else (F.relu(x) if act == RELU else x)


def _timed(fn):  # noqa: ANN001, ANN202
    """``fn()`` and the kernels it launched (``mtrssm_last_kernel()`` after every library call)."""
    from multimodal_mtrssm_amd import _lib

    _lib.TIMERS.enable()
    try:
        out = fn()
        kernels = list(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
    return out, kernels


# ---------------------------------------------------------------------------------------------------------------------
# residual block: fused forward, backward-data with act'(x) and the skip gradient


def block_case(mid: int, act: int, kind: str) -> dict:
    """Inputs, parameters, upstream gradients (CPU, fp32) and the float64 results of one case: ``a`` the first problem
    (8x8 planes for the 128-wide block, 16x4 for 64 -> 64), ``v`` the second (the other plane)."""
    import torch.nn.functional as F  # noqa: N812

    n_single, n_pair, n_v = frame_counts(kind, 1 if mid == 128 else 2)  # noqa: PLR2004
    plane_a, plane_v = ((8, 8), (16, 4)) if mid == 128 else ((16, 4), (8, 8))  # noqa: PLR2004
    gen = torch.Generator(device="cpu").manual_seed(1000 * mid + 10 * act + len(kind))
    case = {"n_pair": n_pair}
    for tag, n, plane in (("a", n_single, plane_a), ("v", n_v, plane_v)):
        x = torch.randn(n, 64, *plane, generator=gen)
        p = (torch.randn(mid, 64, 3, 3, generator=gen) * 0.05, torch.randn(mid, generator=gen) * 0.1,
             torch.randn(64, mid, 1, 1, generator=gen) * 0.1, torch.randn(64, generator=gen) * 0.1)
        x64 = x.double().requires_grad_(True)
        w3, b3, w1, b1 = (t.double() for t in p)
        h64 = F.conv2d(_act64(x64, act), w3, b3, 1, 1)
        y64 = x64 + F.conv2d(_act64(h64, act), w1, b1)
        safe = (h64.detach().abs().amin(1, keepdim=True) >= H_GUARD).float()
        gy = torch.randn(n, 64, *plane, generator=gen) * safe
        (y64 * gy.double()).sum().backward()
        case[tag] = {"x": x, "p": p, "gy": gy, "y64": y64.detach(), "gx64": x64.grad}
    return case


def run_block(case: dict, act: int) -> dict:
    """``(y, g_x)`` of both problems from single launches and of the pair from paired launches, with the kernels that ran."""
    from multimodal_mtrssm_amd import conv

    def dev(side: dict, n: int) -> tuple:
        return (side["x"][:n].to(DEV).requires_grad_(True), tuple(t.to(DEV).requires_grad_(True) for t in side["p"]), side["gy"][:n].to(DEV))

    def single(side: dict) -> tuple:
        x, p, gy = dev(side, side["x"].shape[0])
        y = conv.residual_block(x, *p, act=act)
        y.backward(gy)
        return y.detach(), x.grad

    def pair() -> tuple:
        xa, pa, gya = dev(case["a"], case["n_pair"])
        xv, pv, gyv = dev(case["v"], case["v"]["x"].shape[0])
        ya, yv = conv.residual_block_pair(xa, pa, xv, pv, act=act)
        torch.autograd.backward([ya, yv], [gya, gyv])
        return ya.detach(), xa.grad, yv.detach(), xv.grad

    out = {}
    out["a"], out["k_a"] = _timed(lambda: single(case["a"]))
    out["v"], out["k_v"] = _timed(lambda: single(case["v"]))
    out["pair"], out["k_pair"] = _timed(pair)
    torch.cuda.synchronize()
    return out


def block_kernels(mid: int, act: int) -> tuple[str, str]:
    elu = _flag(act == ELU)
    fwd = f"{KERNEL}<64, {mid // 32}, 1, true, {elu}, false, true>"
    bwd = f"{KERNEL}<128, 2, 2, false, {elu}, true, false>" if mid == 128 else f"{KERNEL}<64, 2, 1, false, {elu}, true, false>"  # noqa: PLR2004
    return fwd, bwd


def _check64(got: torch.Tensor, y64: torch.Tensor, what: str, *, atol: float) -> None:
    print(f"float64 {what}: max |diff| {float((got.double().cpu() - y64).abs().max()):.3e} of max |ref| {float(y64.abs().max()):.3e}")
    np.testing.assert_allclose(_np(got), y64.numpy(), rtol=1e-4, atol=atol, err_msg=f"float64 {what}")


BLOCK_CASES = [(mid, ELU, kind) for mid in (128, 64) for kind in ("two", "few", "multi")]
BLOCK_CASES += [(mid, act, kind) for act in (RELU, IDENTITY) for mid in (128, 64) for kind in ("two", "few")]
BLOCK_CASES += [(128, RELU, "multi"), (64, IDENTITY, "multi")]


@pytest.mark.parametrize(("mid", "act", "kind"), BLOCK_CASES)
def test_residual_block_backward_with_both_epilogue_operands(lib_loaded: None, mid: int, act: int, kind: str) -> None:
    case = block_case(mid, act, kind)
    res = run_block(case, act)
    fwd, bwd = block_kernels(mid, act)
    for k in (res["k_a"], res["k_v"], res["k_pair"]):
        assert fwd in k and bwd in k, (fwd, bwd, k)
        assert [n for n in k if "conv3x3_resident_kernel" in n] == [fwd, bwd], k
    n_pair = case["n_pair"]
    ya, gxa, yv, gxv = res["pair"]
    for tag, got_y, got_gx, (one_y, one_gx), n in (("a", ya, gxa, res["a"], n_pair), ("v", yv, gxv, res["v"], yv.shape[0])):
        label = f"{mid} act {act} {kind} {tag}"
        # the pair against the single launches, bitwise (a frame's arithmetic does not depend on the grid it runs in)
        assert torch.equal(got_y, one_y[:n]), f"{label}: y of the paired launch differs from the single launch"
        assert torch.equal(got_gx, one_gx[:n]), f"{label}: g_x of the paired launch differs from the single launch"
        _check64(one_y, case[tag]["y64"], f"{label} y", atol=4e-5 * float(case[tag]["y64"].abs().max()))
        _check64(one_gx, case[tag]["gx64"], f"{label} g_x", atol=max(1e-4, 1e-5 * float(case[tag]["gx64"].abs().max())))


# ---------------------------------------------------------------------------------------------------------------------
# the first stack conv, 32 -> 64: backward-data 64 -> 32 with act'(x) only, two frames per tile, K split over wave pairs


def stack_case(act: int, kind: str) -> dict:
    import torch.nn.functional as F  # noqa: N812

    n = frame_counts(kind, 2)[0]
    gen = torch.Generator(device="cpu").manual_seed(77 + 10 * act + len(kind))
    x = torch.randn(n, 32, 8, 8, generator=gen)
    w, b = torch.randn(64, 32, 3, 3, generator=gen) * 0.1, torch.randn(64, generator=gen) * 0.1
    gy = torch.randn(n, 64, 8, 8, generator=gen)
    x64 = x.double().requires_grad_(True)
    y64 = F.conv2d(_act64(x64, act), w.double(), b.double(), 1, 1)
    (y64 * gy.double()).sum().backward()
    return {"x": x, "w": w, "b": b, "gy": gy, "y64": y64.detach(), "gx64": x64.grad}


def run_stack(case: dict, act: int) -> tuple:
    """``(y, g_x)`` and the kernels of the forward and of the backward-data launch (the weights take no gradient here: the
    backward is the data gradient alone)."""
    from multimodal_mtrssm_amd import conv

    x = case["x"].to(DEV).requires_grad_(True)
    w, b, gy = case["w"].to(DEV), case["b"].to(DEV), case["gy"].to(DEV)
    y, k_fwd = _timed(lambda: conv.conv2d(x, w, b, stride=1, padding=1, pre_act=True, act=act))
    _, k_bwd = _timed(lambda: y.backward(gy))
    torch.cuda.synchronize()
    return y.detach(), x.grad, k_fwd, k_bwd


@pytest.mark.parametrize("act", [ELU, RELU, IDENTITY])
def test_first_stack_conv_backward_data_with_the_act_operand(lib_loaded: None, act: int) -> None:
    for kind in ("two", "few", "multi"):
        case = stack_case(act, kind)
        y, gx, k_fwd, k_bwd = run_stack(case, act)
        res_fwd, res_bwd = ([k for k in ks if "conv3x3_resident_kernel" in k] for ks in (k_fwd, k_bwd))
        assert res_fwd == [f"{KERNEL}<32, 2, 1, true, {_flag(act == ELU)}, false, false>"], k_fwd
        assert res_bwd == [f"{KERNEL}<64, 1, 2, false, {_flag(act == ELU)}, true, false>"], k_bwd
        _check64(y, case["y64"], f"32->64 act {act} {kind} y", atol=1e-4)  # test_conv2d_kernel's forward tolerance
        _check64(gx, case["gx64"], f"32->64 act {act} {kind} g_x", atol=max(1e-4, 1e-5 * float(case["gx64"].abs().max())))
