"""The residual blocks' 1x1 backward in one pass (``mtrssm_residual_bwd1x1``: ``conv1x1_bwd_fused_kernel<128 | 64>``).

``g_h = (W1^T g_y) act'(h)``, the dW1 partial sets and ``db1`` come from one read of ``g_y`` and ``h`` instead of
``conv1x1_stream_kernel<64, C, false>`` followed by ``conv1x1_wgrad_staged_kernel<2, C>``.  Frame counts, planes, activations
and mid widths are those of ``test_fused_residual_block_matches_two_launches_and_float64``: fewer frames than CUs, uneven
pairs, several frames per workgroup.

Tolerances: switch off against on, the project's A/B tolerance for re-ordered sums (``rtol=2e-5, atol=3e-6 * max|ref|``);
``g_x`` bit-equal, because the fused kernel keeps the stream kernel's pieces, product order and k-block order, so ``g_h`` and
everything computed from it is the same; against float64 on the CPU the existing test's ``rtol=1e-4, atol=4e-5 * max`` (ReLU
gradients skipped as there: an intermediate within rounding of 0 switches its gradient on or off).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

CASES = [(1, 0, (8, 8), None, 2, 128), (37, 50, (8, 8), (16, 4), 2, 128), (300, 700, (4, 16), (8, 8), 2, 128),
         (260, 0, (8, 8), None, 1, 128), (2, 0, (8, 8), None, 2, 64), (38, 50, (16, 4), (8, 8), 2, 64),
         (700, 300, (8, 8), (4, 16), 2, 64), (520, 0, (8, 8), None, 1, 64)]


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


@pytest.mark.parametrize(("na", "nv", "plane_a", "plane_v", "act", "mid"), CASES)
def test_fused_1x1_backward_matches_two_launches_and_float64(lib_loaded: None, na: int, nv: int, plane_a: tuple, plane_v: tuple | None,  # noqa: PLR0913
                                                             act: int, mid: int) -> None:
    import torch.nn.functional as F  # noqa: N812

    from multimodal_mtrssm_amd import _lib, conv

    gen = torch.Generator(device="cpu").manual_seed(7 + na)

    def rnd(*shape: int, scale: float = 1.0) -> torch.Tensor:
        return (torch.randn(*shape, generator=gen) * scale).to(DEV).requires_grad_(True)

    def params() -> tuple:
        return (rnd(mid, 64, 3, 3, scale=0.05), rnd(mid, scale=0.1), rnd(64, mid, 1, 1, scale=0.1), rnd(64, scale=0.1))

    xa, pa = rnd(na, 64, *plane_a), params()
    xv, pv = (rnd(nv, 64, *plane_v), params()) if nv else (None, None)
    leaves = [xa, *pa] + ([xv, *pv] if nv else [])  # per block: x, w3, b3, w1, b1

    def run(fused: bool) -> tuple[list[torch.Tensor], list[str]]:  # noqa: FBT001
        conv.RESBLOCK_BWD1X1_FUSE = fused
        conv.invalidate_packs()
        for t in leaves:
            t.grad = None
        try:
            if nv:
                ya, yv = conv.residual_block_pair(xa, pa, xv, pv, act=act)
                loss = ya.square().sum() + yv.sin().sum()
            else:
                loss = conv.residual_block(xa, *pa, act=act).square().sum()
            _lib.TIMERS.enable()
            loss.backward()
            kernels = list(_lib.TIMERS.summary())  # keyed by mtrssm_last_kernel() after every launch
        finally:
            _lib.TIMERS.disable()
            conv.RESBLOCK_BWD1X1_FUSE = True
        torch.cuda.synchronize()
        return [t.grad.clone() for t in leaves], kernels

    two, k_two = run(False)
    one, k_one = run(True)
    again, _ = run(True)
    # kernel identity
    name = f"mtrssm::conv1x1_bwd_fused_kernel<{mid}>"
    assert name in k_one, k_one
    assert not any("conv1x1_stream_kernel" in k or "conv1x1_wgrad_staged_kernel" in k for k in k_one), k_one
    assert any("conv1x1_wgrad_staged_kernel" in k for k in k_two) and not any("bwd_fused" in k for k in k_two), k_two

    for i, (a, b) in enumerate(zip(one, two, strict=True)):
        diff = float((a - b).abs().max())
        print(f"A/B tensor {i}: max |diff| {diff:.3e} of max |ref| {float(b.abs().max()):.3e}")
        np.testing.assert_allclose(_np(a), _np(b), rtol=2e-5, atol=3e-6 * float(b.abs().max()), err_msg=str(i))
    for i in range(0, len(leaves), 5):
        assert torch.equal(one[i], two[i]), f"g_x of block {i // 5} is not bit-equal"
    # determinism: partial sets, no atomics
    for i in range(0, len(leaves), 5):
        assert torch.equal(one[i + 3], again[i + 3]) and torch.equal(one[i + 4], again[i + 4]), f"w1 / b1 gradient of block {i // 5}"

    # float64 on the CPU
    def ref(x: torch.Tensor, p: tuple) -> torch.Tensor:
        w3, b3, w1, b1 = p
        fn = F.elu if act == 2 else F.relu  # noqa: PLR2004  (_lib.ACT_IDS)
        return x + F.conv2d(fn(F.conv2d(fn(x), w3, b3, 1, 1)), w1, b1)

    if act == 1:
        return  # ReLU: gradients are not compared against float64 (see the module docstring)
    cpu = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    loss = ref(cpu[0], tuple(cpu[1:5])).square().sum()
    if nv:
        loss = loss + ref(cpu[5], tuple(cpu[6:10])).sin().sum()
    loss.backward()
    for i, (a, b) in enumerate(zip(one, [t.grad for t in cpu], strict=True)):
        np.testing.assert_allclose(_np(a), b.numpy(), rtol=1e-4, atol=4e-5 * float(b.abs().max()), err_msg=f"float64 {i}")


def test_fused_1x1_backward_query_and_refusal(lib_loaded: None) -> None:
    """Only the residual stacks' shapes in the ``bf16x2`` mode have the fused kernel; elsewhere the entry point is an error."""
    import ctypes as C

    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()

    def geom(c: int, hw: tuple = (8, 8), split: int = 2, act: int = 2, cout: int = 64) -> C.Structure:
        g = conv._geom(N=6, C=c, Hs=hw[0], Ws=hw[1], C2=0, Cpad=c, KH=1, KW=1, SS=1, TS=1, OFFY=0, OFFX=0, Hq=hw[0], Wq=hw[1], OS=1,  # noqa: SLF001
                       QY=0, QX=0, Ho=hw[0], Wo=hw[1], Cout=cout, CoutPad=64, pre_act=1, act=act)
        g.mfma_split = split
        return g

    for c in (64, 128):
        for hw in ((8, 8), (16, 4), (4, 16)):
            assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(c, hw))) == 1
        assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(c, split=3))) == 0
        assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(c, split=0))) == 0
        assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(c, act=3))) == 0
        assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(c, hw=(16, 16)))) == 0
    assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom(32))) == 0
    assert lib.mtrssm_residual_bwd1x1(C.byref(geom(32)), *([None] * 6), None, 0, 0, None) == -1
    assert b"residual_bwd1x1" in lib.mtrssm_last_error()
