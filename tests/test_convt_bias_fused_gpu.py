"""ConvTranspose2d bias gradients from inside the staged weight-gradient kernels (``mtrssm_conv_weight_grad_src_bias``).

The three decoder layers (k = 4, stride 2, pad 1: 64 -> 32 on 64-pixel planes, 32 -> 16 on 256-pixel planes, 16 -> 1 on
1024-pixel planes) stream their output gradient once for the weight gradient; the per-channel sums of that tensor -- the
bias gradient -- are added up in the same pass instead of by a ``channel_sum_kernel`` launch that re-reads it.

Bounds: against float64 the sum of ``n`` fp32 terms in a tree of partial sums is good to a few ulp of ``sum |g|``; the bound
below is ``1e-5 * sum |g|`` per channel (about 80 ulp, no cancellation assumed).  Against the ``_channel_sum`` path the
project's A/B tolerance for re-ordered sums, ``rtol=2e-5, atol=3e-6 * max |ref|``, with ``sum |g| / |sum g|`` of order
one by construction (every channel of the gradient has an offset between 0.5 and 1.5 on top of unit noise).
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (input channels, output channels, input plane, frames): vision and audio planes of the three layers; fewer frames than
# CUs, a frame count that leaves uneven runs, several frames per workgroup
SHAPES = [(64, 32, (8, 8), 37), (64, 32, (16, 4), 700), (32, 16, (16, 16), 300), (32, 16, (32, 8), 37), (16, 1, (32, 32), 300),
          (16, 1, (64, 16), 37), (16, 1, (32, 32), 1)]


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


class _Layer(torch.nn.Module):
    def __init__(self, cin: int, cout: int, gen: torch.Generator) -> None:
        super().__init__()
        self.weight = torch.nn.Parameter((torch.randn(cin, cout, 4, 4, generator=gen) * 0.05).to(DEV))
        self.bias = torch.nn.Parameter((torch.randn(cout, generator=gen) * 0.1).to(DEV))


def _backward(layer: _Layer, x: torch.Tensor, g_out: torch.Tensor, *, fused: bool) -> tuple[list[torch.Tensor], list[str]]:
    """One forward + backward of the layer; (x.grad, weight.grad, bias.grad) and the device kernels of the backward."""
    from multimodal_mtrssm_amd import _lib, conv

    conv.CONVT_BIAS_FUSE = fused
    conv.invalidate_packs()
    x.grad = None
    for p in (layer.weight, layer.bias):
        if p.grad is not None:
            p.grad.zero_()
    try:
        y = conv.conv_transpose2d(x, layer.weight, layer.bias, stride=2, padding=1, output_padding=0, pre_act=True, act=2)
        _lib.TIMERS.enable()
        y.backward(g_out)
        kernels = list(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
        conv.CONVT_BIAS_FUSE = True
    torch.cuda.synchronize()
    return [x.grad.clone(), layer.weight.grad.clone(), layer.bias.grad.clone()], kernels


@pytest.mark.parametrize("flat", [False, True], ids=["leaf", "flat"])
@pytest.mark.parametrize(("cin", "cout", "plane", "n"), SHAPES)
def test_convt_bias_grad_rides_in_weight_grad(lib_loaded: None, cin: int, cout: int, plane: tuple, n: int, flat: bool) -> None:  # noqa: FBT001
    """Bias gradient of the fused pass against float64, against the ``_channel_sum`` path, bit-identical from run to run, and
    no ``channel_sum_kernel`` in the backward; ``flat``: the parameters live in an ``optim.FlatParameters`` buffer, so the
    partial sets wait for the end of the backward pass (the train step's path) -- ``leaf``: they are summed on the spot."""
    import multimodal_mtrssm_amd as mt

    gen = torch.Generator(device="cpu").manual_seed(17 + n + cin)
    layer = _Layer(cin, cout, gen)
    keep = mt.optim.FlatParameters(layer) if flat else None
    x = torch.randn(n, cin, *plane, generator=gen).to(DEV).requires_grad_(True)
    g_out = (torch.randn(n, cout, 2 * plane[0], 2 * plane[1], generator=gen) + torch.linspace(0.5, 1.5, cout).view(1, -1, 1, 1)).to(DEV)

    ref, ref_kernels = _backward(layer, x, g_out, fused=False)
    got, kernels = _backward(layer, x, g_out, fused=True)
    again, _ = _backward(layer, x, g_out, fused=True)
    assert any("channel_sum_kernel" in k for k in ref_kernels), ref_kernels
    assert not any("channel_sum_kernel" in k for k in kernels), kernels
    assert any("wgrad_staged_kernel" in k for k in kernels), kernels

    g64 = g_out.double().cpu()
    want = g64.sum((0, 2, 3)).numpy()
    bound = 1e-5 * g64.abs().sum((0, 2, 3)).numpy()
    err = np.abs(_np(got[2]).astype(np.float64) - want)
    print(f"bias grad vs float64: max err / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all(), (err, bound)
    for i, (a, b) in enumerate(zip(got, ref, strict=True)):
        np.testing.assert_allclose(_np(a), _np(b), rtol=2e-5, atol=3e-6 * float(b.abs().max()), err_msg=str(i))
    # the weight gradient is the same kernel with the same partial sets: the extra sums change none of its bits
    assert torch.equal(got[1], ref[1])
    assert torch.equal(got[2], again[2]) and torch.equal(got[1], again[1])
    del keep


def test_src_bias_entry_point_refuses_other_kernels(lib_loaded: None) -> None:
    """The query is 1 exactly for the three staged kernels; the entry point errors elsewhere instead of dropping the sums."""
    import ctypes as C

    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()

    def geom(cin: int, cout: int, h: int, w: int, split: int = 2) -> C.Structure:
        g = conv._geom(N=8, C=cout, Hs=2 * h, Ws=2 * w, C2=0, Cpad=16 * ((cout + 15) // 16), KH=4, KW=4, SS=2, TS=1, OFFY=-1, OFFX=-1,  # noqa: SLF001
                       Hq=h, Wq=w, OS=1, QY=0, QX=0, Ho=h, Wo=w, Cout=cin, CoutPad=64 if cin > 32 else 32, pre_act=0, act=2)
        g.mfma_split = split
        return g

    for cin, cout, h, w in [(64, 32, 8, 8), (64, 32, 16, 4), (32, 16, 16, 16), (32, 16, 32, 8), (16, 1, 32, 32), (16, 1, 64, 16)]:
        assert lib.mtrssm_conv_weight_grad_src_bias_supported(C.byref(geom(cin, cout, h, w)), 1) == 1, (cin, cout, h, w)
        assert lib.mtrssm_conv_weight_grad_src_bias_supported(C.byref(geom(cin, cout, h, w, split=0)), 1) == 0
    odd = geom(64, 32, 4, 4)
    assert lib.mtrssm_conv_weight_grad_src_bias_supported(C.byref(odd), 1) == 0
    a = torch.zeros(8, 64, 4, 4, device=DEV)
    src = torch.zeros(8, 32, 8, 8, device=DEV)
    dwp = torch.zeros(64, 16, 32, device=DEV)
    db = torch.zeros(32, device=DEV)
    rc = lib.mtrssm_conv_weight_grad_src_bias(C.byref(odd), _lib.ptr(a), _lib.ptr(src), 1, _lib.ptr(dwp), _lib.ptr(db), None, 0, 0,
                                              _lib.stream_ptr(a.device))
    assert rc == -1
    assert b"src_bias" in lib.mtrssm_last_error()
