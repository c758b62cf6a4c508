"""Staged weight-gradient kernels past the first lap of their unrolled frame loop.

Every staged kernel of ``csrc/conv_wgrad_resident.h`` walks its workgroup's run of frames in a loop unrolled by the period
of its raw register sets and image buffers (2, 3 or 6 frames: ``wg_frame_loop``).  The cases of ``tests/test_gpu_parity.py``
give a workgroup at most 3 frames (6 in the paired 1x1 launch) on a 256-CU device, so none of them reaches the second lap,
where the set and buffer literals wrap, the third register set is reused and the clamped requests of the last two frames
land.  Here ``N = 6 P + 1`` and ``N = 4 P + 1`` frames (``P`` = the device's CU count): 7 frames per workgroup with a last
workgroup of fewer, and 5 frames per workgroup.  The frames a workgroup received are taken from the library's own workspace
query and the kernel's set size, so the test cannot pass without a second lap whatever the device's CU count.

One geometry per staged family (the layer shapes of ``CONV_CASES`` / ``DECONV_CASES``), ``bf16x2``, ELU on the operand the
layer activates, weight gradient and fused bias gradient; plus the fused 1x1 backward (``mtrssm_residual_bwd1x1``).  Every
case runs twice: with its partial-set workspace, and with a workspace one byte too small (the atomics form of the same
kernel).  The staged kernel is asserted by name.

Reference: torch's conv weight gradient on float64 tensors on the host.  Bound: the one ``test_conv2d_kernel`` applies to
weight and bias gradients in this mode, ``rtol=1e-4, atol=max(2e-4, 2e-5 * max |ref|)``, not scaled with the frame count.
Measured with the library of the commit BEFORE the one that added this file (``P = 256``, 1537 and 1025 frames): worst error
over bound 0.15 - 0.21 for the weight gradients in either form, at most 0.012 for the bias gradients; per case in
``profiles/wgrad_staged_refactor_notes.md`` section 7.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELU = 2  # _lib.ACT_IDS

# family -> (kind, a channels, src channels, plane of `a`, taps per side, floats of one workgroup's partial set, kernel name)
#   conv:   a = output gradient [N][co][H][W], src = layer input [N][ci][2H][2W] (stride 2) or [N][ci][H][W]
#   deconv: a = layer input [N][ci][H][W] (activated), src = output gradient [N][co][2H][2W]; the bias gradient sums src
FAMILIES = {
    "res3x3": ("conv", 64, 64, (8, 8), 3, 1, 2 * 2 * 9 * 1024 + 64, "mtrssm::conv3x3_wgrad_resident_kernel<2, 64, 8>"),
    "res1x1": ("conv", 64, 64, (8, 8), 1, 1, 8 * 1024 + 64, "mtrssm::conv1x1_wgrad_staged_kernel<2, 64>"),
    "enc1": ("conv", 8, 1, (32, 32), 3, 2, 8 * 64 * 4 + 8, "mtrssm::conv3x3s2_thin_wgrad_staged_kernel<2, 32>"),
    "enc2": ("conv", 16, 8, (16, 16), 3, 2, 8 * 2 * 64 * 4 + 16, "mtrssm::conv3x3s2_wgrad_staged_kernel<2, 16>"),
    "enc3": ("conv", 32, 16, (8, 8), 3, 2, 8 * 4 * 64 * 4 + 32, "mtrssm::conv3x3s2c_wgrad_staged_kernel<2, 8>"),
    "dec1": ("deconv", 64, 32, (8, 8), 4, 2, 8 * 4 * 4 * 64 * 4 + 32, "mtrssm::convt4s2b_wgrad_staged_kernel<2, 8>"),
    "dec2": ("deconv", 32, 16, (16, 16), 4, 2, 8 * 4 * 64 * 4 + 16, "mtrssm::convt4s2_wgrad_staged_kernel<2, 16>"),
    "dec3": ("deconv", 16, 1, (32, 32), 4, 2, 8 * 2 * 64 * 4 + 8, "mtrssm::convt4s2_thin_wgrad_staged_kernel<2, 32>"),
    "bwd1x1": ("bwd1x1", 64, 128, (8, 8), 1, 1, 8 * 1024 + 64, "mtrssm::conv1x1_bwd_fused_kernel<128>"),
}


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


def _close(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    """``test_conv2d_kernel``'s bound for weight and bias gradients; prints the worst error over its bound first."""
    g, r = got.detach().double().cpu().numpy(), ref.numpy()
    atol = max(2e-4, 2e-5 * float(np.abs(r).max()))
    ratio = float((np.abs(g - r) / (atol + 1e-4 * np.abs(r))).max())
    print(f"{what}: error / bound = {ratio:.3f} (max |ref| {float(np.abs(r).max()):.3e})")
    np.testing.assert_allclose(g, r, rtol=1e-4, atol=atol, err_msg=what)


def _operands(family: str, laps: int) -> dict:
    """Host tensors and the geometry of one case: ``a`` and ``src`` as the layer's weight-gradient launch takes them."""
    from multimodal_mtrssm_amd import conv

    kind, ca, cs, (h, w), k, stride, _, _ = FAMILIES[family]
    n = laps * torch.cuda.get_device_properties(0).multi_processor_count + 1
    gen = torch.Generator(device="cpu").manual_seed(1000 * laps + len(family) + ca + cs)
    a = torch.randn(n, ca, h, w, generator=gen)
    src = torch.randn(n, cs, stride * h, stride * w, generator=gen)
    coords = torch.randn(2, stride * h, stride * w, generator=gen) if family == "enc1" else None
    w1 = torch.randn(ca, cs, 1, 1, generator=gen) * 0.1 if kind == "bwd1x1" else None
    c2 = 0 if coords is None else 2
    opad, ipad = conv._pads(ca, cs + c2)  # noqa: SLF001
    pad = 0 if k == 1 else 1
    geom = conv._geom(N=n, C=cs, Hs=stride * h, Ws=stride * w, C2=c2, Cpad=ipad, KH=k, KW=k, SS=stride, TS=1, OFFY=-pad, OFFX=-pad,  # noqa: SLF001
                      Hq=h, Wq=w, OS=1, QY=0, QX=0, Ho=h, Wo=w, Cout=ca, CoutPad=opad, pre_act=0 if kind == "deconv" else 1, act=ELU)
    return {"family": family, "n": n, "a": a, "src": src, "coords": coords, "w1": w1, "c2": c2, "pad": pad, "geom": geom,
            "pre_act_a": 1 if kind == "deconv" else 0}


def _forms(ops: dict):  # noqa: ANN202
    """Runs the case with its partial-set workspace and with one a byte too small (the atomics form of the same kernel);
    yields ``(form, dW, db, g_h or None)``.  Asserts the frames per workgroup and the kernel's name."""
    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()
    stream = _lib.stream_ptr(torch.device(DEV))
    family, n, geom, pre_act_a, c2 = ops["family"], ops["n"], ops["geom"], ops["pre_act_a"], ops["c2"]
    kind, ca, cs, _, k, _, set_floats, kernel = FAMILIES[family]
    ad, sd = ops["a"].to(DEV), ops["src"].to(DEV)
    cd = None if ops["coords"] is None else ops["coords"].to(DEV)
    need = int(lib.mtrssm_conv_weight_grad_workspace_bytes(C.byref(geom), pre_act_a))
    assert need > 0 and need % (4 * set_floats) == 0, (need, set_floats)
    blocks = need // (4 * set_floats)  # one partial set per workgroup, one co group in every case
    per = -(-n // blocks)
    print(f"{family}: N = {n}, {blocks} workgroups, {per} frames per workgroup, {n - (blocks - 1) * per} in the last one")
    laps = (n - 1) // torch.cuda.get_device_properties(0).multi_processor_count
    assert per > (6 if laps == 6 else 4), f"{family}: {per} frames per workgroup: no second lap of the frame loop"  # noqa: PLR2004
    if kind == "bwd1x1":
        assert lib.mtrssm_residual_bwd1x1_supported(C.byref(geom)) == 1
        conv.invalidate_packs()
        _, wq1t = conv.pack_weight(ops["w1"].to(DEV).permute(1, 0, 2, 3))
    for form, ws_bytes in (("partial sets", need), ("atomics", need - 1)):
        ws = torch.empty(need // 4 + 64, device=DEV)
        dwp = torch.zeros(geom.CoutPad, k * k, geom.Cpad, device=DEV)
        db = torch.zeros(cs if kind == "deconv" else ca, device=DEV)
        gh = None
        if kind == "deconv":
            assert lib.mtrssm_conv_weight_grad_src_bias_supported(C.byref(geom), pre_act_a) == 1
            rc = lib.mtrssm_conv_weight_grad_src_bias(C.byref(geom), _lib.ptr(ad), _lib.ptr(sd), pre_act_a, _lib.ptr(dwp), _lib.ptr(db),
                                                      _lib.raw_ptr(ws), ws_bytes, 0, stream)
        elif kind == "bwd1x1":
            gh = torch.empty_like(sd)
            rc = lib.mtrssm_residual_bwd1x1(C.byref(geom), _lib.ptr(ad), _lib.ptr(sd), _lib.raw_ptr(wq1t), _lib.ptr(gh), _lib.ptr(dwp),
                                            _lib.ptr(db), _lib.raw_ptr(ws), ws_bytes, 0, stream)
        else:
            rc = lib.mtrssm_conv_weight_grad(C.byref(geom), _lib.ptr(ad), _lib.ptr(sd), _lib.ptr(cd), pre_act_a, _lib.ptr(dwp), _lib.ptr(db),
                                             _lib.raw_ptr(ws), ws_bytes, stream)
        _lib.check(rc, family)
        assert lib.mtrssm_last_kernel().decode() == kernel, (family, form, lib.mtrssm_last_kernel().decode())
        torch.cuda.synchronize()
        yield form, dwp[:ca, :, : cs + c2].reshape(ca, k, k, cs + c2).permute(0, 3, 1, 2), db, gh


@pytest.mark.parametrize("laps", [6, 4], ids=["6P+1", "4P+1"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_staged_wgrad_second_lap(lib_loaded: None, family: str, laps: int) -> None:
    import torch.nn.functional as F  # noqa: N812

    from multimodal_mtrssm_amd import conv

    assert conv.mfma_mode() == "bf16x2"
    kind, ca, cs, _, k, stride, _, _ = FAMILIES[family]
    ops = _operands(family, laps)
    n, c2, pad = ops["n"], ops["c2"], ops["pad"]
    # ---- float64 on the host: torch's conv weight gradient
    a64, s64 = ops["a"].double(), ops["src"].double()
    if kind == "deconv":  # dW[ci][co][ky][kx] = sum elu(a)[n,ci,y,x] src[n,co,2y-1+ky,2x-1+kx];  db[co] = sum src
        w64 = torch.nn.grad.conv2d_weight(s64, (ca, cs, k, k), F.elu(a64), stride=stride, padding=pad)
        b64 = s64.sum((0, 2, 3))
    else:  # dW[co][ci][ky][kx] = sum a[n,co,y,x] elu(src ++ coords)[n,ci,sy-p+ky,sx-p+kx];  db[co] = sum a
        full = s64 if c2 == 0 else torch.cat([s64, ops["coords"].double().unsqueeze(0).expand(n, -1, -1, -1)], 1)
        w64 = torch.nn.grad.conv2d_weight(F.elu(full), (ca, cs + c2, k, k), a64, stride=stride, padding=pad)
        b64 = a64.sum((0, 2, 3))
    if kind == "bwd1x1":  # g_h = (W1^T g_y) elu'(h)
        gh64 = torch.einsum("om,nohw->nmhw", ops["w1"].double()[:, :, 0, 0], a64) * torch.where(s64 > 0, torch.ones_like(s64), s64.exp())

    for form, gw, db, gh in _forms(ops):
        _close(gw, w64, f"{family} N={n} {form} dW")
        _close(db, b64, f"{family} N={n} {form} db")
        if gh is not None:  # stored inside the frame loop: tests/test_resblock_bwd1x1_gpu.py's float64 bound
            np.testing.assert_allclose(gh.double().cpu().numpy(), gh64.numpy(), rtol=1e-4, atol=4e-5 * float(gh64.abs().max()),
                                       err_msg=f"{family} N={n} {form} g_h")
