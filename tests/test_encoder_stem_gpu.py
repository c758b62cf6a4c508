"""The encoders' strided stem as one launch (``mtrssm_encoder_stem_fwd``, csrc/conv_stem.h) against a float64 chain and against
the per-layer path (``MTRSSM_ENCODER_STEM=0``: ``conv.ENCODER_STEM = False``).

Bounds.  Outputs against float64: ``test_conv2d_kernel``'s ``rtol = 1e-4, atol = 1e-4`` (two bf16 pieces per operand: 8e-6
measured there), for the whole chain; the weights are scaled so that y1, y2, y3 stay O(1) like that test's outputs.
Against the per-layer path's own error, layer by layer ON THE SAME INPUT (y1 from the frame, y3 from the fused y2; y2 from the
same y1 is bit-identical): both paths truncate their operands to the same two pieces and differ only in the order of the fp32
sums (and in the coordinate planes' term of y1, which the fused kernel forms in fp32, exactly); either path rounds its
accumulator once per MFMA, so another order moves a result by a few ulp of its partial sums: the fused error may exceed the
per-layer one by ``2^-21 max |y|`` (four ulp of the largest output), no more.
Gradients with the switch on and off: ``test_conv2d_kernel``'s gradient bounds (the backward is the same code).
"""

from __future__ import annotations

import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLANES = [(64, 64), (128, 32)]
ACTS = {1: F.relu, 2: F.elu}
STEM_KERNEL = b"mtrssm::encoder_stem_kernel"


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


@pytest.fixture
def bf16x2_mode():  # noqa: ANN201
    from multimodal_mtrssm_amd import conv

    before = conv.mfma_mode()
    conv.set_mfma_mode("bf16x2")
    yield
    conv.set_mfma_mode(before)


@contextlib.contextmanager
def stem_switch(on: bool):  # noqa: ANN201, FBT001
    from multimodal_mtrssm_amd import conv

    before = conv.ENCODER_STEM
    conv.ENCODER_STEM = on
    try:
        yield
    finally:
        conv.ENCODER_STEM = before


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().double().cpu().numpy()


def _problem(n: int, plane: tuple[int, int], *, bias: bool, seed: int) -> dict:
    """Frames in (-1.5, 1.5) (so y1 / y2 take both branches of the activation), non-zero in every border row and column."""
    g = torch.Generator().manual_seed(seed)
    h, w = plane
    x = torch.rand(n, 1, h, w, generator=g) * 3 - 1.5
    assert bool(((x > -1) & (x < 0)).any())
    for edge in (x[..., 0, :], x[..., -1, :], x[..., :, 0], x[..., :, -1]):
        assert bool((edge != 0).all())
    cc = torch.stack([torch.linspace(-1, 1, h)[:, None].expand(h, w), torch.linspace(-1, 1, w)[None, :].expand(h, w)])
    ws = [torch.randn(co, ci, 3, 3, generator=g) * sc for co, ci, sc in ((8, 3, 0.2), (16, 8, 0.12), (32, 16, 0.08))]
    bs = [torch.randn(co, generator=g) if bias else None for co in (8, 16, 32)]
    return {"x": x, "cc": cc, "ws": ws, "bs": bs}


def _reference(p: dict, act: int) -> list[np.ndarray]:
    x = torch.cat([p["x"], p["cc"].unsqueeze(0).expand(p["x"].shape[0], -1, -1, -1)], 1).double()
    outs = []
    for i, (w, b) in enumerate(zip(p["ws"], p["bs"], strict=True)):
        x = F.conv2d(ACTS[act](x) if i else x, w.double(), None if b is None else b.double(), 2, 1)
        outs.append(x.numpy())
    return outs


def _device(p: dict) -> dict:
    return {"x": p["x"].to(DEV), "cc": p["cc"].to(DEV).contiguous(), "ws": [w.to(DEV) for w in p["ws"]],
            "bs": [None if b is None else b.to(DEV) for b in p["bs"]]}


def _job(d: dict, act: int) -> tuple:
    return d["x"], d["cc"], [(w, b, 2, 1) for w, b in zip(d["ws"], d["bs"], strict=True)], act


def _layers(d: dict, act: int) -> list[torch.Tensor]:
    from multimodal_mtrssm_amd.conv import conv2d

    x, outs = d["x"], []
    for i, (w, b) in enumerate(zip(d["ws"], d["bs"], strict=True)):
        x = conv2d(x, w, b, stride=2, padding=1, pre_act=i > 0, act=act, coords=d["cc"] if i == 0 else None)
        outs.append(x)
    return outs


def _run(ds: list[dict], act: int, *, fused: bool) -> list[list[torch.Tensor]]:
    """y1, y2, y3 of one or two problems through ``conv.encoder_stem`` + the per-layer calls, as ``cnn.encode_pair`` makes them."""
    from multimodal_mtrssm_amd import _lib, conv

    conv.invalidate_packs()
    with stem_switch(fused), conv.encoder_stem([_job(d, act) for d in ds]) as launched:
        assert launched == fused
        if fused:
            assert _lib.load().mtrssm_last_kernel() == STEM_KERNEL
        outs = [_layers(d, act) for d in ds]
        if fused:  # no conv call above launched anything: the outputs are the fused launch's
            assert _lib.load().mtrssm_last_kernel() == STEM_KERNEL
        else:
            assert b"encoder_stem" not in _lib.load().mtrssm_last_kernel()
    torch.cuda.synchronize()
    return outs


def _check(got: list[torch.Tensor], want: list[np.ndarray], tag: str) -> None:
    for i, (g, w) in enumerate(zip(got, want, strict=True)):
        print(f"{tag} y{i + 1}: fused chain vs float64 {float(np.abs(_np(g) - w).max()):.3e} (max |y| {float(np.abs(w).max()):.2f})")
        np.testing.assert_allclose(_np(g), w, rtol=1e-4, atol=1e-4, err_msg=f"{tag} y{i + 1}")


def _check_layer(fused: torch.Tensor, layer: torch.Tensor, want: np.ndarray, tag: str) -> None:
    """One layer of both paths on the same input against float64: the fused error is the per-layer one up to re-ordered sums."""
    err, err_layer = float(np.abs(_np(fused) - want).max()), float(np.abs(_np(layer) - want).max())
    print(f"{tag}: fused vs float64 {err:.3e}, per-layer vs float64 {err_layer:.3e}")
    assert err <= err_layer + 2.0 ** -21 * float(np.abs(want).max()), (tag, err, err_layer)


def _layer3_reference(p: dict, y2: torch.Tensor, act: int) -> np.ndarray:
    b = p["bs"][2]
    return F.conv2d(ACTS[act](y2.double().cpu()), p["ws"][2].double(), None if b is None else b.double(), 2, 1).numpy()


@pytest.mark.parametrize("act", [2, 1], ids=["elu", "relu"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("plane", PLANES, ids=["64x64", "128x32"])
def test_outputs_match_float64_and_the_per_layer_path(plane: tuple, n: int, bias: bool, act: int, bf16x2_mode: None, lib_loaded: None) -> None:  # noqa: FBT001
    from multimodal_mtrssm_amd.conv import conv2d

    p = _problem(n, plane, bias=bias, seed=100 * n + plane[0])
    d = _device(p)
    want = _reference(p, act)
    (got,) = _run([d], act, fused=True)
    (layer,) = _run([d], act, fused=False)
    assert [tuple(t.shape) for t in got] == [w.shape for w in want]
    tag = f"{plane} n={n} bias={bias} act={act}"
    _check(got, want, tag)
    _check(layer, want, tag + " per-layer")
    _check_layer(got[0], layer[0], want[0], tag + " y1")
    with stem_switch(False):  # the per-layer kernels on the fused launch's y1 and y2
        y2 = conv2d(got[0], d["ws"][1], d["bs"][1], stride=2, padding=1, pre_act=True, act=act)
        y3 = conv2d(got[1], d["ws"][2], d["bs"][2], stride=2, padding=1, pre_act=True, act=act)
    assert torch.equal(y2, got[1])  # the band kernel's k-blocks and product order: the same bits
    _check_layer(got[2], y3, _layer3_reference(p, got[1], act), tag + " y3 from the same y2")


def _cu_count() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("rounds", [1, 2])
def test_uneven_runs_of_frames(rounds: int, bf16x2_mode: None, lib_loaded: None) -> None:
    """N = workgroups + 1 and 2 x workgroups + 1 (one workgroup per CU): some workgroups walk one frame more than the others,
    and the request registers are refilled while a frame is in flight."""
    n = rounds * _cu_count() + 1
    p = _problem(n, (64, 64), bias=True, seed=7 + rounds)
    (got,) = _run([_device(p)], 2, fused=True)
    _check(got, _reference(p, 2), f"n={n}")


def test_pair_with_different_frame_counts(bf16x2_mode: None, lib_loaded: None) -> None:
    pa, pv = _problem(5, (128, 32), bias=True, seed=21), _problem(3, (64, 64), bias=True, seed=22)
    da, dv = _device(pa), _device(pv)
    got_a, got_v = _run([da, dv], 2, fused=True)
    lay_a, lay_v = _run([da, dv], 2, fused=False)
    want_a, want_v = _reference(pa, 2), _reference(pv, 2)
    _check(got_a, want_a, "pair audio")
    _check(got_v, want_v, "pair vision")
    _check_layer(got_a[0], lay_a[0], want_a[0], "pair audio y1")
    _check_layer(got_v[0], lay_v[0], want_v[0], "pair vision y1")
    # more frames than workgroups in both halves of the grid: 2 x CUs + 1 frames over CUs workgroups
    n = _cu_count()
    pa, pv = _problem(n + 1, (128, 32), bias=False, seed=23), _problem(n, (64, 64), bias=False, seed=24)
    got_a, got_v = _run([_device(pa), _device(pv)], 2, fused=True)
    _check(got_a, _reference(pa, 2), "long pair audio")
    _check(got_v, _reference(pv, 2), "long pair vision")


def _encoders() -> tuple:
    from multimodal_mtrssm_amd.cnn import Encoder
    from oracle.cases import encoder_config

    torch.manual_seed(5)
    enc_a = Encoder(encoder_config((1, 128, 32), 24, res_blocks=1, res_inter=16, res_out=16)).to(DEV)
    enc_v = Encoder(encoder_config((1, 64, 64), 24, res_blocks=1, res_inter=16, res_out=16)).to(DEV)
    return enc_a, enc_v


def test_encode_pair_gradients_agree_with_the_switch_off(bf16x2_mode: None, lib_loaded: None) -> None:
    from multimodal_mtrssm_amd import _lib, conv
    from multimodal_mtrssm_amd.cnn import encode_pair

    enc_a, enc_v = _encoders()
    g = torch.Generator().manual_seed(6)
    xa = (torch.rand(3, 1, 128, 32, generator=g) * 2 - 1).to(DEV)
    xv = (torch.rand(3, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
    ga, gv = torch.randn(3, 24, generator=g).to(DEV), torch.randn(3, 24, generator=g).to(DEV)
    stem = [p for enc in (enc_a, enc_v) for m in enc.convs for p in (m.weight, m.bias)]
    grads = {}
    for fused in (True, False):
        for p in list(enc_a.parameters()) + list(enc_v.parameters()):
            p.grad = None
        conv.invalidate_packs()
        with stem_switch(fused):
            _lib.TIMERS.enable()
            try:
                ea, ev = encode_pair(enc_a, enc_v, xa, xv)
                kernels = list(_lib.TIMERS.summary())
            finally:
                _lib.TIMERS.disable()
            assert any("encoder_stem_kernel" in k for k in kernels) == fused, kernels
            assert any("conv3x3s2_band_kernel" in k for k in kernels) != fused, kernels
            ((ea * ga).sum() + (ev * gv).sum()).backward()
            conv.flush_pending_grads()
        torch.cuda.synchronize()
        grads[fused] = [p.grad.clone() for p in stem]
    for i, (got, want) in enumerate(zip(grads[True], grads[False], strict=True)):
        assert float(want.abs().max()) > 0
        np.testing.assert_allclose(_np(got), _np(want), rtol=1e-4, atol=max(2e-4, 2e-5 * float(want.abs().max())), err_msg=str(i))


def test_one_modality_alone_is_a_single_problem(bf16x2_mode: None, lib_loaded: None) -> None:
    from multimodal_mtrssm_amd import _lib

    enc_a, _ = _encoders()
    x = (torch.rand(2, 2, 1, 128, 32, generator=torch.Generator().manual_seed(9)) * 2 - 1).to(DEV)
    outs = {}
    for fused in (True, False):
        with stem_switch(fused):
            _lib.TIMERS.enable()
            try:
                outs[fused] = enc_a(x)
                kernels = list(_lib.TIMERS.summary())
            finally:
                _lib.TIMERS.disable()
        assert any("encoder_stem_kernel" in k for k in kernels) == fused, kernels
    np.testing.assert_allclose(_np(outs[True]), _np(outs[False]), rtol=1e-4, atol=1e-4)


def test_captured_step_replays_the_fused_launch(bf16x2_mode: None, lib_loaded: None) -> None:
    """``test_captured_train_step_matches_eager`` on the bench's frame shapes (B = 2, T = 3), whose encoders take the fused stem:
    same learning rate, seed and criteria."""
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import _lib, scan
    from multimodal_mtrssm_amd.graph import CapturedTrainStep
    from multimodal_mtrssm_amd.optim import FlatParameters
    from oracle.cases import CASES, build_batch, build_model, with_sizes
    from tests.conftest import product_from_case

    case = with_sizes(CASES["mrssm_bench"], 2, 3)
    oracle = build_model(case)
    batch = tuple(b.to(DEV) for b in build_batch(case))
    results = {}
    for mode in ("eager", "graph"):
        model = product_from_case(case, oracle, DEV)
        flat = FlatParameters(model, extra=8)
        dp = mt.FlatDataParallel(flat)
        opt = mt.FlatAdamW(flat, lr=1e-5, clip_norm=10.0)
        source = dp.noise_source(seed=11)
        shapes = model.noise_shapes(2, 3)
        losses = []
        if mode == "eager":
            for step in range(5):
                noise = source.draw(shapes)
                opt.zero_grad()
                if step == 0:
                    _lib.TIMERS.enable()
                try:
                    out = model.shared_step(batch, noise)
                    if step == 0:
                        assert any("encoder_stem_kernel" in k for k in _lib.TIMERS.summary())
                finally:
                    _lib.TIMERS.disable()
                out["loss"].backward()
                dp.sync({k: out[k] for k in out})
                opt.step(grad_scale=dp.grad_scale)
                losses.append(float(out["loss"]))
        else:
            cap = CapturedTrainStep(model, flat, opt, dp, batch, source, warmup=3)
            for _ in range(5):
                losses.append(float(cap.step()["loss"]))
            assert opt.steps == 5  # noqa: PLR2004
            cap.close()
        scan.check_cluster_status()
        results[mode] = (losses, flat.param.clone())
    np.testing.assert_allclose(results["graph"][0], results["eager"][0], rtol=1e-4)
    diff = (results["graph"][1] - results["eager"][1]).abs()
    assert float(diff.max()) < 2e-4 and float(diff.mean()) < 2e-7, (float(diff.max()), float(diff.mean()))  # noqa: PLR2004
