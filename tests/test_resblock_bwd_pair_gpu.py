"""The residual stacks' backward with the audio and the vision stack in ONE persistent grid: ``mtrssm_conv_weight_grad_pair``
(``conv3x3_wgrad_pair_resident_kernel<2, 64 | 32, 4, 8>``) and ``mtrssm_residual_bwd1x1_pair``
(``conv1x1_bwd_fused_pair_kernel<128 | 64>``), ``bf16x2``, ELU, planes 16x4 (audio) and 8x8 (vision).

Frame counts ``(Na, Nv)``: one frame each; fewer frames than x blocks, uneven; and one pair above a modality's x-block count
(taken from the device's CU count) so that workgroups hold runs of different lengths, the last one a short run.

Tolerances.  Paired against one launch per modality (same pieces, same products, the partial sums regrouped): the A/B
tolerance of ``tests/test_resblock_bwd1x1_gpu.py``, ``rtol=2e-5, atol=3e-6 * max|ref|`` (``g_h`` of the 1x1 call: bit-equal).
Against float64 on the host: that file's ``rtol=1e-4, atol=4e-5 * max|ref|``.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ELU = 2  # _lib.ACT_IDS
PLANE_A, PLANE_V = (16, 4), (8, 8)


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _blocks(per_cu: int = 1) -> int:
    """x blocks of one modality in a paired grid for one co group."""
    return max(1, per_cu * torch.cuda.get_device_properties(0).multi_processor_count // 2)


def _frame_pairs(blocks: int) -> list[tuple[int, int]]:
    return [(1, 1), (3, 5), (7, 2), (2 * blocks + 3, blocks + 2)]


def _close_ab(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    print(f"A/B {what}: max |diff| {float((got - ref).abs().max()):.3e} of max |ref| {float(ref.abs().max()):.3e}")
    np.testing.assert_allclose(_np(got), _np(ref), rtol=2e-5, atol=3e-6 * float(ref.abs().max()), err_msg=what)


def _close_f64(got: torch.Tensor, ref: torch.Tensor, what: str) -> None:
    print(f"float64 {what}: max |diff| {float((got.double().cpu() - ref).abs().max()):.3e} of max |ref| {float(ref.abs().max()):.3e}")
    np.testing.assert_allclose(_np(got), ref.numpy(), rtol=1e-4, atol=4e-5 * float(ref.abs().max()), err_msg=f"float64 {what}")


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
# 3x3 weight gradient


def _wgrad3_f64(a: torch.Tensor, src: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """dW[o][i][ky][kx] = sum a[n,o,y,x] elu(src)[n,i,y+ky-1,x+kx-1], db[o] = sum a -- float64 on the host."""
    import torch.nn.functional as F  # noqa: N812

    a64, s64 = a.double().cpu(), F.elu(src.double().cpu())
    w = torch.zeros(a.shape[1], src.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(s64, w, None, 1, 1) * a64).sum().backward()
    return w.grad, a64.sum((0, 2, 3))


@pytest.mark.parametrize(("cin", "cout"), [(64, 64), (64, 128), (32, 64)])
def test_paired_3x3_weight_grad_matches_single_launches_and_float64(lib_loaded: None, cin: int, cout: int) -> None:
    from multimodal_mtrssm_amd import conv

    blocks = _blocks(2 if cin == 32 else 1) // (cout // 64)  # noqa: PLR2004
    gen = torch.Generator(device="cpu").manual_seed(100 + cin + cout)
    name = f"mtrssm::conv3x3_wgrad_pair_resident_kernel<2, {cin}, 4, 8>"
    for na, nv in _frame_pairs(blocks):
        def side(n: int, plane: tuple[int, int]) -> tuple:
            a = torch.randn(n, cout, *plane, generator=gen).to(DEV)
            src = torch.randn(n, cin, *plane, generator=gen).to(DEV)
            return (a, src, torch.zeros(cout, cin, 3, 3, device=DEV), torch.zeros(cout, device=DEV))  # (weights without a flat home)

        sa, sv = side(na, PLANE_A), side(nv, PLANE_V)
        (pa, pv), k_pair = _timed(lambda: conv._weight_grad_pair(sa, sv, 1, ELU))  # noqa: SLF001, B023
        (pv2, pa2), k_swap = _timed(lambda: conv._weight_grad_pair(sv, sa, 1, ELU))  # noqa: SLF001, B023  (8-wide plane first)
        singles, k_single = _timed(lambda: (conv._weight_grad_single(sa, 1, ELU), conv._weight_grad_single(sv, 1, ELU)))  # noqa: SLF001, B023
        torch.cuda.synchronize()
        assert k_pair == [name] and k_swap == [name], (k_pair, k_swap)
        assert all("conv3x3_wgrad_resident_kernel<2" in k for k in k_single) and len(k_single) == 2, k_single  # noqa: PLR2004
        for tag, s, got, swapped, one in (("audio", sa, pa, pa2, singles[0]), ("vision", sv, pv, pv2, singles[1])):
            w64, b64 = _wgrad3_f64(s[0], s[1])
            for what, g, g2, r, r64 in (("dW", got[0], swapped[0], one[0], w64), ("db", got[1], swapped[1], one[1], b64)):
                label = f"{cin}->{cout} N=({na}, {nv}) {tag} {what}"
                assert torch.equal(g.contiguous(), g2.contiguous()), f"{label}: the order of the two problems changed the result"
                _close_ab(g, r, label)
                _close_f64(g, r64, label)


def test_paired_3x3_weight_grad_atomics_and_deferred_forms(lib_loaded: None) -> None:
    """No workspace: fp32 atomics per problem (also: only ONE problem without workspace).  defer = 1: nothing is summed until
    ``mtrssm_conv_weight_grad_reduce``."""
    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()
    gen = torch.Generator(device="cpu").manual_seed(5)
    na, nv, c = 7, _blocks() + 2, 64
    sides = []
    for n, plane in ((na, PLANE_A), (nv, PLANE_V)):
        a = torch.randn(n, c, *plane, generator=gen).to(DEV)
        src = torch.randn(n, c, *plane, generator=gen).to(DEV)
        geom = conv._geom(N=n, C=c, Hs=plane[0], Ws=plane[1], C2=0, Cpad=c, KH=3, KW=3, SS=1, TS=1, OFFY=-1, OFFX=-1, Hq=plane[0],  # noqa: SLF001
                          Wq=plane[1], OS=1, QY=0, QX=0, Ho=plane[0], Wo=plane[1], Cout=c, CoutPad=c, pre_act=1, act=ELU)
        need = int(lib.mtrssm_conv_weight_grad_workspace_bytes(C.byref(geom), 0))
        assert need > 0
        sides.append((geom, a, src, need, *_wgrad3_f64(a, src)))
    assert lib.mtrssm_conv_weight_grad_pair_supported(C.byref(sides[0][0]), C.byref(sides[1][0])) == 1

    def run(ws_a: bool, ws_v: bool, defer: int) -> list[tuple[torch.Tensor, torch.Tensor]]:  # noqa: FBT001
        args: list = []
        outs = []
        keep = []
        for (geom, a, src, need, _, _), with_ws in zip(sides, (ws_a, ws_v), strict=True):
            dwp, db = torch.zeros(c, 9, c, device=DEV), torch.zeros(c, device=DEV)
            ws = torch.empty(need // 4 + 64, device=DEV) if with_ws else None
            keep.append(ws)
            outs.append((dwp, db))
            args += [C.byref(geom), _lib.ptr(a), _lib.ptr(src), _lib.ptr(dwp), _lib.ptr(db), _lib.raw_ptr(ws), 0 if ws is None else ws.numel() * 4]
        _lib.check(lib.mtrssm_conv_weight_grad_pair(*args, defer, _lib.stream_ptr(torch.device(DEV))), "mtrssm_conv_weight_grad_pair")
        if defer:
            torch.cuda.synchronize()
            assert all(float(dwp.abs().max()) == 0.0 and float(db.abs().max()) == 0.0 for dwp, db in outs), "summed before the reduce"
            _lib.check(lib.mtrssm_conv_weight_grad_reduce(_lib.stream_ptr(torch.device(DEV))), "mtrssm_conv_weight_grad_reduce")
        torch.cuda.synchronize()
        return outs

    sets = run(True, True, 0)
    for form, got in (("atomics", run(False, False, 0)), ("atomics + sets", run(False, True, 0)), ("deferred", run(True, True, 1))):
        for (_, _, _, _, w64, b64), (dwp, db), (dwp_s, db_s), tag in zip(sides, got, sets, ("audio", "vision"), strict=True):
            if form == "deferred":
                assert torch.equal(dwp, dwp_s) and torch.equal(db, db_s), f"{tag}: the deferred sum differs from the immediate one"
            _close_ab(dwp, dwp_s, f"{form} {tag} dW")
            _close_ab(db, db_s, f"{form} {tag} db")
            _close_f64(dwp.view(c, 3, 3, c).permute(0, 3, 1, 2), w64, f"{form} {tag} dW")
            _close_f64(db, b64, f"{form} {tag} db")


def test_paired_queries_refuse_other_shapes(lib_loaded: None) -> None:
    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()

    def g3(c: int, plane: tuple, cout: int = 64, split: int = 2, n: int = 6) -> C.Structure:
        g = conv._geom(N=n, C=c, Hs=plane[0], Ws=plane[1], C2=0, Cpad=c, KH=3, KW=3, SS=1, TS=1, OFFY=-1, OFFX=-1, Hq=plane[0], Wq=plane[1],  # noqa: SLF001
                       OS=1, QY=0, QX=0, Ho=plane[0], Wo=plane[1], Cout=cout, CoutPad=cout, pre_act=1, act=ELU)
        g.mfma_split = split
        return g

    def g1(c: int, plane: tuple) -> C.Structure:
        return conv._geom(N=6, C=c, Hs=plane[0], Ws=plane[1], C2=0, Cpad=c, KH=1, KW=1, SS=1, TS=1, OFFY=0, OFFX=0, Hq=plane[0], Wq=plane[1],  # noqa: SLF001
                          OS=1, QY=0, QX=0, Ho=plane[0], Wo=plane[1], Cout=64, CoutPad=64, pre_act=1, act=ELU)

    def q3(a: C.Structure, b: C.Structure) -> int:
        return lib.mtrssm_conv_weight_grad_pair_supported(C.byref(a), C.byref(b))

    for c in (64, 32):
        assert q3(g3(c, PLANE_A), g3(c, PLANE_V)) == 1 and q3(g3(c, PLANE_V), g3(c, PLANE_A, n=9)) == 1
    assert q3(g3(64, PLANE_V), g3(64, PLANE_V)) == 0        # two 8-wide planes: no instantiation
    assert q3(g3(64, PLANE_A), g3(32, PLANE_V)) == 0        # different layers
    assert q3(g3(64, PLANE_A), g3(64, PLANE_V, cout=128)) == 0
    assert q3(g3(64, PLANE_A, split=1), g3(64, PLANE_V, split=1)) == 0
    assert lib.mtrssm_conv_weight_grad_pair(C.byref(g3(64, PLANE_V)), *([None] * 5), 0, C.byref(g3(64, PLANE_V)), *([None] * 5), 0, 0, None) == -1
    assert b"conv_weight_grad_pair" in lib.mtrssm_last_error()
    for c in (64, 128):
        assert lib.mtrssm_residual_bwd1x1_pair_supported(C.byref(g1(c, PLANE_A)), C.byref(g1(c, PLANE_V))) == 1
        assert lib.mtrssm_residual_bwd1x1_pair_supported(C.byref(g1(c, PLANE_V)), C.byref(g1(c, PLANE_V))) == 1
    assert lib.mtrssm_residual_bwd1x1_pair_supported(C.byref(g1(64, PLANE_A)), C.byref(g1(128, PLANE_V))) == 0
    assert lib.mtrssm_residual_bwd1x1_pair_supported(C.byref(g1(32, PLANE_A)), C.byref(g1(32, PLANE_V))) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 1x1 backward


@pytest.mark.parametrize("mid", [128, 64])
def test_paired_1x1_backward_matches_single_launches_and_float64(lib_loaded: None, mid: int) -> None:
    """Library level, fresh buffers: sets summed on the spot, the atomics form (no workspace) and the deferred form."""
    import torch.nn.functional as F  # noqa: N812

    from multimodal_mtrssm_amd import _lib, conv

    lib = _lib.load()
    stream = _lib.stream_ptr(torch.device(DEV))
    gen = torch.Generator(device="cpu").manual_seed(30 + mid)
    for na, nv in _frame_pairs(_blocks()):
        sides = []
        for n, plane in ((na, PLANE_A), (nv, PLANE_V)):
            gy = torch.randn(n, 64, *plane, generator=gen).to(DEV)
            h = torch.randn(n, mid, *plane, generator=gen).to(DEV)
            w1 = (torch.randn(64, mid, 1, 1, generator=gen) * 0.1).to(DEV)
            geom = conv._bwd1x1_geom(gy, h, w1, ELU)  # noqa: SLF001
            assert geom is not None
            sides.append((geom, gy, h, w1, int(lib.mtrssm_conv_weight_grad_workspace_bytes(C.byref(geom), 0))))
        assert lib.mtrssm_residual_bwd1x1_pair_supported(C.byref(sides[0][0]), C.byref(sides[1][0])) == 1

        def run(paired: bool, with_ws: bool = True, defer: int = 0) -> tuple[list, str]:  # noqa: FBT001, FBT002
            outs, args, keep = [], [], []
            conv.invalidate_packs()
            for k, (geom, gy, h, w1, need) in enumerate(sides):  # noqa: B023
                _, wq1t = conv.pack_weight(w1.permute(1, 0, 2, 3), k)
                gh, dwp, db = torch.empty_like(h), torch.zeros(64, 1, geom.Cpad, device=DEV), torch.zeros(64, device=DEV)
                ws = torch.empty(need // 4 + 64, device=DEV) if with_ws else None
                keep.append((wq1t, ws))
                outs.append((gh, dwp, db))
                one = [C.byref(geom), _lib.ptr(gy), _lib.ptr(h), _lib.raw_ptr(wq1t), _lib.ptr(gh), _lib.ptr(dwp), _lib.ptr(db), _lib.raw_ptr(ws),
                       0 if ws is None else ws.numel() * 4]
                if paired:
                    args += one
                else:
                    _lib.check(lib.mtrssm_residual_bwd1x1(*one, 0, stream), "mtrssm_residual_bwd1x1")
            if paired:
                _lib.check(lib.mtrssm_residual_bwd1x1_pair(*args, defer, stream), "mtrssm_residual_bwd1x1_pair")
            kernel = lib.mtrssm_last_kernel().decode()
            if defer:
                torch.cuda.synchronize()
                assert all(float(dwp.abs().max()) == 0.0 for _, dwp, _ in outs), "summed before the reduce"
                _lib.check(lib.mtrssm_conv_weight_grad_reduce(stream), "mtrssm_conv_weight_grad_reduce")
            torch.cuda.synchronize()
            return outs, kernel

        single, k_single = run(False)
        pair, k_pair = run(True)
        assert k_pair == f"mtrssm::conv1x1_bwd_fused_pair_kernel<{mid}>", k_pair
        assert k_single == f"mtrssm::conv1x1_bwd_fused_kernel<{mid}>", k_single
        forms = [("sets", pair)]
        if (na, nv) == (7, 2):
            forms += [("atomics", run(True, with_ws=False)[0]), ("deferred", run(True, defer=1)[0])]
        for form, got in forms:
            for (geom, gy, h, w1, _), (gh, dwp, db), (gh1, dwp1, db1), tag in zip(sides, got, single, ("audio", "vision"), strict=True):
                label = f"C={mid} N=({na}, {nv}) {form} {tag}"
                assert torch.equal(gh, gh1), f"{label}: g_h is not bit-equal to the single launch's"
                _close_ab(dwp, dwp1, f"{label} dW1")
                _close_ab(db, db1, f"{label} db1")
                if form == "deferred":
                    assert torch.equal(dwp, pair[0 if tag == "audio" else 1][1]), f"{label}: the deferred sum differs from the immediate one"
                gy64, h64, w64 = gy.double().cpu(), h.double().cpu().requires_grad_(True), w1.double().cpu().requires_grad_(True)
                (F.conv2d(F.elu(h64), w64) * gy64).sum().backward()
                _close_f64(gh, h64.grad, f"{label} g_h")
                _close_f64(dwp[:, 0, :mid], w64.grad[:, :, 0, 0], f"{label} dW1")
                _close_f64(db, gy64.sum((0, 2, 3)), f"{label} db1")


# ---------------------------------------------------------------------------------------------------------------------
# the autograd node, end to end, gradients in the flat buffer (the train step's form: deferred sums)


class _TwoBlocks(torch.nn.Module):
    def __init__(self, mid: int, gen: torch.Generator) -> None:
        super().__init__()

        def p(*shape: int, scale: float) -> torch.nn.Parameter:
            return torch.nn.Parameter((torch.randn(*shape, generator=gen) * scale).to(DEV))

        for tag in ("a", "v"):
            setattr(self, f"w3{tag}", p(mid, 64, 3, 3, scale=0.05))
            setattr(self, f"b3{tag}", p(mid, scale=0.1))
            setattr(self, f"w1{tag}", p(64, mid, 1, 1, scale=0.1))
            setattr(self, f"b1{tag}", p(64, scale=0.1))

    def block(self, tag: str) -> tuple:
        return tuple(getattr(self, f"{n}{tag}") for n in ("w3", "b3", "w1", "b1"))


def _run_pair_block(mid: int, na: int, nv: int) -> dict:
    """``_PairResidualBlock`` forward and backward with the parameters in a flat buffer: paired launches, two ``_ResidualBlock``
    nodes, float64 on the host; the kernels of the paired backward."""
    import torch.nn.functional as F  # noqa: N812

    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import conv

    gen = torch.Generator(device="cpu").manual_seed(11 + mid)
    model = _TwoBlocks(mid, gen)
    flat = mt.optim.FlatParameters(model)
    xa = torch.randn(na, 64, *PLANE_A, generator=gen).to(DEV).requires_grad_(True)
    xv = torch.randn(nv, 64, *PLANE_V, generator=gen).to(DEV).requires_grad_(True)

    def run(pair: bool) -> tuple[list[torch.Tensor], list[str]]:  # noqa: FBT001
        conv.invalidate_packs()
        flat.grad_full.zero_()
        xa.grad = xv.grad = None
        if pair:
            ya, yv = conv.residual_block_pair(xa, model.block("a"), xv, model.block("v"), act=ELU)
        else:
            ya, yv = conv.residual_block(xa, *model.block("a"), act=ELU), conv.residual_block(xv, *model.block("v"), act=ELU)
        loss = ya.square().sum() + yv.sin().sum()
        _, kernels = _timed(loss.backward)
        torch.cuda.synchronize()
        return [ya.detach(), yv.detach(), xa.grad.clone(), xv.grad.clone(), *(p.grad.clone() for p in model.parameters())], kernels

    two, k_two = run(False)
    one, k_one = run(True)
    names = ["ya", "yv", "g_xa", "g_xv", *(n for n, _ in model.named_parameters())]
    cpu = [t.detach().double().cpu().requires_grad_(True) for t in (xa, xv, *model.parameters())]

    def ref(x: torch.Tensor, w3: torch.Tensor, b3: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor) -> torch.Tensor:
        return x + F.conv2d(F.elu(F.conv2d(F.elu(x), w3, b3, 1, 1)), w1, b1)

    by_name = dict(zip(["xa", "xv", *(n for n, _ in model.named_parameters())], cpu, strict=True))
    ya64 = ref(by_name["xa"], *(by_name[f"{n}a"] for n in ("w3", "b3", "w1", "b1")))
    yv64 = ref(by_name["xv"], *(by_name[f"{n}v"] for n in ("w3", "b3", "w1", "b1")))
    (ya64.square().sum() + yv64.sin().sum()).backward()
    f64 = [ya64.detach(), yv64.detach(), *(t.grad for t in cpu)]
    return {"names": names, "one": one, "two": two, "f64": f64, "k_one": k_one, "k_two": k_two}


@pytest.mark.parametrize(("mid", "na", "nv"), [(128, 3, 5), (64, 7, 2)])
def test_pair_residual_block_end_to_end(lib_loaded: None, mid: int, na: int, nv: int) -> None:
    r = _run_pair_block(mid, na, nv)
    assert "mtrssm::conv3x3_wgrad_pair_resident_kernel<2, 64, 4, 8>" in r["k_one"], r["k_one"]
    assert f"mtrssm::conv1x1_bwd_fused_pair_kernel<{mid}>" in r["k_one"], r["k_one"]
    assert not any("wgrad_resident_kernel" in k and "pair" not in k for k in r["k_one"]), r["k_one"]
    assert not any("pair_resident" in k or "fused_pair" in k for k in r["k_two"]), r["k_two"]
    for name, a, b, c in zip(r["names"], r["one"], r["two"], r["f64"], strict=True):
        _close_ab(a, b, name)
        _close_f64(a, c, name)


_WORKER = """
import sys, json
sys.path.insert(0, {root!r})
from tests.test_resblock_bwd_pair_gpu import _run_pair_block
r = _run_pair_block(128, 3, 5)
print("KERNELS " + json.dumps(r["k_one"]))
"""


def test_switch_off_takes_the_single_launches(lib_loaded: None) -> None:
    """``MTRSSM_PAIR_WGRAD=0`` (read once by the library, hence a process of its own): the same node, one launch per modality."""
    import json

    root = str(Path(__file__).resolve().parent.parent)
    env = dict(os.environ, MTRSSM_PAIR_WGRAD="0")
    out = subprocess.run([sys.executable, "-c", _WORKER.format(root=root)], env=env, capture_output=True, text=True, timeout=300, check=False)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels = json.loads(next(line for line in out.stdout.splitlines() if line.startswith("KERNELS "))[8:])
    assert "mtrssm::conv1x1_bwd_fused_kernel<128>" in kernels, kernels
    assert "mtrssm::conv3x3_wgrad_resident_kernel<2, 64, 4>" in kernels and "mtrssm::conv3x3_wgrad_resident_kernel<2, 64, 8>" in kernels, kernels
    assert not any("pair_resident" in k or "fused_pair" in k for k in kernels), kernels
