"""CPU: what the fused encoder stem (``mtrssm_encoder_stem_fwd``) takes and what it leaves to the per-layer path.

``mtrssm_encoder_stem_supported`` is a host-side query of the shape fields; ``conv._stem_desc`` adds the Python-side conditions
(three k3 s2 p1 layers, coordinate planes, contiguous tensors, the switch).  Nothing is launched here.
"""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from multimodal_mtrssm_amd import _lib, conv


def _desc(**kw: int) -> C.Structure:
    p = _lib.EncoderStem()
    fields = {"N": 3200, "C": 1, "C2": 2, "Hs": 64, "Ws": 64, "Cout1": 8, "Cout2": 16, "Cout3": 32, "act": 2, "mfma_split": 2}
    fields.update(kw)
    for k, v in fields.items():
        setattr(p, k, v)
    return p


def test_supported_shapes_and_refusals() -> None:
    lib = _lib.load()
    ok = lib.mtrssm_encoder_stem_supported
    assert ok(C.byref(_desc())) == 1
    assert ok(C.byref(_desc(Hs=128, Ws=32))) == 1
    assert ok(C.byref(_desc(act=0))) == 1 and ok(C.byref(_desc(act=1))) == 1
    assert ok(None) == 0
    assert ok(C.byref(_desc(mfma_split=3))) == 0 and ok(C.byref(_desc(mfma_split=0))) == 0   # bf16x3, f32
    assert ok(C.byref(_desc(Hs=32, Ws=32))) == 0 and ok(C.byref(_desc(Hs=32, Ws=128))) == 0   # other planes
    assert ok(C.byref(_desc(C=2))) == 0 and ok(C.byref(_desc(C2=0))) == 0                     # 4 input channels; no coordinate planes
    assert ok(C.byref(_desc(Cout1=16))) == 0 and ok(C.byref(_desc(Cout3=64))) == 0
    assert ok(C.byref(_desc(act=3))) == 0 and ok(C.byref(_desc(act=7))) == 0                  # Tanh: not staged by the band recipe
    assert ok(C.byref(_desc(N=0))) == 0 and ok(C.byref(_desc(N=1 << 18))) == 0                # y1 index range: N * 8192 < 2^31
    # the launch refuses what the query refuses, and null pointers, before anything is enqueued
    assert lib.mtrssm_encoder_stem_fwd(C.byref(_desc(Hs=32, Ws=32)), None, None) == -1
    assert b"encoder_stem" in lib.mtrssm_last_error()
    assert lib.mtrssm_encoder_stem_fwd(C.byref(_desc()), None, None) == -1 and b"null" in lib.mtrssm_last_error()
    assert lib.mtrssm_encoder_stem_fwd(None, None, None) == -1


def _layers(cin: int = 3, k: int = 3, stride: int = 2, chans: tuple = (8, 16, 32)) -> list[tuple]:
    out = []
    for co in chans:
        out.append((torch.zeros(co, cin, k, k), torch.zeros(co), stride, 1))
        cin = co
    return out


def test_python_side_conditions(monkeypatch: pytest.MonkeyPatch) -> None:
    x, cc = torch.zeros(3, 1, 64, 64), torch.zeros(2, 64, 64)
    monkeypatch.setattr(conv, "ENCODER_STEM", True)
    monkeypatch.setattr(conv, "_MFMA_SPLIT", 2)
    d = conv._stem_desc(x, cc, _layers(), 2)  # noqa: SLF001
    assert d is not None and (d.N, d.C, d.C2, d.Hs, d.Ws, d.Cout1, d.Cout2, d.Cout3, d.act, d.mfma_split) == (3, 1, 2, 64, 64, 8, 16, 32, 2, 2)
    assert conv._stem_desc(torch.zeros(3, 1, 128, 32), torch.zeros(2, 128, 32), _layers(), 2) is not None  # noqa: SLF001
    assert conv._stem_desc(x, None, _layers(cin=1), 2) is None  # noqa: SLF001
    assert conv._stem_desc(torch.zeros(3, 1, 32, 32), torch.zeros(2, 32, 32), _layers(), 2) is None  # noqa: SLF001
    assert conv._stem_desc(torch.zeros(3, 2, 64, 64), cc, _layers(cin=4), 2) is None  # noqa: SLF001
    assert conv._stem_desc(x, cc, _layers(k=4), 2) is None  # noqa: SLF001
    assert conv._stem_desc(x, cc, _layers(stride=1), 2) is None  # noqa: SLF001
    assert conv._stem_desc(x, cc, _layers()[:2], 2) is None  # noqa: SLF001
    assert conv._stem_desc(x, cc, _layers(chans=(8, 16, 64)), 2) is None  # noqa: SLF001
    assert conv._stem_desc(x.transpose(2, 3), cc, _layers(), 2) is None  # noqa: SLF001
    assert conv._stem_desc(x, cc, _layers(), 3) is None  # noqa: SLF001
    for split in (3, 0):  # bf16x3, f32
        monkeypatch.setattr(conv, "_MFMA_SPLIT", split)
        assert conv._stem_desc(x, cc, _layers(), 2) is None  # noqa: SLF001
    monkeypatch.setattr(conv, "_MFMA_SPLIT", 2)
    monkeypatch.setattr(conv, "ENCODER_STEM", False)  # MTRSSM_ENCODER_STEM=0
    assert conv._stem_desc(x, cc, _layers(), 2) is None  # noqa: SLF001
    with conv.encoder_stem([(x, cc, _layers(), 2)]) as launched:  # host tensors: the per-layer path, nothing launched
        assert launched is False
