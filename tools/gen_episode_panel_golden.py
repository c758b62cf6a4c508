#!/usr/bin/env python3
"""Regenerate ``tests/golden/episode_panel.npz``: the bytes the reference's logging callback makes of seeded frames.

    python tools/gen_episode_panel_golden.py --reference <checkout of the reference project> [--out tests/golden/episode_panel.npz]

The reference's ``src/multimodal_rssm/models/mrssm/callback.py`` is imported by path at run time; nothing of it is copied here.  Its two
imports from its own package (``multimodal_rssm.models.callback``, ``.state``: the Lightning callback base and the state classes) are
stubbed in ``sys.modules`` -- the function that is run, ``LogMultimodalMRSSMOutput._process_multimodal_batch`` (the vision RGB path plus
the magma path), touches neither.  It needs matplotlib and PIL, as the reference does.  The frames are 1 x 8 x 8 in [-1, 1] for both
modalities (``b = 2``, ``t = 3``), denormalised as the callback does (``(v + 1.0) / 2.0`` in torch fp32) and laid side by side
``prior | observation | posterior``.  They contain a ramp that hits all 256 magma indices, every ``k / 255`` vision boundary and every
``k / 256`` magma boundary with its two fp32 neighbours, and -1, 0, 1.  The fixture holds the input arrays and the output bytes only.
"""

from __future__ import annotations

import argparse
import importlib.util
import sys
import types
from pathlib import Path

import numpy as np
import torch

B, T, SIDE = 2, 3, 8
KINDS = ("prior", "obs", "post")


def _stub(name: str, **attrs: object) -> None:
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        sub = ".".join(parts[:i])
        if sub not in sys.modules:
            mod = types.ModuleType(sub)
            mod.__path__ = []  # type: ignore[attr-defined]
            sys.modules[sub] = mod
    for k, v in attrs.items():
        setattr(sys.modules[name], k, v)


def load_reference(root: Path) -> types.ModuleType:
    _stub("multimodal_rssm.models.callback", RGB_CHANNELS=3, BaseLogRSSMOutput=object)
    _stub("multimodal_rssm.models.state", State=object, cat_states=None)
    path = root / "src" / "multimodal_rssm" / "models" / "mrssm" / "callback.py"
    spec = importlib.util.spec_from_file_location("reference_mrssm_callback", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)  # type: ignore[union-attr]
    return module


def boundaries(levels: int) -> np.ndarray:
    """fp32 ``v`` around every ``x = k / levels`` boundary of ``x = (v + 1) / 2``: the value and its two fp32 neighbours."""
    x = np.arange(levels + 1, dtype=np.float32) / np.float32(levels)
    v = x * np.float32(2.0) - np.float32(1.0)
    return np.concatenate([np.nextafter(v, np.float32(-2.0)), v, np.nextafter(v, np.float32(2.0))]).astype(np.float32)


def seeded_frames(rng: np.random.Generator, special: np.ndarray) -> dict[str, np.ndarray]:
    """Three ``[B, T, 1, 8, 8]`` arrays in [-1, 1]: ``special`` first, the rest uniform."""
    total = len(KINDS) * B * T * SIDE * SIDE
    if len(special) > total:
        msg = f"{len(special)} special values do not fit {total} elements"
        raise ValueError(msg)
    flat = rng.uniform(-1.0, 1.0, size=total).astype(np.float32)
    flat[: len(special)] = special
    flat = np.clip(flat, np.float32(-1.0), np.float32(1.0))
    parts = flat.reshape(len(KINDS), B, T, 1, SIDE, SIDE)
    return {k: parts[i] for i, k in enumerate(KINDS)}


def main() -> None:
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--reference", type=Path, required=True, help="root of the reference project's checkout")
    parser.add_argument("--out", type=Path, default=Path(__file__).resolve().parents[1] / "tests" / "golden" / "episode_panel.npz")
    args = parser.parse_args()
    ref = load_reference(args.reference.resolve())
    rng = np.random.default_rng(20240611)
    edge = np.asarray([-1.0, 0.0, 1.0], dtype=np.float32)
    ramp = ((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256.0)) * np.float32(2.0) - np.float32(1.0)
    vision = seeded_frames(rng, np.concatenate([edge, boundaries(255)]))
    audio = seeded_frames(rng, np.concatenate([edge, ramp, boundaries(256)]))

    def side_by_side(frames: dict[str, np.ndarray]) -> np.ndarray:  # the callback's denormalisation and horizontal cat
        return torch.cat([(torch.from_numpy(frames[k]) + 1.0) / 2.0 for k in KINDS], dim=4).numpy()

    params = {"b": B, "t": T, "c": 1, "vision_h": SIDE, "audio_h": SIDE, "w": len(KINDS) * SIDE}
    rgb = ref.LogMultimodalMRSSMOutput._process_multimodal_batch(side_by_side(vision), side_by_side(audio), params)  # noqa: SLF001
    assert rgb.dtype == np.uint8 and rgb.shape == (B, T, 3, 2 * SIDE, len(KINDS) * SIDE), (rgb.dtype, rgb.shape)
    out = {f"{k}_v": vision[k] for k in KINDS} | {f"{k}_a": audio[k] for k in KINDS} | {"rgb": rgb}
    args.out.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({args.out.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
