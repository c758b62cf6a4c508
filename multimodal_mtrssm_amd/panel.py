"""Episode panels: the video ``prior | observation | posterior`` of chosen episodes from one kernel.

The reference's logging callback (``models/callback.py``, ``mrssm/callback.py``) decodes a closed-loop and an open-loop rollout and then
composes every frame on the host: numpy per frame, a matplotlib colormap call per frame, PIL per frame.  Here the decodes sit on the
device as fp32 ``[N, T, C, H, W]`` and the whole composition is one pass of byte-producing arithmetic (``mtrssm_episode_panel``).

The pixel rule (fp32, in this order; the reference's bytes exactly):

    x     = min(max((v + 1) / 2, 0), 1)                       v in [-1, 1]: a target frame or a decoder's activated output; NaN -> 0
    vision byte = trunc(x * 255)                                  C = 1 replicated to RGB, C = 3 as is
    audio (channel 0):  n = x * 2 - 1;  db = (n + 1) / 2 * 80 - 80;  s = clamp((clamp(db, -80, 0) - (-80)) / 80, 0, 1)
                        rgb = MAGMA[min(trunc(s * 256), 255)]
    error column:       e = |prior01 - observation01|  (C = 3: ((e0 + e1) + e2) / 3);  rgb = MAGMA[min(trunc(e * 256), 255)]

The canvas (this package's own; the reference assumes equal frame sizes): with ``s = scale``, ``cw = max(Wv, Wa) s``, ``J`` columns,
``g = gap``, ``r = bar``: ``Wc = J cw + (J - 1) g``, ``Hc = r + Hv s + g + Ha s``; cell (vision, j) starts at ``(r, j (cw + g))``, cell
(audio, j) at ``(r + Hv s + g, j (cw + g))``; a frame is drawn left-aligned by nearest neighbour, the rest of its cell is 0 (the
reference's zero padding).  Gap pixels are (64, 64, 64).  The ``r`` top rows are a phase bar over the full width: (0, 160, 0) while
``t < context[n]`` (the model sees observations), (255, 140, 0) from there on (the prior runs open loop).  With ``blank_unseen`` the
observation cell of a modality the model does not see at that step is black; frames at or past a row's end are black altogether.  The
frame number ``frame0 + t`` is drawn last in a 3 x 5 font (``FONT``) of ``label`` x ``label`` pixels, white on a black box at (0, 0).

``EpisodePanel.reference`` states all of it in torch on any device; ``EpisodePanel.render`` is the kernel, used for GPU tensors.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from pathlib import Path
from typing import Any

import numpy as np
import torch
from torch import Tensor

from multimodal_mtrssm_amd import _lib
from multimodal_mtrssm_amd.skill import OBSERVE_BITS, ObservingConfig

COLUMNS = ("prior", "observation", "posterior", "error")
GAP_COLOUR = (64, 64, 64)
BAR_CONTEXT = (0, 160, 0)
BAR_OPEN = (255, 140, 0)
MAX_EPISODES = 60  # the reference's callbacks look at the first 60 episodes of a loader only (models/callback.py:14)
_LIMITS = {"scale": (1, 64), "gap": (0, 64), "bar": (0, 64), "label": (0, 16)}  # the kernel's (include/mtrssm.h)
_MAX_CANVAS = 32768

# the frame number's digits: five rows top to bottom, three bits each, left to right
FONT = (
    "111 101 101 101 111",
    "010 110 010 010 111",
    "111 001 111 100 111",
    "111 001 111 001 111",
    "101 101 111 001 001",
    "111 100 111 001 111",
    "111 100 111 101 111",
    "111 001 001 001 001",
    "111 101 111 101 111",
    "111 101 111 001 111",
)

# trunc(matplotlib magma(k)[:3] * 255), k = 0 .. 255 (matplotlib's data; it is not imported here)
MAGMA = np.array([
    0, 0, 3, 0, 0, 4, 0, 0, 6, 1, 0, 7, 1, 1, 9, 1, 1, 11, 2, 2, 13, 2, 2, 15,
    3, 3, 17, 4, 3, 19, 4, 4, 21, 5, 4, 23, 6, 5, 25, 7, 5, 27, 8, 6, 29, 9, 7, 31,
    10, 7, 34, 11, 8, 36, 12, 9, 38, 13, 10, 40, 14, 10, 42, 15, 11, 44, 16, 12, 47, 17, 12, 49,
    18, 13, 51, 20, 13, 53, 21, 14, 56, 22, 14, 58, 23, 15, 60, 24, 15, 63, 26, 16, 65, 27, 16, 68,
    28, 16, 70, 30, 16, 73, 31, 17, 75, 32, 17, 77, 34, 17, 80, 35, 17, 82, 37, 17, 85, 38, 17, 87,
    40, 17, 89, 42, 17, 92, 43, 17, 94, 45, 16, 96, 47, 16, 98, 48, 16, 101, 50, 16, 103, 52, 16, 104,
    53, 15, 106, 55, 15, 108, 57, 15, 110, 59, 15, 111, 60, 15, 113, 62, 15, 114, 64, 15, 115, 66, 15, 116,
    67, 15, 117, 69, 15, 118, 71, 15, 119, 72, 16, 120, 74, 16, 121, 75, 16, 121, 77, 17, 122, 79, 17, 123,
    80, 18, 123, 82, 18, 124, 83, 19, 124, 85, 19, 125, 87, 20, 125, 88, 21, 126, 90, 21, 126, 91, 22, 126,
    93, 23, 126, 94, 23, 127, 96, 24, 127, 97, 24, 127, 99, 25, 127, 101, 26, 128, 102, 26, 128, 104, 27, 128,
    105, 28, 128, 107, 28, 128, 108, 29, 128, 110, 30, 129, 111, 30, 129, 113, 31, 129, 115, 31, 129, 116, 32, 129,
    118, 33, 129, 119, 33, 129, 121, 34, 129, 122, 34, 129, 124, 35, 129, 126, 36, 129, 127, 36, 129, 129, 37, 129,
    130, 37, 129, 132, 38, 129, 133, 38, 129, 135, 39, 129, 137, 40, 129, 138, 40, 129, 140, 41, 128, 141, 41, 128,
    143, 42, 128, 145, 42, 128, 146, 43, 128, 148, 43, 128, 149, 44, 128, 151, 44, 127, 153, 45, 127, 154, 45, 127,
    156, 46, 127, 158, 46, 126, 159, 47, 126, 161, 47, 126, 163, 48, 126, 164, 48, 125, 166, 49, 125, 167, 49, 125,
    169, 50, 124, 171, 51, 124, 172, 51, 123, 174, 52, 123, 176, 52, 123, 177, 53, 122, 179, 53, 122, 181, 54, 121,
    182, 54, 121, 184, 55, 120, 185, 55, 120, 187, 56, 119, 189, 57, 119, 190, 57, 118, 192, 58, 117, 194, 58, 117,
    195, 59, 116, 197, 60, 116, 198, 60, 115, 200, 61, 114, 202, 62, 114, 203, 62, 113, 205, 63, 112, 206, 64, 112,
    208, 65, 111, 209, 66, 110, 211, 66, 109, 212, 67, 109, 214, 68, 108, 215, 69, 107, 217, 70, 106, 218, 71, 105,
    220, 72, 105, 221, 73, 104, 222, 74, 103, 224, 75, 102, 225, 76, 102, 226, 77, 101, 228, 78, 100, 229, 80, 99,
    230, 81, 98, 231, 82, 98, 232, 84, 97, 234, 85, 96, 235, 86, 96, 236, 88, 95, 237, 89, 95, 238, 91, 94,
    238, 93, 93, 239, 94, 93, 240, 96, 93, 241, 97, 92, 242, 99, 92, 243, 101, 92, 243, 103, 91, 244, 104, 91,
    245, 106, 91, 245, 108, 91, 246, 110, 91, 246, 112, 91, 247, 113, 91, 247, 115, 92, 248, 117, 92, 248, 119, 92,
    249, 121, 92, 249, 123, 93, 249, 125, 93, 250, 127, 94, 250, 128, 94, 250, 130, 95, 251, 132, 96, 251, 134, 96,
    251, 136, 97, 251, 138, 98, 252, 140, 99, 252, 142, 99, 252, 144, 100, 252, 146, 101, 252, 147, 102, 253, 149, 103,
    253, 151, 104, 253, 153, 105, 253, 155, 106, 253, 157, 107, 253, 159, 108, 253, 161, 110, 253, 162, 111, 253, 164, 112,
    254, 166, 113, 254, 168, 115, 254, 170, 116, 254, 172, 117, 254, 174, 118, 254, 175, 120, 254, 177, 121, 254, 179, 123,
    254, 181, 124, 254, 183, 125, 254, 185, 127, 254, 187, 128, 254, 188, 130, 254, 190, 131, 254, 192, 133, 254, 194, 134,
    254, 196, 136, 254, 198, 137, 254, 199, 139, 254, 201, 141, 254, 203, 142, 253, 205, 144, 253, 207, 146, 253, 209, 147,
    253, 210, 149, 253, 212, 151, 253, 214, 152, 253, 216, 154, 253, 218, 156, 253, 220, 157, 253, 221, 159, 253, 223, 161,
    253, 225, 163, 252, 227, 165, 252, 229, 166, 252, 230, 168, 252, 232, 170, 252, 234, 172, 252, 236, 174, 252, 238, 176,
    252, 240, 177, 252, 241, 179, 252, 243, 181, 252, 245, 183, 251, 247, 185, 251, 249, 187, 251, 250, 189, 251, 252, 191,
], dtype=np.uint8).reshape(256, 3)
MAGMA.setflags(write=False)


def _whole(name: str, value: object, lo: int, hi: int) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
        msg = f"{name} must be an integer in {lo} .. {hi}, got {value!r}"
        raise ValueError(msg)
    return value


def _frame_chw(name: str, chw: tuple[int, int, int]) -> tuple[int, int, int]:
    chw = tuple(int(v) for v in chw)
    if len(chw) != 3 or min(chw) < 1:  # noqa: PLR2004
        msg = f"{name} frames are (C, H, W) with positive sizes, got {chw}"
        raise ValueError(msg)
    return chw  # type: ignore[return-value]


class EpisodePanel(ObservingConfig):
    """``EpisodePanel(q, observe=..., columns=..., scale=2, gap=1, bar=2, label=1, blank_unseen=True)``: the model observes ``q >= 1``
    frames (of ``observe``: both modalities, audio only or vision only) and then the prior runs open loop; ``columns`` is a choice of
    ``"prior"``, ``"observation"``, ``"posterior"`` and ``"error"`` (|prior - observation| through magma) without repeats, left to right.
    ``max_frames``: the decoders run over chunks of whole rows of at most this many frames."""

    def __init__(self, query_length: int, observe: str = "both", columns: tuple[str, ...] = ("prior", "observation", "posterior"),  # noqa: PLR0913
                 scale: int = 2, gap: int = 1, bar: int = 2, label: int = 1, blank_unseen: bool = True) -> None:  # noqa: FBT001, FBT002
        if isinstance(query_length, bool) or not isinstance(query_length, int) or not 1 <= query_length < 1 << 31:
            msg = f"query_length must be an integer 1 <= q < 2^31 (frame 0 is always observed), got {query_length!r}"
            raise ValueError(msg)
        if observe not in OBSERVE_BITS:
            msg = f"observe must be one of {sorted(OBSERVE_BITS)}, got {observe!r}"
            raise ValueError(msg)
        if isinstance(columns, str) or not 1 <= len(tuple(columns)) <= len(COLUMNS) or any(c not in COLUMNS for c in columns) \
                or len(set(columns)) != len(tuple(columns)):
            msg = f"columns must be one to four of {COLUMNS} without repeats, got {columns!r}"
            raise ValueError(msg)
        if not isinstance(blank_unseen, bool):
            msg = f"blank_unseen must be a bool, got {blank_unseen!r}"
            raise ValueError(msg)
        self.query_length, self.observe, self.columns = query_length, observe, tuple(columns)
        self.scale = _whole("scale", scale, *_LIMITS["scale"])
        self.gap = _whole("gap", gap, *_LIMITS["gap"])
        self.bar = _whole("bar", bar, *_LIMITS["bar"])
        self.label = _whole("label", label, *_LIMITS["label"])
        self.blank_unseen = blank_unseen
        self.max_frames = 4096

    def __repr__(self) -> str:
        return (f"EpisodePanel({self.query_length}, observe={self.observe!r}, columns={self.columns!r}, scale={self.scale}, gap={self.gap}, "
                f"bar={self.bar}, label={self.label}, blank_unseen={self.blank_unseen})")

    @property
    def context(self) -> int:
        return self.query_length

    def plan(self):  # noqa: ANN201
        """Two copies of a row in copy order: rows ``[0, N)`` observe every live frame (the posterior), rows ``[N, 2 N)`` the first
        ``query_length`` (the prior); both share the row's uniforms, so they agree bit for bit on the context."""
        from multimodal_mtrssm_amd.evaluation import CopyPlan  # noqa: PLC0415  (evaluation imports this module)

        return CopyPlan(2, self.bits, (None, self.query_length), order="copy")

    # -- geometry ----------------------------------------------------------------------------------------------------------------------
    def shape(self, audio_chw: tuple[int, int, int], vision_chw: tuple[int, int, int]) -> tuple[int, int]:
        """``(Hc, Wc)`` of the canvas for audio frames ``(Ca, Ha, Wa)`` and vision frames ``(Cv, Hv, Wv)``."""
        _, ha, wa = _frame_chw("audio", audio_chw)
        cv, hv, wv = _frame_chw("vision", vision_chw)
        if cv not in (1, 3):
            msg = f"vision frames have 1 or 3 channels, got {cv}"
            raise ValueError(msg)
        cols = len(self.columns)
        hc = self.bar + hv * self.scale + self.gap + ha * self.scale
        wc = cols * max(wv, wa) * self.scale + (cols - 1) * self.gap
        if max(hc, wc) > _MAX_CANVAS:
            msg = f"the canvas is {hc} x {wc}, at most {_MAX_CANVAS} each way"
            raise ValueError(msg)
        return hc, wc

    def cell(self, modality: str, column: str | int, audio_chw: tuple[int, int, int], vision_chw: tuple[int, int, int]) -> tuple[slice, slice]:
        """The canvas slices ``(rows, columns)`` the frame of (``modality``, ``column``) is drawn into (the frame's own extent: the
        zero padding right of a narrower frame is not part of it)."""
        _, ha, wa = _frame_chw("audio", audio_chw)
        _, hv, wv = _frame_chw("vision", vision_chw)
        j = self.columns.index(column) if isinstance(column, str) else int(column)
        x0 = j * (max(wv, wa) * self.scale + self.gap)
        if modality == "vision":
            return slice(self.bar, self.bar + hv * self.scale), slice(x0, x0 + wv * self.scale)
        if modality != "audio":
            msg = f"modality is 'audio' or 'vision', got {modality!r}"
            raise ValueError(msg)
        y0 = self.bar + hv * self.scale + self.gap
        return slice(y0, y0 + ha * self.scale), slice(x0, x0 + wa * self.scale)

    def _checked(self, frames: dict[str, tuple[Tensor | None, Tensor | None]], codes: Tensor | None, valid: Tensor | None,  # noqa: C901, PLR0912
                 context: Tensor | None, frame0: int) -> tuple[int, int, tuple[int, int, int], tuple[int, int, int], Tensor]:
        needed = {("prior" if c == "error" else c) for c in self.columns} | ({"observation"} if "error" in self.columns else set())
        ref = None
        shapes: list[tuple[int, ...] | None] = [None, None]
        for kind in ("prior", "observation", "posterior"):
            for m, name in enumerate(("audio", "vision")):
                t = frames[kind][m]
                if t is None:
                    if kind in needed:
                        msg = f"the columns {self.columns} need the {kind} frames of {name}"
                        raise ValueError(msg)
                    continue
                if not isinstance(t, Tensor) or t.dim() != 5 or t.dtype != torch.float32:  # noqa: PLR2004
                    msg = f"{kind} {name} frames must be a float32 [N, T, C, H, W] tensor, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}"
                    raise ValueError(msg)
                if shapes[m] is None:
                    shapes[m] = tuple(t.shape)
                if tuple(t.shape) != shapes[m] or (ref is not None and (t.device != ref.device or tuple(t.shape[:2]) != tuple(ref.shape[:2]))):
                    msg = f"{kind} {name} frames {tuple(t.shape)} on {t.device} do not match the others ({shapes[m]})"
                    raise ValueError(msg)
                ref = t if ref is None else ref
        n, steps = ref.shape[:2]
        if min(n, steps) < 1:
            msg = f"need N >= 1 and T >= 1, got {n} and {steps}"
            raise ValueError(msg)
        audio_chw, vision_chw = tuple(shapes[0][2:]), tuple(shapes[1][2:])
        self.shape(audio_chw, vision_chw)
        for name, t, want in (("codes", codes, (n, steps)), ("valid", valid, (n,)), ("context", context, (n,))):
            if t is not None and (not isinstance(t, Tensor) or t.dtype != torch.int32 or tuple(t.shape) != want or t.device != ref.device):
                msg = f"{name} must be an int32 tensor of shape {want} on {ref.device}, got {getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))}"
                raise ValueError(msg)
        if isinstance(frame0, bool) or not isinstance(frame0, int) or not 0 <= frame0 < (1 << 31) - steps:
            msg = f"frame0 must be an integer with 0 <= frame0 and frame0 + T < 2^31, got {frame0!r}"
            raise ValueError(msg)
        if context is None:
            context = torch.full((n,), min(self.query_length, (1 << 31) - 1), dtype=torch.int32, device=ref.device)
        return n, steps, audio_chw, vision_chw, context  # type: ignore[return-value]

    # -- the rule in torch ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def unit(v: Tensor) -> Tensor:
        """``min(max((v + 1) / 2, 0), 1)`` in fp32, NaN -> 0."""
        x = (v.to(torch.float32) + 1.0) / 2.0
        return torch.where(torch.isnan(x), torch.zeros_like(x), x).clamp(0.0, 1.0)

    @staticmethod
    def _magma(s: Tensor) -> Tensor:
        lut = torch.from_numpy(MAGMA.copy()).to(s.device)
        return lut[(s * 256.0).to(torch.int64).clamp(max=255)]

    @staticmethod
    def _colours(kind: str, m: int, frames: dict[str, tuple[Tensor | None, Tensor | None]]) -> Tensor:
        """uint8 ``[N, T, H, W, 3]``: the frames of modality ``m`` (0 audio, 1 vision) in a column of kind ``kind``, unscaled."""
        if kind == "error":
            e = (EpisodePanel.unit(frames["prior"][m]) - EpisodePanel.unit(frames["observation"][m])).abs()
            e = ((e[:, :, 0] + e[:, :, 1]) + e[:, :, 2]) / 3.0 if m == 1 and e.shape[2] == 3 else e[:, :, 0]  # noqa: PLR2004
            return EpisodePanel._magma(e)
        x = EpisodePanel.unit(frames[kind][m])
        if m == 0:
            n = x[:, :, 0] * 2.0 - 1.0
            db = (n + 1.0) / 2.0 * 80.0 - 80.0
            s = ((db.clamp(-80.0, 0.0) - (-80.0)) / 80.0).clamp(0.0, 1.0)
            return EpisodePanel._magma(s)
        rgb = (x * 255.0).to(torch.int32).to(torch.uint8)
        if rgb.shape[2] == 1:
            rgb = rgb.expand(-1, -1, 3, -1, -1)
        return rgb.permute(0, 1, 3, 4, 2)

    def label_box(self, value: int) -> np.ndarray:
        """uint8 ``[7 p, (4 d + 1) p]`` in {0, 255}: the box of the frame number ``value`` (``d`` digits) at font pixel size ``p = label``."""
        digits = str(int(value))
        box = np.zeros((7, 4 * len(digits) + 1), dtype=np.uint8)
        for i, d in enumerate(digits):
            for r, row in enumerate(FONT[int(d)].split()):
                for c, bit in enumerate(row):
                    box[1 + r, 1 + 4 * i + c] = 255 * int(bit)
        return np.kron(box, np.ones((self.label, self.label), dtype=np.uint8))

    def reference(self, obs_a: Tensor | None, post_a: Tensor | None, prior_a: Tensor | None, obs_v: Tensor | None, post_v: Tensor | None,  # noqa: PLR0913, PLR0914
                  prior_v: Tensor | None, *, codes: Tensor | None = None, valid: Tensor | None = None, context: Tensor | None = None,
                  frame0: int = 0) -> Tensor:
        """The video in torch on the inputs' device: uint8 ``[N, T, Hc, Wc, 3]``.  Inputs fp32 ``[N, T, C, H, W]`` in [-1, 1] (frames a
        column does not read may be None); ``codes`` int32 ``[N, T]`` (bit 0 audio, bit 1 vision; None: both), ``valid`` int32 ``[N]``
        (None: every frame is live), ``context`` int32 ``[N]`` (None: ``query_length`` for every row)."""
        frames = {"prior": (prior_a, prior_v), "observation": (obs_a, obs_v), "posterior": (post_a, post_v)}
        n, steps, audio_chw, vision_chw, context = self._checked(frames, codes, valid, context, frame0)
        hc, wc = self.shape(audio_chw, vision_chw)
        dev = context.device
        s = self.scale
        canvas = torch.zeros(n, steps, hc, wc, 3, dtype=torch.uint8, device=dev)
        t = torch.arange(steps, device=dev)
        gap = torch.tensor(GAP_COLOUR, dtype=torch.uint8, device=dev)
        y_gap = self.bar + vision_chw[1] * s
        canvas[:, :, y_gap : y_gap + self.gap] = gap
        for j, kind in enumerate(self.columns):
            for m, name in enumerate(("audio", "vision")):
                rgb = self._colours(kind, m, frames)
                if kind == "observation" and self.blank_unseen and codes is not None:
                    seen = ((codes >> m) & 1).to(torch.uint8)
                    rgb = rgb * seen[:, :, None, None, None]
                rows, cols = self.cell(name, j, audio_chw, vision_chw)
                canvas[:, :, rows, cols] = rgb.repeat_interleave(s, dim=2).repeat_interleave(s, dim=3)
            if j + 1 < len(self.columns):
                x_gap = self.cell("audio", j + 1, audio_chw, vision_chw)[1].start - self.gap
                canvas[:, :, self.bar :, x_gap : x_gap + self.gap] = gap
        if self.bar:
            seeing = (t[None, :] < context[:, None])[:, :, None, None, None]
            bar = torch.where(seeing, torch.tensor(BAR_CONTEXT, dtype=torch.uint8, device=dev), torch.tensor(BAR_OPEN, dtype=torch.uint8, device=dev))
            canvas[:, :, : self.bar] = bar.expand(n, steps, self.bar, wc, 3)
        if self.label:
            for i in range(steps):
                box = torch.from_numpy(self.label_box(frame0 + i)[:hc, :wc]).to(dev)
                canvas[:, i, : box.shape[0], : box.shape[1]] = box[None, :, :, None]
        if valid is not None:
            live = t[None, :] < valid.clamp(min=0)[:, None]
            canvas = canvas * live[:, :, None, None, None].to(torch.uint8)
        return canvas

    # -- the kernel ----------------------------------------------------------------------------------------------------------------------
    def geometry(self, n: int, steps: int, audio_chw: tuple[int, int, int], vision_chw: tuple[int, int, int], frame0: int = 0) -> C.Structure:
        """The ``MtrssmPanelGeom`` of ``n`` episodes of ``steps`` frames."""
        g = _lib.PanelGeom()
        g.N, g.T = n, steps
        g.Ca, g.Ha, g.Wa = audio_chw
        g.Cv, g.Hv, g.Wv = vision_chw
        g.scale, g.gap, g.bar, g.label, g.frame0 = self.scale, self.gap, self.bar, self.label, frame0
        for j, c in enumerate(self.columns):
            g.columns[j] = _lib.PANEL_COLUMNS[c]
        g.n_columns, g.blank_unseen = len(self.columns), int(self.blank_unseen)
        return g

    def render(self, obs_a: Tensor | None, post_a: Tensor | None, prior_a: Tensor | None, obs_v: Tensor | None, post_v: Tensor | None,  # noqa: PLR0913
               prior_v: Tensor | None, *, codes: Tensor | None = None, valid: Tensor | None = None, context: Tensor | None = None,
               frame0: int = 0, out: Tensor | None = None) -> Tensor:
        """One ``mtrssm_episode_panel`` launch on torch's current stream (non-GPU tensors: ``reference``): ``reference``'s arguments and
        result.  ``out``: a contiguous uint8 ``[N, T, Hc, Wc, 3]`` buffer to write into."""
        frames = {"prior": (prior_a, prior_v), "observation": (obs_a, obs_v), "posterior": (post_a, post_v)}
        n, steps, audio_chw, vision_chw, context = self._checked(frames, codes, valid, context, frame0)
        hc, wc = self.shape(audio_chw, vision_chw)
        if not context.is_cuda:
            got = self.reference(obs_a, post_a, prior_a, obs_v, post_v, prior_v, codes=codes, valid=valid, context=context, frame0=frame0)
            if out is not None:
                out.copy_(got)
                return out
            return got
        dev = context.device
        if out is None:
            out = torch.empty(n, steps, hc, wc, 3, dtype=torch.uint8, device=dev)
        if tuple(out.shape) != (n, steps, hc, wc, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
            msg = f"out must be a contiguous uint8 [{n}, {steps}, {hc}, {wc}, 3] buffer on {dev}, got {out.dtype} {tuple(out.shape)}"
            raise ValueError(msg)
        lib = _lib.load()
        g = self.geometry(n, steps, audio_chw, vision_chw, frame0)
        kept = [None if x is None else x.contiguous() for x in (obs_a, post_a, prior_a, obs_v, post_v, prior_v, codes, valid, context)]
        elems = sum(x.numel() for x in kept[:6] if x is not None)
        _lib.check(_lib.TIMERS.call("mtrssm_episode_panel", lib.mtrssm_episode_panel, C.byref(g), *(_lib.ptr(x) for x in kept[:6]),
                                    *(_lib.index_ptr(x) for x in kept[6:]), _lib.raw_ptr(out), _lib.stream_ptr(dev),
                                    nbytes=float(out.numel() + 4 * elems)), "mtrssm_episode_panel")
        return out


@dataclass
class EpisodeVideo:
    """What ``render_episodes`` returns: ``frames`` uint8 ``[N, T, Hc, Wc, 3]`` on the device, the rows' ``context`` and ``valid`` (int32
    ``[N]``; ``valid`` None when every frame is live), and with ``keep_states`` the rollout ``states`` (``[2 N, T, .]``: closed loop, then
    open loop) and the ``decoded`` frames the panel was drawn from (a dict of fp32 ``[N, T, C, H, W]``)."""

    frames: Tensor
    context: Tensor
    valid: Tensor | None = None
    states: Any = None
    decoded: dict[str, Tensor] | None = None

    def chw(self) -> Tensor:
        """The reference's layout ``[N, T, 3, Hc, Wc]`` (a view)."""
        return self.frames.permute(0, 1, 4, 2, 3)

    def numpy(self) -> np.ndarray:
        return self.frames.cpu().numpy()

    def sheet(self, every: int = 1) -> Tensor:
        """A still contact sheet ``[N, Hc, ceil(T / every) Wc, 3]``: every ``every``-th frame side by side."""
        every = _whole("every", every, 1, (1 << 31) - 1)
        picked = self.frames[:, ::every]
        n, m, hc, wc, _ = picked.shape
        return picked.permute(0, 2, 1, 3, 4).reshape(n, hc, m * wc, 3)

    def save_npy(self, path: str | Path) -> Path:
        path = Path(path)
        path.parent.mkdir(parents=True, exist_ok=True)
        np.save(path, self.numpy())
        return path

    def save_gif(self, pattern: str | Path, fps: float = 10.0, names: list[int] | None = None) -> list[Path]:
        """One GIF per episode at ``pattern.format(i)`` (``i``: the row, or ``names[row]``), each with ONE global palette of at most 256
        colours for all its frames: the video's own colours when it has no more than 256 of them (then the file is exact), else PIL's
        median cut over the whole episode, without dithering."""
        try:
            from PIL import Image  # noqa: PLC0415
        except ImportError as e:
            msg = "save_gif needs PIL (pillow), which is not importable here: use save_npy, or install pillow"
            raise RuntimeError(msg) from e
        if not fps > 0:
            msg = f"fps must be positive, got {fps!r}"
            raise ValueError(msg)
        video = self.numpy()
        n, steps, hc, wc, _ = video.shape
        if names is not None and len(names) != n:
            msg = f"names has {len(names)} entries, the video {n} episodes"
            raise ValueError(msg)
        paths = []
        for row in range(n):
            path = Path(str(pattern).format(row if names is None else names[row]))
            path.parent.mkdir(parents=True, exist_ok=True)
            flat = video[row].reshape(-1, 3)
            packed = flat[:, 0].astype(np.uint32) << 16 | flat[:, 1].astype(np.uint32) << 8 | flat[:, 2].astype(np.uint32)
            colours, index = np.unique(packed, return_inverse=True)
            if len(colours) <= 256:  # noqa: PLR2004
                palette = np.stack([colours >> 16, (colours >> 8) & 255, colours & 255], axis=1).astype(np.uint8)
                index = index.reshape(steps, hc, wc).astype(np.uint8)
            else:
                tall = Image.fromarray(video[row].reshape(steps * hc, wc, 3), "RGB").quantize(colors=256, method=Image.Quantize.MEDIANCUT,
                                                                                              dither=Image.Dither.NONE)
                palette = np.asarray(tall.getpalette(), dtype=np.uint8).reshape(-1, 3)
                index = np.asarray(tall, dtype=np.uint8).reshape(steps, hc, wc)
            images = []
            for i in range(steps):
                im = Image.fromarray(index[i], "P")
                im.putpalette(palette.reshape(-1).tolist())
                images.append(im)
            images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=max(1, round(1000.0 / fps)), loop=0,
                           optimize=False)
            paths.append(path)
        return paths


class EpisodePanelLogger:
    """The reference's ``LogMultimodalMRSSMOutput`` callback without a trainer or WandB: ``EpisodePanelLogger(every_n_epochs=, indices=,
    query_length=, fps=, directory=, **panel_kwargs)`` -- the first four keywords are the callback's own.  ``logger(model, batch, stage,
    epoch, first_index=0)`` renders the rows of ``batch`` whose global episode index ``first_index + row`` is in ``indices`` (and below
    60: the callback looks at a loader's first 60 episodes only) and writes ``{directory}/{stage}/epoch_{E}/episode_{i}.gif``; like the
    callback it does nothing at epoch 0 and on epochs that are no multiple of ``every_n_epochs``.  With a process group initialised only
    rank 0 renders and writes; no collective is used."""

    def __init__(self, *, every_n_epochs: int, indices: list[int], query_length: int, fps: float, directory: str | Path = "episode_panels",  # noqa: PLR0913
                 **panel_kwargs: Any) -> None:  # noqa: ANN401
        self.every_n_epochs = _whole("every_n_epochs", every_n_epochs, 1, (1 << 31) - 1)
        self.indices = [_whole("an episode index", i, 0, (1 << 31) - 1) for i in indices]
        if not fps > 0:
            msg = f"fps must be positive, got {fps!r}"
            raise ValueError(msg)
        self.query_length, self.fps, self.directory = query_length, float(fps), Path(directory)
        self.panel = EpisodePanel(query_length, **panel_kwargs)

    def due(self, epoch: int) -> bool:
        return epoch != 0 and epoch % self.every_n_epochs == 0

    def rows(self, batch_size: int, first_index: int = 0) -> list[int]:
        """The rows of a batch of ``batch_size`` episodes starting at global index ``first_index`` that are logged."""
        wanted = {i for i in self.indices if i < MAX_EPISODES}
        return [r for r in range(batch_size) if first_index + r in wanted]

    def __call__(self, model, batch: tuple[Tensor, ...], stage: str, epoch: int, first_index: int = 0, **render_kwargs: Any) -> list[Path]:  # noqa: ANN001, ANN401
        import torch.distributed as dist  # noqa: PLC0415

        if not self.due(epoch) or (dist.is_available() and dist.is_initialized() and dist.get_rank() != 0):
            return []
        rows = self.rows(batch[0].shape[0], first_index)
        if not rows:
            return []
        video = model.render_episodes(batch, self.panel, rows=rows, **render_kwargs)
        pattern = self.directory / stage / f"epoch_{epoch}" / "episode_{}.gif"
        return video.save_gif(pattern, self.fps, names=[first_index + r for r in rows])


__all__ = ["BAR_CONTEXT", "BAR_OPEN", "COLUMNS", "FONT", "GAP_COLOUR", "MAGMA", "MAX_EPISODES", "EpisodePanel", "EpisodePanelLogger", "EpisodeVideo"]
