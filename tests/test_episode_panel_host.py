"""CPU: the episode panel's rule, geometry and host layers.

What is pinned here: ``EpisodePanel.reference`` gives the reference callback's bytes exactly on the fixture
(``tools/gen_episode_panel_golden.py``); ``MAGMA`` is matplotlib's table; the canvas arithmetic; the frame number's font, stated
literally; the contact sheet; an exact GIF round trip; the header, the ctypes table and the library agree on the two new entries.
"""

from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import EpisodePanel, EpisodePanelLogger, EpisodeVideo, _lib
from multimodal_mtrssm_amd.panel import BAR_CONTEXT, BAR_OPEN, FONT, GAP_COLOUR, MAGMA
from tests.conftest import ROOT, load_golden

AUDIO, VISION = (1, 8, 4), (3, 4, 6)


def fixture_frames(device: str = "cpu") -> tuple[list[torch.Tensor], np.ndarray]:
    """The fixture's inputs in ``reference``'s argument order (obs_a, post_a, prior_a, obs_v, post_v, prior_v) and the reference's
    bytes as ``[b, t, H, W, 3]``."""
    fx = load_golden("episode_panel")
    frames = [torch.from_numpy(fx[f"{k}_{m}"]).to(device) for m in "av" for k in ("obs", "post", "prior")]
    return frames, fx["rgb"].transpose(0, 1, 3, 4, 2)


def hard_frames(seed: int = 5) -> list[torch.Tensor]:
    """``N = 2, T = 3``, audio 1 x 8 x 4 and vision 3 x 4 x 6: values beyond [-1, 1], NaN, and every quantisation boundary."""
    g = torch.Generator().manual_seed(seed)
    x = np.arange(256, dtype=np.float32) / np.float32(255.0)
    v = x * np.float32(2.0) - np.float32(1.0)
    ramp = torch.from_numpy(np.concatenate([np.nextafter(v, np.float32(-2)), v, np.nextafter(v, np.float32(2))]))
    out = []
    for chw in (AUDIO, AUDIO, AUDIO, VISION, VISION, VISION):
        t = torch.rand(2, 3, *chw, generator=g) * 2.2 - 1.1
        flat = t.reshape(-1)
        part = ramp[torch.randperm(len(ramp), generator=g)[: flat.numel() // 2]]
        flat[: len(part)] = part
        flat[-1], flat[-2], flat[-3], flat[-4], flat[-5], flat[-6] = -1.2, 1.3, float("nan"), -1.0, 1.0, 0.0
        out.append(flat[torch.randperm(flat.numel(), generator=g)].reshape(2, 3, *chw).contiguous())
    return out


def test_reference_gives_the_callbacks_bytes_on_the_fixture() -> None:
    frames, want = fixture_frames()
    got = EpisodePanel(1, scale=1, gap=0, bar=0, label=0).reference(*frames).numpy()
    assert got.dtype == np.uint8 and got.shape == want.shape == (2, 3, 16, 24, 3)
    assert int((got != want).sum()) == 0
    audio = got[:, :, 8:].reshape(-1, 3)
    assert len({tuple(c) for c in audio.tolist()}) == len({tuple(c) for c in MAGMA.tolist()})  # every magma entry is hit
    assert set(np.unique(got[:, :, :8])) == set(range(256))  # and every vision byte


def test_magma_is_matplotlibs_table() -> None:
    matplotlib = pytest.importorskip("matplotlib")
    lut = (matplotlib.colormaps["magma"](np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert MAGMA.shape == (256, 3) and MAGMA.dtype == np.uint8 and np.array_equal(MAGMA, lut)


def test_geometry() -> None:
    p = EpisodePanel(3)
    assert p.shape((1, 128, 32), (1, 64, 64)) == (2 + 128 + 1 + 256, 3 * 128 + 2)
    four = EpisodePanel(3, columns=("prior", "observation", "posterior", "error"), scale=3, gap=1, bar=2, label=1)
    assert four.shape(AUDIO, VISION) == (2 + 12 + 1 + 24, 4 * 18 + 3)
    assert EpisodePanel(1, scale=1, gap=0, bar=0, label=0, columns=("observation",)).shape(AUDIO, VISION) == (12, 6)
    rows, cols = four.cell("vision", "observation", AUDIO, VISION)
    assert (rows.start, rows.stop, cols.start, cols.stop) == (2, 14, 19, 37)
    rows, cols = four.cell("audio", 3, AUDIO, VISION)
    assert (rows.start, rows.stop, cols.start, cols.stop) == (15, 39, 57, 69)
    # the canvas itself: separators, the bar's two phases, the zero padding right of the narrower audio frame, blanking, dead frames
    frames = hard_frames()
    codes = torch.tensor([[3, 1, 2], [0, 3, 3]], dtype=torch.int32)
    out = four.reference(*frames, codes=codes, valid=torch.tensor([3, 1], dtype=torch.int32), context=torch.tensor([1, 2], dtype=torch.int32)).numpy()
    assert out.shape == (2, 3, 39, 75, 3)
    assert (out[0, :, 14] == GAP_COLOUR).all() and (out[0, :, 15:, 18] == GAP_COLOUR).all() and (out[0, :, 2:14, 37] == GAP_COLOUR).all()
    assert (out[0, 0, :2, 6:] == BAR_CONTEXT).all() and (out[0, 1, :2, 6:] == BAR_OPEN).all() and (out[1, 0, :2, 6:] == BAR_CONTEXT).all()
    assert not out[0, :, 15:, 12:18].any() and out[0, :, 15:, :12].any()  # audio is 4 * 3 wide in an 18-wide cell
    assert not out[1, 1:].any() and out[1, 0].any()  # valid = 1
    vis_obs, aud_obs = four.cell("vision", "observation", AUDIO, VISION), four.cell("audio", "observation", AUDIO, VISION)
    assert not out[0, 1][vis_obs].any() and out[0, 1][aud_obs].any()  # code 1: audio only
    assert out[0, 2][vis_obs].any() and not out[0, 2][aud_obs].any()  # code 2: vision only
    assert not out[1, 0][vis_obs].any() and not out[1, 0][aud_obs].any()  # code 0
    shown = EpisodePanel(3, columns=four.columns, scale=3, blank_unseen=False).reference(*frames, codes=codes).numpy()
    assert shown[0, 1][vis_obs].any() and shown[1, 0][aud_obs].any()
    # nearest neighbour: a cell is its frame's colours, each repeated scale x scale
    cell = out[0, 0][four.cell("vision", "posterior", AUDIO, VISION)]
    assert np.array_equal(cell, np.kron(cell[::3, ::3], np.ones((3, 3, 1), dtype=np.uint8)))
    x = EpisodePanel.unit(frames[4][0, 0])  # post_v
    assert np.array_equal(cell[::3, ::3], (x * 255.0).to(torch.int32).permute(1, 2, 0).numpy().astype(np.uint8))


def test_argument_errors() -> None:
    for bad in ({"query_length": 0}, {"query_length": True}, {"observe": "sound"}, {"columns": ()}, {"columns": ("prior", "prior")},
                {"columns": ("prior", "mean")}, {"columns": "prior"}, {"scale": 0}, {"scale": 65}, {"gap": -1}, {"bar": 65}, {"label": 17},
                {"label": 1.0}, {"blank_unseen": 1}):
        with pytest.raises(ValueError):
            EpisodePanel(**({"query_length": 2} | bad))
    p = EpisodePanel(2)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        p.shape(AUDIO, (2, 4, 6))
    with pytest.raises(ValueError, match="positive"):
        p.shape((1, 0, 4), VISION)
    frames = hard_frames()
    with pytest.raises(ValueError, match="need the prior frames"):
        p.reference(frames[0], frames[1], None, *frames[3:])
    with pytest.raises(ValueError, match="float32"):
        p.reference(frames[0].double(), *frames[1:])
    with pytest.raises(ValueError, match="do not match"):
        p.reference(frames[0][:1], *frames[1:])
    with pytest.raises(ValueError, match="codes"):
        p.reference(*frames, codes=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="valid"):
        p.reference(*frames, valid=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="frame0"):
        p.reference(*frames, frame0=-1)
    two = [f[:, :, :2] if f.shape[2] == 3 else f for f in frames]  # noqa: PLR2004
    with pytest.raises(ValueError, match="1 or 3 channels"):
        p.reference(*two)
    only_obs = EpisodePanel(2, columns=("observation",))
    assert tuple(only_obs.reference(frames[0], None, None, frames[3], None, None).shape) == (2, 3, 2 + 8 + 1 + 16, 12, 3)
    with pytest.raises(ValueError):
        EpisodePanelLogger(every_n_epochs=0, indices=[0], query_length=2, fps=5.0)
    with pytest.raises(ValueError):
        EpisodePanelLogger(every_n_epochs=1, indices=[0], query_length=2, fps=0.0)
    with pytest.raises(ValueError):
        EpisodePanelLogger(every_n_epochs=1, indices=[-1], query_length=2, fps=5.0)


FONT_ROWS = {  # the issue's font, literally
    0: "111 101 101 101 111", 1: "010 110 010 010 111", 2: "111 001 111 100 111", 3: "111 001 111 001 111", 4: "101 101 111 001 001",
    5: "111 100 111 001 111", 6: "111 100 111 101 111", 7: "111 001 001 001 001", 8: "111 101 111 101 111", 9: "111 101 111 001 111",
}


def expected_label(value: int, p: int) -> np.ndarray:
    digits = [int(d) for d in str(value)]
    unit = np.zeros((7, 4 * len(digits) + 1), dtype=np.uint8)
    for i, d in enumerate(digits):
        glyph = np.array([[int(b) for b in row] for row in FONT_ROWS[d].split()], dtype=np.uint8)
        unit[1:6, 1 + 4 * i : 4 + 4 * i] = glyph
    return np.kron(unit, np.ones((p, p), dtype=np.uint8)) * 255


@pytest.mark.parametrize("p", [1, 2])
def test_frame_number_is_the_literal_font(p: int) -> None:
    assert tuple(FONT) == tuple(FONT_ROWS[d] for d in range(10))
    frames = hard_frames()
    out = EpisodePanel(2, scale=4, label=p).reference(*frames, frame0=7).numpy()
    for t, value in ((0, 7), (3 - 1, 9)):
        want = expected_label(value, p)
        region = out[:, t, : want.shape[0], : want.shape[1]]
        assert (region == want[None, :, :, None]).all(), value
    out = EpisodePanel(2, scale=4, label=p).reference(*frames, frame0=8).numpy()  # frames 8, 9, 10: the box grows with the second digit
    want = expected_label(10, p)
    assert want.shape == (7 * p, 9 * p)
    assert (out[:, 2, : want.shape[0], : want.shape[1]] == want[None, :, :, None]).all()
    one = expected_label(9, p)
    assert (out[:, 1, : one.shape[0], : one.shape[1]] == one[None, :, :, None]).all()
    bar = out[0, 1, 0, one.shape[1] :]
    assert (bar == BAR_CONTEXT).all() or (bar == BAR_OPEN).all()  # right of the one-digit box the bar shows
    assert (EpisodePanel(2, scale=4, label=0).reference(*frames).numpy()[:, 0, 0, 0] == BAR_CONTEXT).all()  # no label: the bar's corner


def test_sheet_and_layouts(tmp_path) -> None:  # noqa: ANN001
    frames = torch.arange(2 * 5 * 3 * 4 * 3, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(2, 5, 3, 4, 3)
    video = EpisodeVideo(frames, torch.tensor([2, 2], dtype=torch.int32))
    assert tuple(video.chw().shape) == (2, 5, 3, 3, 4) and video.chw().data_ptr() == frames.data_ptr()
    assert torch.equal(video.chw()[1, 2, 1], frames[1, 2, :, :, 1])
    sheet = video.sheet(every=2)
    assert tuple(sheet.shape) == (2, 3, 3 * 4, 3)
    for i, t in enumerate((0, 2, 4)):
        assert torch.equal(sheet[:, :, 4 * i : 4 * i + 4], frames[:, t])
    assert tuple(video.sheet().shape) == (2, 3, 20, 3)
    with pytest.raises(ValueError):
        video.sheet(every=0)
    path = video.save_npy(tmp_path / "sub" / "v.npy")
    assert np.array_equal(np.load(path), frames.numpy())


def test_gif_round_trip_of_a_grey_video_is_exact(tmp_path) -> None:  # noqa: ANN001
    image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(3)
    grey = torch.randint(0, 256, (2, 4, 9, 11, 1), generator=g, dtype=torch.uint8).expand(-1, -1, -1, -1, 3).contiguous()
    grey[0, 0, 0, :8, :] = torch.arange(0, 256, 32, dtype=torch.uint8)[:, None]
    video = EpisodeVideo(grey, torch.tensor([1, 1], dtype=torch.int32))
    paths = video.save_gif(str(tmp_path / "ep_{}.gif"), fps=8.0)
    assert [p.name for p in paths] == ["ep_0.gif", "ep_1.gif"]
    for row, path in enumerate(paths):
        with image.open(path) as im:
            assert im.n_frames == 4  # noqa: PLR2004
            for t in range(4):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("RGB")), grey[row, t].numpy()), (row, t)
    named = video.save_gif(str(tmp_path / "e" / "episode_{}.gif"), fps=8.0, names=[7, 12])
    assert [p.name for p in named] == ["episode_7.gif", "episode_12.gif"] and all(p.exists() for p in named)
    # more than 256 colours: one median-cut palette per file, still one file per episode
    many = torch.randint(0, 256, (1, 2, 16, 16, 3), generator=g, dtype=torch.uint8)
    (path,) = EpisodeVideo(many, torch.tensor([1], dtype=torch.int32)).save_gif(str(tmp_path / "many_{}.gif"), fps=4.0)
    with image.open(path) as im:
        assert im.n_frames == 2 and im.size == (16, 16)  # noqa: PLR2004


def test_logger_schedule_and_rows() -> None:
    log = EpisodePanelLogger(every_n_epochs=5, indices=[0, 3, 9, 61, 64], query_length=4, fps=10.0, directory="out", scale=1)
    assert log.panel.query_length == 4 and log.panel.scale == 1 and log.fps == 10.0  # noqa: PLR2004
    assert [log.due(e) for e in (0, 1, 5, 10, 12)] == [False, False, True, True, False]  # (the callback skips epoch 0)
    assert log.rows(8, 0) == [0, 3] and log.rows(8, 8) == [1] and log.rows(8, 56) == []  # 61 and 64 lie past the first 60 episodes
    assert log(None, (torch.zeros(8, 2, 1),), "val", 3) == []  # not due: nothing is rendered, the model is not touched


def _struct_fields(header: str, name: str) -> list[str]:
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", header, flags=re.DOTALL).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.DOTALL)
    fields: list[str] = []
    for decl in body.split(";"):
        decl = re.sub(r"^(const\s+)?(float|int32_t)\s*\*?", "", decl.strip())
        fields += [f.strip() for f in decl.split(",") if f.strip()]
    return fields


def test_header_symbols_and_library_agree() -> None:
    header = (ROOT / "include" / "mtrssm.h").read_text()
    lib = _lib.load()
    for name in ("mtrssm_episode_panel_bytes", "mtrssm_episode_panel"):
        assert re.search(r"^\s*(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.MULTILINE), name
        assert name in _lib.SYMBOLS and hasattr(lib, name)
    declared = _struct_fields(header, "MtrssmPanelGeom")
    mine = [f"{n}[{t._length_}]" if hasattr(t, "_length_") else n for n, t in _lib.PanelGeom._fields_]  # noqa: SLF001
    assert declared == mine and C.sizeof(_lib.PanelGeom) == 4 * 19  # noqa: PLR2004
    for name, value in _lib.PANEL_COLUMNS.items():
        assert re.search(rf"#define MTRSSM_PANEL_{name.upper()} {value}\b", header), name
    # the size query and the argument checks need no device
    p = EpisodePanel(2, columns=("prior", "observation", "posterior", "error"), scale=3)
    geom = p.geometry(2, 3, AUDIO, VISION, frame0=8)
    hc, wc = C.c_int32(), C.c_int32()
    assert lib.mtrssm_episode_panel_bytes(C.byref(geom), C.byref(hc), C.byref(wc)) == 2 * 3 * 39 * 75 * 3
    assert (hc.value, wc.value) == p.shape(AUDIO, VISION) == (39, 75)
    assert lib.mtrssm_episode_panel_bytes(C.byref(geom), None, None) == 2 * 3 * 39 * 75 * 3
    for field, bad, word in (("Cv", 2, b"channels"), ("scale", 0, b"scale"), ("n_columns", 5, b"columns"), ("N", 0, b"positive"),
                             ("frame0", -1, b"frame0"), ("blank_unseen", 2, b"blank_unseen"), ("Wv", 20000, b"canvas")):
        g = p.geometry(2, 3, AUDIO, VISION)
        setattr(g, field, bad)
        assert lib.mtrssm_episode_panel_bytes(C.byref(g), None, None) == -1, field
        assert word in lib.mtrssm_last_error(), (field, lib.mtrssm_last_error())
        assert lib.mtrssm_episode_panel(C.byref(g), *([None] * 11)) == -1, field
    g = p.geometry(2, 3, AUDIO, VISION)
    g.columns[1] = 0  # prior twice
    assert lib.mtrssm_episode_panel_bytes(C.byref(g), None, None) == -1 and b"twice" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_panel(C.byref(geom), *([None] * 11)) == -1 and b"null" in lib.mtrssm_last_error()
    assert lib.mtrssm_episode_panel_bytes(None, None, None) == -1
    assert {"EpisodePanel", "EpisodeVideo", "EpisodePanelLogger"} <= set(mt.__all__)


def test_render_episodes_refuses_before_anything_runs() -> None:
    from oracle.cases import CASES, build_batch, build_model, with_sizes
    from tests.conftest import product_from_case

    case = with_sizes(CASES["mrssm_default"], 2, 4)
    model = product_from_case(case, build_model(case), "cpu")
    batch = build_batch(case)
    panel = EpisodePanel(2)
    with pytest.raises(ValueError, match="7-tuple"):
        model.render_episodes((*batch, torch.ones(2, 4, 2, dtype=torch.bool)), panel)
    with pytest.raises(ValueError, match="EpisodePanel"):
        model.render_episodes(batch, 2)
    model.state_carry = mt.StateCarry.for_model(model, 2)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.render_episodes(batch, panel)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="picks no episode"):
        model.render_episodes(batch, panel, rows=[])
