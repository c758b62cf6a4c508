#!/usr/bin/env python3
"""Episode panels of a checkpoint: per chosen episode one GIF `prior | observation | posterior`, vision over
magma-coloured audio -- what the reference's logging callback sends to WandB, written to a folder instead.

    python tools/render_episodes.py --config panel.json --checkpoint model.ckpt --data-dir data/test --indices 0,3,7 \\
        --query-length 30 --out panels [--fps 10] [--frames 50] [--sheet-every 5]

`--config` is a JSON file (or YAML, where PyYAML is installed) with the model and, optionally, the panel:

    {"model": "mrssm", "dims": [32, 32, 4, 4, 64], "panel": {"scale": 2, "columns": ["prior", "observation", "posterior", "error"]}}

`model` / `dims` are `word_transitions.py`'s `--model` / `--dims` (deter, hidden, classes, cats, embed; the checkpoint is loaded by
parameter name), `panel` holds keywords of `EpisodePanel` (`observe`, `columns`, `scale`, `gap`, `bar`, `label`, `blank_unseen`).  The
data are `word_transitions.py`'s `.npz` episodes (`audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `speaker (T, 6)`); `--indices` counts
them in sorted file order.  All chosen episodes are rendered in ONE `model.render_episodes` call over their first `--frames` frames (an
episode that is shorter is black past its end).  Written: `{out}/episode_{i}.gif`, `{out}/episodes.npy` (uint8 `[N, T, Hc, Wc, 3]`) and,
with `--sheet-every k`, `{out}/sheet_{i}.png` (every k-th frame side by side; needs PIL like the GIFs).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def load_config(path: Path) -> dict:
    text = path.read_text()
    if path.suffix in (".yaml", ".yml"):
        try:
            import yaml
        except ImportError as e:
            msg = f"{path} is YAML and PyYAML is not importable here: give the same keys as JSON"
            raise SystemExit(msg) from e
        return yaml.safe_load(text)
    return json.loads(text)


def main() -> None:
    ap = argparse.ArgumentParser(description="Episode panels: prior | observation | posterior videos of chosen episodes")
    ap.add_argument("--config", required=True, help="JSON (or YAML) with model, dims and optional panel keywords")
    ap.add_argument("--checkpoint", required=True)
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--indices", required=True, help="comma-separated episode indices (sorted file order)")
    ap.add_argument("--query-length", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--fps", type=float, default=10.0)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--sheet-every", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "render_episodes.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.transform import NormalizeAudioMelSpectrogram, NormalizeVisionImage
    from word_transitions import build_model, load_episodes

    cfg = load_config(Path(args.config))
    panel = mt.EpisodePanel(args.query_length, **{k: tuple(v) if isinstance(v, list) else v for k, v in cfg.get("panel", {}).items()})
    episodes = load_episodes(Path(args.data_dir))
    indices = [int(i) for i in args.indices.split(",") if i.strip()]
    if not indices or min(indices) < 0 or max(indices) >= len(episodes):
        ap.error(f"--indices must name some of the {len(episodes)} episodes in {args.data_dir}")
    dev = "cuda:0"
    torch.manual_seed(args.seed)
    model = build_model(cfg.get("model", "mrssm"), tuple(int(x) for x in cfg.get("dims", (32, 32, 4, 4, 64))), dev)
    mt.load_reference_checkpoint(model, args.checkpoint)
    model.eval()
    steps = args.frames
    audio_t, vision_t = NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), NormalizeVisionImage()

    def cut(key: str, e: int, *shape: int) -> torch.Tensor:  # the episode's first `steps` frames, zero-padded past its end
        x = torch.from_numpy(np.asarray(episodes[e][key][:steps])).float().reshape(-1, *shape)
        return torch.cat([x, x.new_zeros(steps - x.shape[0], *shape)])

    lengths = torch.tensor([min(steps, len(episodes[e]["audio"])) for e in indices], dtype=torch.int32, device=dev)
    audio = torch.stack([audio_t(cut("audio", e, 1, 32, 32)) for e in indices]).to(dev)
    vision = torch.stack([vision_t(cut("image", e, 1, 32, 32)) for e in indices]).to(dev)
    action = torch.stack([cut("speaker", e, 6) for e in indices]).to(dev)
    video = model.render_episodes((action, audio, vision, action, audio, vision), panel, lengths=lengths)
    out = Path(args.out)
    video.save_npy(out / "episodes.npy")
    paths = video.save_gif(out / "episode_{}.gif", args.fps, names=indices)
    if args.sheet_every > 0:
        from PIL import Image

        for row, i in enumerate(indices):
            Image.fromarray(video.sheet(args.sheet_every)[row].cpu().numpy(), "RGB").save(out / f"sheet_{i}.png")
    print(f"{len(paths)} episodes of {steps} frames, canvas {tuple(video.frames.shape[2:4])}, in {out}")


if __name__ == "__main__":
    main()
