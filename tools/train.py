#!/usr/bin/env python3
"""Train a model with the fit loop and write the checkpoint every other tool takes as `--checkpoint`.

    python tools/train.py --config train.json --data-dir data/train --out runs/a --epochs 200 [--seed 0] [--resume runs/a/last.ckpt]

`--config` is a JSON file (or YAML, where PyYAML is installed):

    {"model": "mrssm", "dims": [32, 32, 4, 4, 64],
     "trainer": {"lr": 1e-3, "clip_norm": 10.0, "batch_size": 32, "steps": 30, "noise_std": 0.1, "noise_seed": 7, "window": "first",
                 "scheduler": {"factor": 0.5, "patience": 50}, "early_stopping": {"patience": 100}, "monitor": "val/loss",
                 "max_steps": null, "save_every_n_steps": null, "check_every_n_steps": 50,
                 "modality_dropout": {"p_audio": 0.3, "p_vision": 0.3, "span": 5}, "elbo_schedule": {"free_nats": 1.0}, "state_carry": false,
                 "augment": {"vision": {"shift": [2, 2]}, "audio": {"bands": 2, "max_rows": 4, "max_cols": 4, "per_frame": true}},
                 "overshoot": {"depth": 5, "stride": 5}, "val_overshoot": {"depth": 5},
                 "val_census": {"observe": ["both", "audio", "vision"], "active_nats": 0.01},
                 "panel_logger": {"every_n_epochs": 10, "indices": [0, 1, 2], "query_length": 10, "fps": 10.0}},
     "panel": {"scale": 2}}

`model` / `dims` are `word_transitions.py`'s `--model` / `--dims`; every key of `trainer` is optional (the values above are the defaults,
which are the reference's `default.yaml:103-155`; the objects from `modality_dropout` on default to none; `panel` holds `render_episodes.py`'s
keywords of `EpisodePanel` for the logger's videos, so one file serves both tools).  The data are `word_transitions.py`'s
`.npz` episodes (`audio (T, 32, 32)`, `image (T, 1, 32, 32)`, `speaker (T, 6)`), cut to their common length, split 80 / 20 in sorted
file order as the reference's data module splits its files.  A config with the `data:` block of INTEGRATION.md section 2b (`class_path`
/ `init_args`, classes of this package only) goes through `EpisodeDataModule` instead and `--data-dir` is its `data_root`.

Written to `--out`: `best.ckpt`, `last.ckpt` (`{"state_dict": ...}` under the reference's parameter names plus the training state;
`--resume` continues from one, bit for bit), `metrics.jsonl` (one line per epoch) and, with `panel_logger`, `val/epoch_{E}/episode_{i}.gif`.
"""

from __future__ import annotations

import argparse
import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))


def instantiate(node):  # noqa: ANN001, ANN201
    """A `{"class_path": "multimodal_mtrssm_amd...", "init_args": {...}}` tree as objects (lists and dicts are walked)."""
    if isinstance(node, list):
        return [instantiate(v) for v in node]
    if not isinstance(node, dict):
        return node
    if "class_path" not in node:
        return {k: instantiate(v) for k, v in node.items()}
    module, _, name = str(node["class_path"]).rpartition(".")
    if module.split(".")[0] != "multimodal_mtrssm_amd":
        msg = f"class_path {node['class_path']!r}: only classes of multimodal_mtrssm_amd are built from a config"
        raise SystemExit(msg)
    return getattr(importlib.import_module(module), name)(**instantiate(node.get("init_args", {})))


def npz_loaders(folder: Path, cfg: dict, dev: str, rank: int, world: int):  # noqa: ANN201
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import transform as tr
    from word_transitions import load_episodes

    episodes = load_episodes(folder)
    if len(episodes) < 2:  # noqa: PLR2004
        msg = f"{folder} holds {len(episodes)} .npz episodes: need at least two (80 / 20 split)"
        raise SystemExit(msg)
    t_full = min(len(e["audio"]) for e in episodes)
    audio_t, vision_t = tr.NormalizeAudioMelSpectrogram(min_value=-80.0, max_value=0.0), tr.NormalizeVisionImage()
    cut = lambda e, key, *shape: torch.from_numpy(np.asarray(e[key][:t_full])).float().reshape(t_full, *shape)  # noqa: E731
    stores = [torch.stack([cut(e, "speaker", 6) for e in episodes]), torch.stack([audio_t(cut(e, "audio", 1, 32, 32)) for e in episodes]),
              torch.stack([vision_t(cut(e, "image", 1, 32, 32)) for e in episodes])]
    steps, std = min(int(cfg.get("steps", 30)), t_full), cfg.get("noise_std", 0.1)
    plain = tr.Compose([tr.TakeFirstN(steps)])
    noisy = plain if not std else tr.Compose([tr.TakeFirstN(steps), tr.GaussianNoise(float(std))])
    split = int(len(episodes) * 0.8)
    kw = {"rank": rank, "world": world, "window": cfg.get("window", "first"), "noise_seed": cfg.get("noise_seed", 7)}

    def streams(lo: int, hi: int) -> tuple:
        # (the speaker one-hot takes no noise: its six floats do not go through the gather kernel, which a seeded feed needs)
        return tuple(ds._Stream(s[lo:hi].to(dev), plain if k == 0 else noisy, plain) for k, s in enumerate(stores))  # noqa: SLF001

    bs = int(cfg.get("batch_size", 32))
    # (`augment`: {"audio": {"shift": [2, 3], "bands": 2, "max_rows": 4, ...}, "vision": {...}}, FeedAugment's fields; train loader only)
    train = ds.DeviceEpisodeLoader(streams(0, split), bs, shuffle=True, augment=cfg.get("augment"), **kw)
    val = ds.DeviceEpisodeLoader(streams(split, len(episodes)), bs, shuffle=False, noise_epoch="fixed", **kw) if split < len(episodes) else None
    return train, val


def main() -> None:
    ap = argparse.ArgumentParser(description="Train a MoPoE-M(MT)RSSM with the fit loop")
    ap.add_argument("--config", required=True, help="JSON (or YAML) with model, dims and optional trainer / data / panel blocks")
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--epochs", type=int, required=True)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train.py needs the MI355X"

    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.optim import FlatParameters
    from render_episodes import load_config
    from word_transitions import build_model

    cfg = load_config(Path(args.config))
    tc = dict(cfg.get("trainer", {}))
    dev = "cuda:0"
    torch.manual_seed(args.seed)
    model = build_model(cfg.get("model", "mrssm"), tuple(int(x) for x in cfg.get("dims", (32, 32, 4, 4, 64))), dev)
    flat = FlatParameters(model, extra=12 if tc.get("overshoot") else 8)  # (the overshoot term adds up to two logged scalars)
    dp = mt.FlatDataParallel(flat)
    dp.broadcast_parameters(0)
    opt = mt.FlatAdamW(flat, lr=float(tc.get("lr", 1e-3)), clip_norm=float(tc.get("clip_norm", 10.0)))
    if "data" in cfg:
        fields = cfg["data"].get("init_args", cfg["data"]).get("config", {})  # (the data class itself is this package's, whatever is named)
        if "lengths" in fields and fields["lengths"] is not None:
            fields = {**fields, "lengths": torch.tensor(fields["lengths"], dtype=torch.int64)}
        config = mt.EpisodeDataModuleConfig(**{"num_workers": 0, "gdrive_url": "", **instantiate(fields)})
        config.data_root = Path(args.data_dir)
        module = mt.EpisodeDataModule(config, dev, dp.rank, dp.world)
        module.prepare_data()
        module.setup("fit")
        train, val = module.train_dataloader(), (module.val_dataloader() if module.val_streams is not None else None)
    else:
        train, val = npz_loaders(Path(args.data_dir), tc, dev, dp.rank, dp.world)
    if tc.get("modality_dropout"):
        model.modality_dropout = mt.ModalityDropout(**tc["modality_dropout"])
    if tc.get("elbo_schedule"):
        model.elbo_schedule = mt.ElboSchedule(**tc["elbo_schedule"])
    if tc.get("overshoot"):
        model.overshoot = mt.LatentOvershoot(**tc["overshoot"])
    if tc.get("val_overshoot"):
        model.val_overshoot = dp.overshoot(mt.LatentOvershoot(**tc["val_overshoot"]))
    if tc.get("val_census"):
        block = dict(tc["val_census"])
        if "observe" in block:
            block["observe"] = tuple(block["observe"])
        model.val_census = dp.census(mt.LatentCensus(**block))
    if tc.get("state_carry"):
        model.state_carry = mt.StateCarry.for_model(model, train.batch_size // dp.world)
    sched, stop = tc.get("scheduler", {"factor": 0.5, "patience": 50}), tc.get("early_stopping", {"patience": 100})
    monitor = tc.get("monitor", "val/loss") if val is not None else "train/loss"
    panel = None
    if tc.get("panel_logger"):
        keywords = {k: tuple(v) if isinstance(v, list) else v for k, v in cfg.get("panel", {}).items()}
        panel = mt.EpisodePanelLogger(directory=args.out, **tc["panel_logger"], **keywords)
    trainer = mt.Trainer(
        model, flat, opt, dp, seed=args.seed, max_epochs=args.epochs, max_steps=tc.get("max_steps"),
        scheduler=None if sched is None else mt.ReduceLROnPlateau(opt, mode="min", **sched),
        early_stopping=None if stop is None else mt.EarlyStopping(monitor, mode="min", **stop), monitor=monitor, mode="min",
        directory=args.out, save_every_n_steps=tc.get("save_every_n_steps"), check_every_n_steps=int(tc.get("check_every_n_steps", 50)),
        panel_logger=panel)
    lines = trainer.fit(train, val, resume=args.resume)
    for line in lines:
        print(f"epoch {line['epoch']}: step {line['global_step']} lr {line['lr']:g} train/loss {line.get('train/loss', float('nan')):.5f} "
              f"{monitor} {line.get(monitor, float('nan')):.5f}")
    print(f"{len(lines)} epochs, best {trainer.best['value']} at epoch {trainer.best['epoch']}; checkpoints and metrics.jsonl in {args.out}")


if __name__ == "__main__":
    main()
