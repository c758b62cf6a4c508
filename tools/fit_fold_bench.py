"""Time of the fit loop's per-step fold at the three bench models' parameter counts, a same-commit yardstick --
the same reduction composed from torch ops on the same buffers -- and the seq-steps/s of a `Trainer` epoch at the bench shape next to
the hand-written loop of INTEGRATION.md section 5 over the same batches.  One JSON line.

    python tools/fit_fold_bench.py [--steps 5] [--warmup 2] [--models mrssm,mmtrssm,large] [--epoch-batches 32]

Every fold figure is the median of `steps` runs between two HIP events after `warmup` untimed runs, with the min and max beside it:

  fold         EpochMetrics.fold(flat.tail, weight, step): mtrssm_fit_fold, two launches over the flat gradient and parameter buffers
  torch_fp64   per segment sum(g.double()^2), sum(p.double()^2) and the non-finite count, the roots, the global norm and the weighted
               scalar sums into device tensors (no read-back): what a loop without the kernel would enqueue per step
  gbytes_per_s 8 bytes per parameter (both buffers read once) over the fold's median

`trainer` (the model of `--models`' first entry that is not `large`; `--epoch-batches` batches of the bench's B x T per epoch, seeded
feed noise): one untimed epoch, then one timed; `seq_steps_per_s` = batches x B x T / the epoch's `train_time` (the steps, the fold and
the loader; not the checkpoint), `hand_loop` the same number of steps of the loop written out (zero_grad, shared_step, backward, sync,
step) over the same loader, ended by one synchronize.
"""

from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import bench  # noqa: E402  (the workloads, models and batches of the flagship benchmark)
from likelihood_bench import timed  # noqa: E402


def torch_fold(grad, param, offsets, tail, n_scalars, weight, state) -> None:  # noqa: ANN001
    """The fold's sums from torch ops, kept on the device (the yardstick; non-finite steps are not handled)."""
    g2 = torch.stack([grad[a:b].double().square().sum() for a, b in zip(offsets, offsets[1:], strict=False)])
    p2 = torch.stack([param[a:b].double().square().sum() for a, b in zip(offsets, offsets[1:], strict=False)])
    bad = torch.stack([(~torch.isfinite(grad[a:b])).sum() for a, b in zip(offsets, offsets[1:], strict=False)])
    norms, total = g2.sqrt(), g2.sum().sqrt()
    state["seg_sum"] += norms
    state["seg_max"] = torch.maximum(state["seg_max"], norms)
    state["param"] = p2.sqrt()
    state["grad_sum"] += total
    state["grad_max"] = torch.maximum(state["grad_max"], total)
    state["scalars"] += weight * tail[:n_scalars].double()
    state["bad"] += bad


def fold_figures(kind: str, steps: int, warmup: int) -> dict[str, object]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.optim import FlatParameters

    dev = "cuda:0"
    bench.WORKLOAD = bench.WORKLOADS["large" if kind == "large" else "base"]
    model = bench.build_model(dev, kind)
    flat = FlatParameters(model)
    g = torch.Generator(device=dev).manual_seed(1)
    flat.grad.copy_(torch.randn(flat.numel, device=dev, generator=g) * 1e-2)
    flat.tail[:5].copy_(torch.tensor([3.0, 1.0, 2.0, 0.5, 3.5]))
    keys = ["recon", "recon/audio", "recon/vision", "kl", "loss"]
    metrics = mt.EpochMetrics(flat, model, keys, clip_norm=10.0)
    count = [0]

    def fold() -> None:
        metrics.fold(flat.tail, 64.0, count[0])
        count[0] += 1

    n_seg = len(metrics.names)
    zeros = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)  # noqa: E731
    state = {"seg_sum": zeros(n_seg), "seg_max": zeros(n_seg), "param": zeros(n_seg), "grad_sum": zeros(()), "grad_max": zeros(()),
             "scalars": zeros(len(keys)), "bad": torch.zeros(n_seg, dtype=torch.int64, device=dev)}
    res: dict[str, object] = {"numel": flat.numel, "segments": dict(zip(metrics.names, metrics.offsets, strict=False)), "chunk_floats": metrics.chunk}
    res["fold"] = timed(fold, steps, warmup)
    res["torch_fp64"] = timed(lambda: torch_fold(flat.grad, flat.param, metrics.offsets, flat.tail, len(keys), 64.0, state), steps, warmup)
    res["gbytes_per_s"] = 8.0 * flat.numel / (res["fold"]["median_ms"] * 1e-3) / 1e9
    got = metrics.compute()
    res["grad_norm"], res["torch_grad_norm"] = got["grad_norm"], float(state["grad_sum"]) / (steps + warmup)
    assert got["bad_steps"] == 0.0
    return res


def trainer_figures(kind: str, batches: int) -> dict[str, object]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import dataset as ds
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd import transform as tr
    from multimodal_mtrssm_amd.optim import FlatParameters

    dev = "cuda:0"
    bench.WORKLOAD = w = bench.WORKLOADS["base"]
    b, t = w["batch_per_gpu"], w["steps"]
    g = torch.Generator().manual_seed(1000)
    n = b * batches
    stores = [torch.randn(n, t, w["action"], generator=g), torch.rand(n, t, *w["audio"], generator=g) * 2 - 1,
              torch.rand(n, t, *w["vision"], generator=g) * 2 - 1]
    chain = lambda std: tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std else []))  # noqa: E731
    streams = tuple(ds._Stream(s.to(dev), chain(0.1), chain(None)) for s in stores)  # noqa: SLF001
    loader = lambda: ds.DeviceEpisodeLoader(streams, b, shuffle=True, seed=1, noise_seed=7)  # noqa: E731
    res: dict[str, object] = {"model": kind, "batch": b, "steps_per_sequence": t, "batches_per_epoch": batches}

    def parts():  # noqa: ANN202
        model = bench.build_model(dev, kind)
        flat = FlatParameters(model)
        return model, flat, mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0), mt.FlatDataParallel(flat)

    model, flat, opt, dp = parts()
    with tempfile.TemporaryDirectory() as tmp:
        lines = mt.Trainer(model, flat, opt, dp, seed=11, max_epochs=2, directory=tmp).fit(loader())
    scan.check_cluster_status()
    res["trainer"] = {"train_time_s": lines[1]["train_time"], "seq_steps_per_s": batches * b * t / lines[1]["train_time"],
                      "ms_per_step": 1e3 * lines[1]["train_time"] / batches, "train/loss": lines[1]["train/loss"], "grad_norm": lines[1]["grad_norm"]}
    model, flat, opt, dp = parts()
    source, feed = dp.noise_source(11), loader()
    seconds = []
    for epoch in range(2):
        feed.set_epoch(epoch)
        torch.cuda.synchronize()
        start = time.time()
        for batch in feed:
            noise = source.draw(model.noise_shapes(b, t))
            opt.zero_grad()
            out = model.shared_step(batch, noise)
            out["loss"].backward()
            dp.sync({k: out[k] for k in out})
            opt.step(grad_scale=dp.grad_scale)
        torch.cuda.synchronize()
        seconds.append(time.time() - start)
    scan.check_cluster_status()
    res["hand_loop"] = {"train_time_s": seconds[1], "seq_steps_per_s": batches * b * t / seconds[1], "ms_per_step": 1e3 * seconds[1] / batches}
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--models", default="mrssm,mmtrssm,large")
    ap.add_argument("--epoch-batches", type=int, default=32)
    args = ap.parse_args()
    kinds = [k for k in args.models.split(",") if k]
    if args.steps < 1 or not kinds or any(k not in ("mrssm", "mmtrssm", "large") for k in kinds):
        ap.error("steps >= 1, models out of mrssm, mmtrssm, large")
    assert torch.cuda.is_available(), "fit_fold_bench.py needs the MI355X"
    res: dict[str, object] = {"metric": "ms per fit fold; seq-steps/s of a Trainer epoch", "timed_steps": args.steps, "warmup": args.warmup}
    res["fold"] = {k: fold_figures(k, args.steps, args.warmup) for k in kinds}
    small = [k for k in kinds if k != "large"]
    if small and args.epoch_batches > 0:
        res["epoch"] = trainer_figures(small[0], args.epoch_batches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
