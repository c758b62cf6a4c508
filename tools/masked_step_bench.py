"""Step time of the MASKED train step at the bench shape (bench.py's MoPoE-MRSSM, B = 64, T = 50), one JSON line.

    python tools/masked_step_bench.py [--steps 20] [--warmup 5] [--modes unmasked_eager,unmasked_graph,host_mask,dropout_eager,dropout_graph]

Modes (each on a freshly built model, bench.py's warm-up / step discipline: `warmup` untimed steps, then `steps` steps between
two synchronisations, wall clock over all of them and the median of per-step HIP-event intervals):

  unmasked_eager / unmasked_graph   bench.py --graph off / on, for scale
  host_mask                         a bool [B, T, 2] mask built on the host every step and handed in as the batch's 7th entry
                                    (the only way to train with masks before the device-side sampler; runs on older commits too)
  dropout_eager                     shared_step(..., modality_dropout=...): the sampler kernel, no host round trip
  dropout_graph                     CapturedTrainStep(..., modality_dropout=...): sampler and step inside one hipGraph replay
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402  (the workload, model and batch of the flagship benchmark)

MODES = ("unmasked_eager", "unmasked_graph", "host_mask", "dropout_eager", "dropout_graph")
P_AUDIO, P_VISION, SPAN = 0.3, 0.3, 5


def host_mask(gen: torch.Generator, b: int, t: int, device: str) -> torch.Tensor:
    """The dropout rule on the host: what a data pipeline without the sampler has to do every step."""
    s = -(-t // SPAN)
    u = torch.rand(b, s, 2, generator=gen)[:, torch.arange(t) // SPAN]
    mask = u >= torch.tensor([P_AUDIO, P_VISION])
    none0 = ~mask[:, 0].any(dim=-1)
    audio = u[:, 0, 0] >= u[:, 0, 1]
    mask[:, 0, 0] |= none0 & audio
    mask[:, 0, 1] |= none0 & ~audio
    return mask.to(device)


def run_mode(mode: str, steps: int, warmup: int, device: str) -> dict[str, float]:
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import scan
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, "mrssm")
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = bench.synthetic_batch(b, device, seed=1000)
    source = dp.noise_source(seed=7)
    dropout = None
    if mode.startswith("dropout"):
        dropout = mt.ModalityDropout(P_AUDIO, P_VISION, span=SPAN)
        model.modality_dropout = dropout  # (noise_shapes gains "u_mask")
    shapes = model.noise_shapes(b, t)
    gen = torch.Generator().manual_seed(3)

    def eager_step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        if mode == "host_mask":
            out = model.shared_step((*batch, host_mask(gen, b, t, device)), noise)
        elif dropout is not None:
            out = model.shared_step(batch, noise, modality_dropout=dropout)
        else:
            out = model.shared_step(batch, noise)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

    step = eager_step
    captured = None
    if mode.endswith("graph"):
        from multimodal_mtrssm_amd.graph import CapturedTrainStep

        kw = {"modality_dropout": dropout} if dropout is not None else {}
        captured = CapturedTrainStep(model, flat, opt, dp, batch, source, **kw)
        step = captured.step
    for _ in range(warmup):
        step()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        step()
    marks[steps].record()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    scan.check_cluster_status()
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    if captured is not None:
        captured.close()
    return {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0], "max_ms": per_step[-1]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    unknown = set(modes) - set(MODES)
    if unknown or args.steps < 1:
        ap.error(f"unknown modes {sorted(unknown)} (of {MODES}) or steps < 1")
    assert torch.cuda.is_available(), "masked_step_bench.py needs the MI355X"
    results = {m: run_mode(m, args.steps, args.warmup, "cuda:0") for m in modes}
    w = bench.WORKLOAD
    print(json.dumps({"metric": "ms per MoPoE-MRSSM train step, masked", "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"],
                      "p_audio": P_AUDIO, "p_vision": P_VISION, "span": SPAN, "timed_steps": args.steps, "warmup": args.warmup,
                      "modes": results}))


if __name__ == "__main__":
    main()
