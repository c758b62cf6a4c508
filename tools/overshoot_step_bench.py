"""Step time of the train step with LATENT OVERSHOOTING at the bench shape (bench.py's models, B = 64,
T = 50), one JSON line.

    python tools/overshoot_step_bench.py [--steps 20] [--warmup 5] [--models mrssm,mmtrssm] [--modes plain,overshoot_s5,overshoot_s1]
                                         [--no-split] [--no-kernels]

Modes, all in ONE process and each on a freshly built model (`warmup` untimed steps, then `steps` steps between two synchronisations:
wall clock over all of them and the median of the per-step HIP-event intervals):

  plain          shared_step(batch, noise): bench.py --graph off, for scale
  overshoot_s5   shared_step(..., overshoot=LatentOvershoot(5, stride=5)): 10 starts per row, 640 overshoot rows of 5 steps
  overshoot_s1   shared_step(..., overshoot=LatentOvershoot(5, stride=1)): 49 starts per row, 3136 overshoot rows of 5 steps

`split` (unless --no-split): the overshoot modes' cost by kernel from the library's own event timers (`_lib.TIMERS`) over 5 further
steps -- total milliseconds per step of every library kernel, largest first.

`kernels` (unless --no-kernels): the two KL launches (forward, backward) and the gather on tensors of the step's shapes, each against
the same rule composed from torch ops on the same tensors (fp32, on the device); median of `steps` event intervals after `warmup`.
The KL launches' share of the HBM bandwidth is their algorithmic bytes -- 4 (B N D S + B T S + B N D) forward -- over the time, over
`--hbm-gbs` (8000: the MI355X's 8 TB/s).

Under rocprofv3 --kernel-trace --stats this is the program that gives the new kernels' time per launch.
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

MODES = ("plain", "overshoot_s5", "overshoot_s1")
MODELS = ("mrssm", "mmtrssm")
DEPTH = 5


def _overshoot(mode: str):  # noqa: ANN202
    import multimodal_mtrssm_amd as mt

    return None if mode == "plain" else mt.LatentOvershoot(DEPTH, stride=int(mode.rsplit("_s", 1)[1]))


def _median_ms(fn, steps: int, warmup: int) -> float:  # noqa: ANN001
    for _ in range(warmup):
        fn()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    for i in range(steps):
        marks[i].record()
        fn()
    marks[steps].record()
    torch.cuda.synchronize()
    return sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))[steps // 2]


def run_mode(kind: str, mode: str, steps: int, warmup: int, device: str, split: bool) -> dict[str, object]:  # noqa: FBT001, PLR0913
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd import _lib, scan
    from multimodal_mtrssm_amd.optim import FlatParameters

    w = bench.WORKLOAD
    b, t = w["batch_per_gpu"], w["steps"]
    model = bench.build_model(device, kind)
    lo = _overshoot(mode)
    model.overshoot = lo  # (noise_shapes gains the overshoot uniforms in the overshoot modes only: plain draws what bench.py draws)
    flat = FlatParameters(model, extra=8)
    dp = mt.FlatDataParallel(flat)
    opt = mt.FlatAdamW(flat, lr=1e-3, clip_norm=10.0)
    batch = bench.synthetic_batch(b, device, seed=1000)
    source = dp.noise_source(seed=7)
    shapes = model.noise_shapes(b, t)

    def step() -> None:
        noise = source.draw(shapes)
        opt.zero_grad()
        out = model.shared_step(batch, noise, overshoot=lo)
        out["loss"].backward()
        dp.sync({k: out[k] for k in out})
        opt.step(grad_scale=dp.grad_scale)

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
    res: dict[str, object] = {"ms_per_step": elapsed / steps * 1e3, "median_ms": per_step[len(per_step) // 2], "min_ms": per_step[0],
                              "max_ms": per_step[-1]}
    if lo is not None:
        res["overshoot_rows"] = b * lo.rows(t)
    if split and lo is not None:
        timed = 5
        _lib.TIMERS.enable()
        for _ in range(timed):
            step()
        rows = _lib.TIMERS.summary()
        _lib.TIMERS.disable()
        res["split_ms_per_step"] = {k: round(v["total_ms"] / timed, 4) for k, v in sorted(rows.items(), key=lambda kv: -kv[1]["total_ms"])}
        res["split_launches_per_step"] = {k: v["launches"] / timed for k, v in rows.items() if "overshoot" in k}
    return res


def _torch_kl(post: torch.Tensor, os_logits: torch.Tensor, lo, cats: int) -> torch.Tensor:  # noqa: ANN001
    """The forward rule composed from torch ops in fp32 on the device (no lengths): the overshoot scalar."""
    b, t, width = post.shape
    n, d = lo.rows(t), lo.depth
    t0 = lo.offset + lo.stride * torch.arange(n, device=post.device)
    target = t0.unsqueeze(1) + 1 + torch.arange(d, device=post.device).unsqueeze(0)
    live = target < t
    q = post[:, target.clamp(max=t - 1).reshape(-1)].reshape(b, n, d, cats, width // cats)
    lq, lp = torch.log_softmax(q, dim=-1), torch.log_softmax(os_logits.reshape(b, n, d, cats, width // cats), dim=-1)
    kl = (lq.exp() * (lq - lp)).sum(dim=(-1, -2)) * live
    return kl[:, :, 1:].sum() / (live[:, 1:].sum() * b).clamp(min=1)


def run_kernels(kind: str, stride: int, steps: int, warmup: int, device: str, hbm_gbs: float) -> dict[str, object]:  # noqa: PLR0913
    import multimodal_mtrssm_amd as mt

    w = bench.WORKLOAD
    b, t, cats, width = w["batch_per_gpu"], w["steps"], w["cats"], w["cats"] * w["classes"]
    lo = mt.LatentOvershoot(DEPTH, stride=stride)
    n = lo.rows(t)
    g = torch.Generator(device=device).manual_seed(3)
    out: dict[str, object] = {"rows": b * n}
    for level in ("_",) if kind == "mrssm" else ("_l", "_h"):  # (bench.py's two levels have the same K x C)
        post = torch.randn(b, t, width, device=device, generator=g).requires_grad_()
        os_logits = torch.randn(b * n, DEPTH, width, device=device, generator=g).requires_grad_()

        def fwd(post=post, os_logits=os_logits, cats=cats):  # noqa: ANN001, ANN202
            return lo.kl(post.detach(), os_logits.detach(), cats)

        def both(post=post, os_logits=os_logits, cats=cats) -> None:  # noqa: ANN001
            post.grad = os_logits.grad = None
            lo.kl(post, os_logits, cats, weights=(1.0, 1.0)).term.backward()

        def torch_fwd(post=post, os_logits=os_logits, cats=cats):  # noqa: ANN001, ANN202
            with torch.no_grad():
                return _torch_kl(post, os_logits, lo, cats)

        def torch_both(post=post, os_logits=os_logits, cats=cats) -> None:  # noqa: ANN001
            post.grad = os_logits.grad = None
            _torch_kl(post, os_logits, lo, cats).backward()

        f, fb = _median_ms(fwd, steps, warmup), _median_ms(both, steps, warmup)
        tf, tfb = _median_ms(torch_fwd, steps, warmup), _median_ms(torch_both, steps, warmup)
        fwd_bytes = 4.0 * (b * n * DEPTH * width + b * t * width + b * n * DEPTH)
        bwd_bytes = 4.0 * (2 * b * n * DEPTH * width + DEPTH * b * t * width)
        out[f"kl{level}"] = {"width": width, "fwd_ms": f, "fwd_bwd_ms": fb, "torch_fwd_ms": tf, "torch_fwd_bwd_ms": tfb,
                             "fwd_hbm_share": fwd_bytes / (f * 1e-3) / (hbm_gbs * 1e9),
                             "bwd_hbm_share_upper": bwd_bytes / (max(fb - f, 1e-6) * 1e-3) / (hbm_gbs * 1e9)}
    deter, stoch = w["deter"], width
    states = [torch.randn(b, t, wd, device=device, generator=g) for wd in ((deter, stoch) if kind == "mrssm" else (deter, deter, stoch, stoch, deter, deter))]
    actions = torch.randn(b, t, w["action"], device=device, generator=g)
    out["gather"] = {"ms": _median_ms(lambda: lo.gather(states, actions), steps, warmup),
                     "torch_ms": _median_ms(lambda: lo.gather_reference(states, actions), steps, warmup)}
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--models", default=",".join(MODELS))
    ap.add_argument("--no-split", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    args = ap.parse_args()
    modes = [m for m in args.modes.split(",") if m]
    kinds = [k for k in args.models.split(",") if k]
    unknown = (set(modes) - set(MODES)) | (set(kinds) - set(MODELS))
    if unknown or args.steps < 1:
        ap.error(f"unknown modes or models {sorted(unknown)} (of {MODES}, {MODELS}) or steps < 1")
    assert torch.cuda.is_available(), "overshoot_step_bench.py needs the MI355X"
    results = {k: {m: run_mode(k, m, args.steps, args.warmup, "cuda:0", not args.no_split) for m in modes} for k in kinds}
    kernels = {}
    if not args.no_kernels:
        kernels = {k: {f"stride{s}": run_kernels(k, s, args.steps, args.warmup, "cuda:0", args.hbm_gbs) for s in (5, 1)} for k in kinds}
    w = bench.WORKLOAD
    print(json.dumps({"metric": "ms per train step, latent overshooting", "batch": w["batch_per_gpu"], "steps_per_sequence": w["steps"],
                      "depth": DEPTH, "timed_steps": args.steps, "warmup": args.warmup, "models": results, "kernels": kernels}))


if __name__ == "__main__":
    main()
