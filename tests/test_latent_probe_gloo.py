"""CPU, world size 2 over gloo: two ranks with half the rows each fold their own ``ProbeTable``s and
``ProbeTable.all_reduce`` over the group ``FlatDataParallel.probe`` bound gives the single-process table -- the counts and the hits (whole
numbers) exactly, the ``nll`` sums within fp32 addition order; and ``LinearProbe.fit(..., group=...)`` over the sharded rows is the fit
over all rows to fp32 rounding."""

from __future__ import annotations

import socket
from pathlib import Path

import torch
import torch.multiprocessing as mp

from tests.probe_worker import FIT_LR, FIT_STEPS, B, C, F, G, T, evaluate, fit, probe_case, worker

EPS = 2.0 ** -24


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_rank_probe_table_and_fit_match_single_process(tmp_path: Path) -> None:
    mp.spawn(worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    for key in ("reduced", "weight", "bias", "stats"):
        assert torch.equal(r0[key], r1[key]), key  # both ranks hold the same result
    assert not torch.equal(r0["own"], r1["own"])
    # the table
    one = evaluate(slice(0, B))
    _, labels, _, _ = probe_case()
    assert torch.equal(r0["reduced"][2 * G], one.counts) and torch.equal(one.counts, (labels >= 0).float().sum(0))  # counts: exact
    assert torch.equal(r0["reduced"][:G], one.hit) and float(one.hit.sum()) > 0  # hits are whole numbers: exact
    assert int((r0["own"][2 * G] > 0).sum()) == T and int((r1["own"][2 * G] > 0).sum()) == T  # every bin is split over the ranks
    for t in range(T):  # nll >= 0: any summation order of a bin's n addends stays within (n - 1) 2^-24 relative
        n = float(one.counts[t])
        torch.testing.assert_close(r0["reduced"][G : 2 * G, t], one.nll[:, t], rtol=2.0 * n * EPS, atol=0.0)
    # the fit: the sharded gradient is the whole one up to the rounding of two partial sums and their fp32 addition; that is far inside
    # the kernel's gradient tolerance rho = (N + F + 8) 2^-24 relative to mag = sum_n |p_n - y_n| |x_n|.  AdamW's update lr m / sqrt(v)
    # is homogeneous of degree 0 in the gradient history, so to first order a relative gradient error r moves a step by <= 2 lr r:
    # |dW| <= steps * 2 lr * rho * mag / |g| element-wise, mag and g taken at the zero weights the fit starts from.
    single, stats = fit(slice(0, B))
    x, labels, _, _ = probe_case()
    flat = labels.reshape(-1)
    live = flat >= 0
    xs = x.reshape(G, B * T, F)[:, live].double()
    d = torch.full((int(live.sum()), C), 1.0 / C, dtype=torch.float64) - torch.nn.functional.one_hot(flat[live].long(), C).double()
    grad_w, mag_w = torch.einsum("nc,gnf->gcf", d, xs), torch.einsum("nc,gnf->gcf", d.abs(), xs.abs())
    grad_b, mag_b = d.sum(0).expand(G, C), d.abs().sum(0).expand(G, C)
    rho = (B * T + F + 8) * EPS
    for name, got, want, grad, mag in (("weight", r0["weight"], single.weight.detach(), grad_w, mag_w), ("bias", r0["bias"], single.bias.detach(), grad_b, mag_b)):
        bound = FIT_STEPS * 2.0 * FIT_LR * rho * mag / grad.abs().clamp_min(1e-300)
        err = (got.double() - want.double()).abs()
        print(f"fit {name}: worst |sharded - single| {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), name
        assert float(want.abs().max()) > 0.5 * FIT_STEPS * FIT_LR  # (the fit moved)
    torch.testing.assert_close(r0["stats"], torch.stack([stats.nll_sum, stats.hits, stats.count]), rtol=1e-6, atol=0.0)
    assert r0["stats"][2].tolist() == [float(live.sum())] * G
