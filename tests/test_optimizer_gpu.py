"""The optimizer kernels of ``csrc/train_ops.hip`` past one workgroup, against ONE float64 statement of the rule in their header
comment: ``mtrssm_adamw_prepare`` + ``mtrssm_adamw_apply`` (``sumsq_tick_kernel``, ``adamw_masked_kernel``: what ``FlatAdamW``
launches), the legacy ``mtrssm_sumsq`` + ``mtrssm_adamw_step`` (``sumsq_kernel``, ``adamw_kernel``) and ``FlatAdamW`` itself at a
size both kernels split.

The rule (``adamw_rule``), in this order: ``g *= grad_scale``; ``norm = ||g||``; ``g *= min(1, clip / (norm + 1e-6))`` (``clip <= 0``:
off); ``p *= 1 - lr wd``; ``m = b1 m + (1 - b1) g``; ``v = b2 v + (1 - b2) g^2``; ``p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)``.
``test_rule_is_torch_adamw`` (host only) pins it to ``torch.optim.AdamW`` + ``clip_grad_norm_`` in float64.  The C ABI takes its
scalars as C floats, so the rule is handed the float32 values of lr, betas, eps, decay, clip and scale: the comparison is about the
kernels' arithmetic, not about how 0.999 rounds.

Sizes: ``kThreads = 256``, ``grid_for``'s 2048 workgroups and the sums' 512: 525 319 = 2048 * 256 + 1031 (n % 4 = 3) gives the
element-wise kernels a second grid-stride lap, the 512 * 256-quad sums a second lap, and a 3-element tail; n < 4 is the tail alone.

Bounds.  Nothing is picked: for every case the SAME rule is also run in float32 with torch on the CPU, on the case's own inputs
and from the same state, and the kernel may be ``MARGIN = 8`` times as far from float64 as that composition is (max norm per
tensor; the margin of ``tests/test_latent_probe_gpu.py``: another order of the same roundings, not a worse arithmetic), for ``p`` plus
2 ulp of the element's parameter.  ``sum(g^2)``: ``rtol = 2e-6`` (``test_gaussian_nll_kernel``'s bound for a tree sum of non-negative
terms).  Inactive elements, and everything under a set status word, are compared bit for bit.  Each test prints what it measured.

The two kernels of a step are judged one by one.  The sum kernel's ``sum(g^2)`` is compared with the float64 sum at ``2e-6``; it is then
read back and handed, as the number the element-wise kernel really reads, to the float64 rule AND to the float32 composition for the
clip coefficient.  Otherwise ``m`` and ``v`` under a binding clip would measure the sum a second time, against a bound it cannot meet by
design: one float32 atomic per workgroup, 512 of them, leaves ``sum(g^2)`` 2e-7 .. 5e-7 off at 525 319 elements and different every
run, torch's pairwise sum on the CPU 2e-8 .. 6e-8, and ``v`` carries that relative error in full (``m`` half of it), so "8 x the float32
composition" was a statement about two summation orders, not about the element-wise arithmetic, and failed about one run in ten.
``FlatAdamW`` is compared with ``torch.optim.AdamW`` + ``clip_grad_norm_`` as they are (``p`` only: the coefficient cancels in
``m / sqrt(v)``).

Measured on the MI355X (kernel error / bound, worst over sizes and steps; 0.125 = exactly the float32 composition's error; more in
profiles/stream_kernel_tests_notes.md): ``p`` 0.10 .. 0.23 (at most 9.2e-7 off after three steps, float32 torch 9.2e-7), ``FlatAdamW``
0.57; ``m`` 0.125 .. 0.18; ``v`` 0.125 .. 0.22.  ``sum(g^2)``: 3.6e-9 .. 9.1e-8 up to 1027 elements, 1.1e-7 .. 6.8e-7 at 525 319 (bound 2e-6).
"""

from __future__ import annotations

import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu  # set test by test: test_rule_is_torch_adamw needs no GPU and runs with the host suite
DEV = "cuda:0"
MARGIN = 8.0
SIZES = (1, 3, 4, 5, 255, 256, 257, 1027, 525319)
BIG = 525319


def f32(x: float) -> float:
    """The value a C float argument carries."""
    return float(np.float32(x))


LR, B1, B2, EPS, WD = f32(1e-2), f32(0.9), f32(0.999), f32(1e-8), f32(0.01)


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


# the rule ---------------------------------------------------------------------------------------------------------------------------------
def adamw_rule(p, g, m, v, *, step, lr, clip, grad_scale, wd, active=None, b1=B1, b2=B2, eps=EPS, device_sumsq=None):  # noqa: ANN001, ANN201, PLR0913
    """One step of the header comment's rule in the dtype of ``p`` (float64: the reference; float32: the composition that sets
    the bound).  ``g`` is the raw gradient; returns ``(p, m, v, sum(g^2))`` with ``sum(g^2)`` of the raw gradient, as
    ``mtrssm_adamw_prepare`` leaves it.  ``active`` (bool): False elements are returned as they came.
    ``device_sumsq``: the ``sum(g^2)`` the sum kernel left on the device, which is the apply kernel's INPUT: the norm is then
    ``sqrt(device_sumsq) * grad_scale`` (the same number as the norm of the scaled gradient, from that sum)."""
    dt = p.dtype
    raw = g.to(dt)
    sumsq = raw.square().sum()
    gs = raw * grad_scale
    if clip > 0:
        norm = gs.square().sum().sqrt() if device_sumsq is None else torch.tensor(device_sumsq, dtype=dt).sqrt() * grad_scale
        gs = gs * torch.clamp(clip / (norm + 1e-6), max=1.0)
    t = torch.tensor(float(step), dtype=dt)
    bc1 = 1.0 - torch.tensor(b1, dtype=dt).pow(t)
    bc2_sqrt = (1.0 - torch.tensor(b2, dtype=dt).pow(t)).sqrt()
    p2 = p * (1.0 - torch.tensor(lr, dtype=dt) * wd)
    m2 = b1 * m + (1.0 - torch.tensor(b1, dtype=dt)) * gs
    v2 = b2 * v + (1.0 - torch.tensor(b2, dtype=dt)) * gs * gs
    p2 = p2 - (torch.tensor(lr, dtype=dt) / bc1) * m2 / (v2.sqrt() / bc2_sqrt + eps)
    if active is not None:
        p2, m2, v2 = torch.where(active, p2, p), torch.where(active, m2, m), torch.where(active, v2, v)
    return p2, m2, v2, sumsq


def test_rule_is_torch_adamw() -> None:
    """``adamw_rule`` in float64 against ``torch.optim.AdamW`` + ``clip_grad_norm_`` in float64: a ``Linear(300, 7)``, three steps,
    ``grad_scale`` applied to the gradients beforehand.  Rounding only (a few 1e-17 here); asserted at 1e-15."""
    torch.manual_seed(5)
    net = torch.nn.Linear(300, 7).double()
    x = torch.randn(16, 300, dtype=torch.float64)
    lr, wd, clip, scale = 1e-2, 1e-2, 0.5, 0.125
    opt = torch.optim.AdamW(net.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p = torch.cat([q.detach().reshape(-1) for q in net.parameters()]).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    worst = 0.0
    for step in (1, 2, 3):
        opt.zero_grad()
        net(x).square().sum().backward()
        g = torch.cat([q.grad.reshape(-1) for q in net.parameters()]).clone()
        for q in net.parameters():
            q.grad.mul_(scale)
        total = torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
        assert float(total) > clip  # the clip binds
        opt.step()
        p, m, v, sumsq = adamw_rule(p, g, m, v, step=step, lr=lr, clip=clip, grad_scale=scale, wd=wd, b1=0.9, b2=0.999, eps=1e-8)
        np.testing.assert_allclose(float(sumsq) * scale * scale, float(total) ** 2, rtol=1e-14)
        want = torch.cat([q.detach().reshape(-1) for q in net.parameters()])
        worst = max(worst, float((p - want).abs().max()))
        state = [opt.state[q] for q in net.parameters()]
        worst = max(worst, float((m - torch.cat([s["exp_avg"].reshape(-1) for s in state])).abs().max()))
        worst = max(worst, float((v - torch.cat([s["exp_avg_sq"].reshape(-1) for s in state])).abs().max()))
    print(f"adamw_rule vs torch.optim.AdamW (float64, 3 steps): worst |difference| {worst:.2e}")
    assert worst < 1e-15  # noqa: PLR2004


# inputs -----------------------------------------------------------------------------------------------------------------------------------
def _gradient(n: int, gen: torch.Generator) -> torch.Tensor:
    """randn times magnitudes over 10^[-6, 2], every 97th element exactly zero."""
    g = torch.randn(n, generator=gen) * torch.pow(10.0, torch.rand(n, generator=gen) * 8.0 - 6.0)
    g[96::97] = 0.0
    return g


def _problem(n: int, steps: int, seed: int, *, preload: bool, active: torch.Tensor | None = None) -> dict:
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    grads = [_gradient(n, gen) for _ in range(steps)]
    if preload:  # moments a run could have produced
        g0 = _gradient(n, gen)
        m, v = (1.0 - B1) * g0, (1.0 - B2) * g0 * g0
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    if active is not None:  # FlatParameters: an element that never had a gradient holds a zero gradient.  Its moments are
        grads = [torch.where(active, g, torch.zeros(())) for g in grads]  # left non-zero here: a kernel that decayed them would show
    return {"p": p, "m": m.float(), "v": v.float(), "grads": grads, "active": active}


def ulp(x: torch.Tensor) -> torch.Tensor:
    """float32 spacing at |x| (x float64)."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy()).astype(np.float32)).astype(np.float64))


class Worst:
    """The comparisons of one test and the line it prints: largest kernel error / bound per tensor.

    ``check`` (``p``): element by element against 8 x the float32 composition's largest error on the same inputs, plus the floor.
    ``defer`` + ``settle`` (``m``, ``v``, which have no floor): the composition's loss is taken relative to ``max |ref|`` and pooled
    over the sizes of the test at the same step, and applied to each size scaled by its own ``max |ref|``.  The largest error among
    the 1 .. 5 elements of the small sizes is not a measurement of an arithmetic: at n = 5 the composition came out 0.03 ulp from
    float64 on ``m`` after two steps and the kernel, 1 ulp off, would be "28 times worse"; over the 525 319 elements of the same
    case the composition is half an ulp to an ulp off like any float32 product."""

    def __init__(self) -> None:
        self.rows: dict[str, tuple[float, float, float]] = {}
        self.sumsq = 0.0  # worst relative error of sum(g^2)
        self.deferred: list[tuple[str, int, str, float, float, float]] = []

    def _row(self, name: str, ratio: float, err: float, theirs: float) -> None:
        old = self.rows.get(name)
        if old is None or ratio > old[0]:
            self.rows[name] = (ratio, err, theirs)

    def check(self, name: str, got: torch.Tensor, ref: torch.Tensor, cpu: torch.Tensor, *, floor: torch.Tensor | None = None, what: str = "") -> None:
        err = (got.double() - ref).abs()
        theirs = float((cpu.double() - ref).abs().max())
        bound = torch.full_like(err, MARGIN * theirs) + (floor if floor is not None else 0.0)
        ratio = float((err / bound.clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
        self._row(name, ratio, float(err.max()), theirs)
        assert bool((err <= bound).all()), (f"{what} {name}: |kernel - float64| {float(err.max()):.3e} over the bound; |fp32 torch - float64| {theirs:.3e}, "
                                            f"worst err / bound {ratio:.2f}")

    def defer(self, name: str, k: int, got: torch.Tensor, ref: torch.Tensor, cpu: torch.Tensor, *, what: str = "") -> None:
        """``k``: which step of the test's sequence (the pool is per tensor and step)."""
        self.deferred.append((name, k, what, float((got.double() - ref).abs().max()), float((cpu.double() - ref).abs().max()), float(ref.abs().max())))

    def settle(self) -> None:
        for name, k in sorted({(d[0], d[1]) for d in self.deferred}):
            pool = [d for d in self.deferred if d[0] == name and d[1] == k]
            loss = max(theirs / scale for *_, theirs, scale in pool if scale > 0)  # the float32 composition, relative to max |ref|
            for _, _, what, err, theirs, scale in pool:
                bound = MARGIN * loss * scale
                ratio = err / bound if err > 0 else 0.0
                self._row(name, ratio, err, theirs)
                assert err <= bound, (f"{what} {name}: |kernel - float64| {err:.3e} over the bound {bound:.3e} = 8 x {loss:.3e} (float32 torch, relative, "
                                      f"pooled over the test's sizes) x max |ref| {scale:.3e}; float32 torch at this size {theirs:.3e}")
        self.deferred.clear()

    def line(self, title: str) -> None:
        self.settle()
        parts = [f"{k}: err/bound {r:.3f} (|kernel - f64| {e:.2e}, |fp32 torch - f64| {t:.2e})" for k, (r, e, t) in self.rows.items()]
        print(f"{title}: " + "; ".join(parts) + (f"; sumsq relative {self.sumsq:.2e} (bound 2e-6)" if self.sumsq else ""))


def _state_bounds(step: int) -> tuple[float, float, float, float]:
    """Float64 values of state[2], state[3] and how far a float32 ``powf`` (2 ulp of a result below 1), the subtraction and the
    square root (half an ulp each) may leave them."""
    x1, x2 = 1.0 - B1 ** step, 1.0 - B2 ** step
    e = 2.0 ** -24
    tol1 = 2 * e + e * x1
    tol2 = (2 * e + e * x2) / (2.0 * math.sqrt(x2)) + e * math.sqrt(x2)
    return x1, tol1, math.sqrt(x2), tol2


def _run_prepare_apply(prob: dict, *, clip: float, grad_scale: float, wd: float, step0: int = 0, rates: tuple[float, ...] | None = None,  # noqa: PLR0913
                       worst: Worst, what: str) -> None:
    """``len(grads)`` consecutive steps on the device, state and moments carried there, each compared with float64."""
    import multimodal_mtrssm_amd as mt

    lib, L = mt._lib.load(), mt._lib  # noqa: SLF001, N806
    n = prob["p"].numel()
    act = prob["active"]
    p, m, v = prob["p"].to(DEV), prob["m"].to(DEV), prob["v"].to(DEV)
    act_d = act.to(torch.uint8).to(DEV) if act is not None else None
    p0, m0, v0 = prob["p"].clone(), prob["m"].clone(), prob["v"].clone()
    sumsq = torch.full((1,), 7.0, device=DEV)  # prepare has to zero it
    state = torch.tensor([LR, float(step0), 0.25, 0.25], device=DEV)
    stream = L.stream_ptr(p.device)
    p64, m64, v64 = prob["p"].double(), prob["m"].double(), prob["v"].double()
    p32, m32, v32 = prob["p"].clone(), prob["m"].clone(), prob["v"].clone()
    for k, g in enumerate(prob["grads"]):
        step = step0 + k + 1
        lr = f32(rates[k]) if rates else LR
        if rates:
            state[0:1].fill_(lr)  # what FlatAdamW.sync_lr does: the rate reaches the kernel through state[0] only
        gd = g.to(DEV)
        L.check(lib.mtrssm_adamw_prepare(L.ptr(gd), n, L.ptr(sumsq), L.ptr(state), None, B1, B2, stream), "mtrssm_adamw_prepare")
        L.check(lib.mtrssm_adamw_apply(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), L.raw_ptr(act_d), n, L.ptr(sumsq), L.ptr(state), None,
                                       clip, grad_scale, B1, B2, EPS, wd, stream), "mtrssm_adamw_apply")
        kw = {"step": step, "lr": lr, "clip": clip, "grad_scale": grad_scale, "wd": wd, "active": act, "device_sumsq": float(sumsq)}
        p64, m64, v64, ss64 = adamw_rule(p64, g, m64, v64, **kw)
        p32, m32, v32, _ = adamw_rule(p32, g, m32, v32, **kw)
        st = state.cpu().double()
        assert float(st[0]) == lr and float(st[1]) == float(step), (what, st)
        s2, t2, s3, t3 = _state_bounds(step)
        assert abs(float(st[2]) - s2) <= t2 and abs(float(st[3]) - s3) <= t3, (what, step, st, s2, s3)
        worst.sumsq = max(worst.sumsq, abs(float(sumsq) - float(ss64)) / float(ss64))
        np.testing.assert_allclose(float(sumsq), float(ss64), rtol=2e-6, err_msg=f"{what} sumsq step {step}")
        tag = f"{what} n={n} step {step}"
        worst.check("p", p.cpu(), p64, p32, floor=2.0 * ulp(p64), what=tag)
        worst.defer("m", k, m.cpu(), m64, m32, what=tag)
        worst.defer("v", k, v.cpu(), v64, v32, what=tag)
    if act is not None:  # bit for bit
        idle = ~act
        assert torch.equal(p.cpu()[idle].view(torch.int32), p0[idle].view(torch.int32)), what
        assert torch.equal(m.cpu()[idle].view(torch.int32), m0[idle].view(torch.int32)), what
        assert torch.equal(v.cpu()[idle].view(torch.int32), v0[idle].view(torch.int32)), what
        assert bool((p.cpu()[act] != p0[act]).any())


# mtrssm_adamw_prepare + mtrssm_adamw_apply ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("wd", [WD, 0.0])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("clip", [0.5, 1e9, 0.0])
def test_prepare_apply_three_steps(clip: float, grad_scale: float, wd: float, lib_loaded: None) -> None:
    """Three steps from zero moments at every size; binding clip, a clip that never binds, no clip.  The largest gradient norm
    is ~1e4 (the binding case scales by ~1e-5: eps then dominates the denominator), so ``clip = 1e9`` is far from binding."""
    worst = Worst()
    for n in SIZES:
        prob = _problem(n, 3, seed=1000 + n, preload=False)
        if clip == 0.5 and n >= 255:  # noqa: PLR2004
            assert all(float(g.double().norm()) * grad_scale > 2.0 * clip for g in prob["grads"])
        if clip == 1e9:  # noqa: PLR2004
            assert all(float(g.double().norm()) * grad_scale < 1e-3 * clip for g in prob["grads"])
        _run_prepare_apply(prob, clip=f32(clip), grad_scale=grad_scale, wd=wd, worst=worst, what=f"clip {clip} scale {grad_scale} wd {wd}")
    worst.line(f"prepare+apply clip {clip} grad_scale {grad_scale} wd {wd:.2g}")


def _masks(n: int) -> dict[str, torch.Tensor]:
    gen = torch.Generator().manual_seed(77)
    rnd = torch.rand(n, generator=gen) < 0.7  # noqa: PLR2004  (changes inside every workgroup)
    rnd[1000:5000] = False
    run = torch.ones(n, dtype=torch.bool)
    run[524288 - 300 : 524288 + 517] = False  # crosses the first lap's last element (2048 * 256)
    ends = torch.ones(n, dtype=torch.bool)
    ends[0] = ends[-1] = False
    return {"random": rnd, "run": run, "ends": ends}


@gpu
@pytest.mark.parametrize("kind", ["random", "run", "ends"])
def test_prepare_apply_active_mask(kind: str, lib_loaded: None) -> None:
    """``active`` masks at 525 319 elements (NULL is every other test of this file): a random mask with a False run over 1000..4999,
    a False run across element 524 288, first and last element False (the last one is in the 3-element tail of the sums).  Three
    steps from preloaded moments; inactive ``p``, ``m``, ``v`` stay bit-identical.  ``ends`` also at n = 5 and 1027."""
    worst = Worst()
    for n in ((BIG, 1027, 5) if kind == "ends" else (BIG,)):
        active = _masks(n)[kind]
        assert not bool(active.all()) and bool(active.any())
        prob = _problem(n, 3, seed=2000 + n, preload=True, active=active)
        _run_prepare_apply(prob, clip=f32(0.5), grad_scale=0.125, wd=WD, worst=worst, what=f"mask {kind}")
    worst.line(f"prepare+apply active mask '{kind}'")


@gpu
@pytest.mark.parametrize("step0", [999, 99999])
def test_prepare_apply_late_steps(step0: int, lib_loaded: None) -> None:
    """``state[1]`` preset: steps 1000.. and 100 000.. take their bias corrections from the kernel's own ``powf``
    (0.999^1000 = 0.368; 0.999^100000 underflows to a correction of exactly 1)."""
    worst = Worst()
    for n in (5, 1027, BIG):
        prob = _problem(n, 3, seed=3000 + n + step0, preload=True)
        _run_prepare_apply(prob, clip=f32(0.5), grad_scale=1.0, wd=WD, step0=step0, worst=worst, what=f"step0 {step0}")
    worst.line(f"prepare+apply from step {step0 + 1}")


@gpu
def test_prepare_apply_rate_through_state(lib_loaded: None) -> None:
    """The learning rate changes between steps through ``state[0]`` alone."""
    worst = Worst()
    for n in (257, BIG):
        prob = _problem(n, 3, seed=4000 + n, preload=False)
        _run_prepare_apply(prob, clip=f32(0.5), grad_scale=1.0, wd=WD, rates=(1e-2, 5e-3, 3e-2), worst=worst, what="rates")
    worst.line("prepare+apply, rate 1e-2 -> 5e-3 -> 3e-2")


@gpu
@pytest.mark.parametrize("n", [1027, BIG])
def test_status_word_skips_the_step(n: int, lib_loaded: None) -> None:
    """A non-zero status word: ``p``, ``m``, ``v`` and ``state[1..3]`` stay bit-identical after both launches (``sumsq`` is still
    formed), and the next step with the word cleared is the reference's step k, not k + 1."""
    import multimodal_mtrssm_amd as mt

    lib, L = mt._lib.load(), mt._lib  # noqa: SLF001, N806
    prob = _problem(n, 3, seed=5000 + n, preload=False)
    p, m, v = prob["p"].to(DEV), prob["m"].to(DEV), prob["v"].to(DEV)
    sumsq, state = torch.zeros(1, device=DEV), torch.tensor([LR, 0.0, 0.0, 0.0], device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = L.stream_ptr(p.device)
    clip, scale = f32(0.5), 0.125
    p64, m64, v64 = prob["p"].double(), prob["m"].double(), prob["v"].double()
    p32, m32, v32 = prob["p"].clone(), prob["m"].clone(), prob["v"].clone()
    worst = Worst()

    def launch(g: torch.Tensor) -> None:
        L.check(lib.mtrssm_adamw_prepare(L.ptr(g), n, L.ptr(sumsq), L.ptr(state), L.raw_ptr(status), B1, B2, stream), "mtrssm_adamw_prepare")
        L.check(lib.mtrssm_adamw_apply(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), None, n, L.ptr(sumsq), L.ptr(state), L.raw_ptr(status),
                                       clip, scale, B1, B2, EPS, WD, stream), "mtrssm_adamw_apply")

    def bits() -> list[torch.Tensor]:
        return [t.cpu().view(torch.int32).clone() for t in (p, m, v, state)]

    def follow(k: int, step: int) -> None:
        nonlocal p64, m64, v64, p32, m32, v32
        kw = {"step": step, "lr": LR, "clip": clip, "grad_scale": scale, "wd": WD, "device_sumsq": float(sumsq)}
        np.testing.assert_allclose(float(sumsq), float(prob["grads"][k].double().square().sum()), rtol=2e-6)
        p64, m64, v64, _ = adamw_rule(p64, prob["grads"][k], m64, v64, **kw)
        p32, m32, v32, _ = adamw_rule(p32, prob["grads"][k], m32, v32, **kw)
        assert float(state[1]) == float(step)
        worst.check("p", p.cpu(), p64, p32, floor=2.0 * ulp(p64), what=f"status n={n} step {step}")
        worst.defer("m", k, m.cpu(), m64, m32, what=f"status n={n} step {step}")
        worst.defer("v", k, v.cpu(), v64, v32, what=f"status n={n} step {step}")

    launch(prob["grads"][0].to(DEV))
    follow(0, 1)
    before = bits()
    status.fill_(3)
    bad = prob["grads"][1].to(DEV)
    launch(bad)
    for a, b in zip(bits(), before, strict=True):
        assert torch.equal(a, b)
    np.testing.assert_allclose(float(sumsq), float(prob["grads"][1].double().square().sum()), rtol=2e-6)
    status.zero_()
    launch(prob["grads"][2].to(DEV))
    follow(2, 2)  # the skipped step was not counted
    worst.line(f"status word, n={n}")


# mtrssm_sumsq + mtrssm_adamw_step -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_sumsq(n: int, lib_loaded: None) -> None:
    import multimodal_mtrssm_amd as mt

    lib, L = mt._lib.load(), mt._lib  # noqa: SLF001, N806
    g = _gradient(n, torch.Generator().manual_seed(6000 + n))
    gd, out = g.to(DEV), torch.full((1,), 7.0, device=DEV)
    L.check(lib.mtrssm_sumsq(L.ptr(gd), n, L.ptr(out), L.stream_ptr(gd.device)), "mtrssm_sumsq")
    want = float(g.double().square().sum())
    print(f"mtrssm_sumsq n={n}: {float(out):.9e} vs float64 {want:.9e}, relative {abs(float(out) - want) / want:.2e} (bound 2e-6)")
    np.testing.assert_allclose(float(out), want, rtol=2e-6)


@gpu
@pytest.mark.parametrize("mode", ["clip", "no_sumsq", "clip_off"])
@pytest.mark.parametrize("step0", [0, 999])
def test_legacy_sumsq_adamw_step(step0: int, mode: str, lib_loaded: None) -> None:
    """``mtrssm_sumsq`` + ``mtrssm_adamw_step`` (host-side step count and bias corrections) against the same rule: two steps from
    step 1 (zero moments) and from step 1000 (preloaded); a binding clip, ``sumsq = NULL`` with a positive clip (no clipping) and
    ``clip <= 0`` with a sum given (no clipping)."""
    import multimodal_mtrssm_amd as mt

    lib, L = mt._lib.load(), mt._lib  # noqa: SLF001, N806
    clip = {"clip": f32(0.5), "no_sumsq": f32(0.5), "clip_off": -1.0}[mode]
    rule_clip = clip if mode == "clip" else 0.0
    scale = 0.125
    worst = Worst()
    for n in (5, 1027, BIG):
        prob = _problem(n, 2, seed=7000 + n + step0, preload=step0 > 0)
        p, m, v = prob["p"].to(DEV), prob["m"].to(DEV), prob["v"].to(DEV)
        sumsq = torch.full((1,), 7.0, device=DEV)
        stream = L.stream_ptr(p.device)
        p64, m64, v64 = prob["p"].double(), prob["m"].double(), prob["v"].double()
        p32, m32, v32 = prob["p"].clone(), prob["m"].clone(), prob["v"].clone()
        for k, g in enumerate(prob["grads"]):
            step = step0 + k + 1
            gd = g.to(DEV)
            if mode != "no_sumsq":
                L.check(lib.mtrssm_sumsq(L.ptr(gd), n, L.ptr(sumsq), stream), "mtrssm_sumsq")
            L.check(lib.mtrssm_adamw_step(L.ptr(p), L.ptr(gd), L.ptr(m), L.ptr(v), n, None if mode == "no_sumsq" else L.ptr(sumsq), clip,
                                          scale, LR, B1, B2, EPS, WD, step, stream), "mtrssm_adamw_step")
            kw = {"step": step, "lr": LR, "clip": rule_clip, "grad_scale": scale, "wd": WD, "device_sumsq": float(sumsq) if mode == "clip" else None}
            p64, m64, v64, ss64 = adamw_rule(p64, g, m64, v64, **kw)
            p32, m32, v32, _ = adamw_rule(p32, g, m32, v32, **kw)
            if mode != "no_sumsq":
                np.testing.assert_allclose(float(sumsq), float(ss64), rtol=2e-6)
            if mode == "clip" and n > 5:  # noqa: PLR2004
                assert math.sqrt(float(ss64)) * scale > 2.0 * clip
            tag = f"legacy {mode} n={n} step {step}"
            worst.check("p", p.cpu(), p64, p32, floor=2.0 * ulp(p64), what=tag)
            worst.defer("m", k, m.cpu(), m64, m32, what=tag)
            worst.defer("v", k, v.cpu(), v64, v32, what=tag)
    worst.line(f"sumsq+adamw_step '{mode}' from step {step0 + 1}")


# FlatAdamW ----------------------------------------------------------------------------------------------------------------------------------
class _Split(torch.nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.a = torch.nn.Linear(700, 700)
        self.dead = torch.nn.Linear(77, 301)  # registered, never called; 23 478 elements in the middle of the flat buffer
        self.b = torch.nn.Linear(700, 700)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.b(torch.tanh(self.a(x)))


@gpu
def test_flat_adamw_at_a_split_size(lib_loaded: None) -> None:
    """``FlatAdamW`` over ~1.0 M elements (four grid-stride laps' worth of threads in two, two laps of the sum) with a dead block in
    the middle: four steps, ``clip_norm = 0.5``, ``step(grad_scale = 0.5)``, against ``torch.optim.AdamW`` on a float64 twin whose
    gradients are halved before ``clip_grad_norm_``.  The twins are fed the device's own gradients, so that only the optimizer is
    compared; a float32 twin on the CPU sets the bound.  The dead layer stays bit-identical; the returned ``sumsq`` is the twin's
    unscaled squared norm."""
    import multimodal_mtrssm_amd as mt
    from multimodal_mtrssm_amd.optim import FlatParameters

    torch.manual_seed(11)
    net = _Split()
    twins = {dt: _Split().to(dt) for dt in (torch.float64, torch.float32)}
    for tw in twins.values():
        tw.load_state_dict(net.state_dict())
    net = net.to(DEV)
    dead0 = [q.detach().clone() for q in net.dead.parameters()]
    flat = FlatParameters(net)
    assert flat.numel > 2 * 2048 * 256 - 100000 and flat.numel > 4 * 512 * 256  # noqa: PLR2004
    opt = mt.FlatAdamW(flat, lr=1e-2, clip_norm=0.5)
    refs = {dt: torch.optim.AdamW(tw.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD) for dt, tw in twins.items()}
    live = [(k, q) for k, q in net.named_parameters() if not k.startswith("dead")]
    x = torch.randn(24, 700, device=DEV)
    for _ in range(4):
        opt.zero_grad()
        net(x).square().sum().backward()
        got_ss = opt.step(grad_scale=0.5)
        for dt, tw in twins.items():
            named = dict(tw.named_parameters())
            for k, q in live:
                named[k].grad = q.grad.detach().cpu().to(dt) * 0.5
            total = torch.nn.utils.clip_grad_norm_([named[k] for k, _ in live], 0.5)
            assert float(total) > 1.0  # noqa: PLR2004  (binding)
            if dt is torch.float64:
                want_ss = sum(float(q.grad.detach().cpu().double().square().sum()) for _, q in live)
                np.testing.assert_allclose(float(got_ss), want_ss, rtol=2e-6)
            refs[dt].step()
    worst = Worst()
    n64, n32 = dict(twins[torch.float64].named_parameters()), dict(twins[torch.float32].named_parameters())
    for k, q in live:
        ref = n64[k].detach().reshape(-1)
        worst.check("p", q.detach().cpu().reshape(-1), ref, n32[k].detach().reshape(-1), floor=2.0 * ulp(ref), what=f"FlatAdamW {k}")
    for q, q0, t64 in zip(net.dead.parameters(), dead0, twins[torch.float64].dead.parameters(), strict=True):
        assert torch.equal(q.view(torch.int32), q0.view(torch.int32)) and torch.equal(t64.float().cpu(), q0.cpu())
    assert float(opt.state[1]) == 4.0  # noqa: PLR2004
    worst.line(f"FlatAdamW, {flat.numel} elements, 4 steps")
