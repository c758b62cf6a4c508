"""GPU (MI355X): linear word probes, the kernel and end to end.

What is pinned here.  ``mtrssm_linear_probe_step`` against the float64 rule on seeded inputs (``tests/test_latent_probe_host.py``):

* logits through ``nll`` and ``pred``: ``|dz| <= (F + 2) 2^-24 (sum_f |x_f w_f| + |b|)`` (``logit_bound``; any summation order);
* ``nll`` per frame within ``2 max_c`` of that bound plus ``tau max(1, |ref|)``, ``tau`` = 8 x the worst residual of fp32 torch's
  ``log_softmax`` on the CPU against float64 on the same fp32 logits (``softmax_tau``: the allowance for exp / log);
* ``g_weight`` / ``g_bias`` element-wise within ``rho sum_n |p_n - y_n| |x_n|``, ``rho`` = 8 x the worst such ratio of the fp32 torch
  composition on the CPU on the same inputs, never above ``(N + F + 8) 2^-24``; the stats by the same scheme;
* ``pred`` equal to the float64 arg-max except on frames whose float64 top-two margin is under 4 x the larger logit bound, at most 2 %
  of the live frames; dead frames exactly 0 / -1; two calls bitwise equal; ``normalize`` = sums over the count.

Model level: group ``g`` of ``probe_features`` is the posterior feature of a ``likelihood_bound`` step that observes subset ``g`` under
the same uniforms, and ``probe_evaluate``'s table is the composition of ``probe_features``, the float64 rule and a torch fold.  The fit:
30 steps against ``torch.optim.AdamW`` on the float64 rule, bounded by 8 x what the fp32 torch composition shows on the CPU.
"""

from __future__ import annotations

import functools
import math

import pytest
import torch

import multimodal_mtrssm_amd as mt
from multimodal_mtrssm_amd import LatentProbe, LikelihoodBound, LinearProbe, _lib
from oracle.cases import CASES, build_batch, build_model, with_sizes
from tests.conftest import product_from_case
from tests.test_latent_probe_host import EPS, SHAPES, check_c_refusals, fp32_cpu, grad_scale, logit_bound, probe_inputs, probe_of, softmax_tau

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(inp: dict[str, torch.Tensor], col0: int, **kw) -> tuple[mt.ProbeStats, torch.Tensor, torch.Tensor]:  # noqa: ANN003
    probe = probe_of(inp, DEV)
    stats = probe.step(inp["x"].to(DEV), inp["labels"].to(DEV), col0=col0, planes=True, **kw)
    torch.cuda.synchronize()
    return stats, probe.weight.grad.clone(), probe.bias.grad.clone()


# 1. the kernel is the rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_probe_kernel_equals_the_float64_rule(shape: tuple[int, ...]) -> None:  # noqa: PLR0914, PLR0915
    g, n, f, c, _, col0 = shape
    inp = probe_inputs(*shape)
    labels = inp["labels"]
    live = labels >= 0
    inp["x"][:, ~live] = float("nan")  # a dead frame is not read
    want, _, _ = LinearProbe.rule(inp["x"], labels, inp["weight"], inp["bias"], col0=col0, grad=False)
    stats, g_w, g_b = _run(inp, col0, normalize=False)
    again, g_w2, g_b2 = _run(inp, col0, normalize=False)
    for a, b in zip((*stats, g_w, g_b), (*again, g_w2, g_b2), strict=True):
        assert torch.equal(a, b)  # two calls agree bitwise
    nll, hit, pred = stats.nll.cpu(), stats.hit.cpu(), stats.pred.cpu()
    # dead frames
    assert not bool(nll[:, ~live].any()) and not bool(hit[:, ~live].any()) and bool((pred[:, ~live] == -1).all())
    assert bool(torch.isfinite(nll).all()) and bool(torch.isfinite(g_w).all()) and bool(torch.isfinite(g_b).all())
    # nll
    lb = logit_bound(inp, col0)[:, live]  # [G, n_live, C]
    xs = inp["x"][:, live, col0 : col0 + f].double()
    z64 = torch.einsum("gnf,gcf->gnc", xs, inp["weight"].double()) + inp["bias"].double()[:, None]
    tau = softmax_tau(z64, labels[live])
    ref = want.nll[:, live]
    bound = 2.0 * lb.max(-1).values + tau * ref.abs().clamp_min(1.0)
    err = (nll[:, live].double() - ref).abs()
    cpu = fp32_cpu(inp, col0)
    print(f"shape {shape}: tau {tau:.3e}; nll worst err {float(err.max()):.3e}, worst err / bound {float((err / bound).max()):.3f}, "
          f"kernel's own residual / max(1, |ref|) {float((err / ref.abs().clamp_min(1.0)).max()):.3e}, "
          f"fp32 torch-CPU's {float(((cpu['nll'].double() - ref).abs() / ref.abs().clamp_min(1.0)).max()):.3e}")
    assert bool((err <= bound).all())
    # pred: the float64 arg-max outside the margin exemption
    top = z64.topk(2, dim=-1).values
    exempt = (top[..., 0] - top[..., 1]) < 4.0 * lb.max(-1).values
    frac = float(exempt.double().mean())
    print(f"shape {shape}: exempt {frac:.5f} of the live frames")
    assert frac <= 0.02  # noqa: PLR2004
    got_pred = pred[:, live]
    assert bool(((got_pred == want.pred[:, live]) | exempt).all()) and bool(((got_pred >= 0) & (got_pred < c)).all())
    assert torch.equal(hit[:, live], (got_pred == labels[live]).float())
    # the stats: count and hits exact (of the kernel's own planes), the nll sum by the frames' bounds plus its one rounding
    assert torch.equal(stats.count.cpu(), torch.full((g,), float(live.sum()))) and torch.equal(stats.hits.cpu(), hit.sum(1))
    total = stats.nll_sum.cpu().double()
    assert bool(((total - want.nll_sum).abs() <= bound.sum(1) + EPS * want.nll_sum.abs()).all())
    torch.testing.assert_close(total, nll.double().sum(1), rtol=2.0 * EPS, atol=0.0)
    # the gradients
    ref_w, ref_b, mag_w, mag_b = grad_scale(inp, col0)
    cap = (n + f + 8) * EPS
    for name, got, ref_g, mag, cpu_g in (("g_weight", g_w, ref_w, mag_w, cpu["g_weight"]), ("g_bias", g_b, ref_b, mag_b, cpu["g_bias"])):
        ratio_cpu = float(((cpu_g.double() - ref_g).abs() / mag).max())
        rho = min(8.0 * ratio_cpu, cap)
        ratio = float(((got.cpu().double() - ref_g).abs() / mag).max())
        print(f"shape {shape}: {name} kernel {ratio / EPS:.2f} x 2^-24, fp32 torch-CPU {ratio_cpu / EPS:.2f} x 2^-24, rho {rho / EPS:.2f} x 2^-24 "
              f"(cap {cap / EPS:.0f})")
        assert ratio <= rho, name
    # normalize = sums over the count (one fp32 division)
    _, m_w, m_b = _run(inp, col0, normalize=True)
    count = float(live.sum())
    torch.testing.assert_close(m_w, g_w / count, rtol=2.0 * EPS, atol=0.0)
    torch.testing.assert_close(m_b, g_b / count, rtol=2.0 * EPS, atol=0.0)


def test_probe_kernel_with_every_label_dead_and_without_grad() -> None:
    shape = SHAPES[2]
    inp = probe_inputs(*shape)
    dead = {**inp, "labels": torch.full_like(inp["labels"], -1), "x": torch.full_like(inp["x"], float("nan"))}
    for normalize in (False, True):
        stats, g_w, g_b = _run(dead, shape[5], normalize=normalize)
        for t in (stats.nll_sum, stats.hits, stats.count, stats.nll, stats.hit, g_w, g_b):
            assert not bool(t.any()) and bool(torch.isfinite(t).all())  # every sum exactly 0, nothing NaN
        assert bool((stats.pred == -1).all())
    # grad=False: the same stats and planes, the gradient buffers untouched
    probe = probe_of(inp, DEV)
    x, labels = inp["x"].to(DEV), inp["labels"].to(DEV)
    full = probe.step(x, labels, col0=shape[5], planes=True)
    probe.weight.grad.fill_(7.0)
    probe.bias.grad.fill_(7.0)
    only = probe.step(x, labels, col0=shape[5], grad=False, planes=True)
    torch.cuda.synchronize()
    for a, b in zip(full, only, strict=True):
        assert torch.equal(a, b)
    assert bool((probe.weight.grad == 7.0).all()) and bool((probe.bias.grad == 7.0).all())  # noqa: PLR2004
    assert probe.step(x, labels, col0=shape[5], grad=False).nll is None
    assert _lib.load().mtrssm_last_kernel() == b"mtrssm::linear_probe_kernel<eval>"


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


# 2. the model level ----------------------------------------------------------------------------------------------------------------------------
B, T = 3, 6
LENGTHS = (6, 4, 1)


@functools.lru_cache(maxsize=None)
def _setup(name: str):  # noqa: ANN202
    case = with_sizes(CASES[name], B, T)
    model = product_from_case(case, build_model(case), DEV)
    batch = tuple(x.to(DEV) for x in build_batch(case))
    return case, model, batch


def _noise(model, probe: LatentProbe, seed: int = 13) -> dict[str, torch.Tensor]:  # noqa: ANN001
    g = torch.Generator().manual_seed(seed)
    return {k: torch.rand(shape, generator=g).to(DEV) for k, shape in probe.noise_shapes(model, B, T).items()}


def _labels(seed: int = 7) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, 10, (B, T), generator=g).to(torch.int32)
    labels[torch.rand(B, T, generator=g) < 0.2] = -1  # noqa: PLR2004
    return labels


MODEL_CASES = [("mrssm_default", False), ("mmtrssm_default", False), ("mrssm_default", True), ("mmtrssm_default", True)]


@pytest.mark.parametrize(("name", "ragged"), MODEL_CASES)
def test_probe_features_are_the_subset_posteriors(name: str, ragged: bool) -> None:  # noqa: FBT001
    case, model, batch = _setup(name)
    probe = LatentProbe()
    noise = _noise(model, probe)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV) if ragged else None
    x, valid = model.probe_features(batch, probe, dict(noise), lengths)
    assert tuple(x.shape) == (3, B, T, LatentProbe.layout(model)["feature"][1]) and x.is_contiguous()
    assert (valid is None) if lengths is None else torch.equal(valid, lengths)
    for g, observe in enumerate(probe.observe):
        bound = LikelihoodBound(1, observe=observe)
        table = model.likelihood_bound(batch, bound, {k: v.unsqueeze(1) for k, v in noise.items()}, lengths, keep_states=True)
        s = table.states
        if case.kind == "mrssm":
            want = torch.cat([s.deter, s.stoch], dim=-1)
        else:
            want = torch.cat([s.deter_h, s.stoch_h, s.deter_l, s.stoch_l], dim=-1)
        # the same kernels on the same rows inside a batch of B * 3 instead of B rows: only a GEMM's tiling can differ
        print(name, observe, "bitwise" if torch.equal(x[g], want) else f"worst {float((x[g] - want).abs().max()):.3e}")
        torch.testing.assert_close(x[g], want, rtol=1e-5, atol=1e-6)
    assert not torch.equal(x[1], x[2])  # audio-only and vision-only posteriors differ


@pytest.mark.parametrize(("name", "ragged"), MODEL_CASES[1:3])
def test_probe_evaluate_is_features_rule_and_fold(name: str, ragged: bool) -> None:  # noqa: FBT001, PLR0914
    _, model, batch = _setup(name)
    probe = LatentProbe(part="lower" if name.startswith("mmtrssm") else "stoch")
    col0, width = probe.columns(model)
    linear = probe.linear(model)
    gen = torch.Generator().manual_seed(19)
    with torch.no_grad():
        linear.weight.copy_(torch.randn(linear.weight.shape, generator=gen) / math.sqrt(width))
        linear.bias.copy_(0.5 * torch.randn(linear.bias.shape, generator=gen))
    noise, labels = _noise(model, probe), _labels().to(DEV)
    lengths = torch.tensor(LENGTHS, dtype=torch.int32, device=DEV) if ragged else None
    table = model.probe_evaluate(batch, labels, probe, linear, None, dict(noise), lengths)
    table = model.probe_evaluate(batch, labels, probe, linear, table, dict(noise), lengths)  # (twice into one table)
    x, valid = model.probe_features(batch, probe, dict(noise), lengths)
    flat = mt.probe.frame_labels(labels, valid).cpu()
    live = flat >= 0
    inp = {"x": x.reshape(3, B * T, -1).cpu(), "labels": flat, "weight": linear.weight.detach().cpu(), "bias": linear.bias.detach().cpu()}
    want, _, _ = LinearProbe.rule(inp["x"], flat, inp["weight"], inp["bias"], col0=col0, grad=False)
    lb = logit_bound(inp, col0).max(-1).values  # [G, N]
    z64 = torch.einsum("gnf,gcf->gnc", inp["x"][:, live, col0 : col0 + width].double(), inp["weight"].double()) + inp["bias"].double()[:, None]
    tau = softmax_tau(z64, flat[live])
    bound = torch.where(live[None], 2.0 * lb + tau * want.nll.abs().clamp_min(1.0), torch.zeros(()).double()).reshape(3, B, T)
    assert torch.equal(table.counts.cpu(), 2.0 * live.reshape(B, T).float().sum(0))
    got_nll, ref_nll = table.nll.cpu().double(), 2.0 * want.nll.reshape(3, B, T).sum(1)
    assert bool(((got_nll - ref_nll).abs() <= 2.0 * bound.sum(1) + 2 * B * EPS * ref_nll.abs()).all())
    top = z64.topk(2, dim=-1).values
    exempt = torch.zeros(3, B * T, dtype=torch.bool)
    exempt[:, live] = (top[..., 0] - top[..., 1]) < 4.0 * lb[:, live]
    stats = table.stats
    assert bool(((stats.pred.cpu() == want.pred) | exempt).all())
    assert torch.equal(table.hit.cpu(), 2.0 * stats.hit.cpu().reshape(3, B, T).sum(1))  # small whole numbers: exact in fp32
    scalars = table.scalars("probe")
    assert float(scalars["probe/audio/acc"]) == pytest.approx(float(stats.hit[1].sum()) / float(live.sum()))


# 3. the fit ------------------------------------------------------------------------------------------------------------------------------------
def _planted(n: int = 2048, f: int = 48, c: int = 10) -> tuple[torch.Tensor, torch.Tensor]:
    gen = torch.Generator().manual_seed(31)
    x0 = torch.tanh(torch.randn(n, f, generator=gen))
    x = torch.stack([x0, torch.tanh(x0 + 0.5 * torch.randn(n, f, generator=gen))]).contiguous()
    labels = (x0 @ torch.randn(f, c, generator=gen)).argmax(-1).to(torch.int32)
    labels[torch.rand(n, generator=gen) < 0.1] = -1  # noqa: PLR2004
    return x, labels


def test_fit_follows_adamw_on_the_float64_rule() -> None:
    x, labels = _planted()
    live = labels >= 0
    steps, lr = 30, 1e-2

    def torch_fit(dtype: torch.dtype) -> tuple[torch.Tensor, torch.Tensor]:
        w = torch.zeros(2, 10, 48, dtype=dtype, requires_grad=True)
        b = torch.zeros(2, 10, dtype=dtype, requires_grad=True)
        opt = torch.optim.AdamW([w, b], lr=lr, weight_decay=0.0)
        xs, lab = x[:, live].to(dtype), labels[live].long()
        for _ in range(steps):
            opt.zero_grad()
            z = torch.einsum("gnf,gcf->gnc", xs, w) + b[:, None]
            sum(torch.nn.functional.cross_entropy(z[i], lab) for i in range(2)).backward()
            opt.step()
        return w.detach().double(), b.detach().double()

    w64, b64 = torch_fit(torch.float64)
    w32, b32 = torch_fit(torch.float32)
    probe = LinearProbe(2, 48, 10).to(DEV)
    probe.fit(x.to(DEV), labels.to(DEV), steps, lr=lr)
    torch.cuda.synchronize()
    for name, got, ref, cpu in (("weight", probe.weight, w64, w32), ("bias", probe.bias, b64, b32)):
        ours, theirs = float((got.detach().cpu().double() - ref).abs().max()), float((cpu - ref).abs().max())
        print(f"fit {name}: |kernel - float64| {ours:.3e}, |fp32 torch-CPU - float64| {theirs:.3e}, max |{name}| {float(ref.abs().max()):.3e}")
        assert ours <= 8.0 * theirs, name


def test_fit_beats_the_zero_classifier() -> None:
    x, labels = _planted()
    x, labels = x.to(DEV), labels.to(DEV)
    probe = LinearProbe(2, 48, 10).to(DEV)
    zero = probe.step(x, labels, grad=False)
    probe.fit(x, labels, 300, lr=1e-2)
    after = probe.step(x, labels, grad=False)
    acc0, acc = (zero.hits / zero.count).cpu(), (after.hits / after.count).cpu()
    print("training accuracy: zero weights", acc0.tolist(), "after 300 steps", acc.tolist())
    assert bool((acc > acc0).all())


# 4. the command-line tool ------------------------------------------------------------------------------------------------------------------------
def test_latent_probe_cli_writes_the_subset_by_part_table(tmp_path, monkeypatch) -> None:  # noqa: ANN001
    """``tools/latent_probe.py`` end to end, in process, on four synthetic episodes (one shorter than a window) and an untrained model."""
    import json
    import sys

    import numpy as np

    sys.path.insert(0, str(mt._lib._HERE.parent / "tools"))  # noqa: SLF001
    import latent_probe
    import word_transitions

    rng = np.random.default_rng(3)
    for split, lengths in (("train", (12, 9)), ("test", (12, 5))):
        (tmp_path / split).mkdir()
        for i, n in enumerate(lengths):
            label = rng.integers(-1, 10, n).astype(np.int64)
            label[0] = 3
            np.savez(tmp_path / split / f"ep{i}.npz", audio=rng.uniform(-80.0, 0.0, (n, 32, 32)).astype(np.float32),
                     image=rng.uniform(0.0, 255.0, (n, 1, 32, 32)).astype(np.float32), label=label,
                     speaker=np.eye(6, dtype=np.float32)[np.full(n, i)])
    dims = (8, 8, 4, 2, 16)
    torch.manual_seed(0)
    torch.save(word_transitions.build_model("mrssm", dims, "cpu").state_dict(), tmp_path / "model.ckpt")
    out = tmp_path / "results" / "probe"
    monkeypatch.setattr(sys, "argv", ["latent_probe.py", "--checkpoint", str(tmp_path / "model.ckpt"), "--train-data-dir", str(tmp_path / "train"),
                                      "--test-data-dir", str(tmp_path / "test"), "--output", str(out), "--dims", ",".join(map(str, dims)),
                                      "--window", "6", "--batch", "3", "--fit-steps", "20"])
    latent_probe.main()
    results = json.loads(out.with_suffix(".json").read_text())
    assert list(results) == ["feature", "deter", "stoch"] and results["stoch"]["columns"] == [8, 8]
    for part in results.values():
        assert part["train_frames"] > 0 and part["test_frames"] > 0
        for subset in ("both", "audio", "vision"):
            assert 0.0 <= part[subset]["acc"] <= 1.0 and math.isfinite(part[subset]["nll"]) and len(part[subset]["acc_by_position"]) == 6  # noqa: PLR2004
    table = out.with_suffix(".md").read_text()
    assert "| Observes | feature | deter | stoch |" in table and "| vision |" in table
