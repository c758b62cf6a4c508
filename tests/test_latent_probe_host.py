"""CPU: linear word probes on subset posteriors -- validation, the feature layouts, ``ProbeTable`` against a hand
count, the torch rule against ``torch.nn.functional.cross_entropy``'s autograd in float64, and the C entry points' refusals (they return
before any launch).  The inputs and tolerance helpers (``probe_inputs``, ``logit_bound``, ...) are shared with
``tests/test_latent_probe_gpu.py`` and ``tests/test_latent_probe_gloo.py``."""

from __future__ import annotations

import math

import pytest
import torch

from multimodal_mtrssm_amd import LatentProbe, LinearProbe, ProbeTable, StateCarry, _lib
from multimodal_mtrssm_amd.probe import frame_labels
from oracle.cases import CASES, build_batch, build_model
from tests.conftest import product_from_case

EPS = 2.0 ** -24

# (G, N, F, C, ld, col0): one row and an odd F; the default MRSSM feature; a slice at an unaligned col0 with F no multiple of 4; the
# bench F over many workgroups with a ragged last tile; a large F with the full class tile
SHAPES = [(1, 1, 7, 2, 7, 0), (3, 300, 48, 10, 48, 0), (2, 257, 46, 10, 96, 50), (3, 4099, 230, 10, 230, 0), (1, 513, 1152, 16, 1152, 0)]


def probe_inputs(g: int, n: int, f: int, c: int, ld: int, col0: int, seed: int = 5, dead: float = 0.2) -> dict[str, torch.Tensor]:  # noqa: PLR0913
    """Seeded ``tanh(randn)`` features, ``W ~ randn / sqrt(F)``, ``b ~ 0.5 randn`` and random labels, about ``dead`` of them -1 (at
    least one live frame)."""
    gen = torch.Generator().manual_seed(seed + 1000 * f + n)
    x = torch.tanh(torch.randn(g, n, ld, generator=gen))
    weight = torch.randn(g, c, f, generator=gen) / math.sqrt(f)
    bias = 0.5 * torch.randn(g, c, generator=gen)
    labels = torch.randint(0, c, (n,), generator=gen).to(torch.int32)
    labels[torch.rand(n, generator=gen) < dead] = -1
    if dead < 1.0:
        labels[0] = labels[0].clamp_min(0)
    del col0
    return {"x": x, "weight": weight, "bias": bias, "labels": labels}


def probe_of(inp: dict[str, torch.Tensor], device: str = "cpu") -> LinearProbe:
    g, c, f = inp["weight"].shape
    probe = LinearProbe(g, f, c)
    with torch.no_grad():
        probe.weight.copy_(inp["weight"])
        probe.bias.copy_(inp["bias"])
    return probe.to(device)


def logit_bound(inp: dict[str, torch.Tensor], col0: int) -> torch.Tensor:
    """``[G, N, C]`` in float64: ``(F + 2) 2^-24 (sum_f |x_f w_f| + |b|)``, which bounds the error of an fp32 dot product plus bias in
    any summation order."""
    f = inp["weight"].shape[-1]
    xs = inp["x"][:, :, col0 : col0 + f].double().abs().nan_to_num(0.0)
    return (f + 2) * EPS * (torch.einsum("gnf,gcf->gnc", xs, inp["weight"].double().abs()) + inp["bias"].double().abs()[:, None])


def fp32_cpu(inp: dict[str, torch.Tensor], col0: int) -> dict[str, torch.Tensor]:
    """The same step composed from fp32 torch ops on the CPU: the yardstick the measured parts of the tolerances come from."""
    f = inp["weight"].shape[-1]
    c = inp["weight"].shape[1]
    live = inp["labels"] >= 0
    xs = inp["x"][:, live, col0 : col0 + f]
    lab = inp["labels"][live].long()
    z = torch.einsum("gnf,gcf->gnc", xs, inp["weight"]) + inp["bias"][:, None]
    logp = torch.log_softmax(z, dim=-1)
    nll = -logp.gather(-1, lab[None, :, None].expand(z.shape[0], -1, 1)).squeeze(-1)
    d = torch.softmax(z, dim=-1) - torch.nn.functional.one_hot(lab, c).to(torch.float32)
    return {"nll": nll, "g_weight": torch.einsum("gnc,gnf->gcf", d, xs), "g_bias": d.sum(1), "live": live}


def softmax_tau(z64: torch.Tensor, lab: torch.Tensor) -> float:
    """8 x the worst residual of fp32 torch's ``log_softmax`` on the CPU against float64 ON THE SAME fp32 logits, relative to
    ``max(1, |nll|)``: the allowance for exp / log (the device's are not correctly rounded either, hence the margin)."""
    z32 = z64.to(torch.float32)
    idx = lab.long()[None, :, None].expand(z32.shape[0], -1, 1)
    got = -torch.log_softmax(z32, dim=-1).gather(-1, idx).squeeze(-1).double()
    want = -torch.log_softmax(z32.double(), dim=-1).gather(-1, idx).squeeze(-1)
    return 8.0 * float(((got - want).abs() / want.abs().clamp_min(1.0)).max())


def grad_scale(inp: dict[str, torch.Tensor], col0: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Float64 sums (not normalised) ``g_weight``, ``g_bias`` and their magnitudes ``sum_n |p - y| |x|`` and ``sum_n |p - y|``."""
    f = inp["weight"].shape[-1]
    c = inp["weight"].shape[1]
    live = inp["labels"] >= 0
    xs = inp["x"][:, live, col0 : col0 + f].double()
    z = torch.einsum("gnf,gcf->gnc", xs, inp["weight"].double()) + inp["bias"].double()[:, None]
    d = torch.softmax(z, dim=-1) - torch.nn.functional.one_hot(inp["labels"][live].long(), c).double()
    return (torch.einsum("gnc,gnf->gcf", d, xs), d.sum(1), torch.einsum("gnc,gnf->gcf", d.abs(), xs.abs()), d.abs().sum(1))


# -- 1. validation ------------------------------------------------------------------------------------------------------------------------
def test_latent_probe_validation() -> None:
    assert LatentProbe().observe == ("both", "audio", "vision") and LatentProbe().groups == 3 and LatentProbe().samples == 3  # noqa: PLR2004
    assert LatentProbe(("vision",), "stoch").groups == 1
    for bad in ("both", (), ("both", "both"), ("sound",), ("audio", 3)):
        with pytest.raises(ValueError, match="observe"):
            LatentProbe(bad)
    with pytest.raises(ValueError, match="part"):
        LatentProbe(part="hidden")
    probe = LatentProbe(("audio", "both"))
    assert probe.copy_bits("cpu").tolist() == [1, 3] and probe.copy_observed("cpu").tolist() == [[True, False], [True, True]]
    bound = probe.for_group("a group")
    assert bound is not probe and bound.group == "a group" and probe.group is None and bound.observe == probe.observe


def test_linear_probe_validation() -> None:
    for kw in ({"groups": 0}, {"features": 0}, {"classes": 1}, {"classes": 17}, {"groups": True}, {"features": 2.0}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            LinearProbe(**{"groups": 2, "features": 5, "classes": 4, **kw})
    probe = LinearProbe(2, 5, 4)
    assert tuple(probe.weight.shape) == (2, 4, 5) and tuple(probe.bias.shape) == (2, 4) and not bool(probe.weight.any()) and not bool(probe.bias.any())
    x, labels = torch.zeros(2, 6, 8), torch.zeros(6, dtype=torch.int32)
    with pytest.raises(ValueError, match="float32"):
        probe.step(x.double(), labels)
    with pytest.raises(ValueError, match="float32"):
        probe.step(x[:1], labels)
    with pytest.raises(ValueError, match="columns"):
        probe.step(x, labels, col0=4)
    with pytest.raises(ValueError, match="columns"):
        probe.step(x, labels, col0=-1)
    with pytest.raises(ValueError, match="labels"):
        probe.step(x, labels.long())
    with pytest.raises(ValueError, match="labels"):
        probe.step(x, labels[:5])
    with pytest.raises(ValueError, match="2\\^24"):
        LinearProbe.rule(torch.zeros(2, 1 << 24, 8, device="meta"), torch.zeros(1 << 24, dtype=torch.int32, device="meta"), probe.weight, probe.bias)
    with pytest.raises(ValueError, match="steps"):
        probe.fit(x, labels, 0)
    # the zero classifier: nll = log C per live frame, pred = class 0
    labels = torch.tensor([0, 3, -1, 2, 7, 0], dtype=torch.int32)  # (7 >= C: dead)
    stats = probe.step(x, labels, col0=3, planes=True)
    assert stats.count.tolist() == [4.0, 4.0] and stats.hits.tolist() == [2.0, 2.0]
    torch.testing.assert_close(stats.nll_sum, torch.full((2,), 4 * math.log(4.0)))
    assert stats.pred.tolist() == [[0, 0, -1, 0, -1, 0]] * 2 and stats.nll[:, 2].tolist() == [0.0, 0.0] and stats.hit[:, 4].tolist() == [0.0, 0.0]


# -- 2. part -> (col0, F) -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["mrssm_nonsquare", "mmtrssm_default"])
def cpu_model(request):  # noqa: ANN001, ANN201
    case = CASES[request.param]
    return case, product_from_case(case, build_model(case), "cpu")


def test_parts_resolve_to_columns_of_the_feature(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    d = case.dims
    if case.kind == "mrssm":
        stoch = d.cats * d.classes
        want = {"feature": (0, d.deter + stoch), "deter": (0, d.deter), "stoch": (d.deter, stoch)}
        refused = ("higher", "lower")
        shapes = {"u_init": (4, d.cats), "u_post": (4, 6, d.cats)}
    else:
        hs, ls = d.hs_cats * d.hs_classes, d.ls_cats * d.ls_classes
        want = {"feature": (0, model.feature_dim), "higher": (0, model.hd_dim + hs), "lower": (model.hd_dim + hs, model.ld_dim + ls)}
        assert model.hs_dim == hs and model.ls_dim == ls
        refused = ("deter", "stoch")
        shapes = {"u_init_h": (4, d.hs_cats), "u_init_l": (4, d.ls_cats), "u_post_l": (4, 6, d.ls_cats), "u_post_h": (4, 6, d.hs_cats)}
    assert LatentProbe.layout(model) == want
    for part, cols in want.items():
        assert LatentProbe(part=part).columns(model) == cols
        linear = LatentProbe(("audio", "vision"), part).linear(model, classes=7)
        assert (linear.groups, linear.features, linear.classes) == (2, cols[1], 7)
    for part in refused:
        with pytest.raises(ValueError, match="contiguous"):
            LatentProbe(part=part).columns(model)
    assert LatentProbe().noise_shapes(model, 4, 6) == shapes  # the model's own: the copies of a row share them


def test_probe_steps_refuse_masked_batches_and_a_set_carry(cpu_model) -> None:  # noqa: ANN001
    case, model = cpu_model
    batch = build_batch(case)
    b, t = batch[0].shape[:2]
    probe = LatentProbe()
    linear = probe.linear(model)
    labels = torch.zeros(b, t, dtype=torch.int32)
    with pytest.raises(ValueError, match="masked"):
        model.probe_features((*batch, torch.ones(b, t, 2, dtype=torch.bool)), probe)
    with pytest.raises(ValueError, match="LatentProbe"):
        model.probe_features(batch, 3)
    model.state_carry = StateCarry.for_model(model, b)
    try:
        with pytest.raises(ValueError, match="state_carry"):
            model.probe_features(batch, probe)
        with pytest.raises(ValueError, match="state_carry"):
            model.probe_evaluate(batch, labels, probe, linear)
    finally:
        model.state_carry = None
    with pytest.raises(ValueError, match="LinearProbe"):
        model.probe_evaluate(batch, labels, probe, torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="groups"):
        model.probe_evaluate(batch, labels, LatentProbe(("audio",)), linear)
    with pytest.raises(ValueError, match="labels"):
        model.probe_evaluate(batch, labels[:, :-1], probe, linear)
    with pytest.raises(ValueError, match="ProbeTable"):
        model.probe_evaluate(batch, labels, probe, linear, table=ProbeTable(3, t + 1))


# -- 3. ProbeTable against a hand count ----------------------------------------------------------------------------------------------------------
def test_probe_table_fold_add_scalars() -> None:
    g, b, t = 2, 3, 4
    labels = torch.tensor([[1, -1, 0, 2], [0, 0, -1, -1], [2, 1, 1, 5]], dtype=torch.int32)
    flat = frame_labels(labels, torch.tensor([4, 2, 3], dtype=torch.int32))  # row 2's last frame is past its end
    assert flat.tolist() == [1, -1, 0, 2, 0, 0, -1, -1, 2, 1, 1, -1]
    live = (flat >= 0).reshape(b, t)
    gen = torch.Generator().manual_seed(3)
    hit = (torch.rand(g, b, t, generator=gen) < 0.5).float() * live  # noqa: PLR2004
    nll = torch.rand(g, b, t, generator=gen) * live
    table = ProbeTable(g, t).fold(hit, nll, live)
    assert table.observe == ("both", "audio") and tuple(table.buffer.shape) == (2 * g + 1, t)
    assert table.counts.tolist() == [3.0, 2.0, 2.0, 1.0]
    for i in range(g):
        for pos in range(t):  # the fold adds a bin's frames in ascending b
            want_hit, want_nll = torch.zeros(()), torch.zeros(())
            for row in range(b):
                if live[row, pos]:
                    want_hit, want_nll = want_hit + hit[i, row, pos], want_nll + nll[i, row, pos]
            assert float(table.hit[i, pos]) == float(want_hit) and float(table.nll[i, pos]) == float(want_nll)
    twice = ProbeTable(g, t).add(table).add(table)
    assert torch.equal(twice.buffer, 2 * table.buffer)
    assert table.all_reduce() is table  # no process group: a no-op
    with pytest.raises(ValueError, match="do not add"):
        table.add(ProbeTable(g, t + 1))
    with pytest.raises(ValueError, match="need hit"):
        table.fold(hit, nll[:1], live)
    scalars = table.scalars("val/probe")
    assert set(scalars) == {f"val/probe/{s}/{k}" for s in ("both", "audio") for k in ("acc", "nll")}
    assert float(scalars["val/probe/audio/acc"]) == pytest.approx(float(hit[1].sum()) / 8.0)
    assert float(scalars["val/probe/both/nll"]) == pytest.approx(float(nll[0].sum()) / 8.0)
    assert set(ProbeTable(3, t).scalars("p")) == {f"p/{s}/{k}" for s in ("both", "audio", "vision") for k in ("acc", "nll")}
    assert all(math.isnan(float(v)) for v in ProbeTable(3, t).scalars("p").values())
    curves = table.curves()
    assert float(curves["both"]["acc"][3]) == float(hit[0, 0, 3])


# -- 4. the rule against autograd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES[:3])
def test_rule_equals_cross_entropy_autograd_in_float64(shape: tuple[int, ...]) -> None:
    g, n, f, c, _, col0 = shape
    inp = probe_inputs(*shape)
    live = inp["labels"] >= 0
    w = inp["weight"].double().requires_grad_()
    b = inp["bias"].double().requires_grad_()
    z = torch.einsum("gnf,gcf->gnc", inp["x"][:, :, col0 : col0 + f].double(), w) + b[:, None]
    lab = inp["labels"][live].long()
    per = torch.stack([torch.nn.functional.cross_entropy(z[i][live], lab, reduction="none") for i in range(g)])
    per.sum().backward()
    stats, g_w, g_b = LinearProbe.rule(inp["x"], inp["labels"], inp["weight"], inp["bias"], col0=col0, normalize=False)
    torch.testing.assert_close(stats.nll[:, live], per.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g_w, w.grad, rtol=1e-11, atol=1e-12)
    torch.testing.assert_close(g_b, b.grad, rtol=1e-11, atol=1e-12)
    assert torch.equal(stats.pred[:, live], z.detach()[:, live].argmax(-1).to(torch.int32)) and bool((stats.pred[:, ~live] == -1).all())
    assert not bool(stats.nll[:, ~live].any()) and not bool(stats.hit[:, ~live].any())
    assert stats.count.tolist() == [float(live.sum())] * g
    torch.testing.assert_close(stats.hits, ((stats.pred == inp["labels"]) & live).double().sum(1))
    _, m_w, m_b = LinearProbe.rule(inp["x"], inp["labels"], inp["weight"], inp["bias"], col0=col0, normalize=True)
    torch.testing.assert_close(m_w, g_w / float(live.sum()), rtol=1e-14, atol=0.0)
    torch.testing.assert_close(m_b, g_b / float(live.sum()), rtol=1e-14, atol=0.0)
    # the non-GPU route of step: the rule, rounded to fp32, into .grad
    probe = probe_of(inp)
    got = probe.step(inp["x"], inp["labels"], col0=col0, planes=True)
    assert torch.equal(probe.weight.grad, m_w.float()) and torch.equal(probe.bias.grad, m_b.float())
    assert torch.equal(got.nll, stats.nll.float()) and torch.equal(got.pred, stats.pred) and got.nll_sum.dtype == torch.float32
    probe.weight.grad.fill_(7.0)
    assert probe.step(inp["x"], inp["labels"], col0=col0, grad=False).nll is None and bool((probe.weight.grad == 7.0).all())  # noqa: PLR2004


def test_rule_with_no_live_frame_and_a_lowest_index_tie() -> None:
    inp = probe_inputs(2, 9, 5, 4, 5, 0, dead=1.0)
    inp["x"][0, 3] = float("nan")  # a dead frame is not read
    stats, g_w, g_b = LinearProbe.rule(inp["x"], inp["labels"], inp["weight"], inp["bias"])
    for t in (stats.nll_sum, stats.hits, stats.count, stats.nll, stats.hit, g_w, g_b):
        assert not bool(t.any()) and bool(torch.isfinite(t).all())
    assert bool((stats.pred == -1).all())
    weight = torch.zeros(1, 3, 2)
    weight[0, 1, 0] = weight[0, 2, 0] = 1.0  # classes 1 and 2 tie for the largest logit
    stats, _, _ = LinearProbe.rule(torch.ones(1, 1, 2), torch.tensor([2], dtype=torch.int32), weight, torch.zeros(1, 3))
    assert stats.pred.tolist() == [[1]] and stats.hits.tolist() == [0.0]


def test_fit_learns_planted_labels_on_the_cpu() -> None:
    gen = torch.Generator().manual_seed(2)
    x = torch.tanh(torch.randn(2, 256, 12, generator=gen))
    labels = (x[0] @ torch.randn(12, 4, generator=gen)).argmax(-1).to(torch.int32)
    probe = LinearProbe(2, 12, 4)
    zero = probe.step(x, labels, grad=False)
    probe.fit(x, labels, 60, lr=5e-2)
    after = probe.step(x, labels, grad=False)
    assert float(after.hits[0]) > float(zero.hits[0]) + 64 and float(after.nll_sum[0]) < float(zero.nll_sum[0])  # noqa: PLR2004


# -- 5. the C entry points ------------------------------------------------------------------------------------------------------------------------
def workspace_rule(g: int, n: int, c: int, f: int) -> int:
    """The workspace of a step: per group ``P`` partial sets of 3 doubles and ``C F + C`` floats, ``P`` = the tiles of 16 rows cut into
    runs of ``max(2, ceil(tiles / 256))`` (of all of them when there are fewer)."""
    tiles = -(-n // 16)
    per = min(max(2, -(-tiles // 256)), tiles)
    return g * -(-tiles // per) * (24 + 4 * (c * f + c))


def check_c_refusals(lib) -> None:  # noqa: ANN001
    """Every ``-1`` return of the probe's entry points; each call returns before a launch (also run on the GPU machine)."""
    ok = 0x10000  # never dereferenced
    good = {"x": ok, "ld": 96, "col0": 50, "labels": ok, "weight": ok, "bias": ok, "G": 2, "N": 257, "C": 10, "F": 46, "normalize": 1, "g_weight": ok,
            "g_bias": ok, "stats": ok, "nll": ok, "hit": ok, "pred": ok, "workspace": ok, "bytes": workspace_rule(2, 257, 10, 46)}

    def step(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_linear_probe_step(a["x"], a["ld"], a["col0"], a["labels"], a["weight"], a["bias"], a["G"], a["N"], a["C"], a["F"],
                                            a["normalize"], a["g_weight"], a["g_bias"], a["stats"], a["nll"], a["hit"], a["pred"], a["workspace"],
                                            a["bytes"], None)

    for name in ("x", "labels", "weight", "bias", "stats", "workspace"):
        assert step(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
    assert step(g_weight=None) == -1 and step(g_bias=None) == -1 and b"neither" in lib.mtrssm_last_error()
    for name in ("x", "labels", "weight", "bias", "g_weight", "g_bias", "stats", "nll", "hit", "pred", "workspace"):
        assert step(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    assert step(workspace=ok + 4) == -1 and b"aligned" in lib.mtrssm_last_error()
    for kw in ({"C": 1}, {"C": 17}, {"C": 0}, {"N": 0}, {"N": -4}, {"N": 1 << 24}, {"G": 0}, {"F": 0}, {"F": 2049}):
        assert step(**kw) == -1 and b"linear_probe_step: need G" in lib.mtrssm_last_error(), kw
        assert lib.mtrssm_linear_probe_workspace_bytes(*({**good, **kw}[k] for k in ("G", "N", "C", "F"))) == -1, kw
    for kw in ({"col0": -1}, {"col0": 51}, {"ld": 45}, {"G": 1 << 10, "N": 1 << 20, "ld": 2, "F": 1, "col0": 0}, {"G": 1 << 30, "N": 1 << 23, "ld": 1 << 20}):
        assert step(**{"bytes": 1 << 62, **kw}) == -1 and b"col0" in lib.mtrssm_last_error(), kw
    assert step(normalize=2) == -1 and step(normalize=-1) == -1 and b"normalize" in lib.mtrssm_last_error()
    assert step(bytes=good["bytes"] - 1) == -1 and b"workspace" in lib.mtrssm_last_error()
    assert step(bytes=0) == -1


def test_c_entries_reject_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


def test_workspace_size_is_pinned() -> None:
    lib = _lib.load()
    assert lib.mtrssm_linear_probe_workspace_bytes(3, 4099, 10, 230) == workspace_rule(3, 4099, 10, 230) == 3 * 129 * (24 + 4 * 2310)
    assert lib.mtrssm_linear_probe_workspace_bytes(1, 1, 2, 7) == workspace_rule(1, 1, 2, 7) == 24 + 4 * 16
    assert lib.mtrssm_linear_probe_workspace_bytes(3, 65536, 10, 230) == 3 * 256 * (24 + 4 * 2310)
