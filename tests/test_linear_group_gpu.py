"""GPU (MI355X): ``linear.linear_group`` against separate ``linear()`` calls on the same operands: outputs and every gradient
within 1e-6 of the tensor's largest entry (both run the fp32-MFMA kernel; sharing a launch may cut a reduction differently, which
reorders fp32 sums).  Whether the outputs came out bitwise equal is printed."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(3200, 4, 200), (3200, 256, 200), (130, 37, 30)]   # (M, in, out), mixed in one group
ELU = 2


def _operands(bias: bool, seed: int) -> list[tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]]:
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, (m, k, n) in enumerate(SHAPES):
        x = torch.randn(m, k, generator=g).to(DEV).requires_grad_(i != 0)   # the first input needs no gradient (the actions)
        w = (torch.randn(n, k, generator=g) / k**0.5).to(DEV).requires_grad_()
        b = torch.randn(n, generator=g).to(DEV).requires_grad_() if bias else None
        out.append((x, w, b))
    return out


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("pre_act", [0, ELU], ids=["plain", "preact"])
def test_group_equals_separate_calls(bias: bool, pre_act: int) -> None:
    from multimodal_mtrssm_amd.linear import linear, linear_group

    g = torch.Generator().manual_seed(7)
    gys = [torch.randn(m, n, generator=g).to(DEV) for m, _k, n in SHAPES]
    results = []
    for grouped in (True, False):
        ops = _operands(bias, 11)
        if grouped:
            ys = linear_group([(x, w, b, pre_act) for x, w, b in ops])
        else:
            ys = [linear(x, w, b, pre_act=pre_act) for x, w, b in ops]
        sum((y * gy).sum() for y, gy in zip(ys, gys, strict=True)).backward()
        torch.cuda.synchronize()
        assert ops[0][0].grad is None
        results.append(([y.detach() for y in ys], [t.grad for op in ops for t in op if t is not None and t.requires_grad]))
    (ys_g, grads_g), (ys_s, grads_s) = results
    print("outputs bitwise equal:", [bool(torch.equal(a, b)) for a, b in zip(ys_g, ys_s, strict=True)])
    print("gradients bitwise equal:", [bool(torch.equal(a, b)) for a, b in zip(grads_g, grads_s, strict=True)])
    assert len(grads_g) == len(grads_s) == 2 + 3 * (2 if bias else 1) - 0
    for what, got, want in [("output", a, b) for a, b in zip(ys_g, ys_s, strict=True)] + [("gradient", a, b) for a, b in zip(grads_g, grads_s, strict=True)]:
        scale = float(want.abs().max()) + 1e-30
        err = float((got - want).abs().max())
        print(f"{what} {tuple(want.shape)}: max error {err:.3e}, largest entry {scale:.3e}")
        assert err <= 1e-6 * scale, (what, tuple(want.shape), err, scale)  # noqa: PLR2004
