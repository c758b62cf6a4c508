"""GPU (MI355X): ``mtrssm_mrssm_scan_prepare`` -- the cooperative MRSSM scans' weight layouts in one launch -- against the torch
expressions it replaces.  The three transposes are exact copies (bitwise).  ``wf_t`` and ``bf`` are fp32 fma chains of H terms:
each element is compared with the float64 sum within ``H * 2^-24 * sum_h |term|``, the bound of such a chain, computed per
element from the float64 terms.  The parameters are views of one flat buffer, as in a ``FlatParameters`` model."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E = 24  # embedding width: wa1 / wv1 are [H, D + E], only their first D columns are read


@pytest.mark.parametrize(("D", "H", "S", "A"), [(200, 200, 30, 4), (32, 64, 12, 3), (1024, 1024, 128, 4)])
def test_layouts_match_the_torch_expressions(D: int, H: int, S: int, A: int) -> None:  # noqa: N803
    from multimodal_mtrssm_amd import scan

    shapes = {"w1": (H, A + S), "w2": (H, H), "b2": (H,), "wih": (3 * D, H), "bih": (3 * D,), "whh": (3 * D, D), "w3": (H, D),
              "wa1": (H, D + E), "wv1": (H, D + E)}
    g = torch.Generator().manual_seed(D + H)
    flat = ((torch.rand(3 + sum(torch.Size(s).numel() for s in shapes.values()), generator=g) * 2 - 1) / H**0.5).to(DEV)
    p, at = {}, 3  # (three floats in: the views do not start on 16-byte boundaries)
    for name, s in shapes.items():
        n = torch.Size(s).numel()
        p[name] = flat[at : at + n].view(s)
        at += n
    w1s_t, whh_t, wh1_t, wf_t, bf = scan._cluster_layouts(p["w1"], p["w2"], p["b2"], p["wih"], p["bih"], p["whh"], p["w3"], p["wa1"], p["wv1"],
                                                          D, H, S, A)
    if 2.0 * H * 3 * D * H >= scan._linear.SPLIT_MIN_FLOPS:
        # at this size the step leaves the product to the MFMA tile GEMM: ask the launch itself for it, as the small dims get it
        big = scan._linear.SPLIT_MIN_FLOPS
        scan._linear.SPLIT_MIN_FLOPS = float("inf")
        try:
            _, _, _, wf_t, bf = scan._cluster_layouts(p["w1"], p["w2"], p["b2"], p["wih"], p["bih"], p["whh"], p["w3"], p["wa1"], p["wv1"],
                                                      D, H, S, A)
        finally:
            scan._linear.SPLIT_MIN_FLOPS = big
    torch.cuda.synchronize()
    assert torch.equal(w1s_t, p["w1"][:, A:].t().contiguous())
    assert torch.equal(whh_t, p["whh"].t().contiguous())
    assert torch.equal(wh1_t, torch.cat([p["w3"], p["wa1"][:, :D], p["wv1"][:, :D]], dim=0).t().contiguous())
    w2, wih, b2, bih = (p[k].double().cpu() for k in ("w2", "wih", "b2", "bih"))
    eps = H * 2.0**-24
    want = w2.t() @ wih.t()                       # [H, 3D]: sum_h W2[h][k] W_ih[j][h]
    bound = eps * (w2.abs().t() @ wih.abs().t())
    err = (wf_t.double().cpu() - want).abs()
    print(f"wf_t: max error {float(err.max()):.3e}, smallest bound {float(bound.min()):.3e}, max error / bound {float((err / bound).max()):.3e}")
    assert bool((err <= bound).all())
    want_b = wih @ b2 + bih
    bound_b = eps * (wih.abs() @ b2.abs() + bih.abs())
    err_b = (bf.double().cpu() - want_b).abs()
    print(f"bf: max error {float(err_b.max()):.3e}, max error / bound {float((err_b / bound_b).max()):.3e}")
    assert bool((err_b <= bound_b).all())
