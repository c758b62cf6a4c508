"""GPU (MI355X): the options every other parity test leaves at one value -- the four activations of ``_lib.ACT_IDS`` in the scan,
conv and GEMM kernels, both KL weightings with ``kl_coeff`` / ``w_kl_h`` != 1, the cluster scan's 64 and 128 instances and the
wide scans with D != H -- against the oracle resp. float64 on the CPU (``tests/config_matrix.py`` holds the cases).

Tolerances are those of the existing tests of the same quantities (``tests/test_gpu_parity.py``):
  scan losses                 2e-5 relative                         (test_shared_step_matches_golden_and_oracle)
  deter / hidden / probs      1e-5 absolute, wide families + 5e-6   (test_mrssm_rollout_matches_golden, test_wide_* at three pieces)
  one-hot samples             exact
  scan gradients              2e-4 of the tensor's max; wide: 1e-3  (test_shared_step_..., test_large_dims_match_oracle)
  conv / deconv kernels       test_conv2d_kernel / test_conv_transpose2d_kernel, unchanged
  GEMM                        2e-6 of the scale, two pieces 3e-5    (test_gemm_kernel)
  conv stacks                 test_encoder_decoder_match_oracle, unchanged
"""

from __future__ import annotations

import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F  # noqa: N812

from oracle.cases import CASES, build_batch, build_model
from oracle.ref_model import cat_probs
from tests.config_matrix import OPTION_SETS, RELU_VALUES_ONLY, SCAN_CASES, options, relu_margin_for, screened, screened_prior, with_options
from tests.conftest import product_from_case
from tests.test_gpu_parity import CONV_CASES, DECONV_CASES, GEMM_CASES, fp32_grade_mode  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().float().cpu().numpy()


def _to(noise: dict[str, torch.Tensor], device: str) -> dict[str, torch.Tensor]:
    return {k: v.to(device) for k, v in noise.items()}


def _index(stoch: torch.Tensor, cats: int, classes: int) -> np.ndarray:
    return _np(stoch).reshape(*stoch.shape[:-1], cats, classes).argmax(-1)


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


# ---------------------------------------------------------------------------------------------
# 3a. scan families x options, against the oracle
# ---------------------------------------------------------------------------------------------
def _scan_kernels(family: str, case, pieces: int) -> tuple[str, str]:  # noqa: ANN001
    """The device kernels (forward, BPTT) a family's train step must launch, as ``mtrssm_last_kernel()`` names them."""
    if family == "scan":
        return "mtrssm::mrssm_fwd_kernel<", "mtrssm::mrssm_bwd_kernel<"
    if family == "cluster":
        return f"mtrssm::mrssm_fwd_cluster_kernel<{case.dims.deter}, ", f"mtrssm::mrssm_bwd_cluster_kernel<{case.dims.deter}, "
    if family == "wide":
        return f"mtrssm::mrssm_wide_fwd_kernel<{pieces}, ", f"mtrssm::mrssm_wide_bwd_kernel<{pieces}, "
    if family == "mt_scan":
        return "mtrssm::mmtrssm_fwd_kernel<", "mtrssm::mmtrssm_bwd_kernel<"
    assert family == "mt_wide"
    return f"mtrssm::mmtrssm_wide_fwd_kernel<{pieces}, ", f"mtrssm::mmtrssm_wide_bwd_kernel<{pieces}, "


_WIDE_PIECES = 3  # the wide families run on three bf16 pieces per operand: what the value tolerance below is stated for


def compare_scan_family(case, family: str, oracle, batch, noise, *, pieces: int = _WIDE_PIECES, grads: bool = True):  # noqa: ANN001, ANN201, PLR0913, PLR0914, PLR0915
    """One train step of ``case`` on the GPU against ``oracle`` on the same batch and noise: the rollout's values and samples,
    every loss, every parameter gradient (unless ``grads`` is off) and the names of the forward and BPTT kernels that ran, which
    must be ``family``'s.  The wide families run on ``pieces`` bf16 pieces per operand; the tolerances are the docstring's at
    three pieces, and at two those ``scan.py`` states for them (probabilities 1e-5 + 5e-6, losses 1e-4 relative, gradients 1e-3;
    deter / hidden carry no stated bound there and are left to the three-piece run).  Returns (model, train step's output,
    initial state, posterior, prior) for further checks."""
    from multimodal_mtrssm_amd import _lib, scan

    d = case.dims
    wide = family in {"wide", "mt_wide"}
    two = wide and pieces == 2  # noqa: PLR2004
    ref = oracle.shared_step(batch, noise)
    oracle.zero_grad(set_to_none=True)
    ref["loss"].backward()
    model = product_from_case(case, oracle, DEV)
    gbatch, gnoise = tuple(b.to(DEV) for b in batch), _to(noise, DEV)
    saved = scan.WIDE_PIECES
    scan.WIDE_PIECES = pieces
    _lib.TIMERS.enable()
    try:
        with torch.no_grad():
            state0 = model.initial_state((gbatch[1][:, 0], gbatch[2][:, 0]), gnoise)
            post, prior = model.rollout_representation(actions=gbatch[0], observations=(gbatch[1], gbatch[2]), prev_state=state0,
                                                       noise=gnoise)
        out = model.shared_step(gbatch, gnoise)
        out["loss"].backward()
        torch.cuda.synchronize()
        launched = set(_lib.TIMERS.summary())
    finally:
        _lib.TIMERS.disable()
        scan.WIDE_PIECES = saved
    # (2) the family that ran: the scan kernels among the timed launches are exactly the intended forward and BPTT kernels
    # (a silent fallback to the single-CU scan would pass everything below for the wrong kernel)
    fwd, bwd = _scan_kernels(family, case, pieces)
    scans = {k for k in launched if k.startswith(("mtrssm::mrssm_", "mtrssm::mmtrssm_"))}
    assert any(k.startswith(fwd) for k in scans), (fwd, sorted(scans))
    assert any(k.startswith(bwd) for k in scans), (bwd, sorted(scans))
    assert all(k.startswith((fwd, bwd)) for k in scans), sorted(scans)
    # (3) the rollout's values
    atol = 1e-5 + (5e-6 if wide else 0.0)
    if case.kind == "mrssm":
        np.testing.assert_allclose(_np(state0.deter), ref["_deter0"].detach().numpy(), atol=1e-5)
        assert (_index(state0.stoch, d.cats, d.classes) == _index(ref["_stoch0"], d.cats, d.classes)).all()
        if not two:
            np.testing.assert_allclose(_np(post.deter), ref["_deter"].detach().numpy(), atol=atol, err_msg="deter")
        pairs = [(post.distribution.probs, ref["_post_logits"], post.stoch, ref["_post_stoch"], d.cats, d.classes),
                 (prior.distribution.probs, ref["_prior_logits"], prior.stoch, ref["_prior_stoch"], d.cats, d.classes)]
    else:
        for k in ("deter_l", "deter_h", "hidden_l", "hidden_h"):
            np.testing.assert_allclose(_np(getattr(state0, k)), ref[f"_init_{k}"].detach().numpy(), atol=1e-5, err_msg=f"init {k}")
            if not two:
                np.testing.assert_allclose(_np(getattr(post, k)), ref[f"_{k}"].detach().numpy(), atol=atol, err_msg=k)
        assert (_index(state0.stoch_l, d.ls_cats, d.ls_classes) == _index(ref["_init_stoch_l"], d.ls_cats, d.ls_classes)).all()
        assert (_index(state0.stoch_h, d.hs_cats, d.hs_classes) == _index(ref["_init_stoch_h"], d.hs_cats, d.hs_classes)).all()
        pairs = [(post.distribution_l.probs, ref["_post_logits_l"], post.stoch_l, ref["_post_stoch_l"], d.ls_cats, d.ls_classes),
                 (post.distribution_h.probs, ref["_post_logits_h"], post.stoch_h, ref["_post_stoch_h"], d.hs_cats, d.hs_classes),
                 (prior.distribution_l.probs, ref["_prior_logits_l"], prior.stoch_l, ref["_prior_stoch_l"], d.ls_cats, d.ls_classes),
                 (prior.distribution_h.probs, ref["_prior_logits_h"], prior.stoch_h, ref["_prior_stoch_h"], d.hs_cats, d.hs_classes)]
    for i, (probs, ref_logits, stoch, ref_stoch, cats, classes) in enumerate(pairs):
        _, want_p = cat_probs(ref_logits.detach(), cats, classes)
        np.testing.assert_allclose(_np(probs), want_p.numpy(), atol=atol, err_msg=f"probs {i}")
        s = _np(stoch).reshape(*stoch.shape[:-1], cats, classes)
        assert ((s == 0) | (s == 1)).all() and (s.sum(-1) == 1).all()
        assert (_index(stoch, cats, classes) == _index(ref_stoch, cats, classes)).all(), f"samples {i}"
    # (4) losses and gradients
    assert set(out) == {k for k in ref if not k.startswith("_")}
    for k in out:
        np.testing.assert_allclose(float(out[k].detach()), float(ref[k].detach()), rtol=1e-4 if two else 2e-5, err_msg=k)
    if grads:
        want = {k: p.grad for k, p in oracle.named_parameters() if p.grad is not None}
        got = dict(model.named_parameters())
        assert len(want) > 40
        tol = 1e-3 if wide else 2e-4
        for k, g in want.items():
            assert got[k].grad is not None, k
            scale = float(g.abs().max()) + 1e-12
            np.testing.assert_allclose(_np(got[k].grad), g.numpy(), rtol=tol, atol=tol * scale, err_msg=f"grad {k}")
    # (5) no cooperative launch gave up on an exchange
    if family != "scan" and family != "mt_scan":
        scan.check_cluster_status()
    return model, out, state0, post, prior


@pytest.mark.parametrize("option_set", OPTION_SETS)
@pytest.mark.parametrize("case_id", list(SCAN_CASES))
def test_scan_family_with_options_matches_oracle(case_id: str, option_set: str, lib_loaded: None) -> None:
    """One scan family (single-CU MRSSM / cluster 32, 64, 128, 200 / wide MRSSM with D != H / single-CU and wide MMTRSSM) under one
    option set (ReLU; Tanh with plain KL, kl_coeff 0.7, w_kl_h 0.3; Identity) against the oracle: the rollout's values and
    samples, every loss and every parameter gradient, and the names of the forward and BPTT kernels that ran."""
    base, family = SCAN_CASES[case_id]
    case = with_options(base, **options(base, option_set))
    oracle = build_model(case)
    batch = build_batch(case)
    noise, _margin, _seed = screened(case, oracle, batch, relu_margin_for(case_id, option_set))
    compare_scan_family(case, family, oracle, batch, noise, grads=not (option_set == "relu" and case_id in RELU_VALUES_ONLY))


@pytest.mark.parametrize("case_id", ["mrssm_nonsquare", "mmtrssm_default"])
def test_prior_only_rollout_with_tanh_matches_oracle(case_id: str, lib_loaded: None) -> None:
    """The prior-only scan (``post = 0``) with Tanh, as test_prior_rollout_is_differentiable_and_matches_the_oracle runs it with ELU:
    the fused inference kernel and the differentiable composed form against the oracle's loop, values to 1e-5 and the gradients
    of a fixed random functional of every output (parameters, actions, start state) to 2e-4 of each tensor's max."""
    from multimodal_mtrssm_amd import _lib, scan

    case = with_options(CASES[case_id], activation="Tanh")
    oracle = build_model(case)
    model = product_from_case(case, oracle, DEV)
    batch = build_batch(case)
    q = case.query
    mr = case.kind == "mrssm"
    actions = batch[0][:, q:].clone()
    half = functools.partial(torch.full, fill_value=0.5)  # the start state's draws: any uniforms do, the oracle's state goes to both sides
    with torch.no_grad():  # the start state is the oracle's and is handed to both sides
        if mr:
            s0 = oracle.initial_state(batch[1][:, 0], batch[2][:, 0], half((case.batch, case.dims.cats)))
            state0 = {"deter": s0["deter"], "stoch": s0["stoch"]}
        else:
            s0 = oracle.initial_state(batch[1][:, 0], batch[2][:, 0], half((case.batch, case.dims.hs_cats)), half((case.batch, case.dims.ls_cats)))
            state0 = {k: s0[k] for k in ("deter_l", "deter_h", "hidden_l", "hidden_h", "stoch_l", "stoch_h")}
    u, _seed = screened_prior(case, oracle, actions, state0)
    gen = torch.Generator().manual_seed(5)

    def run(on_gpu: bool):  # noqa: ANN202
        dev = DEV if on_gpu else "cpu"
        a = actions.detach().clone().to(dev).requires_grad_(True)
        st = {k: v.detach().clone().to(dev).requires_grad_(not k.startswith("stoch")) for k, v in state0.items()}
        un = {k: v.to(dev) for k, v in u.items()}
        if on_gpu:
            out = (scan.mrssm_prior_rollout(model.transition, a, st["deter"], st["stoch"], un["u_prior"]) if mr
                   else scan.mmtrssm_prior_rollout(model, a, st, un))
            with torch.no_grad():  # the fused inference kernel on the same inputs
                fused = (scan.mrssm_prior_rollout(model.transition, a.detach(), st["deter"].detach(), st["stoch"], un["u_prior"]) if mr
                         else scan.mmtrssm_prior_rollout(model, a.detach(), {k: v.detach() for k, v in st.items()}, un))
            last = _lib.load().mtrssm_last_kernel().decode()
            assert last.startswith("mtrssm::mrssm_fwd_kernel<1, false, " if mr else "mtrssm::mmtrssm_fwd_kernel<1, false, "), last
        else:
            out = oracle.rollout_transition(a, st, un["u_prior"]) if mr else oracle.rollout_transition(a, st, un)
            fused = None
        gen.manual_seed(5)
        loss = sum((v * torch.randn(v.shape, generator=gen).to(dev)).sum() for _, v in sorted(out.items()))
        for p_ in (model.parameters() if on_gpu else oracle.parameters()):
            p_.grad = None
        loss.backward()
        return out, fused, a.grad, {k: v.grad for k, v in st.items() if v.requires_grad}

    ref_out, _, ref_ga, ref_gs = run(False)
    out, fused, ga, gs = run(True)
    torch.cuda.synchronize()
    for k, v in ref_out.items():
        np.testing.assert_allclose(_np(out[k]), v.detach().numpy(), atol=1e-5, err_msg=f"composed {k}")
        np.testing.assert_allclose(_np(fused[k]), v.detach().numpy(), atol=1e-5, err_msg=f"fused {k}")
    scale = float(ref_ga.abs().max()) + 1e-12
    np.testing.assert_allclose(_np(ga), ref_ga.numpy(), rtol=2e-4, atol=2e-4 * scale, err_msg="d actions")
    for k, g in ref_gs.items():
        scale = float(g.abs().max()) + 1e-12
        np.testing.assert_allclose(_np(gs[k]), g.numpy(), rtol=2e-4, atol=2e-4 * scale, err_msg=f"d {k}")
    got = dict(model.named_parameters())
    seen = 0
    for k, p_ in oracle.named_parameters():
        if p_.grad is None:
            continue
        assert got[k].grad is not None, k
        scale = float(p_.grad.abs().max()) + 1e-12
        np.testing.assert_allclose(_np(got[k].grad), p_.grad.numpy(), rtol=2e-4, atol=2e-4 * scale, err_msg=f"grad {k}")
        seen += 1
    assert seen >= 6  # the prior path's Linear layers


# ---------------------------------------------------------------------------------------------
# 3b. conv kernels x activation, against float64 on the CPU
# ---------------------------------------------------------------------------------------------
_ACT_FN = {0: lambda t: t, 1: F.relu, 2: F.elu, 3: torch.tanh}  # _lib.ACT_IDS
# (act, force pre_act): ReLU and Tanh wherever the case has a pre-activation, Identity THROUGH the pre-activation path.  The
# pre-activation is applied to the given input, bit-identical on both sides: ReLU's kink is exact and nothing is left out.
_CONV_VARIANTS = [(1, False), (3, False), (0, True)]
_SMALL_CONV = [c for c in CONV_CASES if c[0] <= 70]    # noqa: PLR2004
_SMALL_DECONV = [c for c in DECONV_CASES if c[0] <= 70]  # noqa: PLR2004


@pytest.fixture
def bf16x2_mode():  # noqa: ANN201
    from multimodal_mtrssm_amd import conv

    before = conv.mfma_mode()
    conv.set_mfma_mode("bf16x2")
    yield
    conv.set_mfma_mode(before)


@pytest.mark.parametrize(("act", "force_pre"), _CONV_VARIANTS)
@pytest.mark.parametrize(("n", "cin", "h", "w", "cout", "k", "s", "p", "pre", "coords"), _SMALL_CONV)
def test_conv2d_kernel_activations(n, cin, h, w, cout, k, s, p, pre, coords, act, force_pre, bf16x2_mode: None, lib_loaded: None) -> None:  # noqa: ANN001, PLR0913
    """test_conv2d_kernel (hard-wired to ELU) with ReLU, Tanh and Identity-as-pre-activation, float64 reference.  A Tanh or ReLU
    case that reached a kernel knowing another activation is off by O(1)."""
    from multimodal_mtrssm_amd.conv import conv2d

    pre = pre or force_pre
    fn = _ACT_FN[act]
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, cin, h, w, generator=g)
    cc = torch.randn(2, h, w, generator=g) if coords else None
    wt = torch.randn(cout, cin + (2 if coords else 0), k, k, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, wt, b))
    xin = fn(x64) if pre else x64
    if coords:
        c64 = cc.double()
        xin = torch.cat([xin, (fn(c64) if pre else c64).unsqueeze(0).expand(n, -1, -1, -1)], 1)
    want = F.conv2d(xin, w64, b64, s, p)
    gout = torch.randn(want.shape, generator=g)
    want.backward(gout.double())
    xg, wg, bg = (t.to(DEV).requires_grad_() for t in (x, wt, b))
    got = conv2d(xg, wg, bg, stride=s, padding=p, pre_act=pre, act=act, coords=None if cc is None else cc.to(DEV))
    got.backward(gout.to(DEV))
    np.testing.assert_allclose(_np(got), want.detach().float().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_np(xg.grad), x64.grad.float().numpy(), rtol=1e-4, atol=max(1e-4, 1e-5 * float(x64.grad.abs().max())))
    np.testing.assert_allclose(_np(wg.grad), w64.grad.float().numpy(), rtol=1e-4, atol=max(2e-4, 2e-5 * float(w64.grad.abs().max())))
    np.testing.assert_allclose(_np(bg.grad), b64.grad.float().numpy(), rtol=1e-4, atol=max(2e-4, 2e-5 * float(b64.grad.abs().max())))


@pytest.mark.parametrize(("act", "force_pre"), _CONV_VARIANTS)
@pytest.mark.parametrize(("n", "cin", "h", "w", "cout", "k", "s", "p", "op", "pre"), _SMALL_DECONV)
def test_conv_transpose2d_kernel_activations(n, cin, h, w, cout, k, s, p, op, pre, act, force_pre, bf16x2_mode: None, lib_loaded: None) -> None:  # noqa: ANN001, PLR0913
    """test_conv_transpose2d_kernel with ReLU, Tanh and Identity-as-pre-activation, float64 reference."""
    from multimodal_mtrssm_amd.conv import conv_transpose2d

    pre = pre or force_pre
    fn = _ACT_FN[act]
    g = torch.Generator().manual_seed(12)
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cin, cout, k, k, generator=g) * 0.2
    b = torch.randn(cout, generator=g)
    x64, w64, b64 = (t.double().requires_grad_() for t in (x, wt, b))
    want = F.conv_transpose2d(fn(x64) if pre else x64, w64, b64, s, p, op)
    gout = torch.randn(want.shape, generator=g)
    want.backward(gout.double())
    xg, wg, bg = (t.to(DEV).requires_grad_() for t in (x, wt, b))
    got = conv_transpose2d(xg, wg, bg, stride=s, padding=p, output_padding=op, pre_act=pre, act=act)
    got.backward(gout.to(DEV))
    assert got.shape == want.shape
    np.testing.assert_allclose(_np(got), want.detach().float().numpy(), rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(_np(xg.grad), x64.grad.float().numpy(), rtol=1e-4, atol=max(1e-4, 1e-5 * float(x64.grad.abs().max())))
    np.testing.assert_allclose(_np(wg.grad), w64.grad.float().numpy(), rtol=1e-4, atol=max(2e-4, 2e-5 * float(w64.grad.abs().max())))
    np.testing.assert_allclose(_np(bg.grad), b64.grad.float().numpy(), rtol=1e-4, atol=max(2e-4, 2e-5 * float(b64.grad.abs().max())))


# ---------------------------------------------------------------------------------------------
# 3c. GEMM epilogues x activation, against float64 on the CPU
# ---------------------------------------------------------------------------------------------
_GEMM_ROWS = [c for c in GEMM_CASES if c[5] in {"bias+act_a", "zgrad", "acc+act_b"}] + [
    (*c[:5], "views+act_a") for c in GEMM_CASES if c[5] == "views"]
assert len(_GEMM_ROWS) == 5  # noqa: PLR2004


@functools.lru_cache(maxsize=1)  # `pieces` varies fastest: its three runs share one problem
def _gemm_problem(m: int, n: int, r: int, a_rm: bool, b_rm: bool, extras: str, act: int) -> dict:  # noqa: FBT001, PLR0913
    """Operands and the float64 result of one row, shared by the three ``pieces`` runs (test_gemm_kernel's construction)."""
    fn = _ACT_FN[act]
    g = torch.Generator().manual_seed(m * 7 + n * 3 + r)
    pad = 5 if "views" in extras else 0
    a_full = torch.randn((r, m + pad) if a_rm else (m, r + pad), generator=g)
    b_full = torch.randn((r, n + pad) if b_rm else (n, r + pad), generator=g)
    a = a_full[:, pad:] if pad else a_full
    b = b_full[:, pad:] if pad else b_full
    a_ir = (a.t() if a_rm else a).double()   # [M, R]
    b_jr = (b.t() if b_rm else b).double()   # [N, R]
    if "act_a" in extras:
        a_ir = fn(a_ir)
    if "act_b" in extras:
        b_jr = fn(b_jr)
    want = a_ir @ b_jr.t()
    bias = torch.randn(n, generator=g) if "bias" in extras else None
    if bias is not None:
        want = want + bias.double()
    z = torch.randn(m, n, generator=g) if "zgrad" in extras else None
    if z is not None:  # act'(z) of the pre-activation z
        z64 = z.double()
        want = want * ((z64 > 0).double() if act == 1 else 1.0 - torch.tanh(z64) ** 2)
    c0 = torch.randn(m, n + pad, generator=g) if "acc" in extras else torch.full((m, n + pad), float("nan"))
    if "acc" in extras:
        want = want + c0[:, pad:].double()
    return {"a_full": a_full, "b_full": b_full, "pad": pad, "bias": bias, "z": z, "c0": c0, "want": want.float().numpy(),
            "scale": float(want.abs().max())}


@pytest.mark.parametrize("pieces", [0, 2, 3])
@pytest.mark.parametrize("act", [1, 3])
@pytest.mark.parametrize(("m", "n", "r", "a_rm", "b_rm", "extras"), _GEMM_ROWS)
def test_gemm_kernel_activations(m: int, n: int, r: int, a_rm: bool, b_rm: bool, extras: str, act: int, pieces: int, lib_loaded: None) -> None:  # noqa: PLR0913
    """test_gemm_kernel's fused activations (act_a / act_b while staging, act' of z in the epilogue; ELU there) with ReLU and
    with the hand-written Tanh ``1 - 2 / (exp(2 z) + 1)``, on the fp32 MFMA, split-bf16 and tile kernels.  z and the operands
    are inputs: ReLU is exact."""
    from multimodal_mtrssm_amd.linear import gemm

    pr = _gemm_problem(m, n, r, a_rm, b_rm, extras, act)
    pad, bias, z = pr["pad"], pr["bias"], pr["z"]
    c = pr["c0"].to(DEV)
    ag, bg = pr["a_full"].to(DEV), pr["b_full"].to(DEV)
    gemm(ag[:, pad:] if pad else ag, bg[:, pad:] if pad else bg, c[:, pad:] if pad else c, a_rmajor=a_rm, b_rmajor=b_rm,
         bias=None if bias is None else bias.to(DEV), zgrad=None if z is None else z.to(DEV), colsum=None,
         act_a=act if "act_a" in extras else 0, act_b=act if "act_b" in extras else 0, act_z=act if z is not None else 0,
         accumulate="acc" in extras, mfma_split=pieces)
    got = c[:, pad:] if pad else c
    rtol, tol = (1e-4, 3e-5) if pieces == 2 else (1e-5, 2e-6)  # noqa: PLR2004
    np.testing.assert_allclose(_np(got), pr["want"], rtol=rtol, atol=tol * pr["scale"])
    if pad and "acc" not in extras:
        assert torch.isnan(c[:, :pad]).all()  # nothing outside the view was written


# ---------------------------------------------------------------------------------------------
# 3d. whole conv stacks with Tanh and ReLU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("activation", ["Tanh", "ReLU"])
def test_encoder_decoder_activations_match_oracle(activation: str, fp32_grade_mode: str, lib_loaded: None) -> None:  # noqa: F811
    """test_encoder_decoder_match_oracle's comparison at mrssm_nonsquare with the stacks' ``activation_name`` set to Tanh and to
    ReLU.  Tanh compares values and every gradient; ReLU the values only: its intermediates are computed, and one within
    rounding of 0 switches its gradient on or off (the rule of test_fused_residual_block_matches_two_launches_and_float64)."""
    import multimodal_mtrssm_amd as mt
    from oracle.ref_cnn import Decoder, Encoder

    case = CASES["mrssm_nonsquare"]
    d = case.dims
    torch.manual_seed(5)
    for cfg, ref_cls, mine_cls, shape in ((d.enc_audio, Encoder, mt.Encoder, (2, 3, *case.audio_shape)),
                                           (d.dec_vision, Decoder, mt.Decoder, (2, 3, d.deter + d.stoch))):
        cfg = {**cfg, "activation_name": activation}
        ref = ref_cls(cfg)
        mine = mine_cls(cfg)
        mine.load_state_dict(ref.state_dict())
        mine = mine.to(DEV)
        x = torch.randn(shape).requires_grad_()
        y = ref(x)
        gy = torch.randn(y.shape)
        y.backward(gy)
        xg = x.detach().to(DEV).requires_grad_()
        yg = mine(xg)
        yg.backward(gy.to(DEV))
        np.testing.assert_allclose(_np(yg), y.detach().numpy(), rtol=1e-4, atol=1e-5)
        if activation != "ReLU":
            np.testing.assert_allclose(_np(xg.grad), x.grad.numpy(), rtol=1e-3, atol=1e-5 * float(x.grad.abs().max() + 1))
            for (k, pr), (_, pm) in zip(ref.named_parameters(), mine.named_parameters(), strict=True):
                scale = float(pr.grad.abs().max()) + 1e-12
                np.testing.assert_allclose(_np(pm.grad), pr.grad.numpy(), rtol=1e-3, atol=2e-4 * scale, err_msg=k)
        # a single frame gives the same embedding as that frame inside a [B,T] batch
        np.testing.assert_allclose(_np(mine(xg[:, 0])), _np(yg[:, 0]), rtol=1e-5, atol=1e-6)
