"""GPU (MI355X): the four kernels of ragged batches, each against its torch restatement, exact equality."""

from __future__ import annotations

import ctypes as C

import pytest
import torch

from multimodal_mtrssm_amd import ElboSchedule, _lib, carry, dropout, scan
from multimodal_mtrssm_amd import dataset as ds
from multimodal_mtrssm_amd import transform as tr
from multimodal_mtrssm_amd.core import _elbo
from multimodal_mtrssm_amd.dropout import ModalityDropout, StepMask

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# 1. the gather ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("std", [0.1, None])
def test_ragged_gather_equals_its_restatement(std: float | None) -> None:
    n, t_full, t = 5, 7, 4
    g = torch.Generator().manual_seed(3)
    store = torch.randn(n, t_full, 2, 4, generator=g).to(DEV)  # E = 8
    chain = tr.Compose([tr.TakeFirstN(t)] + ([tr.GaussianNoise(std)] if std is not None else []))
    stream = ds._Stream(store, chain, tr.Compose([tr.TakeFirstN(t)]))  # noqa: SLF001
    assert stream.fused and stream.event == 8
    lens = torch.tensor([7, 5, 1, 4, 2], dtype=torch.int32, device=DEV)
    idx = torch.tensor([0, 1, 2, 3, 4, 0, 1], device=DEV)
    start = torch.tensor([0, 3, 0, 4, -1, 7, 4], dtype=torch.int32, device=DEV)  # 0, 3, 4, 7 and a negative one
    noise = torch.randn(7, t, 2, 4, generator=g).to(DEV) if std is not None else None
    valid = torch.full((7,), -9, dtype=torch.int32, device=DEV)
    inp, tgt = stream.batch(idx, noise, start, None, lens, valid)
    want_inp, want_tgt, want_valid = ds.gather_ragged_reference(store, idx, start, lens, t, noise, std)
    assert torch.equal(tgt, want_tgt) and torch.equal(inp, want_inp) and torch.equal(valid, want_valid)
    assert want_valid.tolist() == [4, 2, 1, 0, 2, 0, 1]
    for b, v in enumerate(want_valid.tolist()):  # dead frames: exactly zero in both outputs, no noise added
        assert not bool(tgt[b, v:].any()) and not bool(inp[b, v:].any())
        assert bool(tgt[b, :v].any()) or v == 0
    inp2, tgt2 = stream.batch(idx, noise, start, None, lens, None)  # the other two streams' calls pass no valid_out
    assert torch.equal(inp2, inp) and torch.equal(tgt2, tgt)
    # every frame live: the window gather's result
    full = torch.full((n,), t_full, dtype=torch.int32, device=DEV)
    ok_start = torch.tensor([0, 3, 1, 2, 0, 3, 3], dtype=torch.int32, device=DEV)
    a, b = stream.batch(idx, noise, ok_start, None, full, None)
    wa, wb = stream.batch(idx, noise, ok_start, None)
    assert torch.equal(a, wa) and torch.equal(b, wb)


# 2. the step mask ------------------------------------------------------------------------------------------------------------
def _hand_u(md: ModalityDropout, b: int, t: int) -> torch.Tensor:
    """Uniforms whose first rows take the t = 0 fix-up (audio larger, vision larger) and a tie."""
    u = torch.rand(md.noise_shape(b, t), generator=torch.Generator().manual_seed(12))
    lo = min(md.p_audio, md.p_vision)
    for row, (a, v) in enumerate([(0.5 * lo, 0.25 * lo), (0.25 * lo, 0.5 * lo), (0.5 * lo, 0.5 * lo), (0.5 * lo, 0.5 * lo)]):
        u[row, 0, 0], u[row, 0, 1] = a, v
    return u.to(DEV)


@pytest.mark.parametrize(("world", "rank"), [(1, 0), (5, 2), (5, 4)])
@pytest.mark.parametrize("with_u", [False, True])
def test_step_mask_equals_its_restatement(with_u: bool, world: int, rank: int) -> None:  # noqa: FBT001
    b, t = 5, 7
    md = ModalityDropout(0.6, 0.5, span=3) if with_u else None
    u = _hand_u(md, b, t) if with_u else None
    valid = torch.tensor([7, 4, 0, 1, 6], dtype=torch.int32, device=DEV)
    ref = dropout.ragged_reference(valid, u, t, md)
    if with_u:  # the fix-up fired on live rows (rows 0, 1, 3) and row 2's is ANDed away
        plain = u[:, torch.arange(t, device=DEV) // 3] >= torch.tensor([0.6, 0.5], device=DEV)
        assert not bool(plain[:4, 0].any()) and ref.mask[0, 0].tolist() == [True, False] and ref.mask[1, 0].tolist() == [False, True]
        assert ref.mask[3, 0].tolist() == [True, False] and not bool(ref.mask[2].any())
    local = b // world
    rows = slice(rank * local, (rank + 1) * local)
    sm = dropout.ragged_step_mask(valid, u, t, md, world=world, rank=rank)
    assert sm.codes.dtype == torch.int32 and torch.equal(sm.codes, scan.modality_codes(ref.mask[rows]))
    assert torch.equal(sm.present_audio, ref.mask[rows][..., 0].reshape(-1).float())
    assert torch.equal(sm.present_vision, ref.mask[rows][..., 1].reshape(-1).float())
    assert torch.equal(sm.live, ref.live[rows].reshape(-1).float())
    assert sm.mask0.dtype == torch.bool and torch.equal(sm.mask0, ref.mask[rows][:, 0])
    assert sm.last.dtype == torch.int32 and torch.equal(sm.last, ref.last[rows]) and ref.last.tolist() == [6, 3, -1, 0, 5]
    got = torch.stack([sm.count_audio, sm.count_vision, sm.count_live])  # GLOBAL counts / world, the same on every rank
    assert torch.equal(got, ref.counts / float(world) if world > 1 else ref.counts) and float(ref.counts[2]) == 18.0
    if not with_u:
        assert ref.counts.tolist() == [18.0, 18.0, 18.0]


def test_step_mask_many_workgroups_counts_are_exact() -> None:
    """More than one workgroup and more than 64 x 256 steps (the grid-stride loop turns over): the atomics' counts are exact."""
    b, t = 700, 50
    g = torch.Generator().manual_seed(2)
    valid = torch.randint(0, t + 1, (b,), generator=g).to(torch.int32).to(DEV)
    md = ModalityDropout(0.3, 0.4, span=10)
    u = torch.rand(md.noise_shape(b, t), generator=g).to(DEV)
    ref = dropout.ragged_reference(valid, u, t, md)
    sm = dropout.ragged_step_mask(valid, u, t, md, world=2, rank=1)
    assert torch.equal(sm.codes, ref.codes[350:]) and torch.equal(sm.last, ref.last[350:])
    assert torch.equal(torch.stack([sm.count_audio, sm.count_vision, sm.count_live]), ref.counts / 2.0)


# 3. the counted ELBO epilogue --------------------------------------------------------------------------------------------------
def _mask_with(live: torch.Tensor, count: torch.Tensor) -> StepMask:
    z = torch.zeros(1, device=DEV)
    return StepMask(z, z, z, z, z, z, live, count, None)


@pytest.mark.parametrize("two", [False, True])
def test_counted_combine(two: bool) -> None:  # noqa: FBT001
    n = 21
    g = torch.Generator().manual_seed(5)
    nll = [torch.rand((), generator=g).to(DEV).requires_grad_() for _ in range(2)]
    kls = [torch.rand(3, 7, generator=g).to(DEV).requires_grad_() for _ in range(2 if two else 1)]
    live = (torch.rand(n, generator=g) < 0.6).float().to(DEV)
    c0, c1 = 0.7, 0.3
    count = live.sum() / 2.0  # (a data-parallel rank divides by global count / world: any positive scalar)

    def run(sm: StepMask | None) -> tuple[list[torch.Tensor], list[torch.Tensor]]:
        for x in (*nll, *kls):
            x.grad = None
        out = _elbo(nll[0], nll[1], kls[0], c0, kls[1] if two else None, c1, step_mask=sm)
        (out[3] + 0.5 * out[1]).backward()
        keep = (0, 1, 2, 3) if two else (0, 1, 3)  # (without a second KL its scalar is not written)
        return [out[j].detach().clone() if j in keep else torch.zeros((), device=DEV) for j in range(4)], [x.grad.clone() for x in (*nll, *kls)]

    out, grads = run(_mask_with(live, count))
    k = [c * (kl.detach().reshape(-1) * live).sum() / count for c, kl in zip((c0, c1), kls, strict=False)]
    recon = nll[0].detach() + nll[1].detach()
    torch.testing.assert_close(out[0], recon, rtol=0, atol=0)
    torch.testing.assert_close(out[1], k[0], rtol=2e-6, atol=0)
    torch.testing.assert_close(out[3], recon + sum(k), rtol=2e-6, atol=0)
    if two:
        torch.testing.assert_close(out[2], k[1], rtol=2e-6, atol=0)
    assert float(grads[0]) == 1.0 and float(grads[1]) == 1.0
    for j, (c, head) in enumerate(zip((c0, c1), (1.5, 1.0), strict=False)):
        if j < len(kls):
            want = (live * (head * c) / count).reshape(3, 7)
            torch.testing.assert_close(grads[2 + j], want, rtol=2e-6, atol=0)
            assert not bool(grads[2 + j].reshape(-1)[live == 0].any())  # a dead step gets an explicit zero
    # every step live, count = n: bitwise the uncounted kernel
    ones = torch.ones(n, device=DEV)
    a_out, a_grads = run(_mask_with(ones, torch.tensor(float(n), device=DEV)))
    b_out, b_grads = run(None)
    for x, y in zip(a_out + a_grads, b_out + b_grads, strict=True):
        assert torch.equal(x, y)
    # count = 0: the KL terms are 0 and so are their gradients
    z_out, z_grads = run(_mask_with(torch.zeros(n, device=DEV), torch.zeros((), device=DEV)))
    assert float(z_out[1]) == 0.0 and float(z_out[2]) == 0.0 and torch.equal(z_out[3], z_out[0])
    assert all(not bool(gk.any()) for gk in z_grads[2:])


def test_unscheduled_epilogue_keeps_negative_kl_and_refuses_mismatched_planes() -> None:
    """Without a schedule nothing is clipped: negative per-step KLs enter the plain and the counted sums as they are (n = 257: one
    step past a block).  Reference: ``_elbo``'s eager rule on the same fp32 values in float64; 2e-6 as ``test_counted_combine``.  And
    two KL planes of different sizes raise before any launch on every path."""
    n, c0, c1 = 257, 0.7, 0.3
    g = torch.Generator().manual_seed(8)
    nll = [torch.rand((), generator=g) for _ in range(2)]
    kls = [torch.rand(n, generator=g) * 3.0 - 0.75, torch.rand(n, generator=g) * 2.0 - 0.5]
    assert all(bool((kl < 0).any()) for kl in kls)
    live = (torch.rand(n, generator=g) < 0.6).float()
    live[kls[0].argmin()] = 1.0  # (the most negative step is a live one)
    count = live.sum() / 2.0
    for two, counted in ((False, False), (True, False), (False, True), (True, True)):
        runs = []
        for where, dtype in (("cpu", torch.float64), (DEV, torch.float32)):
            a, v, k0, k1 = (x.to(where, dtype).requires_grad_() for x in (*nll, *kls))
            z = torch.zeros(1, device=where)
            sm = StepMask(z, z, z, z, z, z, live.to(where), count.to(where), None) if counted else None
            out = _elbo(a, v, k0, c0, k1 if two else None, c1, step_mask=sm)
            (out[3] + 0.5 * out[1] + (0.25 * out[2] if two else 0.0)).backward()
            keep = (0, 1, 2, 3) if two else (0, 1, 3)
            runs.append([out[j].detach().cpu().double() for j in keep] + [x.grad.cpu().double() for x in (a, v, k0, *([k1] if two else []))])
        for want, got in zip(*runs, strict=True):
            torch.testing.assert_close(got, want, rtol=2e-6, atol=0)
        clipped = c0 * (kls[0].double().clamp(min=0) * (live.double() if counted else 1.0)).sum() / (float(count) if counted else n)
        assert float(runs[1][1]) < float(clipped) * (1 - 1e-3)  # (what free bits of 0 would have given)
    short = torch.rand(4, device=DEV)
    masks = (None, StepMask(*(torch.zeros(1, device=DEV),) * 6, torch.ones(6, device=DEV), torch.tensor(6.0, device=DEV), None))
    for sm, schedule in ((masks[0], None), (masks[1], None), (masks[0], ElboSchedule()), (masks[1], ElboSchedule())):
        with pytest.raises(ValueError, match="same number of steps"):
            _elbo(nll[0].to(DEV), nll[1].to(DEV), torch.rand(6, device=DEV), c0, short, c1, step_mask=sm, schedule=schedule)


# 4. save-at ----------------------------------------------------------------------------------------------------------------------
def test_save_at_equals_its_restatement() -> None:
    b, steps = 4, 5
    g = torch.Generator().manual_seed(9)
    sc = carry.StateCarry({"deter": 4, "stoch": 3}, b, DEV)  # a 16-byte lane entry and a 4-byte lane one
    held = {k: torch.randn(b, w, generator=g).to(DEV) for k, w in sc.widths.items()}
    for k, v in held.items():
        sc.buffers["train"][k].copy_(v)
    outs = {k: torch.randn(b, steps, w, generator=g).to(DEV).requires_grad_() for k, w in sc.widths.items()}
    last = torch.tensor([4, 0, -1, 2], dtype=torch.int32, device=DEV)
    sc.save("train", outs, last)
    assert sc.filled["train"]
    for k in sc.widths:
        got = sc.buffers["train"][k]
        assert torch.equal(got, carry.save_at_reference(outs[k], last, held[k])), k
        assert torch.equal(got[2], held[k][2]) and torch.equal(got[0], outs[k][0, 4].detach())  # row 2 keeps what dst held
    beyond = torch.tensor([5, 4, 4, 4], dtype=torch.int32, device=DEV)  # a step past the end: left as it is, nothing read
    before = {k: v.clone() for k, v in sc.buffers["train"].items()}
    sc.save("train", outs, beyond)
    for k in sc.widths:
        assert torch.equal(sc.buffers["train"][k][0], before[k][0]) and torch.equal(sc.buffers["train"][k][1:], outs[k][1:, 4].detach())
    sc.save("val", outs, torch.full((b,), steps - 1, dtype=torch.int32, device=DEV))  # every row at T - 1: the plain save
    for k in sc.widths:
        assert torch.equal(sc.buffers["val"][k], carry.save_reference(outs[k]))
    with pytest.raises(ValueError, match="int32"):
        sc.save("train", outs, last.long())


# 5. bad arguments: -1, nothing launched ----------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one() -> None:
    lib = _lib.load()
    x = torch.zeros(64, device=DEV)
    i = torch.zeros(16, dtype=torch.int32, device=DEV)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    p, q, r = x.data_ptr(), i.data_ptr(), idx.data_ptr()
    assert lib.mtrssm_episode_gather_ragged(p, r, q, None, None, 1, 2, 2, 2, 4, 0.0, p, None, None, None) == -1
    assert lib.mtrssm_episode_gather_ragged(p, r, q, q, None, 1, 2, 2, 2, 4, 0.0, None, None, None, None) == -1  # no output
    assert lib.mtrssm_step_mask_ragged(q, None, 2, 2, 1, 0.0, 0.0, 0, 2, q, p, p, p, p, q, None, None) == -1  # no counts
    assert lib.mtrssm_step_mask_ragged(q, p, 2, 2, 1, 0.0, 1.5, 0, 2, q, p, p, p, p, q, p, None) == -1
    assert lib.mtrssm_elbo_combine_counted_fwd(p, p, p, None, p, None, 4, 1.0, 0.0, p, p, None, p, None) == -1
    assert lib.mtrssm_elbo_combine_counted_bwd(None, None, None, p, None, p, 4, 1.0, 0.0, p, p, p, None, None) == -1
    table = _lib.StateTable()
    table.count = 1
    table.width[0], table.src[0], table.dst[0] = 4, p, p
    assert lib.mtrssm_state_save_at(C.byref(table), None, 2, 2, None) == -1
    assert lib.mtrssm_state_save_at(C.byref(table), q, 0, 2, None) == -1
    torch.cuda.synchronize()
    assert not bool(x.any()) and not bool(i.any())
