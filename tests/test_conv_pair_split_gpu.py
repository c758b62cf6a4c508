"""Paired gather and paired ConvTranspose launches with UNEQUAL frame counts, (1, 5) and (5, 1): the persistent workgroups of one
grid are shared between the two problems in proportion to their frames (csrc/conv.hip: split_slots), and with one frame against
five each clamp of that rule is taken.  The band and parity-class kernels compute every output element from its own inputs
alone, whatever workgroup gets it, so the pair must give the two single launches' values BIT for bit (no tolerance)."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib_loaded() -> None:
    import multimodal_mtrssm_amd as mt

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert mt._lib.load().mtrssm_version() == 100  # noqa: SLF001


@pytest.fixture
def bf16x2_mode():  # noqa: ANN201
    from multimodal_mtrssm_amd import conv

    before = conv.mfma_mode()
    conv.set_mfma_mode("bf16x2")
    yield
    conv.set_mfma_mode(before)


def _rnd(gen: torch.Generator, *shape: int, scale: float = 1.0) -> torch.Tensor:
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


@pytest.mark.parametrize(("na", "nv"), [(1, 5), (5, 1)])
def test_unequal_pairs_equal_single_launches_bitwise(na: int, nv: int, bf16x2_mode: None, lib_loaded: None) -> None:
    from multimodal_mtrssm_amd import _lib, conv

    gen = torch.Generator().manual_seed(31 + na)
    last = _lib.load().mtrssm_last_kernel

    # second encoder layer (3x3 / stride 2, 8 -> 16) on the audio and the vision plane: conv3x3s2_band_kernel<8, 0> forward,
    # convt_quad's rows kernel with the act' operand for the backward-data
    enc = [(_rnd(gen, n, 8, *plane), _rnd(gen, 16, 8, 3, 3, scale=0.2), _rnd(gen, 16)) for n, plane in ((na, (64, 16)), (nv, (32, 32)))]
    # second decoder layer (ConvTranspose2d k 4 / stride 2, 32 -> 16): the rows kernel forward, conv4s2_band_kernel<16, 32, 1024>
    # for the backward-data
    dec = [(_rnd(gen, n, 32, *plane), _rnd(gen, 32, 16, 4, 4, scale=0.05), _rnd(gen, 16, scale=0.1)) for n, plane in ((na, (32, 8)), (nv, (16, 16)))]
    g_enc = [_rnd(gen, n, 16, *plane) for n, plane in ((na, (32, 8)), (nv, (16, 16)))]
    g_dec = [_rnd(gen, n, 16, *plane) for n, plane in ((na, (64, 16)), (nv, (32, 32)))]

    def leaves(ts: list) -> list:
        return [tuple(t.detach().clone().requires_grad_(True) for t in p) for p in ts]

    def run(paired: bool) -> tuple[list, list]:
        conv.invalidate_packs()
        e, d = leaves(enc), leaves(dec)
        names = []
        if paired:
            with torch.no_grad():  # which kernels the pair is
                conv.conv2d_pair((*e[0], 2, 1, True, 2, None), (*e[1], 2, 1, True, 2, None))
                names.append(last())
                conv.conv_transpose2d_pair((*d[0], 2, 1, 0, True, 2), (*d[1], 2, 1, 0, True, 2))
                names.append(last())
            ye = conv.conv2d_pair((*e[0], 2, 1, True, 2, None), (*e[1], 2, 1, True, 2, None))
            yd = conv.conv_transpose2d_pair((*d[0], 2, 1, 0, True, 2), (*d[1], 2, 1, 0, True, 2))
        else:
            ye = [conv.conv2d(*p, stride=2, padding=1, pre_act=True, act=2) for p in e]
            yd = [conv.conv_transpose2d(*p, stride=2, padding=1, output_padding=0, pre_act=True, act=2) for p in d]
        torch.autograd.backward([*ye, *yd], [*g_enc, *g_dec])
        torch.cuda.synchronize()
        return [*ye, *yd, *(p[0].grad for p in (*e, *d))], names

    one, names = run(paired=True)
    two, _ = run(paired=False)
    assert names == [b"mtrssm::conv3x3s2_band_kernel<8, 0>", b"mtrssm::convt4s2_rows_kernel<32, 16, 256, false>"], names
    for i, (a, b) in enumerate(zip(one, two, strict=True)):
        assert a.shape == b.shape
        assert torch.equal(a, b), (i, float((a - b).abs().max()))
