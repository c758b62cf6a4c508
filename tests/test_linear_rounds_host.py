"""CPU: ``linear._rounds`` -- which grouped GEMM problems may share a launch -- on CPU tensors (only addresses, shapes and strides
are looked at).  Disjoint column views of one matrix share a round, overlapping views do not, a view and its own bias behave
as before."""

from __future__ import annotations

import torch

from multimodal_mtrssm_amd.linear import _rounds


def _problem(c: torch.Tensor, colsum: torch.Tensor | None = None) -> tuple:
    a = torch.zeros(8, c.shape[0])
    b = torch.zeros(8, c.shape[1])
    return ((a, b, c), {"a_rmajor": True, "b_rmajor": True, "accumulate": True, "colsum": colsum})


def test_disjoint_column_views_share_a_round() -> None:
    w = torch.zeros(20, 48)   # a posterior head's first layer [H, D + E]
    rounds = _rounds([_problem(w[:, :16]), _problem(w[:, 16:]), _problem(torch.zeros(20, 16))])
    assert [len(r) for r in rounds] == [3]
    # three-way cut, given in another order
    rounds = _rounds([_problem(w[:, 40:]), _problem(w[:, :8]), _problem(w[:, 8:40])])
    assert [len(r) for r in rounds] == [3]
    # row blocks of one matrix never met in bytes
    assert [len(r) for r in _rounds([_problem(w[:10]), _problem(w[10:])])] == [2]


def test_overlapping_views_do_not() -> None:
    w = torch.zeros(20, 48)
    assert [len(r) for r in _rounds([_problem(w[:, :17]), _problem(w[:, 16:])])] == [1, 1]   # one shared column
    assert [len(r) for r in _rounds([_problem(w), _problem(w[:, 16:])])] == [1, 1]           # the matrix and a part of it
    assert [len(r) for r in _rounds([_problem(w[:, :16]), _problem(w[:, :16])])] == [1, 1]   # the same view twice
    # the same columns of different rows of one buffer, reached with another pitch: not provably disjoint -> separate rounds
    flat = torch.zeros(20 * 48)
    a, b = flat.as_strided((20, 16), (48, 1), 0), flat.as_strided((10, 16), (96, 1), 16)
    assert [len(r) for r in _rounds([_problem(a), _problem(b)])] == [1, 1]
    # a view whose rows run over the matrix's row end into the next row's first columns
    c = flat.as_strided((5, 40), (48, 1), 20)
    assert [len(r) for r in _rounds([_problem(flat.as_strided((5, 8), (48, 1), 10)), _problem(c)])] == [1, 1]
    # a single-row view has no pitch: byte ranges decide
    assert [len(r) for r in _rounds([_problem(w[:1, :16]), _problem(w[:1, 8:24])])] == [1, 1]
    assert [len(r) for r in _rounds([_problem(w[:1, :16]), _problem(w[:1, 16:])])] == [2]


def test_a_view_and_its_bias_behave_as_before() -> None:
    w, bias = torch.zeros(20, 48), torch.zeros(20)
    other, other_bias = torch.zeros(20, 48), torch.zeros(20)
    # distinct weights with distinct biases: one round
    assert [len(r) for r in _rounds([_problem(w, bias), _problem(other, other_bias)])] == [2]
    # two problems that sum into the same bias: successive rounds, even when their weight views are disjoint
    assert [len(r) for r in _rounds([_problem(w[:, :16], bias), _problem(w[:, 16:], bias)])] == [1, 1]
    # the same weight twice (the prior head: initial state and scan): successive rounds
    assert [len(r) for r in _rounds([_problem(w, bias), _problem(w, None)])] == [1, 1]
    # a bias that is a slice of a flat buffer next to its weight
    flat = torch.zeros(20 * 48 + 20)
    wv, bv = flat[: 20 * 48].view(20, 48), flat[20 * 48 :]
    assert [len(r) for r in _rounds([_problem(wv[:, :16], bv), _problem(wv[:, 16:])])] == [2]
