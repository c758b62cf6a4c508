"""CPU: the C-ABI of the latent census -- the two symbols are exported and declared, every refusal returns -1
before a launch and says why, and the workspace size is positive in range and -1 out of it.  ``check_c_refusals`` also runs on the
GPU machine (``tests/test_census_gpu.py``)."""

from __future__ import annotations

from multimodal_mtrssm_amd import _lib
from tests.test_capi import declared_functions

NAMES = ("mtrssm_latent_census", "mtrssm_latent_census_workspace_bytes")


def test_the_census_symbols_are_declared_and_exported() -> None:
    lib = _lib.load()
    for name in NAMES:
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name), name


def check_c_refusals(lib) -> None:  # noqa: ANN001
    """Every ``-1`` return of ``mtrssm_latent_census``; each call returns before a launch."""
    ok = 0x10000  # never dereferenced
    size = lib.mtrssm_latent_census_workspace_bytes(3, 2, 5, 6, 5)
    good = {"post": ok, "prior": ok, "stoch": ok, "valid": None, "B": 3, "G": 2, "T": 5, "K": 6, "C": 5, "planes": ok, "table": ok, "ws": ok,
            "bytes": size}

    def census(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_latent_census(a["post"], a["prior"], a["stoch"], a["valid"], a["B"], a["G"], a["T"], a["K"], a["C"], a["planes"],
                                        a["table"], a["ws"], a["bytes"], None)

    for name in ("post", "prior", "stoch", "table", "ws"):
        assert census(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
    for name in ("post", "prior", "stoch", "valid", "planes"):
        assert census(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("table", "ws"):
        assert census(**{name: ok + 4}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("B", "T", "K", "C"):
        assert census(**{name: 0}) == -1 and census(**{name: -3}) == -1 and b"latent_census" in lib.mtrssm_last_error(), name
    for g in (0, 5, -1):
        assert census(G=g) == -1 and b"1 <= G <= 4" in lib.mtrssm_last_error(), g
    assert census(B=1 << 11, G=2, T=1 << 12, K=1, C=1, bytes=1 << 40) == -1 and b"2^24" in lib.mtrssm_last_error()  # B * G * T = 2^24
    assert census(B=1 << 10, G=2, T=1 << 10, K=1 << 5, C=1 << 5, bytes=1 << 40) == -1 and b"2^31" in lib.mtrssm_last_error()  # ... * K * C = 2^31
    assert census(B=1 << 40, T=1 << 40, bytes=1 << 40) == -1 and census(K=1 << 40, C=1 << 40, bytes=1 << 40) == -1  # (products overflow 64 bits)
    assert census(bytes=size - 1) == -1 and b"workspace" in lib.mtrssm_last_error()
    assert census(bytes=0) == -1 and census(bytes=-8) == -1


def test_c_entry_rejects_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


def test_workspace_bytes() -> None:
    size = _lib.load().mtrssm_latent_census_workspace_bytes
    b, g, t, k, c = 3, 2, 5, 6, 5
    rows = b * g
    # the row partials (3 K C + 5 K doubles), fp32 planes for a call without them, the previous classes: each a multiple of 8 bytes
    assert size(b, g, t, k, c) == 8 * rows * (3 * k * c + 5 * k) + 4 * 5 * rows * t + 4 * rows * k
    assert size(1, 1, 1, 1, 1) == 8 * 8 + 24 + 8  # (20 and 4 bytes rounded up)
    assert size(64, 3, 50, 6, 5) > 0 and size(256, 4, 100, 32, 32) > 0 and size((1 << 11) - 1, 4, 1 << 11, 1, 1) > 0
    for bad in ((0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 5, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, 0), (-1, 1, 1, 1, 1),
                (1 << 11, 2, 1 << 12, 1, 1), (1 << 10, 2, 1 << 10, 1 << 5, 1 << 5), (1 << 40, 1, 1 << 40, 1, 1), (1, 1, 1, 1 << 40, 1 << 40)):
        assert size(*bad) == -1, bad
