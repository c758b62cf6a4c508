"""CPU: the C-ABI of the feature moments -- the two symbols are exported and declared, every refusal returns -1
before a launch and says why, and the workspace size is the header's formula in range and -1 out of it.  ``check_c_refusals`` also
runs on the GPU machine (``tests/test_frechet_gpu.py``)."""

from __future__ import annotations

from multimodal_mtrssm_amd import _lib
from tests.test_capi import declared_functions

NAMES = ("mtrssm_feature_moments", "mtrssm_feature_moments_workspace_bytes")


def workspace_bytes(n: int, d: int, j: int) -> int:
    """The header's formula: ``8 * S * J * ((P + DT) * 256 + 1)``, ``S = min(16, ceil(N / 32))``, ``DT = ceil(D / 16)``, ``P = DT (DT + 1) / 2``."""
    s, dt = min(16, -(-n // 32)), -(-d // 16)
    return 8 * s * j * ((dt * (dt + 1) // 2 + dt) * 256 + 1)


def test_the_moment_symbols_are_declared_and_exported() -> None:
    lib = _lib.load()
    for name in NAMES:
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name), name


def check_c_refusals(lib) -> None:  # noqa: ANN001
    """Every ``-1`` return of ``mtrssm_feature_moments``; each call returns before a launch."""
    ok = 0x10000  # never dereferenced
    size = lib.mtrssm_feature_moments_workspace_bytes(300, 128, 5)
    good = {"x": ok, "ldx": 128, "bin": ok, "N": 300, "D": 128, "J": 5, "table": ok, "ws": ok, "bytes": size}

    def moments(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_feature_moments(a["x"], a["ldx"], a["bin"], a["N"], a["D"], a["J"], a["table"], a["ws"], a["bytes"], None)

    for name in ("x", "bin", "table", "ws"):
        assert moments(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
    for name in ("x", "bin"):
        assert moments(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("table", "ws"):
        assert moments(**{name: ok + 4}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name, bad in (("N", 0), ("N", -3), ("D", 0), ("D", 257), ("D", -1), ("J", 0), ("J", 17), ("J", -1)):
        assert moments(**{name: bad}, ldx=300, bytes=1 << 40) == -1 and b"feature_moments: need" in lib.mtrssm_last_error(), (name, bad)
    assert moments(N=1 << 20, ldx=1 << 11, bytes=1 << 40) == -1 and b"2^31" in lib.mtrssm_last_error()  # N * ldx = 2^31
    assert moments(N=1 << 40, ldx=1 << 40, bytes=1 << 40) == -1 and moments(N=1 << 30, ldx=1 << 40, bytes=1 << 40) == -1  # (the product overflows)
    assert moments(ldx=127) == -1 and b"ldx" in lib.mtrssm_last_error()
    assert moments(ldx=0) == -1 and moments(ldx=-128) == -1
    assert moments(bytes=size - 1) == -1 and b"workspace" in lib.mtrssm_last_error()
    assert moments(bytes=0) == -1 and moments(bytes=-8) == -1


def test_c_entry_rejects_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


def test_workspace_bytes_is_the_headers_formula() -> None:
    size = _lib.load().mtrssm_feature_moments_workspace_bytes
    assert size(1, 1, 1) == 8 * (2 * 256 + 1)  # one slice, one tile and one sum tile, one count
    assert size(300, 128, 5) == 8 * 10 * 5 * (44 * 256 + 1)  # ten slices of 30 rows; 36 + 8 tiles
    for n, d, j in ((1, 1, 1), (4, 16, 1), (37, 10, 3), (70, 130, 2), (33, 256, 2), (300, 128, 5), (5000, 32, 4), (25600, 128, 5), (1 << 30, 1, 16)):
        assert size(n, d, j) == workspace_bytes(n, d, j), (n, d, j)
    assert size(25600, 128, 5) < 8 << 20  # "a few MB at D = 128"
    for bad in ((0, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 257, 1), (1, 1, 0), (1, 1, 17), (1 << 31, 1, 1), (1 << 62, 1, 1)):
        assert size(*bad) == -1, bad
