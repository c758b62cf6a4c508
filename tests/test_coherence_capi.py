"""CPU: the C-ABI of the coherence fold -- the two symbols are exported, declared with the documented signatures,
every refusal returns -1 before a launch and says why, and the workspace size is positive in range and -1 out of it.
``check_c_refusals`` also runs on the GPU machine (``tests/test_coherence_gpu.py``)."""

from __future__ import annotations

import ctypes as C
import re

from multimodal_mtrssm_amd import _lib
from tests.test_capi import HEADER, declared_functions

NAMES = ("mtrssm_coherence_fold", "mtrssm_coherence_fold_workspace_bytes")
_CTYPES = {"int64_t": C.c_int64, "int": C.c_int}


def _declared_arguments(name: str) -> tuple[type, list[type]]:
    """The header's declaration of ``name`` as ctypes: every pointer is ``c_void_p``."""
    ret, args = re.search(r"^(int|int64_t)\s+" + name + r"\s*\((.*?)\);", HEADER, flags=re.MULTILINE | re.DOTALL).groups()
    kinds = []
    for arg in args.split(","):
        words = re.sub(r"/\*.*?\*/", "", arg).split()
        kinds.append(C.c_void_p if "*" in arg else _CTYPES[words[-2]])
    return _CTYPES[ret], kinds


def test_the_coherence_symbols_are_declared_and_exported_with_the_documented_signatures() -> None:
    lib = _lib.load()
    for name in NAMES:
        assert name in declared_functions() and name in _lib.SYMBOLS and hasattr(lib, name), name
        assert _declared_arguments(name) == (_lib.SYMBOLS[name][0], _lib.SYMBOLS[name][1]), name
    ret, args = _lib.SYMBOLS["mtrssm_coherence_fold"]
    assert ret is C.c_int and args == [C.c_void_p] * 4 + [C.c_int64] * 5 + [C.c_void_p] * 3 + [C.c_int64, C.c_void_p]
    assert _lib.SYMBOLS["mtrssm_coherence_fold_workspace_bytes"] == (C.c_int64, [C.c_int64] * 4)


def check_c_refusals(lib) -> None:  # noqa: ANN001
    """Every ``-1`` return of ``mtrssm_coherence_fold``; each call returns before a launch."""
    ok = 0x10000  # never dereferenced
    size = lib.mtrssm_coherence_fold_workspace_bytes(3, 2, 4, 5)
    good = {"lv": ok, "la": ok, "labels": ok, "valid": None, "B": 3, "G": 2, "S": 4, "T": 5, "context": 2, "planes": ok, "table": ok, "ws": ok,
            "bytes": size}

    def fold(**kw) -> int:  # noqa: ANN003
        a = {**good, **kw}
        return lib.mtrssm_coherence_fold(a["lv"], a["la"], a["labels"], a["valid"], a["B"], a["G"], a["S"], a["T"], a["context"], a["planes"],
                                         a["table"], a["ws"], a["bytes"], None)

    for name in ("lv", "la", "labels", "table", "ws"):
        assert fold(**{name: None}) == -1 and b"null" in lib.mtrssm_last_error(), name
    for name in ("lv", "la", "labels", "valid", "planes"):
        assert fold(**{name: ok + 2}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("table", "ws"):
        assert fold(**{name: ok + 4}) == -1 and b"aligned" in lib.mtrssm_last_error(), name
    for name in ("B", "T", "S", "context"):
        assert fold(**{name: 0}) == -1 and fold(**{name: -3}) == -1 and b"coherence_fold" in lib.mtrssm_last_error(), name
    for g in (0, 5, -1):
        assert fold(G=g) == -1 and b"1 <= G <= 4" in lib.mtrssm_last_error(), g
    assert fold(S=17, bytes=1 << 40) == -1 and b"S <= 16" in lib.mtrssm_last_error()
    assert fold(B=1 << 10, G=2, S=2, T=1 << 12, bytes=1 << 40) == -1 and b"2^24" in lib.mtrssm_last_error()  # B * G * S * T = 2^24
    assert fold(B=1 << 40, T=1 << 40, bytes=1 << 40) == -1  # (the product overflows 64 bits)
    assert fold(bytes=size - 1) == -1 and b"workspace" in lib.mtrssm_last_error()
    assert fold(bytes=0) == -1 and fold(bytes=-8) == -1


def test_c_entry_rejects_bad_arguments_without_a_launch() -> None:
    check_c_refusals(_lib.load())


def test_workspace_bytes() -> None:
    size = _lib.load().mtrssm_coherence_fold_workspace_bytes
    b, g, s, t = 3, 2, 4, 5
    # the frame sums u [5][B * G][T] in double, then one set of 2 x 11 x 11 int32 pair counts per group and workgroup (one per (b, g))
    assert size(b, g, s, t) == 8 * 5 * b * g * t + 4 * (b * g) * g * 242
    assert size(1, 1, 1, 1) == 40 + 968 and size(5000, 1, 1, 3) == 8 * 5 * 5000 * 3 + 4 * 1024 * 242  # (at most 1024 workgroups)
    assert size(70, 1, 16, 33) > 0 and size((1 << 10) - 1, 4, 16, 1 << 8) > 0
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 5, 1, 1), (1, 1, 0, 1), (1, 1, 17, 1), (1, 1, 1, 0), (-1, 1, 1, 1), (1 << 10, 2, 2, 1 << 12),
                (1 << 40, 1, 1, 1 << 40)):
        assert size(*bad) == -1, bad
