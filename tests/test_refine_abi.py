"""Refined search at the C boundary, without a GPU: the three entry points are exported and bound, and they reject null
handles and bad candidate / result counts before any device call (the plain numbers are checked first, so the message
tells which argument was wrong even when the handles are null too)."""
import ctypes as C

import numpy as np
import pytest

from granne_amd import _lib, build

ENTRIES = ("granne_hip_refine_device", "granne_hip_search_refined_batch_device", "granne_hip_search_refined_batch")


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_symbols_are_exported_and_bound(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert lib.granne_hip_abi_version() == 3  # additive entries do not bump it


def test_python_surface():
    import granne_amd
    assert hasattr(granne_amd.Granne, "refine") and hasattr(granne_amd.Granne, "refine_device")
    for m in ("search", "search_batch", "search_batch_device"):
        assert hasattr(granne_amd.RefinedGranne, m)


def test_null_handles_and_bad_counts_need_no_device(lib):
    p = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    err = lambda: lib.granne_hip_last_error()  # noqa: E731
    # the re-rank alone: (index, queries, nq, cand, counts, m, k, ids, dists, counts, status, stream)
    assert lib.granne_hip_refine_device(None, p, 1, p, None, 8, 4, p, p, p, None, None) == _lib.ERR_INVALID
    assert b"refine index is null" in err()
    for m in (0, 1025, 0xFFFFFFFF):
        assert lib.granne_hip_refine_device(None, p, 1, p, None, m, 4, p, p, p, None, None) == _lib.ERR_INVALID
        assert b"candidates per query" in err()
    assert lib.granne_hip_refine_device(None, p, 1, p, None, 8, 0, p, p, p, None, None) == _lib.ERR_INVALID
    assert b"k must be" in err()
    assert lib.granne_hip_refine_device(None, p, 0, p, None, 8, 4, p, p, p, None, None) == _lib.ERR_INVALID  # nq 0 does not excuse a null handle
    # the fused call, device and host pointers: (walk, refine, qW, qR, nq, max_search, refine_from, k, ...)
    dev = lambda *a: lib.granne_hip_search_refined_batch_device(None, None, p, p, *a, p, p, p, None, None, None, None)  # noqa: E731
    host = lambda *a: lib.granne_hip_search_refined_batch(None, None, p, p, *a, p, p, p, None, None)  # noqa: E731
    for call in (dev, host):
        assert call(1, 50, 50, 10) == _lib.ERR_INVALID and b"walk index is null" in err()
        assert call(1, 50, 0, 10) == _lib.ERR_INVALID and b"candidates per query" in err()
        assert call(1, 2000, 1025, 10) == _lib.ERR_INVALID and b"candidates per query" in err()
        assert call(1, 50, 50, 0) == _lib.ERR_INVALID and b"k must be" in err()
        assert call(1, 20, 21, 10) == _lib.ERR_INVALID and b"max_search" in err()
        assert call(1, 0, 1, 10) == _lib.ERR_INVALID and b"max_search" in err()
        assert call(0, 50, 50, 10) == _lib.ERR_INVALID
