"""Refined search over a SumEmbeddings container at the C boundary, without a GPU: the five entry points are exported and
bound the same way in the header and in ctypes, and every argument error -- in the library and in the Python wrappers --
is GRANNE_HIP_ERR_INVALID with a message before any device call. A container is host data until a device entry point
first needs it, so live containers exist here; a live index does not, which the walk side's null check covers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("granne_hip_refine_sum_embeddings_device", "granne_hip_search_refined_sum_embeddings_batch_device",
           "granne_hip_search_refined_sum_embeddings_batch", "granne_hip_sum_embeddings_rows_device",
           "granne_hip_sum_embeddings_rows")
C_TYPES = {"uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "int": C.c_int}


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


@pytest.fixture(scope="module")
def se(lib):
    import granne_amd
    tab = np.arange(5 * 6, dtype=np.float32).reshape(5, 6)
    return granne_amd.SumEmbeddings(tab, [[0, 1], [2], [], [4, 4, 3]])


def test_symbols_are_exported_and_bound(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert lib.granne_hip_abi_version() == 3  # additive entries do not bump it
    header = open(os.path.join(ROOT, "include", "granne_hip.h")).read()
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", header)


def test_prototypes_agree_between_header_and_ctypes():
    """Argument for argument: a pointer in the header is a c_void_p in ctypes, a scalar the ctypes type of its width."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "granne_hip.h")).read(), flags=re.S)
    for name in ENTRIES:
        ret, args = re.search(r"(\w+)\s+%s\s*\(([^;]*?)\)\s*;" % name, header).groups()
        assert ret == "int"
        want = []
        for a in args.split(","):
            a = " ".join(a.split())
            want.append(C.c_void_p if "*" in a else C_TYPES[a.replace("const ", "").rsplit(" ", 1)[0]])
        res, got = _lib.SIGNATURES[name]
        assert res is C.c_int and got == want, (name, got, want)
    # the fused entries mirror the index forms argument for argument
    for a, b in (("granne_hip_search_refined_sum_embeddings_batch_device", "granne_hip_search_refined_batch_device"),
                 ("granne_hip_search_refined_sum_embeddings_batch", "granne_hip_search_refined_batch"),
                 ("granne_hip_refine_sum_embeddings_device", "granne_hip_refine_device")):
        assert _lib.SIGNATURES[a] == _lib.SIGNATURES[b]


def test_python_surface():
    import granne_amd
    for m in ("refine", "refine_device", "to_rows", "to_rows_device", "from_device"):
        assert hasattr(granne_amd.SumEmbeddings, m), m


def test_a_dtype_code_sizes_the_buffer_like_its_name():
    """to_rows takes GRANNE_HIP_F32 / _I8 / _F16 as well as the names: each code maps to the numpy dtype of its rows, so the
    buffer the library fills has count x dim scalars of the right width, never one byte per scalar."""
    from granne_amd.embeddings import _dense_type
    for name, code, dt in (("angular", _lib.F32, np.float32), ("angular_int", _lib.I8, np.int8), ("angular_f16", _lib.F16, np.float16)):
        assert _dense_type(name) == _dense_type(code) == _dense_type(name.upper()) == (code, dt)
        assert _dense_type(np.int64(code)) == (code, dt)


def test_argument_errors_of_the_rerank_need_no_device(lib, se):
    p = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    err = lambda: lib.granne_hip_last_error()  # noqa: E731
    f = lib.granne_hip_refine_sum_embeddings_device  # (se, queries, nq, cand, counts, m, k, ids, dists, counts, status, stream)
    assert f(None, p, 1, p, None, 8, 4, p, p, p, None, None) == _lib.ERR_INVALID and b"container is null" in err()
    assert f(None, p, 0, p, None, 8, 4, p, p, p, None, None) == _lib.ERR_INVALID  # nq 0 does not excuse a null handle
    for m in (0, 1025, 0xFFFFFFFF):
        for h in (None, se._h):  # the plain numbers are checked first
            assert f(h, p, 1, p, None, m, 4, p, p, p, None, None) == _lib.ERR_INVALID and b"candidates per query" in err()
    assert f(se._h, p, 1, p, None, 8, 0, p, p, p, None, None) == _lib.ERR_INVALID and b"k must be" in err()
    assert f(se._h, None, 1, p, None, 8, 4, p, p, p, None, None) == _lib.ERR_INVALID and b"null buffer" in err()
    assert f(se._h, p, 1, p, None, 8, 4, p, p, None, None, None) == _lib.ERR_INVALID and b"null buffer" in err()
    assert f(se._h, None, 0, None, None, 8, 4, None, None, None, None, None) == _lib.OK  # nq 0: nothing to do, no device


def test_argument_errors_of_the_fused_calls_need_no_device(lib, se):
    p = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    err = lambda: lib.granne_hip_last_error()  # noqa: E731
    # (walk, se, qW, qR, nq, max_search, refine_from, k, ...): no index exists without a device, so walk is null throughout
    for h in (None, se._h):
        dev = lambda *a: lib.granne_hip_search_refined_sum_embeddings_batch_device(None, h, p, p, *a, p, p, p, None, None, None, None)  # noqa: E731
        host = lambda *a: lib.granne_hip_search_refined_sum_embeddings_batch(None, h, p, p, *a, p, p, p, None, None)  # noqa: E731
        for call in (dev, host):
            assert call(1, 50, 50, 10) == _lib.ERR_INVALID and b"walk index is null" in err()
            assert call(1, 50, 0, 10) == _lib.ERR_INVALID and b"candidates per query" in err()
            assert call(1, 2000, 1025, 10) == _lib.ERR_INVALID and b"candidates per query" in err()
            assert call(1, 50, 50, 0) == _lib.ERR_INVALID and b"k must be" in err()
            assert call(1, 20, 21, 10) == _lib.ERR_INVALID and b"max_search" in err()
            assert call(1, 0, 1, 10) == _lib.ERR_INVALID and b"max_search" in err()
            assert call(0, 50, 50, 10) == _lib.ERR_INVALID


def test_argument_errors_of_rows_need_no_device(lib, se):
    p = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    err = lambda: lib.granne_hip_last_error()  # noqa: E731
    dev, host = lib.granne_hip_sum_embeddings_rows_device, lib.granne_hip_sum_embeddings_rows
    assert dev(None, 0, 1, _lib.I8, p, 6, None) == _lib.ERR_INVALID and b"container is null" in err()
    assert host(None, 0, 1, _lib.I8, p) == _lib.ERR_INVALID and b"container is null" in err()
    for dtype in (3, -1, 7):
        assert dev(se._h, 0, 1, dtype, p, 24, None) == _lib.ERR_INVALID and b"dtype" in err()
        assert host(se._h, 0, 1, dtype, p) == _lib.ERR_INVALID and b"dtype" in err()
    for first, count in ((5, 0), (0, 5), (3, 2), (1 << 63, 1 << 63)):
        assert dev(se._h, first, count, _lib.F32, p, 24, None) == _lib.ERR_INVALID and b"out of range" in err()
        assert host(se._h, first, count, _lib.F32, p) == _lib.ERR_INVALID and b"out of range" in err()
    for dtype, stride in ((_lib.F32, 23), (_lib.F32, 26), (_lib.F16, 11), (_lib.F16, 13), (_lib.I8, 5)):
        assert dev(se._h, 0, 1, dtype, p, stride, None) == _lib.ERR_INVALID and b"stride" in err()
    assert dev(se._h, 0, 1, _lib.I8, None, 6, None) == _lib.ERR_INVALID and b"out is null" in err()
    assert host(se._h, 0, 1, _lib.I8, None) == _lib.ERR_INVALID and b"out is null" in err()
    assert dev(se._h, 4, 0, _lib.I8, None, 6, None) == _lib.OK and host(se._h, 2, 0, _lib.F16, None) == _lib.OK  # nothing to do


def test_wrapper_errors_need_no_device(lib, se):
    """SumEmbeddings.refine / to_rows and RefinedGranne over a container: dim mismatch, bad counts, bad m and k, an
    unknown element type -- all ERR_INVALID with a message, raised before anything touches a device."""
    import granne_amd
    cand = np.zeros((2, 3), np.uint64)

    def invalid(fn, text):
        with pytest.raises(granne_amd.GranneHipError) as e:
            fn()
        assert e.value.code == _lib.ERR_INVALID and text in str(e.value), str(e.value)

    invalid(lambda: se.refine(np.zeros((2, 5), np.float32), cand), "queries must be [nq, 6]")  # dim mismatch
    invalid(lambda: se.refine(np.zeros((3, 6), np.float32), cand), "queries must be")  # nq mismatch
    invalid(lambda: se.refine(np.zeros((2, 6), np.float32), cand, counts=[1]), "counts must be")
    invalid(lambda: se.refine(np.zeros((2, 6), np.float32), np.zeros((2, 0), np.uint64)), "candidates per query")
    invalid(lambda: se.refine(np.zeros((2, 6), np.float32), np.zeros((2, 1025), np.uint64)), "candidates per query")
    invalid(lambda: se.refine(np.zeros((2, 6), np.float32), cand, k=0), "k must be")
    got = se.refine(np.zeros((0, 6), np.float32), np.zeros((0, 3), np.uint64), k=4, dropped=True)  # nq 0: nothing to do
    assert got[0].shape == (0, 4) and got[1].shape == (0, 4) and got[2].shape == (0,) and got[3] == 0
    invalid(lambda: se.to_rows("angular_bits"), "unknown element type")
    for code in (5, 3, -1, 1.5, True, None):  # refused in Python, before a buffer is sized by the code
        invalid(lambda: se.to_rows(code), "unknown dtype")
        invalid(lambda: se.to_rows_device(code, 0), "unknown dtype")
    invalid(lambda: se.to_rows("angular_int", first=3, count=2), "out of range")
    assert se.to_rows("angular_f16", first=4, count=0).shape == (0, 6)

    class NoIndex:  # stands for a walk index: no live one exists without a device
        _h, device, dim, query_dtype = None, 0, 6, np.int8

    rg = granne_amd.RefinedGranne(NoIndex(), se)
    q8, q = np.zeros((2, 6), np.int8), np.zeros((2, 6), np.float32)
    with pytest.raises(ValueError):  # the wrapper's own dim check, as for two indexes
        rg.search_batch((q8, np.zeros((2, 5), np.float32)), 50, 10)
    invalid(lambda: rg.search_batch((q8, q), 20, 10, refine_from=21), "max_search")
    invalid(lambda: rg.search_batch((q8, q), 50, 10, refine_from=0), "candidates per query")
    invalid(lambda: rg.search_batch((q8, q), 50, 0), "k must be")
    invalid(lambda: rg.search_batch((q8, q), 50, 10), "walk index is null")
    invalid(lambda: rg.search_batch_device(0, 0, 2, 50, 50, 10, 0, 0, 0), "walk index is null")


def test_cpp_mirror_of_the_container_entries(tmp_path):
    """include/granne.hpp: RefinedSumEmbeddingsGranne and SumEmbeddings::rows_i8 compile (g++, host only), and their
    argument errors arrive as exceptions with the library's messages -- run here, no device involved."""
    build.build_library()
    exe = str(tmp_path / "test_refine_se_api")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_refine_se_api.cpp"), "-L", build.LIB_DIR, "-lgranne_hip",
                           "-Wl,-rpath," + build.LIB_DIR, "-Wl,--allow-shlib-undefined", "-o", exe])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok")
