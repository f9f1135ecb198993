"""The entries of filters and the exact selection on a partitioned index at the drop-in boundary: declared -- with the same
names -- in include/granne_hip.h, granne_amd/_lib.py, include/granne.hpp and the extern block of rust/granne-hip/src/gpu.rs
(Rust is source only: it is never compiled here), exported by the built library; the ABI version unchanged; the argument
checks that need no device. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32, u64, vp, i32 = C.c_uint32, C.c_uint64, C.c_void_p, C.c_int
# name -> (result, arguments) as include/granne_hip.h declares them
ENTRIES = {
    "granne_hip_filter_slice_device": (i32, [vp, u64, u64, u32, u64, u64, vp, u64, i32, vp]),
    "granne_hip_sharded_id_span": (u64, [vp]),
    "granne_hip_sharded_search_filtered_batch_device": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_search_filtered_batch": (i32, [vp, vp, u32, u32, u32, vp, u64, u64, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_device": (i32, [vp, vp, u32, u32, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk": (i32, [vp, vp, u32, u32, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_filtered_device": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp, vp]),
    "granne_hip_sharded_exact_topk_filtered": (i32, [vp, vp, u32, u32, vp, u64, vp, vp, vp, vp]),
}
C_TYPES = {"uint32_t": u32, "uint64_t": u64, "int": i32}


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def _declared(header, name):
    """(result, arguments) of `name` as ctypes, read from the header's declaration: a pointer is a void pointer"""
    m = re.search(r"\b(int|uint64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
    assert m, name
    args = [a.strip() for a in m.group(2).split(",")]
    return C_TYPES[m.group(1)], [vp if "*" in a else C_TYPES[a.replace("const ", "").split()[0]] for a in args]


def test_entries_are_declared_in_every_binding_with_one_signature():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    extern = rust[rust.index('extern "C" {'):]
    hpp = _read("include", "granne.hpp")
    for name, sig in ENTRIES.items():
        assert _declared(header, name) == sig, name
        assert _lib.SIGNATURES[name] == sig, name
        assert re.search(r"\bfn %s\(" % name, extern), name
    for name in ("granne_hip_sharded_id_span", "granne_hip_sharded_search_filtered_batch_device", "granne_hip_sharded_exact_topk_device",
                 "granne_hip_sharded_exact_topk_filtered_device"):
        assert name + "(" in hpp, name
    for name in ("granne_hip_sharded_id_span", "granne_hip_sharded_search_filtered_batch_device", "granne_hip_sharded_exact_topk",
                 "granne_hip_sharded_exact_topk_filtered_device"):
        assert "unsafe { %s(" % name in rust, name
    for fn in ("pub fn id_span(&self)", "pub fn search_filtered(&mut self", "pub fn exact_topk(&mut self", "pub fn exact_topk_filtered(&mut self"):
        assert fn in rust[rust.index("impl<E: GpuElements> GpuShardedGranne<E>"):], fn


def test_python_wrappers_exist():
    from granne_amd.sharded import ShardedHost
    for name in ("id_span", "search_filtered_batch", "search_filtered_batch_device", "exact_topk", "exact_topk_filtered"):
        assert callable(getattr(ShardedHost, name)), name


def test_library_exports_the_entries(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name


def test_abi_version_is_still_3(lib):
    assert lib.granne_hip_abi_version() == 3
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", _read("include", "granne_hip.h"))


def test_slice_refusals_need_no_device(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(vp)
    sl = lib.granne_hip_filter_slice_device
    assert sl(None, 100, 0, 1, 3, 10, p, 1, 0, None) == _lib.ERR_INVALID and b"null" in lib.granne_hip_last_error()
    assert sl(p, 100, 0, 1, 3, 10, None, 1, 0, None) == _lib.ERR_INVALID and b"null" in lib.granne_hip_last_error()
    assert sl(p, 100, 0, 0, 3, 10, p, 1, 0, None) == _lib.ERR_INVALID and b"n_filters" in lib.granne_hip_last_error()
    assert sl(p, 100, 0, 2, 3, 10, p, 1, 0, None) == _lib.ERR_INVALID  # stride 0 with two filters
    assert sl(p, 100, 3, 2, 3, 10, p, 1, 0, None) == _lib.ERR_INVALID  # 100 bits are 4 words
    assert b"filter_stride_words" in lib.granne_hip_last_error()
    assert sl(p, 100, 0, 1, 3, 33, p, 1, 0, None) == _lib.ERR_INVALID  # 33 bits are 2 words
    assert b"out_stride_words" in lib.granne_hip_last_error()
    assert sl(p, 100, 0, 1, 101, 0, p, 1, 0, None) == _lib.ERR_INVALID and b"first_bit" in lib.granne_hip_last_error()
    # zero output bits: nothing to do, whatever else is passed (first_bit == n_bits is a valid, empty slice)
    assert sl(None, 100, 0, 0, 100, 0, None, 0, 0, None) == _lib.OK


def test_handle_refusals_need_no_device(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(vp)
    assert lib.granne_hip_sharded_id_span(None) == 0
    assert lib.granne_hip_sharded_search_filtered_batch_device(None, p, 1, 10, 5, p, 0, 0, p, p, p, None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_search_filtered_batch(None, p, 1, 10, 5, p, 0, 0, p, p, p, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk_device(None, p, 1, 5, p, p, p, None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk(None, p, 1, 5, p, p, p, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk_filtered_device(None, p, 1, 5, p, 0, p, p, p, None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk_filtered(None, p, 1, 5, p, 0, p, p, p, None) == _lib.ERR_INVALID
    assert b"sharded index is null" in lib.granne_hip_last_error()
