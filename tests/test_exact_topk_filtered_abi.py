"""The entries of the exact scan under an id bitmap at the drop-in boundary: present -- with the same names -- in
include/granne_hip.h, granne_amd/_lib.py, include/granne.hpp and the extern block of rust/granne-hip/src/gpu.rs, exported by
the built library; the ABI version and the option enum unchanged; the argument checks that need no device. (The checks
that need a handle -- a null filter, a short stride, k of 0 and 1025, nq == 0 -- are in
tests/test_gpu_exact_topk_filtered.py: a handle is made on a device.) No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_filter_to_ids_device", "granne_hip_exact_topk_filtered_device", "granne_hip_exact_topk_filtered"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_entries_are_declared_in_every_binding():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    extern = rust[rust.index('extern "C" {'):]
    hpp = _read("include", "granne.hpp")
    for name in ENTRIES + ["granne_hip_index_num_elements"]:
        assert re.search(r"\b(int|uint64_t)\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bfn %s\(" % name, extern), name
    for name in ENTRIES:
        assert _lib.SIGNATURES[name][0] is C.c_int, name
    # the argument lists: the filter and its stride after k; six arguments for the compaction
    res, args = _lib.SIGNATURES["granne_hip_exact_topk_filtered_device"]
    assert len(args) == 11 and args[2:6] == [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    res, args = _lib.SIGNATURES["granne_hip_exact_topk_filtered"]
    assert len(args) == 10 and args[2:6] == [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]
    res, args = _lib.SIGNATURES["granne_hip_filter_to_ids_device"]
    assert args == [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert _lib.SIGNATURES["granne_hip_index_num_elements"] == (C.c_uint64, [C.c_void_p])
    # the C++ and Rust wrappers reach them
    for name in ("granne_hip_filter_to_ids_device", "granne_hip_exact_topk_filtered_device", "granne_hip_index_num_elements"):
        assert name + "(" in hpp, name
        assert "unsafe { %s(" % name in rust, name
    assert "std::vector<uint64_t> ids() const" in hpp and "exact_topk_filtered(const Element* elements, size_t nq, size_t k," in hpp
    assert "pub fn ids(&self)" in rust and "pub fn exact_topk_filtered(" in rust


def test_python_wrappers_exist():
    from granne_amd import Granne
    from granne_amd.filters import Filter
    assert callable(Filter.ids)
    assert callable(Granne.exact_topk_filtered) and callable(Granne.exact_topk_filtered_device) and callable(Granne.num_elements)


def test_library_exports_the_entries(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES + ["granne_hip_index_num_elements"]:
        assert hasattr(raw, name), name


def test_abi_version_and_options_are_unchanged(lib):
    assert lib.granne_hip_abi_version() == 3
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", _read("include", "granne_hip.h"))
    opts = dict((n, int(v)) for n, v in re.findall(r"\bGRANNE_HIP_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", _read("include", "granne_hip.h")))
    assert max(opts.values()) == 21 == opts["FORCE_GENERAL"]


def test_the_header_states_the_contract():
    h = _read("include", "granne_hip.h")
    for phrase in ("filter_stride_words == 0", "d_status[3] = m", "n_elements up to 2^32 - 1", "A filter that allows nothing gives count 0"):
        assert phrase in h, phrase


def test_argument_checks_need_no_device(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    assert lib.granne_hip_exact_topk_filtered_device(None, p, 1, 10, p, 0, p, p, p, None, None) == _lib.ERR_INVALID
    assert b"index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_exact_topk_filtered(None, p, 1, 10, p, 0, p, p, p, None) == _lib.ERR_INVALID
    assert b"index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_exact_topk_filtered_device(None, p, 0, 10, p, 0, p, p, p, None, None) == _lib.ERR_INVALID  # also with nq == 0
    # the compaction: a null count, a null filter, a null id buffer, more ids than 32 bits name
    assert lib.granne_hip_filter_to_ids_device(p, 10, p, None, 0, None) == _lib.ERR_INVALID
    assert b"out_count" in lib.granne_hip_last_error()
    assert lib.granne_hip_filter_to_ids_device(None, 10, p, p, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_to_ids_device(p, 10, None, p, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_to_ids_device(p, 1 << 32, p, p, 0, None) == _lib.ERR_INVALID
    assert b"2^32 - 1" in lib.granne_hip_last_error()
    assert lib.granne_hip_index_num_elements(None) == 0
