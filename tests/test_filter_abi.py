"""The filtered-search entries at the drop-in boundary: present -- with the same names -- in include/granne_hip.h,
granne_amd/_lib.py, include/granne.hpp and the extern block of rust/granne-hip/src/gpu.rs; the ABI version unchanged; the
bitmap's bit layout; and the argument checks that need no device. No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from granne_amd import _lib, build
from tests import filter_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_search_filtered_batch_device", "granne_hip_search_filtered_batch", "granne_hip_filter_words",
           "granne_hip_filter_from_ids_device", "granne_hip_filter_from_mask_device", "granne_hip_filter_count_device"]


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
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"\bfn %s\(" % name, extern), name
    # the device entry: 14 arguments, the filter and its two u64 after num_neighbors
    res, args = _lib.SIGNATURES["granne_hip_search_filtered_batch_device"]
    assert len(args) == 14 and args[5:8] == [C.c_void_p, C.c_uint64, C.c_uint64]
    assert len(_lib.SIGNATURES["granne_hip_search_filtered_batch"][1]) == 13
    # the C++ and Rust wrappers reach them
    for name in ("granne_hip_search_filtered_batch_device", "granne_hip_filter_from_ids_device", "granne_hip_filter_from_mask_device",
                 "granne_hip_filter_count_device", "granne_hip_filter_words"):
        assert name + "(" in hpp, name
        assert "unsafe { %s(" % name in rust, name
    assert "class Filter" in hpp and "search_filtered(" in hpp
    assert "pub struct GpuFilter" in rust and "pub fn search_filtered(" in rust


def test_library_exports_the_entries(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name


def test_abi_version_is_still_3(lib):
    assert lib.granne_hip_abi_version() == 3
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", _read("include", "granne_hip.h"))
    # the one new option continues the enum at 21, in every binding
    opts = dict((n, int(v)) for n, v in re.findall(r"\bGRANNE_HIP_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", _read("include", "granne_hip.h")))
    assert opts["LAST_SCAN"] == 20 and opts["FORCE_GENERAL"] == 21 == _lib.OPT_FORCE_GENERAL == max(opts.values())
    assert "pub const GRANNE_HIP_OPT_FORCE_GENERAL: c_int = 21;" in _read("rust", "granne-hip", "src", "gpu.rs")


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 4000])
def test_filter_words(lib, n):
    w = C.c_uint64(99)
    assert lib.granne_hip_filter_words(n, C.byref(w)) == _lib.OK
    assert w.value == (n + 31) // 32 == fm.pack_bits(np.zeros(n, bool)).size
    assert lib.granne_hip_filter_words(n, None) == _lib.ERR_INVALID


def test_bit_layout_is_stated_and_modelled():
    """bit (id & 31) of word (id >> 5): the header says so, the model packs so."""
    assert "bit (id & 31) of word (id >> 5)" in _read("include", "granne_hip.h")
    for i in (0, 1, 31, 32, 33, 63, 64, 3999):
        a = np.zeros(4000, bool)
        a[i] = True
        w = fm.pack_bits(a)
        assert w[i >> 5] == np.uint32(1) << np.uint32(i & 31) and np.count_nonzero(w) == 1


def test_argument_checks_need_no_device(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    assert lib.granne_hip_search_filtered_batch_device(None, p, 1, 10, 1, p, 0, 0, p, p, p, None, None, None) == _lib.ERR_INVALID
    assert b"index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_search_filtered_batch(None, p, 1, 10, 1, p, 0, 0, p, p, p, None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_from_ids_device(p, 1, 10, None, None, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_from_ids_device(None, 1, 10, p, None, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_from_mask_device(None, 10, p, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_filter_count_device(p, 10, None, 0, None) == _lib.ERR_INVALID
    # nothing to do: OK without a device
    assert lib.granne_hip_filter_from_mask_device(None, 0, None, 0, None) == _lib.OK
    assert lib.granne_hip_filter_from_ids_device(None, 0, 0, None, None, 0, None) == _lib.OK
