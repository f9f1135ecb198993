"""The removal entries of RwGranneBuilder at the drop-in boundary, without a GPU: declared in include/granne_hip.h,
bound in granne_amd/_lib.py and rust/granne-hip/src/gpu.rs, exported by the library; the two new read-only options carry
one value everywhere; every language's wrapper has the five calls; null arguments are refused before any device call."""
import ctypes as C
import os
import re
import subprocess

import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_rw_builder_remove", "granne_hip_rw_builder_restore", "granne_hip_rw_builder_removed_count",
           "granne_hip_rw_builder_alive", "granne_hip_rw_builder_compact"]
WRAPPERS = ["remove", "restore", "removed_count", "alive_filter", "compact"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_entries_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"\bfn %s\(" % name, rust), name
        assert hasattr(raw, name), name
    assert lib.granne_hip_abi_version() == 3  # entries are only added


def test_options_agree_in_every_binding(tmp_path):
    header = _read("include", "granne_hip.h")
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    for name, value in (("REMOVED", 4), ("FILTERED_SEARCHES", 5)):
        assert int(re.search(r"\bGRANNE_HIP_RW_OPT_%s\s*=\s*(\d+)" % name, header).group(1)) == value
        assert getattr(_lib, "RW_OPT_" + name) == value
        assert "pub const GRANNE_HIP_RW_OPT_%s: c_int = %d;" % (name, value) in rust
    assert int(re.search(r"\bGRANNE_HIP_RW_OPT_SORTED_LAUNCHES\s*=\s*(\d+)", header).group(1)) == 3  # the enum continues
    from granne_amd import rw_builder
    assert (rw_builder.REMOVED, rw_builder.FILTERED_SEARCHES) == (4, 5)
    # include/granne.hpp takes the values from the header it includes: every member of RwGranneBuilder compiles for
    # both dense element types, and the names it uses are the header's 4 and 5
    src = tmp_path / "rw_remove_hpp.cpp"
    src.write_text('#include "granne.hpp"\n'
                   "template class granne::RwGranneBuilder<granne::angular::Vectors>;\n"
                   "template class granne::RwGranneBuilder<granne::angular_int::Vectors>;\n"
                   'static_assert(GRANNE_HIP_RW_OPT_REMOVED == 4 && GRANNE_HIP_RW_OPT_FILTERED_SEARCHES == 5, "");\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    hpp = _read("include", "granne.hpp")
    assert "GRANNE_HIP_RW_OPT_FILTERED_SEARCHES" in hpp and "granne_hip_rw_builder_removed_count" in hpp


def test_every_wrapper_has_the_five_calls():
    from granne_amd import RwGranneBuilder
    for name in WRAPPERS:
        assert callable(getattr(RwGranneBuilder, name)), name
    hpp = _read("include", "granne.hpp")
    body = hpp[hpp.index("class RwGranneBuilder {"):]
    body = body[:body.index("\n};\n")]
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    i = rust.index("impl<E: GpuElements> GpuRwGranneBuilder<E> {")
    rbody = rust[i:rust.index("impl<E: GpuElements> Drop for GpuRwGranneBuilder<E>", i)]
    for name, entry in zip(WRAPPERS, ENTRIES):
        assert re.search(r"\b%s\(" % name, body), name
        assert entry + "(" in body, entry
        assert "pub fn %s(" % name in rbody, name
        assert "unsafe { %s(" % entry in rbody, entry


def test_null_arguments_are_refused_without_a_device(lib):
    counts = (C.c_uint64 * 3)(7, 7, 7)
    ids = (C.c_uint64 * 2)(1, 2)
    out, n = C.c_void_p(), C.c_uint64(9)
    for fn in (lib.granne_hip_rw_builder_remove, lib.granne_hip_rw_builder_restore):
        assert fn(None, ids, 2, counts) == _lib.ERR_INVALID
        assert b"rw builder is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_rw_builder_removed_count(None) == 0
    assert lib.granne_hip_rw_builder_alive(None, None, None) == _lib.ERR_INVALID
    assert lib.granne_hip_rw_builder_compact(None, 10, C.byref(out), ids, C.byref(n)) == _lib.ERR_INVALID
    assert not out.value and n.value == 0
    assert lib.granne_hip_rw_builder_get_option(None, _lib.RW_OPT_REMOVED, None) == _lib.ERR_INVALID
