"""granne_hip_exact_range_screened* at the drop-in boundary: exported by the built library, declared in include/granne_hip.h
with exact_range's arguments in its order, bound in granne_amd/_lib.py, reached by include/granne.hpp and
rust/granne-hip/src/gpu.rs; the argument checks that need no device name the entry. No GPU."""
import ctypes as C
import os
import re

import numpy as np

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, HOST = "granne_hip_exact_range_screened_device", "granne_hip_exact_range_screened"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _params(header, name):
    """the parameter types of `name`'s declaration, names and comments dropped"""
    decl = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S).group(1)
    return [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in decl.split(",")]


def test_declared_with_exact_ranges_signature_in_every_binding():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    rust, hpp = _read("rust", "granne-hip", "src", "gpu.rs"), _read("include", "granne.hpp")
    for name, old in ((DEVICE, "granne_hip_exact_range_device"), (HOST, "granne_hip_exact_range")):
        assert _params(header, name) == _params(header, old), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[old], name
    assert re.search(r"\bfn %s\(" % DEVICE, rust[rust.index('extern "C" {'):]) and "unsafe { %s(" % DEVICE in rust
    assert "pub fn exact_range_screened(" in rust and DEVICE + "(" in hpp and " exact_range_screened(" in hpp


def test_library_exports_the_entries_and_checks_arguments_without_a_device():
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    assert hasattr(raw, DEVICE) and hasattr(raw, HOST)
    lib = _lib.lib()
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    assert lib.granne_hip_exact_range_screened_device(None, p, 1, p, 5, None, 0, p, p, p, p, None, None) == _lib.ERR_INVALID
    assert b"exact_range_screened: index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_exact_range_screened(None, p, 1, p, 5, None, 0, p, p, p, p, None) == _lib.ERR_INVALID
    assert b"exact_range_screened: index is null" in lib.granne_hip_last_error()
