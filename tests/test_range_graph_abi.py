"""granne_hip_range_graph* at the drop-in boundary: declared with one signature in include/granne_hip.h and granne_amd/_lib.py,
exported by the built library, reached by include/granne.hpp and rust/granne-hip/src/gpu.rs; the argument checks that need
no device name the entry. No GPU."""
import ctypes as C
import os
import re

import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, HOST = "granne_hip_range_graph_device", "granne_hip_range_graph"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.mark.parametrize("name,args", [(DEVICE, 11), (HOST, 10)])
def test_every_binding_names_the_entry(name, args):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    assert len(proto.split(",")) == args == len(_lib.SIGNATURES[name][1])
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    decl = re.search(r"fn %s\(([^;]*)\) -> c_int;" % name, rust[rust.index('extern "C" {'):]).group(1)
    assert len(decl.split(",")) == args
    assert "pub fn range_graph(" in rust and "unsafe { %s(" % HOST in rust
    hpp = _read("include", "granne.hpp")
    assert " range_graph(" in hpp and HOST + "(" in hpp


def test_library_exports_the_entries_and_checks_arguments_without_a_device():
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    assert hasattr(raw, DEVICE) and hasattr(raw, HOST)
    lib = _lib.lib()
    assert lib.granne_hip_range_graph_device(None, 0, 1, None, 5, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"range_graph: index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_range_graph(None, 0, 1, None, 5, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"range_graph: index is null" in lib.granne_hip_last_error()
