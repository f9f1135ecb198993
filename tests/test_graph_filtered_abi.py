"""granne_hip_knn_graph_filtered* and granne_hip_range_graph_filtered* at the drop-in boundary: declared with one signature in
include/granne_hip.h, granne_amd/_lib.py and rust/granne-hip/src/gpu.rs, exported by the built library, reached by
include/granne.hpp; the argument checks that need no device name the entry. No GPU."""
import ctypes as C
import os
import re

import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = [("granne_hip_knn_graph_filtered_device", 11), ("granne_hip_knn_graph_filtered", 10),
           ("granne_hip_range_graph_filtered_device", 13), ("granne_hip_range_graph_filtered", 12)]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.mark.parametrize("name,args", ENTRIES)
def test_every_binding_names_the_entry(name, args):
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
    assert len(proto.split(",")) == args == len(_lib.SIGNATURES[name][1])
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    decl = re.search(r"fn %s\(([^;]*)\) -> c_int;" % name, rust[rust.index('extern "C" {'):]).group(1)
    assert len(decl.split(",")) == args
    wrapper = name[len("granne_hip_"):].replace("_device", "")
    assert "pub fn %s(" % wrapper in rust and "unsafe { granne_hip_%s_device(" % wrapper in rust
    hpp = _read("include", "granne.hpp")
    assert " %s(" % wrapper in hpp and "granne_hip_%s_device(" % wrapper in hpp


def test_library_exports_the_entries_and_checks_arguments_without_a_device():
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    lib = _lib.lib()
    for name, args in ENTRIES:
        assert hasattr(raw, name)
        word = name[len("granne_hip_"):].replace("_device", "").encode() + b": index is null"
        mid = (None, 5) if "range" in name else (5,)  # (radii, cap) or k
        assert getattr(lib, name)(None, None, 0, 1, *mid, *([None] * (args - 4 - len(mid)))) == _lib.ERR_INVALID
        assert word in lib.granne_hip_last_error()
