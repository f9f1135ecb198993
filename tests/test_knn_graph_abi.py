"""granne_hip_knn_graph* at the drop-in boundary: exported by the built library, bound in granne_amd/_lib.py, reached by
include/granne.hpp and rust/granne-hip/src/gpu.rs; the argument check that needs no device names the entry. No GPU."""
import ctypes as C
import os

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, HOST = "granne_hip_knn_graph_device", "granne_hip_knn_graph"


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_every_binding_names_the_entries():
    assert len(_lib.SIGNATURES[DEVICE][1]) == 9 and len(_lib.SIGNATURES[HOST][1]) == 8
    rust, hpp = _read("rust", "granne-hip", "src", "gpu.rs"), _read("include", "granne.hpp")
    block = rust[rust.index('extern "C" {'):]
    assert "fn %s(" % DEVICE in block and "fn %s(" % HOST in block
    assert "pub fn knn_graph(" in rust and "unsafe { %s(" % HOST in rust
    assert " knn_graph(" in hpp and HOST + "(" in hpp


def test_library_exports_the_entries_and_checks_arguments_without_a_device():
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    assert hasattr(raw, DEVICE) and hasattr(raw, HOST)
    lib = _lib.lib()
    assert lib.granne_hip_knn_graph_device(None, 0, 1, 5, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"knn_graph: index is null" in lib.granne_hip_last_error()
    assert lib.granne_hip_knn_graph(None, 0, 1, 5, None, None, None, None) == _lib.ERR_INVALID
