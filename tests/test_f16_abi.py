"""GRANNE_HIP_F16 at the C boundary and the CPU facts the container rests on, without a GPU: the dtype's value, the ABI
version, the conversion entries in the header, the ctypes table and the Rust binding; and a numpy model of the definition
(widen -> normalise -> the 32-accumulator dot) showing why the rows are normalised where they are read."""
import ctypes as C
import os
import re

import numpy as np

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "granne_hip.h")
RUST_GPU_RS = os.path.join(ROOT, "rust", "granne-hip", "src", "gpu.rs")
ENTRIES = ("granne_hip_f32_to_f16_device", "granne_hip_f16_to_f32_device", "granne_hip_f32_to_f16", "granne_hip_f16_to_f32")


def test_header_values():
    src = open(HEADER).read()
    assert re.search(r"GRANNE_HIP_F32 = 0, GRANNE_HIP_I8 = 1, GRANNE_HIP_F16 = 2\b", src)
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", src)  # additive entries do not bump it
    assert _lib.F16 == 2 and (_lib.F32, _lib.I8) == (0, 1)
    assert re.search(r"pub const GRANNE_HIP_F16: c_int = 2;", open(RUST_GPU_RS).read())
    assert "struct f16" in open(os.path.join(ROOT, "include", "granne.hpp")).read()


def test_entries_are_exported_and_bound_with_the_headers_types():
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    lib = _lib.lib()
    assert lib.granne_hip_abi_version() == 3
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    protos = {name: (ret, params) for name, ret, params in g.protos()}
    rust = re.sub(r"\s+", "", open(RUST_GPU_RS).read())
    ctype_of = {"u64": C.c_uint64, "u32": C.c_uint32, "c_int": C.c_int}
    for name in ENTRIES:
        assert hasattr(raw, name), name
        assert name in protos, name
        ret, params = protos[name]
        assert re.sub(r"\s+", "", g.decl(name, ret, params)) in rust, name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(params), name
        for (pname, ptype), a in zip(params, args):
            assert a is (C.c_void_p if ptype.startswith("*") else ctype_of[ptype]), (name, pname, ptype)
    # halves cross the boundary as u16
    assert "d_out:*mutu16" in rust and "rows16:*constu16" in rust


def test_python_surface():
    import granne_amd
    from granne_amd import index
    assert index._ELEMENT_TYPES["angular_f16"] == (_lib.F16, np.float16)
    assert callable(granne_amd.to_f16) and callable(granne_amd.from_f16) and granne_amd.F16 == 2


def test_null_arguments_need_no_device():
    build.build_library()
    lib = _lib.lib()
    p = np.zeros(64, np.uint64).ctypes.data_as(C.c_void_p)
    assert lib.granne_hip_f32_to_f16_device(None, p, 4, 8, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_f16_to_f32_device(p, None, 4, 8, 1, 0, None) == _lib.ERR_INVALID
    assert lib.granne_hip_f32_to_f16_device(p, p, 4, 0, 0, None) == _lib.ERR_INVALID and b"dim" in lib.granne_hip_last_error()
    assert lib.granne_hip_f32_to_f16(None, p, 4, 8, 0) == _lib.ERR_INVALID
    assert lib.granne_hip_f16_to_f32(p, None, 4, 8, 1, 0) == _lib.ERR_INVALID
    # dtype 2 is known to the entries that take one; 3 is not
    h = C.c_void_p()
    assert lib.granne_hip_index_create(C.byref(h), p, 1, 0, _lib.F16, 0, None, None, None, 0) == _lib.ERR_INVALID
    assert b"dim" in lib.granne_hip_last_error()
    assert lib.granne_hip_index_create(C.byref(h), p, 1, 8, 3, 0, None, None, None, 0) == _lib.ERR_INVALID
    assert b"unknown dtype" in lib.granne_hip_last_error()
    cfg = _lib.BuildConfig()
    lib.granne_hip_build_config_default(C.byref(cfg))
    sh = C.c_void_p()
    devs = (C.c_int * 1)(0)
    assert lib.granne_hip_sharded_build(C.byref(sh), C.byref(cfg), p, 8, 4, _lib.F16, 1, devs, 1) == _lib.ERR_INVALID
    assert b"F16" in lib.granne_hip_last_error()


def test_rows_rounded_to_halves_must_be_normalised_on_read(oracle):
    """20000 x 100 unit f32 rows, seed 1, rounded to halves. Widened only, more than a fifth of them lie further than
    100 f32 epsilons from the unit sphere -- the reference's builder would treat each as a zero vector and leave it out
    of the graph (src/index/mod.rs:813); normalised on read (the container's definition) none does."""
    rng = np.random.default_rng(1)
    rows = oracle.normalize_f32((rng.random((20000, 100), dtype=np.float32) - np.float32(0.5)).astype(np.float32))
    wide = rows.astype(np.float16).astype(np.float32)
    eps100 = 100.0 * float(np.finfo(np.float32).eps)

    def self_dist(x):  # Vector::dist of a row with itself: max(0, 1 - dot_product_f32(x, x))
        return np.array([max(0.0, float(np.float32(1.0) - np.float32(oracle.dot_f32(r, r)))) for r in x])

    share = float((self_dist(wide) > eps100).mean())
    assert share > 0.2, share
    assert float((self_dist(oracle.normalize_f32(wide)) > eps100).mean()) == 0.0
    # and the model of dist_to_element is the f32 oracle's over the normalised rows
    R = oracle.normalize_f32(wide[:50])
    q = oracle.normalize_f32((rng.random((1, 100), dtype=np.float32) - np.float32(0.5)).astype(np.float32))[0]
    for r in R[:5]:
        d = np.float32(1.0) - np.float32(oracle.dot_f32(r, q))
        assert np.float32(max(np.float32(0.0), d)).tobytes() == np.float32(oracle.dist(r, q)).tobytes()


def test_cpp_templates_reject_f16_elements(tmp_path):
    """include/granne.hpp: granne::f16 and its dtype_of exist, the conversions compile, and the class templates -- whose
    queries have the element type of their Elements -- refuse f16 elements at compile time (an F16 index takes f32 queries)."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    inc = os.path.join(ROOT, "include")
    ok = tmp_path / "ok.cpp"
    ok.write_text('#include "granne.hpp"\n'
                  'static_assert(granne::detail::dtype_of<granne::f16>::value == GRANNE_HIP_F16 && sizeof(granne::f16) == 2, "");\n'
                  'std::vector<granne::f16> f(const std::vector<float>& r) { return granne::angular_f16::to_f16(r, 4); }\n'
                  'std::vector<float> g(const std::vector<granne::f16>& r) { return granne::angular_f16::from_f16(r, 4); }\n')
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", inc, str(ok)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for body in ("granne::Granne<granne::detail::Vectors<granne::f16>>* p; auto n = sizeof(*p);",
                 "granne::GranneBuilder<granne::detail::Vectors<granne::f16>>* p; auto n = sizeof(*p);"):
        bad = tmp_path / "bad.cpp"
        bad.write_text('#include "granne.hpp"\nvoid f() { %s (void)n; }\n' % body)
        r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", inc, str(bad)], capture_output=True, text=True)
        assert r.returncode != 0 and "f32 queries" in r.stderr, r.stderr[-400:]
