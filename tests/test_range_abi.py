"""The entries of range search at the drop-in boundary: declared -- with the same names and types -- in include/granne_hip.h,
granne_amd/_lib.py, include/granne.hpp and rust/granne-hip/src/gpu.rs, exported by the built library with their kernels; the
ABI version and the option and scan-form enums unchanged; every refusal that needs no handle names its cause. (The
refusals that need a handle -- exact_range checks its handle first, as exact_topk does -- are in
tests/test_gpu_exact_range.py and tests/test_gpu_search_range.py.) No GPU."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_exact_range_device", "granne_hip_exact_range", "granne_hip_search_range_batch_device",
           "granne_hip_search_range_batch"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_entries_are_declared_in_every_binding():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "granne_hip.h"), flags=re.S)
    rust = _read("rust", "granne-hip", "src", "gpu.rs")
    extern = re.sub(r"\s+", "", rust[rust.index('extern "C" {'):])
    hpp = _read("include", "granne.hpp")
    spec = importlib.util.spec_from_file_location("gen_rust_sys", os.path.join(ROOT, "tools", "gen_rust_sys.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    protos = dict((name, (ret, params)) for name, ret, params in g.protos())
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.sub(r"\s+", "", g.decl(name, *protos[name])) in extern, name  # type for type, as the header has them
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    # (index, queries, nq, radii, cap, filter, stride, ids, dists, counts, totals, status[, stream])
    want = [vp, vp, u32, vp, u32, vp, u64, vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES[ENTRIES[0]][1] == want + [vp] and _lib.SIGNATURES[ENTRIES[1]][1] == want
    # (index, queries, nq, radii, cap, stages, n_stages, fallback, scratch_bytes, ids, dists, counts, found, stage, status[, stream])
    want = [vp, vp, u32, vp, u32, vp, u32, C.c_int, u64, vp, vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES[ENTRIES[2]][1] == want + [vp] and _lib.SIGNATURES[ENTRIES[3]][1] == want
    # the header's own parameter lists have those lengths and pointer positions
    for name in ENTRIES:
        params = re.search(r"\bint\s+%s\s*\(([^;]*)\);" % name, header).group(1).split(",")
        sig = _lib.SIGNATURES[name][1]
        assert len(params) == len(sig), name
        for text, t in zip(params, sig):
            assert ("*" in text) == (t is vp), (name, text)
            if t is not vp:
                assert ("uint64_t" in text) == (t is u64) and (text.strip().startswith("int ")) == (t is C.c_int), (name, text)
    for name, value in (("RANGE_CAP_MAX", 1024), ("RG_MAX_STAGES", 8), ("RG_FALLBACK_SHORT", 0), ("RG_FALLBACK_EXACT", 1),
                        ("RG_STAGE_EXACT", 0xFFFFFFFF), ("RG_STAGE_SHORT", 0xFFFFFFFE)):
        mm = re.search(r"#define GRANNE_HIP_%s (0x[0-9A-Fa-f]+|\d+)u?\b" % name, header)
        assert mm and int(mm.group(1), 0) == value == getattr(_lib, name), name
        assert re.search(r"pub const GRANNE_HIP_%s: \w+ = " % name, rust), name
    assert _lib.RANGE_CAP_MAX == _lib.EXACT_TOPK_KMAX
    assert "granne_hip_exact_range_device(" in hpp and "exact_range(const Element* elements, size_t nq, const float* radii, size_t cap," in hpp
    assert "granne_hip_search_range_batch_device(" in hpp and "search_range(const Element* elements, size_t nq, const float* radii, size_t cap," in hpp
    assert "unsafe { granne_hip_exact_range_device(" in rust and "pub fn exact_range(" in rust
    assert "unsafe { granne_hip_search_range_batch_device(" in rust and "pub fn search_range(" in rust


def test_python_wrappers_exist():
    from granne_amd import Granne
    from granne_amd.index import RANGE_DEFAULT_STAGES
    for name in ("exact_range", "exact_range_device", "search_range", "search_range_batch", "search_range_batch_device"):
        assert callable(getattr(Granne, name)), name
    assert list(RANGE_DEFAULT_STAGES) == sorted(set(RANGE_DEFAULT_STAGES)) and 1 <= len(RANGE_DEFAULT_STAGES) <= _lib.RG_MAX_STAGES


def test_library_exports_the_entries_and_holds_the_kernels(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
    blob = open(build.LIB_PATH, "rb").read()
    for kernel in (b"er_scan_kernel", b"er_rank_kernel", b"er_scatter_kernel", b"rg_take_kernel", b"pf_gather_rows_kernel", b"et_rank_kernel"):
        assert kernel in blob, kernel


def test_abi_version_and_enums_are_unchanged(lib):
    h = _read("include", "granne_hip.h")
    assert lib.granne_hip_abi_version() == 3
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", h)
    opts = dict((n, int(v)) for n, v in re.findall(r"\bGRANNE_HIP_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", h))
    assert max(opts.values()) == 21 == opts["FORCE_GENERAL"]
    forms = dict((n, int(v)) for n, v in re.findall(r"\bGRANNE_HIP_SCAN_([A-Z0-9_]+)\s*=\s*(\d+)", h))
    assert sorted(forms.values()) == list(range(11))


def test_the_header_states_the_contract():
    h = _read("include", "granne_hip.h")
    for phrase in ("W      = { i < n_elements : allowed(q, i) and dist(i, q) <= r }", "always exact, also beyond cap",
                   "answer = the first min(total, cap) members of W ordered by (distance bits, id)",
                   "A negative\n * radius gives count 0 and total 0", "voided, not partially\n * answered",
                   "L = Granne::search(q, max_search = E_s, num_neighbors = E_s)", "if within < len(L) or len(L) < E_s:",
                   "return exact_range(q, r, cap), found = total, stage = GRANNE_HIP_RG_STAGE_EXACT",
                   "WAITS on `stream` ONCE", "WAITS on `stream` once per stage it goes beyond",
                   "never take part in GRANNE_HIP_OPT_COALESCE", "Out of scope: granne_hip_rw_builder_*"):
        assert phrase in h, phrase


def test_refusals_need_no_device_and_name_their_cause(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)  # (64 zero bytes: as radii, sixteen times 0.0)

    def stages(*v):
        return (C.c_uint32 * max(len(v), 1))(*v)

    def refused(word, ix=None, cap=10, st=(16, 64), n=None, fallback=1, nq=1, q=p, r=p, host_only=False):
        n = len(st) if n is None else n
        calls = [lib.granne_hip_search_range_batch(ix, q, nq, r, cap, stages(*st), n, fallback, 0, p, p, p, None, None, None)]
        if not host_only:
            calls.append(lib.granne_hip_search_range_batch_device(ix, q, nq, r, cap, stages(*st), n, fallback, 0, p, p, p, None, None, None, None))
        for rc in calls:
            assert rc == _lib.ERR_INVALID
            assert word in lib.granne_hip_last_error().decode(), lib.granne_hip_last_error()

    refused("search_range: index is null")
    refused("search_range: index is null", nq=0)  # also with nq == 0
    refused("n_stages (0)", n=0)
    refused("n_stages (9)", st=tuple(range(16, 25)))
    refused("strictly ascending", st=(16, 16))
    refused("strictly ascending", st=(16, 64, 32))
    refused("stages[1] is 0", st=(16, 0))
    refused("stages[0] is 0", st=(0, 16))
    refused("cap (0) must be in [1, 1024]", cap=0)
    refused("cap (1025) must be in [1, 1024]", cap=1025)
    refused("fallback (2)", fallback=2)
    refused("fallback (-1)", fallback=-1)
    refused("null buffer", q=None)
    refused("null buffer", r=None)
    nan = np.array([0.0, 1.0, np.nan, 0.5], np.float32)
    refused("the radius of query 2 is NaN", r=nan.ctypes.data_as(C.c_void_p), nq=4, host_only=True)
    assert lib.granne_hip_search_range_batch_device(None, p, 1, p, 10, None, 2, 1, 0, p, p, p, None, None, None, None) == _lib.ERR_INVALID
    assert b"stages is null" in lib.granne_hip_last_error()
    for rc in (lib.granne_hip_exact_range(None, p, 1, p, 10, None, 0, p, p, p, p, None),
               lib.granne_hip_exact_range(None, p, 0, p, 10, None, 0, p, p, p, p, None),
               lib.granne_hip_exact_range_device(None, p, 1, p, 10, None, 0, p, p, p, p, None, None),
               lib.granne_hip_exact_range_device(None, p, 0, p, 10, None, 0, p, p, p, p, None, None)):
        assert rc == _lib.ERR_INVALID and b"exact_range: index is null" in lib.granne_hip_last_error()
