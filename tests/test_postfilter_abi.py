"""The entries of post-filtered search at the drop-in boundary: declared -- with the same names -- in include/granne_hip.h,
granne_amd/_lib.py, include/granne.hpp and rust/granne-hip/src/gpu.rs, exported by the built library; the ABI version and the
option enum unchanged; every refusal that needs no handle names its cause. (The refusals that need a handle -- a null
filter, a short stride, EXACT on an F16 handle -- are in tests/test_gpu_postfiltered.py.) No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_search_postfiltered_batch_device", "granne_hip_search_postfiltered_batch"]


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
        assert _lib.SIGNATURES[name][0] is C.c_int, name
        assert re.search(r"\bfn %s\(" % name, extern), name
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    # (index, queries, nq, k, min_allowed, stages, n_stages, fallback, filter, stride, scratch_bytes, ids, dists, counts, stage, status[, stream])
    want = [vp, vp, u32, u32, u32, vp, u32, C.c_int, vp, u64, u64, vp, vp, vp, vp, vp]
    assert _lib.SIGNATURES[ENTRIES[0]][1] == want + [vp]
    assert _lib.SIGNATURES[ENTRIES[1]][1] == want
    for name, value in (("MAX_STAGES", 8), ("FALLBACK_SHORT", 0), ("FALLBACK_EXACT", 1), ("STAGE_EXACT", 0xFFFFFFFF), ("STAGE_SHORT", 0xFFFFFFFE)):
        m = re.search(r"#define GRANNE_HIP_PF_%s (0x[0-9A-Fa-f]+|\d+)u?\b" % name, header)
        assert m and int(m.group(1), 0) == value == getattr(_lib, "PF_" + name), name
        assert re.search(r"pub const GRANNE_HIP_PF_%s: \w+ = " % name, rust), name
    assert "granne_hip_search_postfiltered_batch_device(" in hpp and "search_postfiltered(const Element* elements, size_t nq," in hpp
    assert "unsafe { granne_hip_search_postfiltered_batch_device(" in rust and "pub fn search_postfiltered(" in rust


def test_python_wrappers_exist():
    from granne_amd import Granne
    from granne_amd.filters import postfilter_stages
    assert callable(Granne.search_postfiltered) and callable(Granne.search_postfiltered_batch)
    assert callable(Granne.search_postfiltered_batch_device) and callable(postfilter_stages)


def test_library_exports_the_entries(lib):
    raw = C.CDLL(build.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(raw, name), name
    blob = open(build.LIB_PATH, "rb").read()
    for kernel in (b"pf_take_kernel", b"pf_gather_rows_kernel", b"pf_scatter_kernel"):
        assert kernel in blob, kernel


def test_abi_version_and_options_are_unchanged(lib):
    assert lib.granne_hip_abi_version() == 3
    assert re.search(r"#define GRANNE_HIP_ABI_VERSION 3\b", _read("include", "granne_hip.h"))
    opts = dict((n, int(v)) for n, v in re.findall(r"\bGRANNE_HIP_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", _read("include", "granne_hip.h")))
    assert max(opts.values()) == 21 == opts["FORCE_GENERAL"]


def test_the_header_states_the_contract():
    h = _read("include", "granne_hip.h")
    for phrase in ("All bits set: every query ends at stage 0", "L = Granne::search(q, max_search = E_s, num_neighbors = E_s)",
                   "if len(A) >= min_allowed or len(L) < E_s:", "return exact_topk_filtered(q, k), stage = GRANNE_HIP_PF_STAGE_EXACT",
                   "Nothing allowed: count 0 and GRANNE_HIP_OK", "never bit-tested", "[3] += the", "queries no stage finished",
                   "WAITS on `stream` once per stage it goes beyond", "never take part in GRANNE_HIP_OPT_COALESCE"):
        assert phrase in h, phrase


def test_refusals_need_no_device_and_name_their_cause(lib):
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    # (the arguments that need no handle are checked before the handle: a null index reaches each of these messages)

    def stages(*v):
        return (C.c_uint32 * max(len(v), 1))(*v)

    def refused(word, ix=None, k=10, min_allowed=16, st=(16, 64), n=None, fallback=1, nq=1):
        n = len(st) if n is None else n
        for rc in (lib.granne_hip_search_postfiltered_batch_device(ix, p, nq, k, min_allowed, stages(*st), n, fallback, p, 0, 0, p, p, p, None, None, None),
                   lib.granne_hip_search_postfiltered_batch(ix, p, nq, k, min_allowed, stages(*st), n, fallback, p, 0, 0, p, p, p, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in lib.granne_hip_last_error().decode(), lib.granne_hip_last_error()

    refused("index is null")
    refused("index is null", nq=0)  # also with nq == 0
    refused("n_stages (0)", n=0)
    refused("n_stages (9)", st=tuple(range(16, 25)))
    refused("strictly ascending", st=(16, 16))
    refused("strictly ascending", st=(16, 64, 32))
    refused("stages[1] is 0", st=(16, 0))
    refused("stages[0] is 0", st=(0, 16), min_allowed=0, k=0)
    refused("num_neighbors must be > 0", k=0)
    refused("num_neighbors (17) must not exceed min_allowed (16)", k=17)
    refused("min_allowed (17) must not exceed stages[0] (16)", min_allowed=17)
    refused("fallback (2)", fallback=2)
    refused("fallback (-1)", fallback=-1)
    refused("num_neighbors up to 1024", k=1025, min_allowed=2000, st=(2000, 4000))
    assert lib.granne_hip_search_postfiltered_batch_device(None, p, 1, 10, 16, None, 2, 1, p, 0, 0, p, p, p, None, None, None) == _lib.ERR_INVALID
    assert b"stages is null" in lib.granne_hip_last_error()
