"""granne_hip_exact_topk_after* and granne_hip_exact_topk_screened_after* at the drop-in boundary: exported by the built
library, declared in include/granne_hip.h, bound in granne_amd/_lib.py, reached by include/granne.hpp,
rust/granne-hip/src/gpu.rs and granne_amd.Granne; the argument checks that need no device give the siblings' messages.
No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from granne_amd import Granne, _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["granne_hip_exact_topk_after", "granne_hip_exact_topk_screened_after"]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


@pytest.mark.parametrize("host", ENTRIES)
def test_exported_and_bound_in_every_binding(host):
    build.build_library()
    raw = C.CDLL(build.LIB_PATH)
    header, rust, hpp = _read("include", "granne_hip.h"), _read("rust", "granne-hip", "src", "gpu.rs"), _read("include", "granne.hpp")
    for name in (host, host + "_device"):
        assert hasattr(raw, name) and name in _lib.SIGNATURES and re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert re.search(r"\bfn %s\(" % name, rust[rust.index('extern "C" {'):]), name
    method = host[len("granne_hip_"):]
    assert "pub fn %s(" % method in rust and " %s(" % method in hpp and host + "_device" in hpp
    assert callable(getattr(Granne, method)) and callable(getattr(Granne, method + "_device"))


@pytest.mark.parametrize("host,sibling", zip(ENTRIES, ["", "exact_topk_screened: "]))
def test_arguments_are_checked_before_any_device_call(host, sibling):
    lib = _lib.lib()
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    calls = [lambda h, q, k: getattr(lib, host)(h, q, 1, k, p, p, None, 0, p, p, p, None),
             lambda h, q, k: getattr(lib, host + "_device")(h, q, 1, k, p, p, None, 0, p, p, p, None, None)]
    for call in calls:  # (what is checked behind the handle -- k, the buffers, the cursor -- needs a handle: the gpu test below)
        for q, k in ((p, 5), (None, 5), (p, 0), (p, 1025)):
            assert call(None, q, k) == _lib.ERR_INVALID
            assert (sibling + "index is null").encode() in lib.granne_hip_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("host,sibling", zip(ENTRIES, ["", "exact_topk_screened: "]))
def test_gpu_exact_topk_after_refusals(host, sibling):
    import granne_amd
    lib = _lib.lib()
    el = np.eye(8, 32, dtype=np.float32)
    ix = granne_amd.Granne("angular", el, [])
    p = el.ctypes.data_as(C.c_void_p)
    for dev in (False, True):
        fn = getattr(lib, host + ("_device" if dev else ""))
        tail = (None, None) if dev else (None,)
        for k in (0, 1025):
            assert fn(ix._h, p, 1, k, p, p, None, 0, p, p, p, *tail) == _lib.ERR_INVALID
            assert (sibling + "k must be in [1, 1024]").encode() in lib.granne_hip_last_error()
        assert fn(ix._h, None, 1, 5, p, p, None, 0, p, p, p, *tail) == _lib.ERR_INVALID
        assert b"null buffer" in lib.granne_hip_last_error()
        assert fn(ix._h, p, 1, 5, None, p, None, 0, p, p, p, *tail) == _lib.ERR_INVALID
        assert b"after_ids without after_dists" in lib.granne_hip_last_error()
    # the host entry stages what the device entry (the Python methods' way in) is given: the same answer
    ids, ds, cnt = np.zeros((8, 3), np.uint64), np.zeros((8, 3), np.float32), np.zeros(8, np.uint32)
    ad, ai = np.full(8, 1.0, np.float32), np.arange(8, dtype=np.uint64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert getattr(lib, host)(ix._h, p, 8, 3, ptr(ad), ptr(ai), None, 0, ptr(ids), ptr(ds), ptr(cnt), None) == _lib.OK
    want = getattr(ix, host[len("granne_hip_"):])(el, 3, after=(ad, ai))
    assert ids.tobytes() == want[0].tobytes() and ds.tobytes() == want[1].tobytes() and (cnt == want[2]).all()
    ix.close()
