"""granne_hip_index_screen_long_rows and granne_hip_exact_topk_screen_epsilon_long without a device: null handles, the
bound over every shape, and the two new status values in the three bindings."""
import os
import re

import pytest

from granne_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM_MAX = 2048  # ETS_LONG_DIM_MAX


@pytest.fixture(scope="module")
def lib():
    build.build_library()
    return _lib.lib()


def test_null_handle_is_refused(lib):
    assert lib.granne_hip_index_screen_long_rows(None, 1) == _lib.ERR_INVALID
    assert b"index is null" in lib.granne_hip_last_error()


@pytest.mark.parametrize("dtype,short_max", [(0, 208), (1, 128)])
def test_epsilon_long(lib, dtype, short_max):
    eps = [lib.granne_hip_exact_topk_screen_epsilon_long(dtype, d) for d in range(DIM_MAX + 2)]
    assert all(e == 0.0 for e in eps[:short_max + 1])  # dim 0 and the short forms' shapes
    assert all(e > 0.0 for e in eps[short_max + 1:DIM_MAX + 1])
    assert all(a <= b for a, b in zip(eps[short_max + 1:DIM_MAX], eps[short_max + 2:DIM_MAX + 1]))
    assert eps[short_max + 1] >= lib.granne_hip_exact_topk_screen_epsilon(dtype, short_max)  # no smaller than the short bound
    assert eps[DIM_MAX + 1] == 0.0 and lib.granne_hip_exact_topk_screen_epsilon_long(dtype, 1 << 20) == 0.0
    assert lib.granne_hip_exact_topk_screen_epsilon_long(2, 300) == 0.0  # GRANNE_HIP_F16


def test_form_values_agree_in_every_binding():
    header = open(os.path.join(ROOT, "include", "granne_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "granne-hip", "src", "gpu.rs")).read()
    for name, value in (("B16_LONG", 4), ("I8_LONG", 5)):
        assert int(re.search(r"#define GRANNE_HIP_ETS_FORM_%s (\d+)u" % name, header).group(1)) == value
        assert getattr(_lib, "ETS_FORM_" + name) == value
        assert "pub const GRANNE_HIP_ETS_FORM_%s: u32 = %d;" % (name, value) in rust
