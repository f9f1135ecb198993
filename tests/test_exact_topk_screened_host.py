"""The screen's bound (granne_hip_exact_topk_screen_epsilon) against the oracle, on the host: numpy restates
the screen score of exact_topk_screened.h -- f32: two bf16 pieces per component, the three products xh qh + xh ql + xl qh
(each exact in f32), f32 accumulation; int8: the integer dot times the two f32 inverse norms -- and every
|score - (1 - oracle distance)| must lie within the library's eps: the number the kernels are given."""
import numpy as np
import pytest

from granne_amd import _lib, build


@pytest.fixture(scope="module")
def L():
    build.build_library()
    return _lib.lib()


def bf16(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def screen_f32(el, q):
    xh, qh = bf16(el), bf16(q)
    xl, ql = bf16(el - xh), bf16(q - qh)
    acc = np.zeros(len(el), np.float32)
    for c in range(el.shape[1]):
        for a, b in ((xh, qh), (xh, ql), (xl, qh)):
            acc = (acc + a[:, c] * b[c]).astype(np.float32)
    return np.minimum(acc, np.float32(1.0))


def screen_i8(el, q):
    one = np.float32(1.0)
    inv = lambda v: np.where(v > 0, one / np.sqrt(np.maximum(v, 1).astype(np.float32)), np.float32(0)).astype(np.float32)  # noqa: E731
    e, y = el.astype(np.int64), q.astype(np.int64)
    return ((e @ y).astype(np.float32) * inv((e * e).sum(axis=1))).astype(np.float32) * inv((y * y).sum(keepdims=True))[0]


def f32_rows(oracle, rng, kind, n, dim):
    x = (rng.random((n, dim), dtype=np.float32) - np.float32(0.5))
    if kind == "extreme":  # magnitudes over twelve decades (and a few components near the smallest normal numbers)
        x = (np.sign(x) * np.float32(10.0) ** -(rng.random((n, dim), dtype=np.float32) * 12)).astype(np.float32)
        x[:, 0] *= np.float32(1e-30)
    return oracle.normalize_f32(x)


@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("dim", [28, 100, 208])
def test_f32_score_is_within_epsilon(L, oracle, kind, dim):
    rng = np.random.default_rng(8800 + dim)
    n = 1500
    el, q = f32_rows(oracle, rng, kind, n, dim), f32_rows(oracle, rng, kind, 4, dim)
    el[:4] = q  # near the clamp: a row equal to the query
    el[4:8] = -q
    eps = L.granne_hip_exact_topk_screen_epsilon(0, dim)
    assert 0 < eps < 2e-4
    assert (np.einsum("ij,ij->i", el.astype(np.float64), el.astype(np.float64)) <= 1 + 2.0 ** -10).all()
    _, ids, ds = oracle.Index(el, []).scan_topk(q, n)
    for a in range(len(q)):
        d = np.empty(n, np.float32)
        d[ids[a].astype(np.int64)] = ds[a]
        err = np.abs(screen_f32(el, q[a]).astype(np.float64) - (1.0 - d.astype(np.float64)))
        print("f32 %s dim %d query %d: max |score - (1 - d)| = %.3g, eps = %.3g" % (kind, dim, a, err.max(), eps))
        assert err.max() <= eps


@pytest.mark.parametrize("kind", ["random", "extremes"])
@pytest.mark.parametrize("dim", [32, 100, 128])
def test_int8_score_is_within_epsilon(L, oracle, kind, dim):
    rng = np.random.default_rng(8900 + dim)
    n = 1500
    if kind == "random":
        el = np.trunc(rng.uniform(-1.0, 1.0, (n + 4, dim)) * 127.0).astype(np.int8)
    else:  # every component +-127, a few rows with a single +-1 beside zeros, a zero row
        el = (rng.integers(0, 2, (n + 4, dim)) * 254 - 127).astype(np.int8)
        el[10:20] = 0
        el[10:19, 0] = 1
    el, q = np.ascontiguousarray(el[:n]), np.ascontiguousarray(el[n:])
    el[:4], el[4:8] = q, -q
    eps = L.granne_hip_exact_topk_screen_epsilon(1, dim)
    assert 0 < eps <= 2.0 ** -20
    _, ids, ds = oracle.Index(el, []).scan_topk(q, n)
    for a in range(len(q)):
        d = np.empty(n, np.float32)
        d[ids[a].astype(np.int64)] = ds[a]
        err = np.abs(np.minimum(screen_i8(el, q[a]), np.float32(1)).astype(np.float64) - (1.0 - d.astype(np.float64)))
        assert err.max() <= eps, (a, err.max())


def test_no_screen_for_other_shapes(L):
    assert L.granne_hip_exact_topk_screen_epsilon(0, 209) == 0 and L.granne_hip_exact_topk_screen_epsilon(1, 129) == 0
    assert L.granne_hip_exact_topk_screen_epsilon(2, 100) == 0 and L.granne_hip_exact_topk_screen_epsilon(0, 0) == 0
    assert L.granne_hip_exact_topk_screen_epsilon(0, 112) < L.granne_hip_exact_topk_screen_epsilon(0, 113)
