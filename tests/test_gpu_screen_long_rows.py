"""The long-row forms of the screened exact scans (granne_hip_index_screen_long_rows): after
`screen_long_rows()` a handle of f32 rows beyond 208 components or int8 rows beyond 128 is screened, not routed, and every
dense-query entry still answers with its unscreened sibling's ids, distance BYTES and counts -- for the first 8 queries
the oracle's too. No tolerance anywhere."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_filtered_model as fm  # noqa: E402
from tests.test_gpu_exact_topk_screened import _et, _rows, same  # noqa: E402

NQ = 70  # a partial query tile
# one chunk and a remainder (f32 209: no multiple of 4 either), dim 300, whole chunks, and the longest rows there are: the
# largest f32 bound and norm slack, and int8 dots beyond 2^24, whose conversion rounds
SHAPES = [(False, 209), (False, 300), (False, 768), (False, 2048), (True, 129), (True, 300), (True, 1024), (True, 2048)]


def _n(dim):
    """a partial last tile and several ranges. 20003 rows are one stage, counted twice; the dim-300 sets have 40003: a
    prefix of 16384 rows first, the floor raised again over all rows"""
    return 40003 if dim == 300 else 20003


@functools.lru_cache(maxsize=None)
def _data(int8, dim):
    """(rows, queries, float64 scores [nq, n]) -- made once per shape"""
    from oracle import oracle
    rng = np.random.default_rng(9900 + dim + int(int8))
    n = _n(dim)
    el, q = _rows(oracle, rng, n, dim, int8), _rows(oracle, rng, NQ, dim, int8)
    q[:2] = el[[n - 1, n // 2]]  # rows of the set: distance 0, at the clamp
    e64, q64 = el.astype(np.float64), q.astype(np.float64)
    s = (q64 @ e64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(e64, axis=1)[None, :])
    return el, q, s


@functools.lru_cache(maxsize=None)
def _handle(int8, dim):
    import granne_amd
    el = _data(int8, dim)[0]
    ix = granne_amd.Granne(_et(el), el, [])
    ix.screen_long_rows()
    return ix


def _form(int8):
    from granne_amd import _lib
    return _lib.ETS_FORM_I8_LONG if int8 else _lib.ETS_FORM_B16_LONG


@pytest.fixture
def ga_filter():
    import granne_amd
    return lambda mask: granne_amd.Filter.from_words(fm.words(mask, garbage_past_n=True), len(mask))


@pytest.mark.parametrize("k", [1, 100])
@pytest.mark.parametrize("int8,dim", SHAPES)
def test_long_rows_are_screened(oracle, int8, dim, k):
    from granne_amd import _lib
    el, q, s = _data(int8, dim)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon_long(1 if int8 else 0, dim)
    assert eps > 0
    # the reference alone keeps the case inside the cap: fewer than 2048 rows at or above the k-th score - 4 eps - a bucket of
    # the last stage, whose floor is at least the first stage's k-th score - eps - a first-stage bucket
    kth = -np.partition(-s, k - 1, axis=1)[:, k - 1]
    first = s[:, :16384] if _n(dim) > 2 * 16384 else s  # (one stage: all rows)
    kth_first = -np.partition(-first, k - 1, axis=1)[:, k - 1]
    width = (1.0 - (kth_first - eps - 2.25 / 64)) / 64
    assert ((s >= (kth - 4 * eps - width)[:, None]).sum(axis=1) < 2048).all()
    st = same(_handle(int8, dim), oracle, el, q, k)
    assert st[0] == 0 and st[1] == 0 and k <= st[2] < 2048
    assert st[3] == _form(int8)


@pytest.mark.parametrize("entry", ["filtered_shared", "filtered_per_query", "after", "range"])
@pytest.mark.parametrize("int8", [False, True])
def test_every_dense_entry(ga_filter, oracle, int8, entry):
    """each entry against its unscreened sibling, byte for byte, on the dim-300 handle; the long form in status[3]"""
    (el, q, _), ix = _data(int8, 300), _handle(int8, 300)
    rng = np.random.default_rng(9950)
    if entry.startswith("filtered"):
        masks = [fm.random_mask(rng, len(el), 0.3) for _ in range(NQ if entry == "filtered_per_query" else 1)]
        allowed = [ga_filter(a) for a in masks]
        allowed = allowed if entry == "filtered_per_query" else allowed[0]
        got = ix.exact_topk_screened_filtered(q, 10, allowed, stats=True)
        want = ix.exact_topk_filtered(q, 10, allowed, stats=True)
    elif entry == "after":  # page 2 after a page of 50
        i1, d1, _ = ix.exact_topk(q, 50)
        after = (d1[:, -1].copy(), i1[:, -1].copy())
        got = ix.exact_topk_screened_after(q, 50, after=after, stats=True)
        want = ix.exact_topk_after(q, 50, after=after, stats=True)
    else:  # the radius of query a: its 1st, 10th or 300th distance
        _, _, od = oracle.Index(el, []).scan_topk(q, 300)
        radii = od[np.arange(NQ), np.array([0, 9, 299])[np.arange(NQ) % 3]]
        got = ix.exact_range_screened(q, radii, 512, stats=True)
        want = ix.exact_range(q, radii, 512, stats=True)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:-1], want[:-1]))
    st = got[-1]
    assert st[0] == 0 and st[1] == 0 and st[3] == _form(int8)


@pytest.mark.parametrize("int8", [False, True])
def test_switch(oracle, int8):
    """off again: routed; on: the graphs stay routed; a handle of short rows runs its own form either way"""
    import granne_amd
    (el, q, _), ix = _data(int8, 300), _handle(int8, 300)
    st = ix.knn_graph(5, first=0, count=16, stats=True)[-1]
    assert st[1] == 16 and st[3] == 0
    ix.screen_long_rows(False)
    try:
        st = ix.exact_topk_screened(q, 10, stats=True)[-1]
        assert st[1] == NQ and st[3] == 0
    finally:
        ix.screen_long_rows()
    assert ix.exact_topk_screened(q, 10, stats=True)[-1][3] == _form(int8)
    rng = np.random.default_rng(9960)
    rows, few = _rows(oracle, rng, 3000, 100, int8), _rows(oracle, rng, 5, 100, int8)
    short = granne_amd.Granne(_et(rows), rows, [])
    for on in (True, False):
        short.screen_long_rows(on)
        assert same(short, oracle, rows, few, 10)[3] == (3 if int8 else 1)
    short.close()
