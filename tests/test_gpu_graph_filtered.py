"""knn_graph_filtered and range_graph_filtered against the CPU oracle over the allowed rows el[A] alone, ids
mapped through A, and against exact_topk_filtered / exact_range under the same filter with the element struck out: ids,
distance BYTES, counts and totals, no tolerance. tests/README_graph_filtered.md says what each case pins."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402
from tests import range_model as rm  # noqa: E402
from tests.test_gpu_knn_graph import NONE, _et, _rows, same, strip  # noqa: E402

N, FIRST, COUNT = 40003, 16300, 300  # positions: start and end inside 32-row blocks, on both sides of the first prefix's end


def strip_range(ids, ds, cnt, tot, es, cap):
    """exact_range(rows es, r, cap + 1) -> the elements struck out: (ids, dists, counts, totals) at cap. In these inputs
    element e is the nearest row to itself, so it was counted exactly where it is listed."""
    oi, od = np.full((len(es), cap), NONE), np.full((len(es), cap), np.inf, np.float32)
    oc, ot = np.zeros(len(es), np.uint32), tot.copy()
    for r, e in enumerate(es):
        keep = np.nonzero(ids[r, :cnt[r]] != e)[0][:cap]
        oi[r, :len(keep)], od[r, :len(keep)], oc[r] = ids[r, keep], ds[r, keep], len(keep)
        ot[r] -= (ids[r, :cnt[r]] == e).any()
    return oi, od, oc, ot


def through(A, ids):
    """ids of the rows el[A] -> ids of el (A is ascending: (distance, id) order is kept)"""
    out = ids.copy()
    out[ids != NONE] = A[ids[ids != NONE].astype(np.intp)]
    return out


def knn_by_oracle(oracle, el, A, pos, k):
    sub = np.ascontiguousarray(el[A])
    _, ids, ds = oracle.Index(sub, []).scan_topk(sub[pos], min(k + 1, len(A)))
    oi, od, oc = strip(ids, ds, pos, k)
    return through(A, oi), od, oc


def range_by_oracle(oracle, el, A, pos, radii, cap):
    sub = np.ascontiguousarray(el[A])
    ids, ds = rm.full_scan(oracle, sub, sub[pos])
    keep = ids != np.asarray(pos)[:, None].astype(np.uint64)
    ans = rm.exact_range((ids[keep].reshape(len(pos), -1), ds[keep].reshape(len(pos), -1)), radii, cap)
    return through(A, ans.ids), ans.dists, ans.counts, ans.totals


def check_knn(ix, oracle, el, mask, k, first, count, rows=8):
    """knn_graph_filtered == the oracle (the first rows) == exact_topk_filtered(rows, k + 1) stripped (all); the status words"""
    A = np.nonzero(mask)[0]
    pos = np.arange(first, first + count)
    got = ix.knn_graph_filtered(k, mask, first, count, stats=True)
    assert (got[0] == A[pos]).all()
    same(got[1:4], knn_by_oracle(oracle, el, A, pos[:rows], k), slice(0, rows))
    xi, xd, _ = ix.exact_topk_filtered(el[A[pos]], k + 1, mask)
    same(got[1:4], strip(xi, xd, A[pos], k))
    assert (got[3] == min(k, len(A) - 1)).all()
    return got[4]


def check_range(ix, oracle, el, mask, radii, cap, first, count, rows=8):
    A = np.nonzero(mask)[0]
    pos = np.arange(first, first + count)
    got = ix.range_graph_filtered(radii, mask, cap, first, count, stats=True)
    assert (got[0] == A[pos]).all()
    for g, w in zip(got[1:5], range_by_oracle(oracle, el, A, pos[:rows], np.broadcast_to(radii, (count,))[:rows], cap)):
        assert g[:rows].tobytes() == w.tobytes()
    lim = min(cap + 1, 1024)  # exact_range's own entry takes no more: at cap 1024 its listing must not be full, and then
    x = ix.exact_range(el[A[pos]], radii, lim, mask)  # it is the listing that cap + 1 gives
    assert lim == cap + 1 or (x[2] < lim).all()
    for g, w in zip(got[1:5], strip_range(*x, A[pos], cap)):
        assert g.tobytes() == w.tobytes()
    return got[5]


@functools.lru_cache(maxsize=1)
def _ordinary(int8, dim):
    """(rows, handle, mask, float64 scores of the window's rows against the allowed rows, the window's radii) -- once per shape"""
    import granne_amd
    from oracle import oracle
    rng = np.random.default_rng(9900 + dim + int(int8))
    el = _rows(oracle, rng, N, dim, int8)
    mask = rng.random(N) < 0.85
    mask[-1] = True
    A = np.nonzero(mask)[0]
    assert len(A) > 2 * 16384 and FIRST + COUNT < len(A)
    e64 = el[A].astype(np.float64)
    e64 /= np.linalg.norm(e64, axis=1)[:, None]
    ix = granne_amd.Granne(_et(el), el, [])
    es = A[FIRST:FIRST + COUNT]
    xi, xd, _ = ix.exact_topk_filtered(el[es], 301, mask)
    near = strip(xi, xd, es, 300)[1]  # the window's 300 nearest other allowed distances
    ts = np.array([0, 1, 10, 300])[np.arange(COUNT) % 4]  # the t-th itself, on the boundary; 0: one below the nearest
    radii = np.array([np.nextafter(near[i, 0], np.float32(0)) if t == 0 else near[i, t - 1] for i, t in enumerate(ts)], np.float32)
    return el, ix, mask, e64[FIRST:FIRST + COUNT] @ e64.T, radii


SHAPES = [(False, 28), (False, 100), (False, 200), (True, 32), (True, 100)]


@pytest.mark.parametrize("k", [1, 10, 1023])
@pytest.mark.parametrize("int8,dim", SHAPES)
def test_knn_ordinary_data(oracle, int8, dim, k):
    from granne_amd import _lib
    el, ix, mask, s, _ = _ordinary(int8, dim)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if int8 else 0, dim)
    assert eps > 0
    # the reference alone keeps the case inside the cap (test_gpu_knn_graph's condition, in position space): fewer than 2048
    # allowed rows at or above the (k+1)-th score - 4 eps - a last-stage bucket
    kth = -np.partition(-s, k, axis=1)[:, k]
    kth_prefix = -np.partition(-s[:, :16384], k, axis=1)[:, k]
    width = (1.0 - (kth_prefix - eps - 2.25 / 64)) / 64
    assert ((s >= (kth - 4 * eps - width)[:, None]).sum(axis=1) < 2048).all()
    st = check_knn(ix, oracle, el, mask, k, FIRST, COUNT)
    assert st[0] == 0 and st[1] == 0 and st[3] == (3 if int8 else 1 if dim <= 112 else 2)


@pytest.mark.parametrize("cap", [8, 1024])
@pytest.mark.parametrize("int8,dim", SHAPES)
def test_range_ordinary_data(oracle, int8, dim, cap):
    el, ix, mask, _, radii = _ordinary(int8, dim)
    st = check_range(ix, oracle, el, mask, radii, cap, FIRST, COUNT)
    assert st[0] == 0 and st[1] == 0 and st[3] == (3 if int8 else 1 if dim <= 112 else 2)


def test_the_diagonal_in_position_space(oracle):
    """the first 40 words are zero: position = id - 1280 everywhere. 16 elements with 9 allowed bit-copies at larger ids and
    one DISALLOWED copy at a smaller id: self and copies are exactly k allowed rows at distance 0"""
    import granne_amd
    rng = np.random.default_rng(9910)
    el = m.unit_rows(oracle, rng, 5000, 100)
    chosen = 1400 + 37 * np.arange(16)
    for i, e in enumerate(chosen):
        el[3000 + 9 * i + np.arange(9)] = el[e]
        el[100 + i] = el[e]
    mask = np.arange(5000) >= 1280
    A = np.nonzero(mask)[0]
    ix = granne_amd.Granne("angular", el, [])
    for i, e in enumerate(chosen):
        got = ix.knn_graph_filtered(10, mask, int(e) - 1280, 1)
        ids, ds = got[1], got[2]
        assert got[0][0] == e and (ids[0, :9] == 3000 + 9 * i + np.arange(9)).all() and 100 + i not in ids[0]
        assert (ds[0, :9] == ds[0, 0]).all() and ds[0, 9] > ds[0, 0]
        same(got[1:], knn_by_oracle(oracle, el, A, [int(e) - 1280], 10))
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
def test_edges(oracle, int8):
    import granne_amd
    from granne_amd import GranneHipError
    rng = np.random.default_rng(9920 + int(int8))
    n = 700  # a partial last tile
    el = _rows(oracle, rng, n, 100, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    one = np.arange(n) == 333  # m = 1
    e, ids, ds, cnt = ix.knn_graph_filtered(3, one)
    assert e.tolist() == [333] and cnt.tolist() == [0] and (ids == NONE).all() and np.isinf(ds).all()
    e, ids, ds, cnt, tot = ix.range_graph_filtered(2.0, one, 5)
    assert e.tolist() == [333] and cnt.tolist() == [0] and tot.tolist() == [0] and (ids == NONE).all()
    none = np.zeros(n, bool)  # m = 0
    assert ix.knn_graph_filtered(3, none)[1].shape == (0, 3) and ix.range_graph_filtered(0.5, none, 7)[1].shape == (0, 7)
    mask = rng.random(n) < 0.6
    mask[-1] = True
    mm = int(mask.sum())
    for call in (lambda: ix.knn_graph_filtered(3, mask, mm - 2, 3), lambda: ix.range_graph_filtered(0.5, mask, 5, mm - 2, 3)):
        with pytest.raises(GranneHipError, match=r"first \+ count \(%d \+ 3\) is beyond the %d allowed" % (mm - 2, mm)):
            call()
    check_knn(ix, oracle, el, mask, 10, mm - 1, 1, rows=1)  # the very last position
    check_range(ix, oracle, el, mask, np.float32(0.9), 8, mm - 1, 1, rows=1)
    every = np.ones(n, bool)  # all bits set: knn_graph and range_graph, byte for byte
    got = ix.knn_graph_filtered(10, every, 650, 50, stats=True)
    assert (got[0] == np.arange(650, 700)).all()
    same(got[1:4], ix.knn_graph(10, 650, 50))
    got = ix.range_graph_filtered(0.8, every, 16, 650, 50)
    for g, w in zip(got[1:], ix.range_graph(0.8, 16, 650, 50)):
        assert g.tobytes() == w.tobytes()
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
def test_routed_handles(oracle, int8):
    import granne_amd
    rng = np.random.default_rng(9940)
    el = _rows(oracle, rng, 3000, 300, int8)
    mask = rng.random(3000) < 0.7
    mask[-1] = True
    mm = int(mask.sum())
    ix = granne_amd.Granne(_et(el), el, [])
    st = check_knn(ix, oracle, el, mask, 10, mm - 100, 100)
    assert st[1] == 100 and st[0] == 0 and st[3] == 0
    st = check_range(ix, oracle, el, mask, np.float32(0.9 if int8 else 0.85), 8, mm - 9, 9)
    assert st[1] == 9 and st[0] == 0 and st[3] == 0
    ix.close()


def test_too_many_survivors_fall_back(oracle):
    """test_gpu_knn_graph's input under a filter: 5000 allowed near-copies of element 500 inside one bucket of the last stage
    (the bucket edges do not depend on the number of rows of a one-stage scan); a radius that covers them all"""
    import granne_amd
    rng = np.random.default_rng(9925)
    el = m.unit_rows(oracle, rng, 9000, 32)
    b = el[500].astype(np.float64)
    b /= np.linalg.norm(b)
    u = rng.normal(size=(5000, 32))
    u -= (u @ b)[:, None] * b
    u /= np.linalg.norm(u, axis=1)[:, None]
    s = rng.uniform(0.9897, 0.9899, 5000)[:, None]
    el[1000:6000] = (s * b + np.sqrt(1.0 - s * s) * u).astype(np.float32)
    mask = rng.random(9000) < 0.8
    mask[400:6000] = True
    A = np.nonzero(mask)[0]
    first = int(np.searchsorted(A, 498))
    ix = granne_amd.Granne("angular", el, [])
    st = check_knn(ix, oracle, el, mask, 10, first, 5, rows=5)
    assert st[0] == 1 and st[2] >= 5000 and st[3] == 1
    radii = np.array([0.0, 0.0, 0.0104, 0.0, 0.0], np.float32)  # element 500: its 5000 near-copies, past the lists: path B
    st = check_range(ix, oracle, el, mask, radii, 16, first, 5, rows=5)
    assert st[1] == 1 and st[0] == 0 and st[3] == 1
    assert ix.range_graph_filtered(radii, mask, 16, first, 5)[4][2] >= 5000
    ix.close()


def test_refusals(oracle):
    import granne_amd as ga
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(9950)
    el = m.unit_rows(oracle, rng, 300, 32)
    o = np.zeros(8192, np.uint64).ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, cap=5, op=o):
        for rc in (L.granne_hip_knn_graph_filtered(h, o, 0, 4, k, op, o, o, o, None),
                   L.granne_hip_knn_graph_filtered_device(h, o, 0, 4, k, op, o, o, o, None, None),
                   L.granne_hip_range_graph_filtered(h, o, 0, 4, o, cap, op, o, o, o, o, None),
                   L.granne_hip_range_graph_filtered_device(h, o, 0, 4, o, cap, op, o, o, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode() and "_graph_filtered" in L.granne_hip_last_error().decode()

    ix = ga.Granne("angular", el, [])
    for k, cap in ((0, 0), (1024, 1025)):
        refused(ix._h, "must be in [1, 102", k=k, cap=cap)
    refused(ix._h, "null buffer", op=None)
    refused(None, "index is null")
    ix.close()
    se = ga.SumEmbeddings(make_table(rng, 100, 32), make_lists(rng, 300, 100))
    cix = ga.Granne("embeddings", se, [np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))], compact=True)
    refused(cix._h, "needs dense rows")
    cix.close()
    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])
    refused(f16._h, "F16")
    f16.close()
