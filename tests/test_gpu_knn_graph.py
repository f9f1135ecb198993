"""knn_graph (granne_amd/csrc/knn_graph_host.h) against the oracle's scan_topk(rows[e], k + 1) with e dropped
where it is listed and the last entry dropped where it is not: ids, distance BYTES and counts, no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
N, FIRST, COUNT = 40003, 16300, 300  # a partial last tile, several ranges, two stages; a partial query tile whose diagonal
#                                      lies in the blocks on both sides of the first prefix's end at 16384


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def _rows(oracle, rng, n, dim, int8):
    if int8:
        return np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
    return m.unit_rows(oracle, rng, n, dim)


def strip(ids, ds, es, k):
    """[len(es), >= min(k + 1, n)] nearest of the elements es, NONE padded -> (ids, dists, counts) of their k nearest others"""
    oi, od = np.full((len(es), k), NONE), np.full((len(es), k), np.inf, np.float32)
    oc = np.zeros(len(es), np.uint32)
    for r, e in enumerate(es):
        c = int((ids[r] != NONE).sum())
        keep = np.array([j for j in range(c) if ids[r, j] != e][:max(c - 1, 0)], np.intp)
        oi[r, :len(keep)], od[r, :len(keep)], oc[r] = ids[r, keep], ds[r, keep], len(keep)
    return oi, od, oc


def by_oracle(oracle, el, es, k):
    kk = min(k + 1, len(el))
    _, ids, ds = oracle.Index(el, []).scan_topk(el[es], kk)
    return strip(ids, ds, es, k)


def same(got, want, rows=slice(None)):
    for g, w in zip(got[:3], want):
        assert g[rows].tobytes() == w.tobytes()


def check(ix, oracle, el, k, first, count, by_exact_topk=True):
    """knn_graph == the oracle (the first 8 elements) == exact_topk(rows, k + 1) stripped (all of them); the status words"""
    got = ix.knn_graph(k, first, count, stats=True)
    es = np.arange(first, first + count)
    same(got, by_oracle(oracle, el, es[:8], k), slice(0, 8))
    if by_exact_topk:
        xi, xd, _ = ix.exact_topk(el[es], k + 1)
        same(got, strip(xi, xd, es, k))
    assert (got[2] == min(k, len(el) - 1)).all()
    return got[3]


@functools.lru_cache(maxsize=1)
def _ordinary(int8, dim):
    """(rows, handle, float64 scores of the window's rows against all rows) -- made once per shape, shared by its k's"""
    import granne_amd
    from oracle import oracle
    el = _rows(oracle, np.random.default_rng(9700 + dim + int(int8)), N, dim, int8)
    e64 = el.astype(np.float64)
    e64 /= np.linalg.norm(e64, axis=1)[:, None]
    return el, granne_amd.Granne(_et(el), el, []), e64[FIRST:FIRST + COUNT] @ e64.T


@pytest.mark.parametrize("k", [1, 10, 1023])
@pytest.mark.parametrize("int8,dim", [(False, 28), (False, 100), (False, 200), (True, 32), (True, 100)])
def test_ordinary_data(oracle, int8, dim, k):
    from granne_amd import _lib
    el, ix, s = _ordinary(int8, dim)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if int8 else 0, dim)
    assert eps > 0
    # the reference alone keeps the case inside the cap (test_gpu_exact_topk_screened's condition, the element counted among
    # its own rows: its (k+1)-th score): fewer than 2048 rows at or above that score - 4 eps - a last-stage bucket
    kth = -np.partition(-s, k, axis=1)[:, k]
    kth_prefix = -np.partition(-s[:, :16384], k, axis=1)[:, k]
    width = (1.0 - (kth_prefix - eps - 2.25 / 64)) / 64
    assert ((s >= (kth - 4 * eps - width)[:, None]).sum(axis=1) < 2048).all()
    st = check(ix, oracle, el, k, FIRST, COUNT)
    assert st[0] == 0 and st[1] == 0 and st[3] == (3 if int8 else 1 if dim <= 112 else 2)


def test_the_diagonal_is_no_witness(oracle):
    """16 elements with 9 bit-copies each at larger ids: self and copies are exactly k rows at distance 0 -- a floor that
    counted the element as its own witness could pass the true 10th by"""
    import granne_amd
    rng = np.random.default_rng(9710)
    el = m.unit_rows(oracle, rng, 5000, 100)
    chosen = 100 + 37 * np.arange(16)
    for i, e in enumerate(chosen):
        el[3000 + 9 * i + np.arange(9)] = el[e]
    ix = granne_amd.Granne("angular", el, [])
    for i, e in enumerate(chosen):
        ids, ds, cnt = ix.knn_graph(10, int(e), 1)
        assert (ids[0, :9] == 3000 + 9 * i + np.arange(9)).all() and (ds[0, :9] == ds[0, 0]).all() and ds[0, 9] > ds[0, 0]
        same((ids, ds, cnt), by_oracle(oracle, el, [e], 10))
    ix.close()


def test_more_copies_than_k_before_the_element(oracle):
    import granne_amd
    rng = np.random.default_rng(9720)
    el = m.unit_rows(oracle, rng, 4000, 32)
    copies = 200 + 2 * np.arange(1500)
    el[copies] = el[copies[0]]
    ix = granne_amd.Granne("angular", el, [])
    e = int(copies[-1])  # not in its own top k + 1
    ids, ds, cnt = ix.knn_graph(10, e, 1)
    assert (ids[0] == copies[:10]).all() and cnt[0] == 10
    same((ids, ds, cnt), by_oracle(oracle, el, [e], 10))
    ix.close()


def test_too_many_survivors_fall_back(oracle):
    """5000 rows whose scores with element 500 lie inside one bucket of the last stage (9000 rows are one stage, counted twice:
    the floor is -1.25 + 63 * 2.25 / 64 = 0.96484, then that + 45 * (1 - 0.96484) / 64 = 0.98956, the next edge 0.99011) at
    distances 2e-4 apart in all: past the cap for the screen, a few rows per second-level bin for exact_topk's own scan"""
    import granne_amd
    rng = np.random.default_rng(9725)
    el = m.unit_rows(oracle, rng, 9000, 32)
    b = el[500].astype(np.float64)
    b /= np.linalg.norm(b)
    u = rng.normal(size=(5000, 32))
    u -= (u @ b)[:, None] * b
    u /= np.linalg.norm(u, axis=1)[:, None]
    s = rng.uniform(0.9897, 0.9899, 5000)[:, None]
    el[1000:6000] = (s * b + np.sqrt(1.0 - s * s) * u).astype(np.float32)
    ix = granne_amd.Granne("angular", el, [])
    got = ix.knn_graph(10, 498, 5, stats=True)
    same(got, by_oracle(oracle, el, np.arange(498, 503), 10))
    assert got[3][0] == 1 and got[3][2] >= 5000 and got[3][3] == 1
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("n,k,first,count", [(700, 10, 0, 1), (700, 10, 699, 1), (700, 10, 0, 700), (1, 3, 0, 1), (5, 10, 0, 5)])
def test_window_edges(oracle, int8, n, k, first, count):
    import granne_amd
    el = _rows(oracle, np.random.default_rng(9730 + n), n, 100, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    check(ix, oracle, el, k, first, count)
    ids, ds, cnt = ix.knn_graph(k, first, count)
    c = min(k, n - 1)
    assert ids.shape == (count, k) and (cnt == c).all() and (ids[:, c:] == NONE).all() and np.isinf(ds[:, c:]).all()
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
def test_routed_handles(oracle, int8):
    import granne_amd
    el = _rows(oracle, np.random.default_rng(9740), 3000, 300, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    st = check(ix, oracle, el, 10, 2900, 100)
    assert st[1] == 100 and st[0] == 0 and st[3] == 0
    ix.close()


def test_refusals(oracle):
    import granne_amd as ga
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(9750)
    el = m.unit_rows(oracle, rng, 300, 32)
    o = np.zeros(8192, np.uint64).ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, first=0, count=4, op=o):
        for rc in (L.granne_hip_knn_graph(h, first, count, k, op, o, o, None),
                   L.granne_hip_knn_graph_device(h, first, count, k, op, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    ix = ga.Granne("angular", el, [])
    refused(ix._h, "k must be in [1, 1023]", k=0)
    refused(ix._h, "k must be in [1, 1023]", k=1024)
    refused(ix._h, "beyond the 300 elements", first=297)
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
