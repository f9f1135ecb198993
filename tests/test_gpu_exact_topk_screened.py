"""exact_topk_screened (granne_amd/csrc/exact_topk_screened.h) against exact_topk on the same handle -- ids, distance BYTES
and counts of every query -- and, for the first 8 queries, against the oracle's scan. No tolerance anywhere: the screen may
only decide which rows get the reference's arithmetic, never the answer."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
N, NQ = 40003, 70  # a partial last tile and several ranges; a partial query tile; two stages (a prefix of 16384 rows first)


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def _rows(oracle, rng, n, dim, int8):
    if int8:
        return np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
    return m.unit_rows(oracle, rng, n, dim)


def same(ix, oracle, el, q, k):
    """screened == exact_topk (all queries) == the oracle's scan (the first 8); returns the screened status words"""
    ids, ds, cnt, st = ix.exact_topk_screened(q, k, stats=True)
    xi, xd, xc, _ = ix.exact_topk(q, k, stats=True)
    assert (cnt == xc).all()
    assert (ids == xi).all(), np.nonzero((ids != xi).any(axis=1))[0][:5]
    assert ds.tobytes() == xd.tobytes()
    if oracle is not None:
        _, oi, od = oracle.Index(el, []).scan_topk(q[:8], k)
        assert (ids[:8] == oi).all() and ds[:8].tobytes() == od.tobytes()
    return st


@functools.lru_cache(maxsize=None)
def _ordinary(int8, dim):
    """(rows, queries, float64 scores [nq, n]) -- made once per shape, shared by the k's"""
    from oracle import oracle
    rng = np.random.default_rng(9100 + dim + int(int8))
    el, q = _rows(oracle, rng, N, dim, int8), _rows(oracle, rng, NQ, dim, int8)
    q[:2] = el[[N - 1, N // 2]]  # rows of the set: distance 0, at the clamp
    e64, q64 = el.astype(np.float64), q.astype(np.float64)
    s = (q64 @ e64.T) / (np.linalg.norm(q64, axis=1)[:, None] * np.linalg.norm(e64, axis=1)[None, :])
    return el, q, s


@functools.lru_cache(maxsize=None)
def _handle(int8, dim):
    import granne_amd
    el = _ordinary(int8, dim)[0]
    return granne_amd.Granne(_et(el), el, [])


@pytest.mark.parametrize("k", [1, 10, 100, 1024])
@pytest.mark.parametrize("int8,dim", [(False, 28), (False, 100), (False, 200), (True, 32), (True, 100)])
def test_ordinary_data(ga, oracle, int8, dim, k):
    from granne_amd import _lib
    el, q, s = _ordinary(int8, dim)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if int8 else 0, dim)
    assert eps > 0
    # the reference alone keeps the case inside the cap: fewer than 2048 rows at or above the k-th score - 4 eps - a bucket.
    # The last stage's buckets are (1 - floor) / 64 wide, its floor at least the prefix's k-th score - eps - a first-stage bucket
    kth = -np.partition(-s, k - 1, axis=1)[:, k - 1]
    kth_prefix = -np.partition(-s[:, :16384], k - 1, axis=1)[:, k - 1]
    width = (1.0 - (kth_prefix - eps - 2.25 / 64)) / 64
    assert ((s >= (kth - 4 * eps - width)[:, None]).sum(axis=1) < 2048).all()
    st = same(_handle(int8, dim), oracle, el, q, k)
    assert st[0] == 0 and st[1] == 0 and k <= st[2] < 2048
    assert st[3] == (3 if int8 else 1 if dim <= 112 else 2)


@pytest.mark.parametrize("int8,dim", [(False, 300), (True, 300)])
def test_routed_shapes(ga, oracle, int8, dim):
    rng = np.random.default_rng(9200 + dim)
    el, q = _rows(oracle, rng, 5000, dim, int8), _rows(oracle, rng, 9, dim, int8)
    ix = ga.Granne(_et(el), el, [])
    st = same(ix, oracle, el, q, 10)
    assert st[1] == 9 and st[0] == 0 and st[3] == 0
    ix.close()


def test_rows_off_the_sphere_are_routed_and_long_queries_fall_back(ga, oracle):
    """the f32 bound is proven for squared norms up to 1 + 2^-10: a handle beyond it is routed, a query beyond it falls back"""
    from tests import value_edges as ve
    rng = np.random.default_rng(9250)
    el, q = ve.off_sphere_f32(rng, 3000, 100), ve.off_sphere_f32(rng, 12, 100)
    ix = ga.Granne("angular", el, [])
    assert same(ix, oracle, el, q, 16)[1] == 12
    ix.close()
    el = m.unit_rows(oracle, rng, 3000, 100)
    q[6:] = m.unit_rows(oracle, rng, 6, 100)
    ix = ga.Granne("angular", el, [])
    st = same(ix, oracle, el, q, 16)
    assert st[1] == 0 and 1 <= st[0] <= 6 and st[3] == 1
    ix.close()


def test_copies_come_in_id_order(ga, oracle):
    rng = np.random.default_rng(9300)
    el = m.unit_rows(oracle, rng, 20000, 100)
    src = [17, 5000, 19999]
    for j, r in enumerate(src):  # 1000 bit-copies of each of three rows
        el[1000 + j * 1000 + np.arange(1000)] = el[r]
    q = np.concatenate([el[src], m.unit_rows(oracle, rng, 6, 100)])
    ix = ga.Granne("angular", el, [])
    st = same(ix, oracle, el, q, 100)
    assert st[0] == 0 and 1000 <= st[2] <= m.CAP
    ids, ds, _ = ix.exact_topk_screened(q[:3], 100)
    assert (ds == ds[:, :1]).all() and (np.diff(ids.astype(np.int64), axis=1) > 0).all()
    ix.close()


def test_one_ulp_from_the_kth_neighbour(ga, oracle):
    rng = np.random.default_rng(9310)
    k, dim = 10, 100
    el, q = m.unit_rows(oracle, rng, 5000, dim), m.unit_rows(oracle, rng, 5, dim)
    _, oi, _ = oracle.Index(el, []).scan_topk(q, k)
    for a in range(len(q)):  # 16 rows one ulp from query a's k-th neighbour, up or down, in one component each
        kth = el[int(oi[a, k - 1])]
        for j in range(16):
            r = kth.copy()
            r[j] = np.nextafter(r[j], np.float32(2.0 if j % 2 else -2.0))
            el[100 * (a + 1) + j] = r
    ix = ga.Granne("angular", el, [])
    assert same(ix, oracle, el, q, k)[0] == 0
    ix.close()


def test_overflow_goes_to_exact_topk(ga, oracle):
    rng = np.random.default_rng(9400)
    el = np.repeat(m.unit_rows(oracle, rng, 1, 100), 6000, axis=0)
    q = m.unit_rows(oracle, rng, 5, 100)
    ix = ga.Granne("angular", el, [])
    st = same(ix, None, el, q, 10)  # (exact_topk voids these queries itself: 6000 rows inside one bin)
    assert st[0] == 5 and st[1] == 0 and st[2] == 6000 and st[3] & 0x80000000
    with pytest.raises(ga.GranneHipError):
        ix.exact_topk_screened(q, 10)
    ix.close()
    el = m.unit_rows(oracle, rng, 9000, 32)
    el[1000:6000] = el[0]  # 5000 copies: past the cap for the query that is one of them, k rows nearer than the others' bins
    q = np.concatenate([el[:1], m.unit_rows(oracle, rng, 3, 32)])
    ix = ga.Granne("angular", el, [])
    ids, ds, cnt, st = ix.exact_topk_screened(q[1:], 10, stats=True)
    _, oi, od = oracle.Index(el, []).scan_topk(q[1:], 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes()
    assert same(ix, None, el, q, 10)[0] >= 1
    ix.close()


def test_materialised_sum_embeddings_handle_is_screened(ga, oracle):
    """its rows are normalised f32 rows like any other: the norm test decides, and the screen runs"""
    from tests.test_gpu_sum_embeddings import make_lists, make_table, model_rows
    rng = np.random.default_rng(9450)
    tab, lists = make_table(rng, 100, 32), make_lists(rng, 3000, 100)
    el = model_rows(oracle, tab, lists)
    ix = ga.Granne("embeddings", ga.SumEmbeddings(tab, lists), [])
    st = same(ix, oracle, el, m.unit_rows(oracle, rng, 9, 32), 100)
    assert st[1] == 0 and st[3] == 1
    ix.close()


@pytest.mark.parametrize("int8,n,k", [(False, 50, 100), (False, 1, 100), (True, 50, 100), (True, 1, 3)])
def test_small_sets(ga, oracle, int8, n, k):
    rng = np.random.default_rng(9500 + n)
    el, q = _rows(oracle, rng, n, 100, int8), _rows(oracle, rng, 5, 100, int8)
    ix = ga.Granne(_et(el), el, [])
    st = same(ix, oracle, el, q, k)
    ids, ds, cnt = ix.exact_topk_screened(q, k)
    assert (cnt == n).all() and (ids[:, n:] == NONE).all() and np.isinf(ds[:, n:]).all() and st[0] == 0 and st[2] == n
    ix.close()


def test_refusals(ga, oracle):
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(9600)
    el, q = m.unit_rows(oracle, rng, 300, 32), m.unit_rows(oracle, rng, 4, 32)
    out = np.zeros(8192, np.uint64)
    p, o = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, qp=p, op=o):
        for rc in (L.granne_hip_exact_topk_screened(h, qp, 4, k, op, op, op, None),
                   L.granne_hip_exact_topk_screened_device(h, qp, 4, k, op, op, op, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    ix = ga.Granne("angular", el, [])
    refused(ix._h, "k must be in [1, 1024]", k=0)
    refused(ix._h, "k must be in [1, 1024]", k=1025)
    refused(ix._h, "null buffer", qp=None)
    refused(ix._h, "null buffer", op=None)
    refused(None, "index is null")
    assert L.granne_hip_exact_topk_screened_device(ix._h, None, 0, 5, None, None, None, None, None) == _lib.OK  # nq = 0
    ix.close()
    se = ga.SumEmbeddings(make_table(rng, 100, 32), make_lists(rng, 300, 100))
    cix = ga.Granne("embeddings", se, [np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))], compact=True)
    refused(cix._h, "needs dense rows")
    cix.close()
    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])  # exact_topk has no form for rows of halves: nothing to route to
    refused(f16._h, "F16")
    f16.close()
