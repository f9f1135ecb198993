"""exact_topk_screened_filtered (granne_amd/csrc/exact_topk_screened.h, ETS_LIST and ETS_BITS) against exact_topk_filtered on
the same handle and filter -- ids, distance BYTES and counts of every query -- and, for the first 8 queries, against the
oracle's scan of the allowed subset. No tolerance anywhere. The rows, queries and handles of the ordinary cases are
tests/test_gpu_exact_topk_screened.py's."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_filtered_model as fm  # noqa: E402
from tests import exact_topk_model as m  # noqa: E402
from tests.test_gpu_exact_topk_screened import N, NQ, _et, _handle, _ordinary, _rows  # noqa: E402


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _filter(ga, mask):
    return ga.Filter.from_words(fm.words(mask, garbage_past_n=True), len(mask))


def same(ga, ix, oracle, el, q, k, masks):
    """masks: one mask (the shared form) or one per query. screened_filtered == exact_topk_filtered (all queries) == the
    oracle's scan of the subset (the first 8; oracle None: skipped); returns the screened status words and the counts"""
    shared = isinstance(masks, np.ndarray)
    made = {id(a): a for a in ([masks] if shared else masks)}  # (one Filter per distinct bitmap)
    made = {i: _filter(ga, a) for i, a in made.items()}
    allowed = made[id(masks)] if shared else [made[id(a)] for a in masks]
    ids, ds, cnt, st = ix.exact_topk_screened_filtered(q, k, allowed, stats=True)
    xi, xd, xc, _ = ix.exact_topk_filtered(q, k, allowed, stats=True)
    assert (cnt == xc).all()
    assert (ids == xi).all(), np.nonzero((ids != xi).any(axis=1))[0][:5]
    assert ds.tobytes() == xd.tobytes()
    if oracle is not None:
        for a in [slice(0, 8)] if shared else [slice(a, a + 1) for a in range(min(8, len(q)))]:
            oi, od, oc = fm.oracle_subset(oracle, el, masks if shared else masks[a.start], q[a], k)
            assert (ids[a] == oi).all() and ds[a].tobytes() == od.tobytes() and (cnt[a] == oc).all()
    return st, cnt


def inside_cap(s, mask, k, eps):
    """the reference alone keeps the query inside the cap: in float64, fewer than 4096 allowed rows at or above the k-th
    allowed score - 4 eps - a first-stage bucket"""
    sa = s[mask]
    kth = -np.partition(-sa, k - 1)[k - 1] if len(sa) >= k else -np.inf
    return (sa >= kth - 4 * eps - 2.25 / 64).sum() < 4096


@pytest.mark.parametrize("k", [10, 1024])
@pytest.mark.parametrize("int8,dim,form", [(False, 100, 1), (False, 200, 2), (True, 100, 3)])
def test_ordinary_data(ga, oracle, int8, dim, form, k):
    from granne_amd import _lib
    el, q, s = _ordinary(int8, dim)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if int8 else 0, dim)
    rng = np.random.default_rng(9700 + dim + k)
    differ = [fm.random_mask(rng, N, 0.5) for _ in range(NQ)]  # bitmaps that differ from query to query
    differ[1], differ[2] = np.zeros(N, bool), fm.only(N, [N // 7])
    cases = [(differ, oracle)]
    for mask in fm.shared_filters(rng, N, k).values():  # the shared form, and the same bitmap once per query
        cases += [(mask, oracle), ([mask] * NQ, None)]
    for masks, orc in cases:
        if orc is not None:
            assert all(inside_cap(s[a], masks if isinstance(masks, np.ndarray) else masks[a], k, eps) for a in range(NQ))
        st, _ = same(ga, _handle(int8, dim), orc, el, q, k, masks)
        assert st[0] == 0 and st[1] == 0 and st[3] == form


@pytest.mark.parametrize("per_query", [False, True])
def test_priming_trap(ga, oracle, per_query):
    rows, q, mask = fm.trap_input(oracle, np.random.default_rng(9710))
    ix = ga.Granne("angular", rows, [])
    st, cnt = same(ga, ix, oracle, rows, q[None], 17, [mask] if per_query else mask)
    assert cnt[0] == 17 and st[0] == 0 and st[3] == 1
    ix.close()


def test_fallback_under_a_filter(ga, oracle):
    """test_copies_come_in_id_order's data with 1400 copies per row, and a query whose scores to the three rows differ by
    1e-5 -- far below a bucket, far above a float's step: 4200 copies in reach, never 4096 of one distance"""
    rng = np.random.default_rng(9300)
    el = m.unit_rows(oracle, rng, 20000, 100)
    src = [17, 5000, 19999]
    for j, r in enumerate(src):
        el[6000 + j * 1400 + np.arange(1400)] = el[r]
    abc = el[src].astype(np.float64)
    near = np.linalg.solve(abc @ abc.T, [1.0, 1.0 - 1e-5, 1.0 - 2e-5]) @ abc
    q = np.concatenate([oracle.normalize_f32(near.astype(np.float32)[None]), el[src], m.unit_rows(oracle, rng, 5, 100)])
    ix = ga.Granne("angular", el, [])
    ones = np.ones(20000, bool)
    for masks in (ones, [ones] * len(q)):
        st, _ = same(ga, ix, oracle, el, q, 100, masks)
        assert st[0] >= 1 and st[2] >= 4200 and st[3] == 1
    fewer = ones.copy()
    fewer[6000:6600] = False  # 3600 copies allowed
    for masks in (fewer, [fewer] * len(q)):
        st, _ = same(ga, ix, oracle, el, q, 100, masks)
        assert st[0] == 0 and 3600 <= st[2] <= m.CAP
    ix.close()


@pytest.mark.parametrize("int8,dim", [(False, 300), (True, 300)])
def test_routed_shapes(ga, oracle, int8, dim):
    rng = np.random.default_rng(9720 + dim)
    el, q = _rows(oracle, rng, 5000, dim, int8), _rows(oracle, rng, 9, dim, int8)
    mask = fm.random_mask(rng, 5000, 0.5)
    ix = ga.Granne(_et(el), el, [])
    for masks in (mask, [mask] * 9):
        st, _ = same(ga, ix, oracle, el, q, 10, masks)
        assert st[1] == 9 and st[0] == 0 and st[3] == 0
    ix.close()


def test_refusals(ga, oracle):
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(9730)
    el, q = m.unit_rows(oracle, rng, 300, 32), m.unit_rows(oracle, rng, 4, 32)
    mask = fm.random_mask(rng, 300, 0.5)
    w = fm.words(mask)
    f = ga.Filter.from_words(w, 300)
    out = np.zeros(8192, np.uint64)
    p, o = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, host_filter=w.ctypes.data_as(C.c_void_p), dev_filter=C.c_void_p(f.ptr), stride=0):
        for rc in (L.granne_hip_exact_topk_screened_filtered(h, p, 4, k, host_filter, stride, o, o, o, None),
                   L.granne_hip_exact_topk_screened_filtered_device(h, p, 4, k, dev_filter, stride, o, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            msg = L.granne_hip_last_error().decode()
            assert "exact_topk_screened_filtered" in msg and word in msg, msg

    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])
    refused(f16._h, "F16")
    f16.close()
    se = ga.SumEmbeddings(make_table(rng, 100, 32), make_lists(rng, 300, 100))
    cix = ga.Granne("embeddings", se, [np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))], compact=True)
    refused(cix._h, "needs dense rows")
    cix.close()
    ix = ga.Granne("angular", el, [])
    refused(ix._h, "k must be in [1, 1024]", k=0)
    refused(ix._h, "k must be in [1, 1024]", k=1025)
    refused(ix._h, "the filter is null", host_filter=None, dev_filter=None)
    refused(ix._h, "filter_stride_words (9)", stride=9)  # ceil(300 / 32) = 10
    assert L.granne_hip_exact_topk_screened_filtered_device(ix._h, None, 0, 5, None, 0, None, None, None, None, None) == _lib.OK  # nq = 0
    same(ga, ix, oracle, el, q, 5, mask)  # the device still answers
    ix.close()
