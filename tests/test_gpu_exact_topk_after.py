"""exact_topk_after and exact_topk_screened_after against the oracle's scan, taken once for pages x k
entries and cut into pages: a page's cursor is the oracle's entry just before it. Ids, distance BYTES and counts; no
tolerance anywhere. Rows, queries and handles of the ordinary cases are tests/test_gpu_exact_topk_screened.py's."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_filtered_model as fm  # noqa: E402
from tests import exact_topk_model as m  # noqa: E402
from tests.test_gpu_exact_topk_screened import N, NQ, NONE, _handle, _ordinary  # noqa: E402

SHAPES = [(False, 28), (False, 100), (False, 200), (True, 100)]
BOTH = pytest.mark.parametrize("screened", [False, True])


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def page(oi, od, start, k, total):
    """entries start .. start + k - 1 of one query's oracle order of `total` entries, filled as exact_topk fills"""
    ids, ds = np.full(k, NONE, np.uint64), np.full(k, np.inf, np.float32)
    c = max(0, min(k, total - start))
    ids[:c], ds[:c] = oi[start:start + c], od[start:start + c]
    return ids, ds, c


def check(ix, screened, q, k, oi, od, starts, allowed=None, total=None):
    """one call: query a's page starts at entry starts[a] of its oracle order (0: no cursor); returns the status words"""
    ad = np.array([od[a, s - 1] if s else 0 for a, s in enumerate(starts)], np.float32)
    ai = np.array([oi[a, s - 1] if s else NONE for a, s in enumerate(starts)], np.uint64)
    fn = ix.exact_topk_screened_after if screened else ix.exact_topk_after
    ids, ds, cnt, st = fn(q, k, after=(ad, ai), allowed=allowed, stats=True)
    for a, s in enumerate(starts):
        ei, ed, c = page(oi[a], od[a], s, k, oi.shape[1] if total is None else total)
        assert cnt[a] == c and (ids[a] == ei).all() and ds[a].tobytes() == ed.tobytes(), (a, s, int(cnt[a]), c)
    return st


@functools.lru_cache(maxsize=None)
def _order(int8, dim):
    """the oracle's first 3 x 1024 entries of every ordinary query: made once per shape, shared by the k's and the entries"""
    from oracle import oracle
    el, q, _ = _ordinary(int8, dim)
    _, oi, od = oracle.Index(el, []).scan_topk(q, 3 * 1024)
    return oi, od


def inside_cap(s, oi, start, k, eps):
    """the reference alone keeps the query inside the cap: in float64, fewer than 2048 rows between the page's k-th score
    less 4 eps less a last-stage bucket and the cursor's score plus 2 eps. The last stage's buckets end at the cursor's
    score or 1 and start at a floor that is at least the prefix's k-th SURE score less eps less a first-stage bucket."""
    cur = s[oi[start - 1]] if start else np.inf
    sure = np.sort(s[:16384][s[:16384] < cur - 2 * eps])[::-1]
    floor = (sure[k - 1] if len(sure) >= k else -1.25) - eps - 2.25 / 64
    width = (min(1.0, cur) - floor) / 64
    return ((s >= s[oi[start + k - 1]] - 4 * eps - width) & (s <= cur + 2 * eps)).sum() < 2048


@BOTH
@pytest.mark.parametrize("k", [1, 10, 1024])
@pytest.mark.parametrize("int8,dim", SHAPES)
def test_three_pages_in_one_call(ga, int8, dim, k, screened):
    """query a asks for page a % 3: a third of the queries have no cursor"""
    from granne_amd import _lib
    (el, q, s), (oi, od) = _ordinary(int8, dim), _order(int8, dim)
    starts = [(a % 3) * k for a in range(NQ)]
    if screened:
        eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if int8 else 0, dim)
        assert all(inside_cap(s[a], oi[a].astype(np.int64), starts[a], k, eps) for a in range(NQ))
    st = check(_handle(int8, dim), screened, q, k, oi, od, starts)
    if screened:  # no query fell back or was routed; the form is the sibling's
        assert st[0] == 0 and st[1] == 0 and st[3] == (3 if int8 else 1 if dim <= 112 else 2)


@BOTH
@pytest.mark.parametrize("int8,dim", SHAPES)
def test_no_cursor_is_the_sibling(ga, int8, dim, screened):
    ix, q = _handle(int8, dim), _ordinary(int8, dim)[1]
    want = (ix.exact_topk_screened if screened else ix.exact_topk)(q, 10, stats=True)
    fn = ix.exact_topk_screened_after if screened else ix.exact_topk_after
    for after in (None, (np.full(NQ, 0.25, np.float32), np.full(NQ, NONE))):  # the null pointer; the sentinel id
        got = fn(q, 10, after=after, stats=True)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@BOTH
def test_cursor_inside_a_run_of_copies(ga, oracle, screened):
    """test_copies_come_in_id_order's data: 1001 rows at query a's nearest distance. Pages that start inside the run go
    on with its next ids, cross its end into the next distance, and two that meet inside it neither repeat nor skip"""
    rng = np.random.default_rng(9300)
    el = m.unit_rows(oracle, rng, 20000, 100)
    src = [17, 5000, 19999]
    for j, r in enumerate(src):
        el[1000 + j * 1000 + np.arange(1000)] = el[r]
    q = np.ascontiguousarray(el[src])
    _, oi, od = oracle.Index(el, []).scan_topk(q, 1200)
    assert (od[:, :1001] == od[:, :1]).all() and (od[:, 1001] > od[:, 0]).all()
    ix = ga.Granne("angular", el, [])
    for starts in ([500, 600, 950], [600, 700, 1050]):
        st = check(ix, screened, q, 100, oi, od, starts)
        assert st[0] == 0
    ix.close()


@BOTH
@pytest.mark.parametrize("int8", [False, True])
def test_fewer_than_k_rows_after_the_cursor(ga, oracle, int8, screened):
    from tests.test_gpu_exact_topk_screened import _et, _rows
    rng = np.random.default_rng(9820 + int8)
    el, q = _rows(oracle, rng, 600, 100, int8), _rows(oracle, rng, 3, 100, int8)
    _, oi, od = oracle.Index(el, []).scan_topk(q, 600)
    ix = ga.Granne(_et(el), el, [])
    check(ix, screened, q, 1024, oi, od, [501, 600, 0])  # counts 99, 0 (the cursor is the last key) and 600
    ix.close()


@BOTH
@pytest.mark.parametrize("k", [10, 1024])
def test_filtered_pages(ga, oracle, k, screened):
    """one shared bitmap, and one bitmap per query, at selectivity 0.5, against the oracle's scan of the allowed subset"""
    el, q, _ = _ordinary(False, 100)
    rng = np.random.default_rng(9830 + k)
    masks = [fm.random_mask(rng, N, 0.5) for _ in range(6)]
    starts = [(a % 3) * k for a in range(6)]
    oi, od, _ = fm.oracle_subset(oracle, el, masks[0], q[:6], 3 * k)
    check(_handle(False, 100), screened, q[:6], k, oi, od, starts, allowed=masks[0])
    per = [fm.oracle_subset(oracle, el, masks[a], q[a:a + 1], 3 * k) for a in range(6)]
    oi, od = np.concatenate([p[0] for p in per]), np.concatenate([p[1] for p in per])
    filters = [ga.Filter.from_mask(a, 0) for a in masks]
    check(_handle(False, 100), screened, q[:6], k, oi, od, starts, allowed=filters)


def test_a_band_beyond_the_cap_falls_back(ga, oracle):
    """5001 rows at the cursor's distance: the band alone is beyond ETS_CAP, and exact_topk's scan answers with the cursor"""
    rng = np.random.default_rng(9400)
    el = m.unit_rows(oracle, rng, 9000, 32)
    el[1000:6000] = el[0]
    q = np.ascontiguousarray(el[:1])
    _, oi, od = oracle.Index(el, []).scan_topk(q, 3100)
    assert (od[0, :5001] == od[0, 0]).all()
    ix = ga.Granne("angular", el, [])
    st = check(ix, True, q, 10, oi, od, [3000])
    assert st[0] == 1 and st[1] == 0 and st[3] == 1
    check(ix, False, q, 10, oi, od, [3000])
    ix.close()


@BOTH
def test_the_nearest_5000_by_five_pages(ga, oracle, screened):
    """the capability itself: each page's last entry is the next page's cursor"""
    el, q, _ = _ordinary(False, 100)
    q = q[5:6]
    _, oi, od = oracle.Index(el, []).scan_topk(q, 5000)
    ix, after, got = _handle(False, 100), None, []
    fn = ix.exact_topk_screened_after if screened else ix.exact_topk_after
    for _ in range(5):
        ids, ds, cnt = fn(q, 1000, after=after)
        assert cnt[0] == 1000
        got.append((ids, ds))
        after = (ds[:, -1], ids[:, -1])
    assert (np.concatenate([g[0] for g in got], axis=1) == oi).all()
    assert np.concatenate([g[1] for g in got], axis=1).tobytes() == od.tobytes()
