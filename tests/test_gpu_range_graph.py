"""range_graph (granne_amd/csrc/range_graph_host.h) against its model over the CPU oracle: for element e the
oracle's full scan with row e as the query (tests/range_model.py), id e struck out, cut at the radius. Every case compares
the WHOLE ids array, the distance bytes, the counts and the totals; no tolerance. tests/README_range_graph.md says what
each case pins."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402
from tests import range_model as rm  # noqa: E402

FIRST, COUNT = 37, 70  # starts and ends inside 32-row blocks and spans three of them


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def same(ix, oracle, el, first, count, radius, caps):
    """range_graph(radius, cap, first, count) for every cap == the model. radius: a scalar, one value per element, or a
    function of (the struck scan's distances [count, n - 1], the oracle's d(e, e) [count]). Returns (radii, the model of the
    last cap, its status words)."""
    es = np.arange(first, first + (len(el) - first if count is None else count))
    ids, ds = rm.full_scan(oracle, el, np.ascontiguousarray(el[es]))
    keep = ids != es[:, None].astype(np.uint64)  # row e is listed once in its own scan
    self_d = ds[~keep]
    struck = ids[keep].reshape(len(es), -1), ds[keep].reshape(len(es), -1)
    radii = radius(struck[1], self_d) if callable(radius) else radius
    for cap in caps:
        ans = rm.exact_range(struck, radii, cap)
        assert not ans.voided.any()
        g_ids, g_ds, g_cnt, g_tot, st = ix.range_graph(radii, cap, first, count, stats=True)
        assert (g_tot == ans.totals).all(), (cap, np.nonzero(g_tot != ans.totals)[0][:5], g_tot[:8], ans.totals[:8])
        assert (g_cnt == ans.counts).all(), (cap, np.nonzero(g_cnt != ans.counts)[0][:5])
        assert (g_ids == ans.ids).all(), (cap, np.nonzero((g_ids != ans.ids).any(axis=1))[0][:5])
        assert g_ds.tobytes() == ans.dists.tobytes(), cap
    return radii, ans, st


@pytest.mark.parametrize("int8,dim", [(False, 28), (False, 100), (False, 200), (True, 32), (True, 100)])
def test_ordinary_data(oracle, int8, dim):
    """element i: the radius is its t-th OTHER distance itself, t = (1, 10, 300)[i % 4 - 1], the border row exactly on the
    boundary; i % 4 == 0: a radius below the nearest"""
    import granne_amd
    el = rm.rows_of(oracle, np.random.default_rng(9800 + dim + int(int8)), 5000, dim, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    ts = np.array([0, 1, 10, 300])[np.arange(COUNT) % 4]

    def radius(ds, self_d):
        return np.array([rm.radius_for_total(ds[i], 0) if t == 0 else ds[i, t - 1] for i, t in enumerate(ts)], np.float32)

    _, ans, st = same(ix, oracle, el, FIRST, COUNT, radius, (1024, 8))
    assert st[0] == 0 and st[1] == 0 and st[3] == (3 if int8 else 1 if dim <= 112 else 2)
    assert (ans.totals[ts == 0] == 0).all() and (ans.counts[ts == 0] == 0).all() and (ans.totals[ts > 0] >= ts[ts > 0]).all()
    ix.close()


@pytest.mark.parametrize("own", [False, True])
def test_self_and_copies(oracle, own):
    """40 bit-copies of each of three rows, below and above the row's own id; r = 0.0, and r = d(e, e) as the oracle computes
    it. For these rows (unit_rows, 100-d f32) the oracle's d(e, e) is 0.0 for some elements and a few ulps of 1 above 0 for
    others (1 - dot with dot rounded below 1), never negative (distances are clamped at 0): r = 0.0 lists the copies of the
    former only, r = d(e, e) the copies of all. e is never listed; the copies come in id order."""
    import granne_amd
    rng = np.random.default_rng(9810)
    el = m.unit_rows(oracle, rng, 3000, 100)
    es = np.array([40, 55, 70])
    spots = (110 + rng.permutation(2890)[:120]).reshape(3, 40)  # scattered above the window
    spots[:, :3] = [[38, 41, 90], [3, 54, 99], [69, 71, 72]]  # inside the window on both sides of the element, one below it
    for e, at in zip(es, spots):
        el[at] = el[e]
    ix = granne_amd.Granne("angular", el, [])
    radii, ans, st = same(ix, oracle, el, FIRST, COUNT, (lambda ds, self_d: self_d) if own else 0.0, (1024, 8))
    for e, at in zip(es, spots):
        row = ans.ids[e - FIRST]
        assert e not in row and (not own or (row[:8] == np.sort(at)[:8]).all())
    assert not own or (ans.totals[es - FIRST] >= 40).all()
    assert st[1] == 0 and st[0] == 0
    ix.close()


def test_more_neighbours_than_the_lists_hold(oracle):
    """path B: 5,000 of 6,000 rows in one tight cluster, a radius that covers it: total 4,999 from the pass, the 1,024 nearest
    by the screened selection with cap + 1 = 1,025"""
    import granne_amd
    rng = np.random.default_rng(9820)
    el = m.unit_rows(oracle, rng, 6000, 100)
    centre = m.unit_rows(oracle, rng, 1, 100)[0]
    el[500:5500] = oracle.normalize_f32((centre + rng.normal(0.0, 0.005, (5000, 100))).astype(np.float32))
    ix = granne_amd.Granne("angular", el, [])
    _, ans, st = same(ix, oracle, el, 490, 20, 0.05, (1024,))
    assert (ans.totals[10:] == 4999).all() and (ans.totals[:10] == 0).all()
    assert st[1] == 10 and st[0] == 0 and st[3] == 1
    _, ans, st = same(ix, oracle, el, 499, 2, np.inf, (8,))  # every other row, and not the element: -inf >= -inf admits nothing
    assert (ans.totals == 5999).all() and st[1] == 2
    ix.close()


@pytest.mark.parametrize("cap", [16, 1024])
def test_a_band_beyond_the_lists(oracle, cap):
    """path C: 5,000 bit-copies of one row, each element's radius the oracle's distance to that row: all of them on the
    boundary, inside the band of every element"""
    import granne_amd
    from granne_amd import _lib
    rng = np.random.default_rng(9830)
    el = m.unit_rows(oracle, rng, 10000, 100)
    el[5000:] = el[4321]
    es = np.arange(70, 73)
    r = np.array([oracle.dist(el[4321], el[e]) for e in es], np.float32)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(0, 100)
    for e, re in zip(es, r):  # the oracle alone puts more rows than the list holds inside the band
        d = m.all_dists(oracle, el, el[e])
        assert ((d >= re - 2 * eps) & (d <= re + 2 * eps)).sum() > rm.ET_CAP and (d < re - 2 * eps).sum() > cap + 1
    ix = granne_amd.Granne("angular", el, [])
    radii, ans, st = same(ix, oracle, el, 70, 3, r, (cap,))
    assert (ans.totals > 5000).all() and st[1] == 3 and st[0] == 0 and st[3] == 1
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
def test_routed_handles(oracle, int8):
    import granne_amd
    el = rm.rows_of(oracle, np.random.default_rng(9840), 3000, 300, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    _, ans, st = same(ix, oracle, el, 2990, 9, lambda ds, self_d: ds[np.arange(9), [0, 1, 10, 300, 2000, 2998, 5, 5, 5]], (1024, 8))
    assert st[3] == 0 and st[1] == 9 and st[0] == 0 and ans.totals.max() == 2999
    ix.close()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("n", [1, 50])
def test_small_sets_and_edges(oracle, int8, n):
    import granne_amd
    el = rm.rows_of(oracle, np.random.default_rng(9850 + n), n, 100, int8)
    ix = granne_amd.Granne(_et(el), el, [])
    for r in (2.0, np.inf):
        _, ans, _ = same(ix, oracle, el, 0, None, r, (1024, 3))
        assert (ans.totals == n - 1).all()
    if n > 1:
        same(ix, oracle, el, 0, None, lambda ds, self_d: ds[:, 7], (5,))
    ids, ds, cnt, tot = ix.range_graph(0.5, 7, n - 1, 0)
    assert ids.shape == (0, 7) and ds.shape == (0, 7) and cnt.shape == (0,) and tot.shape == (0,)
    ix.close()


def test_refusals(oracle):
    import granne_amd as ga
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(9860)
    el = m.unit_rows(oracle, rng, 300, 32)
    o = np.zeros(8192, np.uint64).ctypes.data_as(C.c_void_p)

    def refused(h, word, cap=5, first=0, count=4, op=o):
        for rc in (L.granne_hip_range_graph(h, first, count, o, cap, op, o, o, o, None),
                   L.granne_hip_range_graph_device(h, first, count, o, cap, op, o, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    ix = ga.Granne("angular", el, [])
    refused(ix._h, "must be in [1, 1024]", cap=0)
    refused(ix._h, "must be in [1, 1024]", cap=1025)
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
