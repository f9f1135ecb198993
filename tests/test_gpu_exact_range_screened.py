"""exact_range_screened (granne_amd/csrc/exact_range_screened_host.h) against exact_range on the same
handle and, where a full scan of the oracle is at hand, against tests/range_model.exact_range: the WHOLE ids array, the
distance bytes, the counts and the totals. No tolerance anywhere: the screen decides which rows get the reference's
arithmetic, never the answer. Status words: [0] voided, [1] not answered by path A, [2] largest S + B, [3] the form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402
from tests import range_model as rm  # noqa: E402
from tests import value_edges as ve  # noqa: E402

VOIDED = 0x80000000


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def same(ix, q, radii, cap, filter=None, model=None):
    """the screened answer equals exact_range's (and the model's); returns the screened status words"""
    want = ix.exact_range(q, radii, cap, allowed=filter, stats=True)
    got = ix.exact_range_screened(q, radii, cap, filter=filter, stats=True)
    refs = [want[:4]] + ([(model.ids, model.dists, model.counts, model.totals)] if model is not None else [])
    for ids, ds, cnt, tot in refs:
        assert (got[3] == tot).all(), (np.nonzero(got[3] != tot)[0][:5], got[3][:8], tot[:8])
        assert (got[2] == cnt).all(), np.nonzero(got[2] != cnt)[0][:5]
        assert (got[0] == ids).all(), np.nonzero((got[0] != ids).any(axis=1))[0][:5]
        assert got[1].tobytes() == ds.tobytes()
    assert got[4][0] == want[4][0]
    return got[4]


def form_of(el):
    int8, dim = el.dtype == np.int8, el.shape[1]
    if int8:
        return 3 if dim <= 128 else 0
    return 1 if dim <= 112 else 2 if dim <= 208 else 0


def near_the_border(el, q, radii, eps):
    """per query, the rows whose float64 score lies within 2 eps of 1 - r: what can be in the band"""
    x, y = el.astype(np.float64), q.astype(np.float64)
    if el.dtype == np.int8:
        x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-300)
        y /= np.maximum(np.linalg.norm(y, axis=1, keepdims=True), 1e-300)
    with np.errstate(invalid="ignore"):
        return (np.abs(y @ x.T - (1.0 - radii.astype(np.float64))[:, None]) <= 2.0 * eps).sum(axis=1)


@pytest.mark.parametrize("shape", rm.SHAPES, ids=rm.shape_id)
def test_every_shape_equals_exact_range_and_the_model(ga, oracle, shape):
    from granne_amd import _lib
    el, q, scan = rm.shape_input(oracle, shape)
    form = form_of(el)
    eps = _lib.lib().granne_hip_exact_topk_screen_epsilon(1 if shape[0] else 0, shape[1])
    ix = ga.Granne(_et(el), el, [])
    for j, cap in enumerate(shape[4]):
        radii = rm.mixed_radii(scan, cap, start=j * 5)
        ans = rm.exact_range(scan, radii, cap)
        st = same(ix, q, radii, cap, model=ans)
        if form == 0:  # no screen for the shape: routed
            assert st[3] == 0 and st[1] == len(q)
            continue
        # the reference alone guarantees that no query takes path C: far fewer rows than the cap can be in the band
        assert near_the_border(el, q, radii, eps).max() < 256
        dense = int((ans.totals > rm.ET_CAP).sum())
        assert st[3] == form and st[0] == 0 and st[1] == dense, (st, dense)
        assert st[2] >= min(int(ans.totals.max()), rm.ET_CAP)
    ix.close()


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "i8"])
def test_the_band_on_both_sides_of_the_radius(ga, oracle, int8):
    """r is the distance of each query's 10th neighbour; 16 rows lie one ulp from that neighbour in one component each, up
    and down (int8: bit-copies of it): rows the screen cannot tell apart, decided by the reference's arithmetic"""
    rng = np.random.default_rng(9510)
    k, dim = 10, 100
    el, q = rm.rows_of(oracle, rng, 5000, dim, int8), rm.rows_of(oracle, rng, 5, dim, int8)
    _, oi, _ = oracle.Index(el, []).scan_topk(q, k)
    for a in range(len(q)):
        kth = el[int(oi[a, k - 1])]
        for j in range(16):
            r = kth.copy()
            if not int8:
                r[j] = np.nextafter(r[j], np.float32(2.0 if j % 2 else -2.0))
            el[100 * (a + 1) + j] = r
    scan = rm.full_scan(oracle, el, q)
    radii = np.ascontiguousarray(scan[1][:, k - 1])
    ix = ga.Granne(_et(el), el, [])
    for cap in (5, 64):
        st = same(ix, q, radii, cap, model=rm.exact_range(scan, radii, cap))
        assert st[1] == 0 and st[2] >= 17 and st[3] == form_of(el)
    ix.close()


def test_ties_in_id_order_and_a_band_past_the_cap(ga, oracle):
    from granne_amd import _lib
    rng = np.random.default_rng(21)
    el = m.tripled(m.unit_rows(oracle, rng, 1200, 32))
    q = m.unit_rows(oracle, rng, 9, 32)
    q[8] = 0  # a zero query: every score 0, every distance exactly 1.0 -- 3,600 rows in the band, path A in id order
    scan = rm.full_scan(oracle, el, q)
    radii = np.array([scan[1][a, 3 * (a + 1) * 40 - 1] for a in range(8)] + [1.0], np.float32)
    ix = ga.Granne("angular", el, [])
    for cap in (17, 1024):
        ans = rm.exact_range(scan, radii, cap)
        assert ans.totals[8] == 3600
        st = same(ix, q, radii, cap, model=ans)
        assert st[1] == 0 and st[2] == 3600
    ix.close()
    # 5,000 copies at the radius: the band's list runs over, path C, exact_range's overflow and its code
    el, q = m.duplicates_nearest(oracle, np.random.default_rng(24))
    scan = rm.full_scan(oracle, el, q)
    radii = np.array([scan[1][0, 4999]] + [scan[1][a, 29] for a in range(1, len(q))], np.float32)
    ans = rm.exact_range(scan, radii, 100)
    assert ans.voided[0] and ans.totals[0] == 5000
    ix = ga.Granne("angular", el, [])
    st = same(ix, q, radii, 100, model=ans)
    assert st[0] == 1 and st[1] == 1 and st[3] == (1 | VOIDED)
    with pytest.raises(ga.GranneHipError) as e:
        ix.exact_range_screened(q, radii, 100)
    assert e.value.code == _lib.ERR_OVERFLOW
    ix.close()


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "i8"])
def test_filters(ga, oracle, int8):
    from granne_amd.filters import Filter
    rng = np.random.default_rng(9530 + int8)
    n, nq, cap = 4037, 12, 17
    el, q = rm.rows_of(oracle, rng, n, 100, int8), rm.rows_of(oracle, rng, nq, 100, int8)
    scan = rm.full_scan(oracle, el, q)
    radii = rm.mixed_radii(scan, cap)
    last = rng.random(n) < 0.3
    last[n - 1] = True
    ix = ga.Granne(_et(el), el, [])
    for mask in (rng.random(n) < 0.5, np.zeros(n, bool), last):  # shared: the compacted list
        for r in (radii, np.float32(2.0)):
            st = same(ix, q, r, cap, filter=mask, model=rm.exact_range(scan, r, cap, mask))
            assert st[3] == form_of(el) and st[1] == 0
    per = rng.random((nq, n)) < 0.5  # one bitmap per query
    per[1] = False
    per[2, n - 1] = True
    filters = [Filter.from_mask(per[a]) for a in range(nq)]
    for r in (radii, np.float32(2.0)):
        same(ix, q, r, cap, filter=filters, model=rm.exact_range(scan, r, cap, per))
    ix.close()


def test_rows_off_the_sphere_are_routed_and_a_long_query_takes_path_c(ga, oracle):
    rng = np.random.default_rng(9540)
    q = m.unit_rows(oracle, rng, 6, 100)
    q[3] *= np.float32(1.5)  # beyond the norm the bound is proven for
    el = ve.off_sphere_f32(rng, 3000, 100)
    scan = rm.full_scan(oracle, el, q)
    radii = np.ascontiguousarray(scan[1][:, 40])
    ix = ga.Granne("angular", el, [])
    st = same(ix, q, radii, 64, model=rm.exact_range(scan, radii, 64))
    assert st[3] == 0 and st[1] == len(q)
    ix.close()
    el = m.unit_rows(oracle, rng, 3000, 100)
    scan = rm.full_scan(oracle, el, q)
    radii = np.ascontiguousarray(scan[1][:, 40])
    ix = ga.Granne("angular", el, [])
    st = same(ix, q, radii, 64, model=rm.exact_range(scan, radii, 64))
    assert st[3] == 1 and st[1] == 1 and st[0] == 0
    ix.close()
