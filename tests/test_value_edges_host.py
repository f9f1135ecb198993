"""The generators of tests/value_edges.py and the reference side of tests/test_gpu_value_edges.py, on the CPU: the C
oracle equals its Python restatement bit for bit on what they make, the generators hold the values they promise, the row
sketch's bound holds off the unit sphere, and the exact-scan inputs have few enough near-tied ranks that the GPU scan
never has to be excused a miss."""
import numpy as np
import pytest

from oracle import pyref
from tests import value_edges as ve
from tests.test_sketch_bound import META, _check_pairs, _f, lower_bound, query_sketch, row_sketch


def _bits(x):
    return np.asarray(x, np.float32).tobytes()


# ---- oracle against pyref on generator output -----------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 31, 100, 200, 333])
def test_oracle_equals_pyref_on_off_sphere_f32(oracle, dim):
    rng = np.random.default_rng(100 + dim)
    rows, q = ve.off_sphere_f32(rng, 48, dim), ve.off_sphere_f32(rng, 12, dim)
    assert np.isfinite(rows).all() and np.isfinite(q).all()
    pairs = [(i, i % 12) for i in range(48)] + [(16, 4), (47, 11), (16, 11)]  # (the zero rows, with each other too)
    with np.errstate(all="ignore"):
        for i, j in pairs:
            assert _bits(oracle.dist(rows[i], q[j])) == _bits(pyref.dist_f32(rows[i], q[j])), (i, j)
        raw = ve.scaled_raw(rng, dim)
        got = oracle.normalize_f32(raw)
        for r in range(len(raw)):
            assert got[r].tobytes() == pyref.normalize_f32(raw[r]).tobytes(), r
    assert np.isfinite(got).all()
    if dim >= 31:  # squares that underflow keep the row, squares that overflow leave +-0
        assert got[0].tobytes() == raw[0].tobytes() and (got[-1] == 0).all() and np.signbit(got[-1]).any()


@pytest.mark.parametrize("dim", [17, 100, 128, 300, 1500, 3000])
def test_oracle_equals_pyref_on_odd_i8(oracle, dim):
    rng = np.random.default_rng(200 + dim)
    rows, q = ve.odd_i8(rng, 60, dim), ve.odd_i8(rng, 12, dim)
    pairs = [(i, j) for i in range(60) for j in (i % 12, 9, 10, 11)]  # (9, 10, 11: zero, all -128, all 127)
    with np.errstate(all="ignore"):
        for i, j in pairs:
            assert _bits(oracle.dist(rows[i], q[j])) == _bits(pyref.dist_i8(rows[i], q[j])), (i, j)
        raw = ve.scaled_raw(rng, min(dim, 333), top=30)
        got = oracle.quantize(raw)
        for r in range(len(raw)):
            assert got[r].tobytes() == pyref.quantize(raw[r]).tobytes(), r
    if dim >= 1500:  # the saturated rows' sums of squares are beyond 2^24, where the conversion to f32 rounds
        assert int((rows[-2].astype(np.int64) ** 2).sum()) > 1 << 24


# ---- what the generators hold -----------------------------------------------------------------------------
def test_generators_hold_no_nan_and_no_infinity():
    rng = np.random.default_rng(1)
    for a in (ve.off_sphere_f32(rng, 500, 100), ve.scaled_raw(rng, 100), ve.scaled_raw(rng, 100, top=30),
              ve.scan_input("short_f32_100")[0]):
        assert a.dtype == np.float32 and np.isfinite(a).all()
        with np.errstate(over="raise"):
            assert np.isfinite(a * np.float32(127)).all()


def test_odd_i8_holds_the_extremes_and_norms_40x_apart():
    rows = ve.odd_i8(np.random.default_rng(2), 3000, 100)
    assert rows.dtype == np.int8 and (rows == -128).any() and (rows == 127).any()
    assert (rows[6::7] == -128).sum() > 100 and not ((rows[:-3] > -128) & (rows[:-3] <= -100))[6::7].any()
    norms = np.sqrt((rows.astype(np.int64) ** 2).sum(axis=1))
    assert norms.min() == 0 and norms.max() == 1280
    assert norms.max() / norms[norms > 0].min() >= 40
    # the scan's block bound: the rows 32 b + 8 g + 4 h + 0..3 are lane half h's. In at least a quarter of the blocks
    # the two halves' largest 1 / |x| differ by more than 2 x: the other half's bound is then not a bound
    inv = np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 0.0)[:2976].reshape(-1, 4, 2, 4)
    gm = inv.max(axis=(1, 3))
    ratio = gm.max(axis=1) / gm.min(axis=1)
    assert (ratio > 2).mean() > 0.25


def test_off_sphere_walks_return_a_third_of_their_distances_clamped(oracle):
    rng = np.random.default_rng(4)
    el, q = ve.off_sphere_f32(rng, 2000, 100), ve.off_sphere_f32(rng, 64, 100)
    norms = np.linalg.norm(el.astype(np.float64), axis=1)
    assert (norms == 0).sum() == 2 and 0.02 < (norms < 1e-22).mean() < 0.05 and norms.max() < 25 and norms.max() > 10
    oix = oracle.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
    _, ds, cnt, _ = oix.search_batch(q, 50, 10)
    assert (cnt == 10).all()
    assert (ds == 0.0).mean() >= 1 / 3
    # rows at scale 1e-25 are at distance exactly 1.0 from everything
    tiny = np.nonzero((norms > 0) & (norms < 1e-22))[0][:5]
    assert all(oracle.dist(el[t], q[j]) == 1.0 for t in tiny for j in range(8))


def test_one_sided_sets_rank_the_zero_row_first(oracle):
    for name in ("one_sided_i8_100", "one_sided_i8_128"):
        el, q, _ = ve.scan_input(name)
        assert (el >= 0).all() and (q <= 0).all() and not el[len(el) // 2].any()
        assert (el.astype(np.int32) @ q.T.astype(np.int32) <= 0).all()
        _, ids, ds = oracle.Index(el, []).scan_topk(q, 2)
        assert (ids[:, 0] == len(el) // 2).all() and (ds[:, 0] == 1.0).all() and (ds[:, 1] > 1.0).all()


# ---- the row sketch's bound off the sphere ----------------------------------------------------------------
def test_sketch_bound_holds_and_stays_usable_off_the_sphere(oracle):
    rng = np.random.default_rng(5)
    xs, qs = ve.off_sphere_f32(rng, 3000, 100), ve.off_sphere_f32(rng, 40, 100)
    worst, n_checked = _check_pairs(qs, xs)
    assert worst < 0 and n_checked > 0
    sk = row_sketch(xs)
    x64 = xs.astype(np.float64)
    nx = np.linalg.norm(x64, axis=1)
    for q in qs:
        lb, usable = lower_bound(query_sketch(q), sk)
        assert usable.all()  # nothing here is near N_q N_x = 2^100
        # usable: the bound stands within 4 % of |q| |x| (+ 2^-19) below the exact distance -- the margins scale with the norms
        slack = (1.0 - x64 @ q.astype(np.float64)) - lb.astype(np.float64)
        assert (slack <= 0.04 * np.linalg.norm(q.astype(np.float64)) * nx + 2.0 ** -19).all()


def _lower_bound_without_nq(qs, sk):
    """tests/test_sketch_bound.py lower_bound with the margin N_q R_x cut to R_x: what the unit sphere cannot tell apart."""
    codes, sq, rq, nq, _ = qs
    ip = sk[:, :META].view(np.int8).astype(np.int64) @ codes[:META].astype(np.int64)
    meta = np.ascontiguousarray(sk[:, META:]).view(np.float32)
    sx, rx, xx, nx = meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]
    t = ((sq * sx).astype(np.float32) * ip.astype(np.float32)).astype(np.float32)
    b = ((rq * xx).astype(np.float32) + rx).astype(np.float32)
    b = (b + ((nq * nx).astype(np.float32) * _f(2.0 ** -17)).astype(np.float32)).astype(np.float32)
    m = ((np.abs(t) * _f(2.0 ** -20)).astype(np.float32) + (b * _f(1.0001)).astype(np.float32)).astype(np.float32)
    return (_f(1) - (t + (m + _f(2.0 ** -20)).astype(np.float32)).astype(np.float32)).astype(np.float32)


def test_sketch_bound_on_rows_whose_error_is_the_whole_margin(oracle):
    """sketch_adversarial_f32: the bound holds, by little; without the factor N_q in N_q R_x it would reject members of
    the true ten nearest of the queries longer than 1 -- the walks of tests/test_gpu_value_edges.py would lose them."""
    rng = np.random.default_rng(6)
    xs, qs = ve.sketch_adversarial_f32(rng, 1500, 16)
    assert np.isfinite(xs).all() and np.linalg.norm(xs.astype(np.float64), axis=1).min() >= 1.0
    worst, n_checked = _check_pairs(qs, xs, exact_all=True)
    assert n_checked == 16 * 1500 and -0.01 < worst < 0
    sk = row_sketch(xs)
    lost = 0
    for j, q in enumerate(qs):
        sketch = query_sketch(q)
        assert sketch[2] < 1e-15  # R_q: no residual
        d = np.array([oracle.dist(x, q) for x in xs], np.float32)
        top = np.lexsort((np.arange(len(xs)), d))[:10]
        wrong = _lower_bound_without_nq(sketch, sk)[top] > d[top[-1]]
        lost += int(wrong.sum())
        if sketch[3] < 1:  # N_q < 1: the cut margin is the larger one
            assert not wrong.any()
    assert lost >= 5


# ---- the exact scan's inputs: few near-tied ranks, by the oracle alone ------------------------------------
@pytest.mark.parametrize("name", sorted(ve.SCAN_INPUTS))
def test_scan_inputs_have_few_near_tied_ranks(oracle, name):
    """The scan in tolerance mode may name another id where two distances lie within its tolerance of each other. The GPU
    tests ask for more than 98 % equal ids: at most 2 % of the positions may be near-tied."""
    el, q, tol = ve.scan_input(name)
    _, ids, ds = oracle.Index(el, []).scan_topk(q, max(ve.SCAN_KS) + 1)
    for k in ve.SCAN_KS:
        share = ve.near_tie_share(ds, k, tol)
        print("%s k=%d: near-tied share %.4f" % (name, k, share))
        assert share <= 0.02, (name, k, share)
    if "f32" in name:  # no dot reaches 1: the clamp is never taken, the score's order is the distance's
        assert (ds > 0).all()
    if name.endswith("primed"):  # the planted low-amplitude rows are their queries' nearest
        n = len(el)
        assert [int(ids[j, 0]) for j in range(ve.PLANTED)] == [ve.planted_at(j, n) for j in range(ve.PLANTED)]
        norms = np.sqrt((el.astype(np.int64) ** 2).sum(axis=1))
        for j in range(ve.PLANTED):
            p = ve.planted_at(j, n)
            block = norms[p // 32 * 32:p // 32 * 32 + 32]
            assert norms[p] > 0 and np.median(block) >= 40 * norms[p]
