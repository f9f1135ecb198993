"""Every distance path of the HIP library on the values of tests/value_edges.py: f32 rows off the unit sphere (norms
10^-1.3 .. 10^1.3, rows whose products underflow, zero rows: nearly half of the distances a walk returns are the clamp's
0.0 and ordered by id alone), int8 rows that hold -128 and 127, saturated rows, norms 0 .. 1280 inside one 32-row block,
sets whose every dot is <= 0, raw rows over every decade of the float range. The C ABI takes rows as they are; the
reference computes max(0, 1 - x.q) whatever the norms, and the oracle is held to its Python restatement on these values
in tests/test_value_edges_host.py. Here the device is held to the oracle: ids, distance bits, counts, padding, counters.

Graphs come from oracle.build_index at n = 1500 .. 3000; every reference is computed once per module."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_model as model  # noqa: E402
from tests import value_edges as ve  # noqa: E402
from tests.conftest import assert_counters  # noqa: E402
from tests.rw_model import RwModel  # noqa: E402
from tests.test_gpu_parity import assert_same  # noqa: E402

MAX_SEARCH = (1, 10, 50, 200, 1500)
K = 10


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


# ---- operators ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 32, 100, 333])
def test_normalize_and_quantize_over_every_decade(ga, oracle, dim):
    """Squares that underflow (norm 0: the row is kept), sub-normal components, squares that overflow (norm +inf: +-0)."""
    rng = np.random.default_rng(300 + dim)
    raw = ve.scaled_raw(rng, dim)
    assert ga.normalize(raw).tobytes() == oracle.normalize_f32(raw).tobytes()
    raw = ve.scaled_raw(rng, dim, top=30)
    assert ga.quantize(raw).tobytes() == oracle.quantize(raw).tobytes()


def _check_dists(ga, oracle, el, q, seed):
    rng = np.random.default_rng(seed)
    n, nq, m = len(el), len(q), 37
    ix = ga.Granne(_et(el), el, [])
    ids = rng.integers(0, n, (nq, m)).astype(np.uint32)
    ids[:, 0], ids[:, 1], ids[:, 2], ids[:, 3] = n - 1, n - 2, n - 3, n // 3  # the generators' fixed rows
    ids[3, 5] = n  # out of range: +inf
    want = np.array([[oracle.dist(el[e], q[a]) if e < n else np.inf for e in ids[a]] for a in range(nq)], np.float32)
    assert ix.dists_many(q, ids).tobytes() == want.tobytes()
    qi, ei = rng.integers(0, nq, 1500), rng.integers(0, n, 1500)
    want = np.array([oracle.dist(el[e], q[a]) for a, e in zip(qi, ei)], np.float32)
    assert ix.dists(q, qi, ei).tobytes() == want.tobytes()
    ix.close()
    return want


@pytest.mark.parametrize("dim", [1, 31, 32, 33, 100, 128, 200, 1500])
def test_dists_off_the_sphere(ga, oracle, dim):
    rng = np.random.default_rng(400 + dim)
    want = _check_dists(ga, oracle, ve.off_sphere_f32(rng, 777, dim), ve.off_sphere_f32(rng, 13, dim), dim)
    assert (want == 0.0).any() and (want == 1.0).any() and (want > 1.0).any()


@pytest.mark.parametrize("dim", [1, 31, 32, 33, 100, 128, 200, 1500, 3000])
def test_dists_at_the_int8_extremes(ga, oracle, dim):
    rng = np.random.default_rng(500 + dim)
    el, q = ve.odd_i8(rng, 777, dim), ve.odd_i8(rng, 13, dim)
    assert (el == -128).any() and (q == -128).any()
    _check_dists(ga, oracle, el, q, dim)


def test_compute_distance_over_every_decade(ga, oracle):
    rng = np.random.default_rng(6)
    a, b = ve.scaled_raw(rng, 100, top=30), ve.scaled_raw(rng, 100, top=30)
    for i in range(len(a)):
        if i < 64:  # up to 1e19 for normalize
            assert ga.compute_distance("angular", a[i], b[i]) == oracle.dist(oracle.normalize_f32(a[i]), oracle.normalize_f32(b[i])), i
        assert ga.compute_distance("angular_int", a[i], b[i]) == oracle.dist(oracle.quantize(a[i]), oracle.quantize(b[i])), i


# ---- walks ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_world(int8, dim, n, nn, nq=64):
    """Elements, queries and the oracle's graph, made once per shape."""
    oracle = _oracle()
    rng = np.random.default_rng(9000 + 2 * dim + n + nn + int(int8))
    if int8:
        el, q = ve.odd_i8(rng, n, dim), ve.odd_i8(rng, nq, dim)
    else:
        el, q = ve.off_sphere_f32(rng, n, dim), ve.off_sphere_f32(rng, nq, dim)
    oix = oracle.build_index(el, num_neighbors=nn, max_search=max(40, nn + 20), n_threads=8)
    return el, q, oix


def _walk_with_and_without_the_sketch(gix, oix, q):
    """Revisits skipped in every launch (the walks the row sketch serves): sketch on and off, inline tails on and off --
    the same bytes, and the oracle's. Returns how many returned distances are 0.0."""
    from granne_amd import _lib
    gix.set_option(_lib.OPT_SEEN_MIN, 0)
    zeros = 0
    for tails in (1, 0):
        gix.set_option(_lib.OPT_INLINE_TAILS, tails)
        for ms in MAX_SEARCH:
            oi, od, oc, octr = oix.search_batch(q, ms, K)
            res = []
            for sketch in (0, 1):
                gix.set_option(_lib.OPT_SKETCH, sketch)
                assert gix.get_option(_lib.OPT_SKETCH) == sketch
                ids, ds, cnt, st = gix.search_batch(q, ms, K, stats=True)
                assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER
                assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes(), (tails, ms, sketch)
                assert_counters(st, octr, exact=False)
                res.append((ids, ds, cnt, st))
            for a, b in zip(*res):
                assert a.tobytes() == b.tobytes(), (tails, ms)
            zeros += int((od[oc > 0] == 0.0).sum())
    gix.set_option(_lib.OPT_SEEN_MIN, 2048)
    gix.set_option(_lib.OPT_INLINE_TAILS, 1)
    return zeros


def test_f32_walk_off_the_sphere_with_and_without_the_sketch(ga, oracle):
    """100-d rows of norms 10^-1.3 .. 10^1.3. Off the sphere the bound's margins scale with |q| |x|."""
    el, q, oix = walk_world(False, 100, 3000, 30)
    gix = ga.Granne("angular", el, oix.layers)
    assert _walk_with_and_without_the_sketch(gix, oix, q) > 1000  # the clamp: ties at 0.0, ordered by id
    for ms in MAX_SEARCH:
        assert_same(oix, gix, q, ms, K)  # without a visited set and with the exact one
    gix.close()


def test_f32_walk_on_rows_whose_sketch_error_is_the_whole_margin(ga, oracle):
    """value_edges.sketch_adversarial_f32: every row's residual points along the queries' signs, the queries have none. A
    margin without the factor N_q (invisible on the unit sphere, where N_q = 1) drops members of the true ten nearest:
    tests/test_value_edges_host.py shows it on the host model."""
    el, q = ve.sketch_adversarial_f32(np.random.default_rng(61), 3000, 64)
    oix = oracle.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
    gix = ga.Granne("angular", el, oix.layers)
    _walk_with_and_without_the_sketch(gix, oix, q)
    gix.close()


def test_f32_default_launch_of_many_walks_off_the_sphere(ga, oracle):
    el, _, oix = walk_world(False, 100, 3000, 30)
    q = ve.off_sphere_f32(np.random.default_rng(22), 2304, 100)
    gix = ga.Granne("angular", el, oix.layers)
    ids, ds, cnt = assert_same(oix, gix, q, 50, K)
    assert (ds[:, 0] == 0.0).mean() > 0.3
    gix.close()


@pytest.mark.parametrize("case", ["f32_200", "f32_97", "f32_300", "f32_100_wide", "f32_100_slow",
                                  "i8_100", "i8_200", "i8_300", "i8_512", "i8_600", "i8_1500", "i8_100_slow"])
def test_walks_on_every_walker(ga, oracle, case):
    """The unrolled 200-d walker, the streamed one (97, 300), the two-pass register walker (40 neighbors), the exact
    walker (forced), int8 rows of 128 / 256 / 512 bytes on the register walker and of 600 / 1500 on the general one -- at
    1500 the saturated rows' sum of squares is beyond 2^24, where its conversion to f32 rounds."""
    from granne_amd import _lib
    int8 = case.startswith("i8")
    dim = int(case.split("_")[1])
    wide, slow = case.endswith("wide"), case.endswith("slow")
    el, q, oix = walk_world(int8, dim, 1500 if dim >= 600 else 2000 if dim >= 200 else 3000, 40 if wide else 30)
    if wide:
        assert max(int((l != oracle.UNUSED).sum(axis=1).max()) for l in oix.layers) > 32
    if dim == 1500:
        assert int((el[-2].astype(np.int64) ** 2).sum()) > 1 << 24
    gix = ga.Granne(_et(el), el, oix.layers)
    if slow:
        gix.set_option(_lib.OPT_FORCE_SLOW, 1)
    want = (_lib.WALKER_EXACT if slow else _lib.WALKER_REGISTER_WIDE if wide else
            _lib.WALKER_GENERAL if int8 and dim > 512 else _lib.WALKER_REGISTER)
    for ms in MAX_SEARCH:
        assert_same(oix, gix, q, ms, K, has_exact_set=not wide)
        if slow:
            assert gix.last_slow_count() == len(q)
        if 10 <= ms <= 200:
            assert gix.get_option(_lib.OPT_LAST_WALKER) == want, (case, ms)
    gix.close()


# ---- refined search -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refine_world():
    oracle = _oracle()
    rng = np.random.default_rng(31)
    n, nq = 3000, 64
    unit, uq = ve.unit_f32(rng, n, 100), ve.unit_f32(rng, nq, 100)
    w = dict(unit=unit, uq=uq, unit8=oracle.quantize(unit), uq8=oracle.quantize(uq),
             off=ve.off_sphere_f32(rng, n, 100), offq=ve.off_sphere_f32(rng, nq, 100),
             odd=ve.odd_i8(rng, n, 100), oddq=ve.odd_i8(rng, nq, 100))
    w["oix8"] = oracle.build_index(w["unit8"], num_neighbors=20, max_search=20, n_threads=8)
    w["oix"] = oracle.build_index(w["unit"], num_neighbors=20, max_search=20, n_threads=8)
    return w


@pytest.mark.parametrize("ms,m", [(64, 64), (300, 257)])
@pytest.mark.parametrize("side", ["int8_walk_off_sphere_rows", "f32_walk_odd_i8_rows"])
def test_refined_search_by_rows_of_any_norm(ga, oracle, side, ms, m):
    """A rows-only handle carries any rows. Candidates at distance 0.0 come out in id order."""
    w = refine_world()
    if side == "int8_walk_off_sphere_rows":
        walk_el, oix, rows, qw, qr = w["unit8"], w["oix8"], w["off"], w["uq8"], w["offq"]
    else:
        walk_el, oix, rows, qw, qr = w["unit"], w["oix"], w["odd"], w["uq"], w["oddq"]
    walk, refine = ga.Granne(_et(walk_el), walk_el, oix.layers), ga.Granne(_et(rows), rows, [])
    ids, ds, cnt, st, dropped = ga.RefinedGranne(walk, refine).search_batch((qw, qr), ms, K, refine_from=m, stats=True, dropped=True)
    eids, eds, ecnt, edropped, ectr = model.search_refined(oracle, oix, rows, qw, qr, ms, m, K)
    assert (ids == eids).all() and ds.tobytes() == eds.tobytes() and (cnt == ecnt).all()
    assert dropped == 0 == edropped
    assert_counters(st, ectr, exact=False)
    if rows.dtype == np.float32:
        clamped = ds == 0.0
        assert clamped.sum() > 100  # (a third of the candidates of most queries)
        tie = clamped[:, 1:] & clamped[:, :-1]
        assert tie.any() and (ids[:, 1:][tie] > ids[:, :-1][tie]).all()
    walk.close()
    refine.close()


# ---- builders -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["off_sphere_f32", "odd_i8", "odd_i8_8d"])
def test_gpu_build_equals_the_oracles_batched_build(ga, oracle, case):
    rng = np.random.default_rng({"off_sphere_f32": 41, "odd_i8": 42, "odd_i8_8d": 43}[case])
    n = 2000
    if case == "off_sphere_f32":
        el, q = ve.off_sphere_f32(rng, n, 100), ve.off_sphere_f32(rng, 16, 100)
    elif case == "odd_i8":
        el, q = ve.odd_i8(rng, n, 100), ve.odd_i8(rng, 16, 100)
    else:  # 8-d: every 25th row cut down to components -1 / 0 / 1 -- duplicates and further zero rows
        el, q = ve.odd_i8(rng, n, 8), ve.odd_i8(rng, 16, 8)
        el[::25] = np.trunc(el[::25] / 100.0).astype(np.int8)
        assert len(np.unique(el, axis=0)) < n - 10 and (~el.any(axis=1)).sum() > 3
    kw = dict(num_neighbors=30, max_search=40, batch_max=256, batch_div=8)
    b = ga.GranneBuilder(_et(el), el, **kw)
    b.build()
    assert len(b) == n
    oix = oracle.build_index(el, n_threads=0, **kw)
    assert b.num_layers() == len(oix.layers)
    for l, want in enumerate(oix.layers):
        got = b.get_layer(l)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (l, bad[:5], got[bad[:1]], want[bad[:1]])
    gix = b.get_index()
    assert_same(oix, gix, q, 30, K)
    gix.close()
    b.close()


@pytest.mark.parametrize("int8", [False, True])
def test_rw_builder_equals_its_model(ga, oracle, int8):
    """800 places (tests/test_gpu_rw_builder.py's smallest case), empty at the start: single inserts, a batch of 20, one
    batch across the promotions, the rest and 100 rows too many; then the live graph is searched."""
    dim, nn, ms, mult, max_el = (28, 10, 20, 5.0, 800) if int8 else (8, 10, 20, 5.0, 800)
    rng = np.random.default_rng(50 + int8)
    if int8:
        el, q = ve.odd_i8(rng, max_el + 100, dim), ve.odd_i8(rng, 32, dim)
    else:  # (norms 0.8 .. 2: a row shorter than 1 is at distance > 0 from itself and stays unindexed, like a zero row; at
        #  larger norms nearly every distance in 8 dimensions is the clamp's and select_neighbors keeps one neighbor per row)
        el, q = ve.off_sphere_f32(rng, max_el + 100, dim, lo=-0.1, hi=0.3), ve.off_sphere_f32(rng, 32, dim)
    m = RwModel.new([], el[:0], {"num_neighbors": nn, "max_search": ms, "layer_multiplier": mult}, max_el)
    b = ga.GranneBuilder(_et(el), None, num_neighbors=nn, max_search=ms, layer_multiplier=mult, reinsert_elements=False)
    rw = ga.RwGranneBuilder(b, max_el, dim=dim)
    steps = [(i, i + 1) for i in range(10)] + [(10, 30), (30, max_el - 5), (max_el - 5, max_el + 100)]
    for lo, hi in steps:
        want = m.insert_batch(el[lo:hi])
        got = [rw.insert(el[lo])] if hi - lo == 1 else [int(x) for x in rw.insert_batch(el[lo:hi])]
        assert got == want, (lo, hi)
    assert len(rw) == len(m) == max_el
    got_layers, want_layers = rw.layers(), m.layers()
    assert len(got_layers) == len(want_layers) >= 2
    for l, (g, w) in enumerate(zip(got_layers, want_layers)):
        assert g.shape == w.shape
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, (l, bad[:5], g[bad[:1]], w[bad[:1]])
    for ef, k in ((20, 10), (1, 1)):
        wi, wd, wc, _ = m.index().search_batch(q, ef, k)
        ids, ds, cnt = rw.search_batch(q, ef, k)
        assert (cnt == wc).all()
        for i in range(len(q)):
            c = int(wc[i])
            assert (ids[i, :c] == wi[i, :c]).all() and ds[i, :c].tobytes() == wd[i, :c].tobytes(), (ef, i)
    rw.close()


# ---- the exact scan, in tolerance mode (its documented contract) --------------------------------------------
@pytest.mark.parametrize("name", sorted(ve.SCAN_INPUTS))
def test_exact_scan_on_value_edges(ga, oracle, name):
    """tests/test_gpu_bruteforce.py's assertions on inputs whose near-tied ranks tests/test_value_edges_host.py caps at
    2 % by the oracle alone: the returned distances are the oracle's bits for the returned ids, ascending by (distance,
    id); every distance within the tolerance of the true one at its rank; ids equal in more than 98 % of the positions
    and within the tolerance elsewhere. Blocks whose lane halves see norms 40 x apart, queries whose best scores are all
    negative, and (primed sizes) a nearest neighbour of 1 / 40 of its block's norms. Every scan asserts the kernel form, the
    ranges and whether the priming pass ran (value_edges.SCAN_RAN)."""
    from granne_amd import _lib
    el, q, tol = ve.scan_input(name)
    n, nq = len(el), len(q)
    primed = name.endswith("primed")
    ix = ga.Granne(_et(el), el, [])
    _, truth_i, truth_d = oracle.Index(el, []).scan_topk(q, max(ve.SCAN_KS))
    checked = range(nq) if not primed else list(range(ve.PLANTED + 8)) + [nq - 1]
    for k in ve.SCAN_KS:
        ids, ds, cnt = ix.brute_force(q, k)
        form, ranges, primed_ks = ve.SCAN_RAN[name]
        ran = _lib.last_scan(ix.get_option(_lib.OPT_LAST_SCAN))
        assert (ran["form"], ran["ranges"], ran["primed"]) == (getattr(_lib, "SCAN_" + form), ranges, k in primed_ks), (k, ran)
        assert not primed or ran["primed"]
        want_i, want_d = truth_i[:, :k], truth_d[:, :k]
        assert (cnt == k).all()
        for qi in checked:
            got = np.array([oracle.dist(el[int(e)], q[qi]) for e in ids[qi]], np.float32)
            assert got.tobytes() == ds[qi].tobytes(), (k, qi)
        for qi in range(nq):
            keys = list(zip(ds[qi].tolist(), ids[qi].tolist()))
            assert keys == sorted(keys) and len(set(ids[qi].tolist())) == k, (k, qi)
        err = np.abs(ds.astype(np.float64) - want_d.astype(np.float64))
        same = ids == want_i
        print("%s k=%d: largest |d - true d| %.3g, ids equal %.4f" % (name, k, err.max(), same.mean()))
        assert err.max() <= tol, (k, np.unravel_index(err.argmax(), err.shape))
        assert same.mean() > 0.98
        assert (err[~same] <= tol).all()
        if primed:  # whatever order the ranges publish in
            ids2, ds2, cnt2 = ix.brute_force(q, k)
            assert (ids == ids2).all() and ds.tobytes() == ds2.tobytes() and (cnt == cnt2).all()
            assert [int(ids[j, 0]) for j in range(ve.PLANTED)] == [ve.planted_at(j, n) for j in range(ve.PLANTED)]
        if name.startswith("one_sided"):
            assert (ids[:, 0] == n // 2).all() and (ds[:, 0] == 1.0).all() and (ds[:, 1:] > 1.0).all()
    ix.close()
