"""Granne::reorder (granne_amd/csrc/reorder_host.h) through every kernel its trail walks can take, on tied and odd rows,
with hand-overs inside a reorder, at a size past remap_rows_kernel's grid, and what follows a reorder (the exact scans,
dists). The inputs are tests/reorder_worlds.py's; tests/test_reorder_worlds_host.py holds them to their conditions on the
CPU. Every comparison is bit for bit: the permutation, the index file's bytes (every row of every layer), every element,
searches -- against the oracle's compute_order / reordered index."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import fileformat, pyref  # noqa: E402
from tests import reorder_worlds as rw  # noqa: E402
from tests import scan_forms  # noqa: E402
from tests.conftest import assert_counters  # noqa: E402


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def gpu_index(ga, oix):
    return ga.Granne("angular" if oix.elements.dtype == np.float32 else "angular_int", oix.elements, oix.layers)


def walker_code(name):
    from granne_amd import _lib
    return {"register": _lib.WALKER_REGISTER, "general": _lib.WALKER_GENERAL, "exact": _lib.WALKER_EXACT}[name]


def assert_searches(gix, oix, q):
    for ms, k in ((25, 10), (1, 1)):
        oi, od, oc, _ = oix.search_batch(q, ms, k)
        ids, ds, cnt = gix.search_batch(q, ms, k)
        assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes(), (ms, k)


def assert_is(gix, oix, q):
    """the handle holds exactly `oix`: the index file's bytes (every row of every layer), every element, searches"""
    assert gix.index_bytes() == fileformat.write_index(oix.layers)
    assert len(gix) == len(oix)
    for i in range(len(oix)):
        assert gix.get_element(i).tobytes() == oix.elements[i].tobytes(), i
    assert_searches(gix, oix, q)


def reorder_and_check(ga, oix, q, walker, twice=False):
    """Everything the module asks of one reorder; returns the hand-overs of the plain reorder."""
    from granne_amd import _lib
    walks = len(oix) - oix.layers[0].shape[0]
    want = oix.compute_order()
    gix = gpu_index(ga, oix)
    hbm = gix.hbm_bytes()
    got = gix.reorder()
    assert got.dtype == np.uint64 and got.tolist() == want.tolist()
    assert gix.get_option(_lib.OPT_LAST_WALKER) == walker_code(walker)
    handed = gix.last_slow_count()
    ore = oix.reordered(want)
    assert_is(gix, ore, q)
    assert gix.hbm_bytes() == hbm
    if twice:  # a reordered index is an index: its own order, from the oracle's reordered index
        want2 = ore.compute_order()
        assert gix.reorder().tolist() == want2.tolist()
        assert_is(gix, ore.reordered(want2), q)
        assert gix.hbm_bytes() == hbm
    # once more, every trail on the exact walker
    slow = gpu_index(ga, oix)
    slow.set_option(_lib.OPT_FORCE_SLOW, 1)
    assert slow.reorder().tolist() == want.tolist()
    assert slow.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_EXACT
    assert slow.last_slow_count() == walks
    slow.set_option(_lib.OPT_FORCE_SLOW, 0)
    assert slow.index_bytes() == fileformat.write_index(ore.layers)
    return handed


# ---- 2. every trail walker ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rw.BUILT) + ["wide_rows"])
def test_every_trail_walker(ga, oracle, name):
    """int8 rows of 256 and 512 bytes on the register trail walkers; rows beyond 512 bytes, layers of 64 device ids
    (num_neighbors 40 and 63) and hand-made rows of up to 100 ids on the general trail walkers; each once more with
    every trail on the exact walker."""
    oix, q = rw.wide_rows() if name == "wide_rows" else rw.built(name)
    walker = "general" if name == "wide_rows" else rw.BUILT[name][4]
    handed = reorder_and_check(ga, oix, q, walker)
    print("%s: %s walker, %d hand-overs in %d walks" % (name, walker, handed, len(oix) - oix.layers[0].shape[0]))
    assert handed == 0  # (uniform rows, the default tables: nothing to hand over)


# ---- 3. ties and odd rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rw.TIED))
def test_reorder_on_tied_rows(ga, oracle, name):
    """Rows with byte-identical copies, a grid of three values per component, every seventh row zero: trails that are
    equal are ordered by idx alone, and equal distances inside a trail walk by the reference's tie rules."""
    oix, q = rw.tied(name)
    handed = reorder_and_check(ga, oix, q, "register", twice=True)
    print("%s: %d hand-overs" % (name, handed))


def test_edge_rows_are_remapped_as_the_reference_does(ga, oracle):
    """Empty rows, full rows, ids named twice and three times, ids after the first UNUSED -- at declared widths 32, 33,
    64 and 100: the reordered layers are pyref.reorder_layers' (sets sorted, repeats kept, what follows an UNUSED
    dropped), and a search with the exact visited set is the oracle's (the twin-row flag is found again)."""
    from granne_amd import _lib
    oix, q = rw.edge_rows()
    gix = gpu_index(ga, oix)
    want = oix.compute_order()
    assert gix.reorder().tolist() == want.tolist()
    assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_GENERAL
    sets = pyref.reorder_layers(oix.layers, want.astype(np.int64).tolist())
    for l, rows in enumerate(sets):
        assert gix.layer_len(l) == len(rows)
        for i, row in enumerate(rows):
            assert gix.get_neighbors(i, l) == row, (l, i)
    ore = oix.reordered(want)
    assert gix.index_bytes() == fileformat.write_index(ore.layers)
    for i in range(len(ore)):
        assert gix.get_element(i).tobytes() == ore.elements[i].tobytes()
    gix.set_option(_lib.OPT_VISITED16, 3)
    oi, od, oc, octr = ore.search_batch(q, 30, 10)
    ids, ds, cnt, st = gix.search_batch(q, 30, 10, stats=True)
    assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes()
    assert_counters(st, octr, exact=True)


# ---- 4. hand-overs inside a reorder ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ring(name):
    oix, q = rw.ring(name)
    walks, lo, hi, _ = rw.ring_bounds(oix)
    return oix, q, walks, lo, hi


@pytest.mark.parametrize("name", list(rw.RING))
def test_trails_are_handed_over_inside_a_reorder(ga, oracle, name):
    """A visited table of 256 slots and no overflow table (test_visited_table_overflow_hands_over's recipe): the exact
    walker's trail branch runs as tail blocks behind trail walkers that handed over. lo = #(n_dist > 256) walks cannot
    keep their ids in 256 slots; hi = #(n_dist > 128) bounds the walks that can fill the table to its limit.
    Observed on an MI355X: 801 of 1,200 walks handed over (lo 606, hi 943) in the three cases of +-8 links, 866 (lo 670,
    hi 997) with +-20 links."""
    from granne_amd import _lib
    oix, q, walks, lo, hi = _ring(name)
    want = oix.compute_order()
    gix = gpu_index(ga, oix)
    gix.set_option(_lib.OPT_VISITED_SLOTS, 256)
    gix.set_option(_lib.OPT_OVERFLOW_SLOTS, 1)
    assert gix.reorder().tolist() == want.tolist()
    assert gix.get_option(_lib.OPT_LAST_WALKER) == walker_code(rw.RING[name][3])
    handed = gix.last_slow_count()
    print("%s: %d of %d walks handed over (lo %d, hi %d)" % (name, handed, walks, lo, hi))
    assert lo <= handed <= hi
    assert gix.index_bytes() == fileformat.write_index(oix.reordered(want).layers)
    # the options back at 0: the same order, nothing handed over
    plain = gpu_index(ga, oix)
    plain.set_option(_lib.OPT_VISITED_SLOTS, 256)
    plain.set_option(_lib.OPT_OVERFLOW_SLOTS, 1)
    plain.set_option(_lib.OPT_VISITED_SLOTS, 0)
    plain.set_option(_lib.OPT_OVERFLOW_SLOTS, 0)
    assert plain.reorder().tolist() == want.tolist()
    assert plain.last_slow_count() == 0


@pytest.mark.parametrize("name", ["f32_100", "i8_100"])
def test_a_reorder_that_exhausts_the_exact_walker_leaves_the_index_untouched(ga, oracle, name):
    """The exact walker's containers at 256 slots (test_slow_scratch_exhaustion_is_reported's value): every walk that is
    handed over outgrows them, reorder() raises, and nothing has been swapped in."""
    from granne_amd import _lib
    oix, q, walks, lo, hi = _ring(name)
    gix = gpu_index(ga, oix)
    slots = gix.get_option(_lib.OPT_SLOW_SLOTS)
    hbm = gix.hbm_bytes()
    gix.set_option(_lib.OPT_VISITED_SLOTS, 256)
    gix.set_option(_lib.OPT_OVERFLOW_SLOTS, 1)
    gix.set_option(_lib.OPT_SLOW_SLOTS, 256)
    with pytest.raises(ga.GranneHipError) as e:
        gix.reorder()
    assert e.value.code == _lib.ERR_OVERFLOW
    assert lo <= gix.last_slow_count() <= hi
    gix.set_option(_lib.OPT_SLOW_SLOTS, slots)
    gix.set_option(_lib.OPT_VISITED_SLOTS, 0)
    gix.set_option(_lib.OPT_OVERFLOW_SLOTS, 0)
    assert_is(gix, oix, q)
    assert gix.hbm_bytes() == hbm
    gix.set_option(_lib.OPT_VISITED_SLOTS, 256)
    gix.set_option(_lib.OPT_OVERFLOW_SLOTS, 1)
    want = oix.compute_order()
    assert gix.reorder().tolist() == want.tolist()
    assert lo <= gix.last_slow_count() <= hi
    gix.set_option(_lib.OPT_VISITED_SLOTS, 0)
    gix.set_option(_lib.OPT_OVERFLOW_SLOTS, 0)
    assert_is(gix, oix.reordered(want), q)


# ---- 5. size and followers ------------------------------------------------------------------------------------------
def test_reorder_of_70000_rows(ga, oracle):
    """More rows than remap_rows_kernel has blocks (65,536): its grid-stride loop runs a second trip; one trail launch of
    61,250 walks; radix sorts beyond one tile."""
    from granne_amd import _lib
    oix = rw.size_70k()
    assert [l.shape[0] for l in oix.layers] == [3, 18, 137, 1094, 8750, 70000]
    want = oix.compute_order()
    gix = gpu_index(ga, oix)
    got = gix.reorder()
    assert got.tolist() == want.tolist()
    assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER and gix.last_slow_count() == 0
    assert gix.index_bytes() == fileformat.write_index(oix.reordered(want).layers)
    for i in (0, 1, 65535, 65536, 65537, 69999):
        assert gix.get_element(i).tobytes() == oix.elements[int(want[i])].tobytes()


def _assert_scans(oracle, gix, ore, q, form):
    """brute_force under tests/test_gpu_bruteforce.py's contract (ids equal on uniform rows), exact_topk bit for bit,
    dists_many over every id"""
    el = ore.elements
    int8 = el.dtype == np.int8
    _sec, want_i, want_d = ore.scan_topk(q, 10)
    ids, ds, cnt = gix.brute_force(q, 10)
    assert scan_forms.reported(gix)["form"] == form
    assert (cnt == 10).all() and (ids == want_i).all()
    assert np.abs(ds - want_d).max() <= (scan_forms.TOL_I8 if int8 else scan_forms.TOL_F32)
    for qi in range(len(q)):
        got = np.array([oracle.dist(el[int(e)], q[qi]) for e in ids[qi]], np.float32)
        assert got.tobytes() == ds[qi].tobytes()
    ids, ds, cnt = gix.exact_topk(q, 10)
    assert (cnt == 10).all() and (ids == want_i).all() and ds.tobytes() == want_d.tobytes()
    every = np.tile(np.arange(len(el), dtype=np.uint32), (4, 1))
    want = np.array([[oracle.dist(el[e], q[a]) for e in range(len(el))] for a in range(4)], np.float32)
    assert gix.dists_many(q[:4], every).tobytes() == want.tobytes()


@pytest.mark.parametrize("int8,dim,form", [(True, 100, "RING"), (True, 17, "I8"), (False, 100, "B16_7_4")])
def test_scans_and_dists_follow_a_reorder(ga, oracle, int8, dim, form):
    """apply_order drops the int8 scan norms and finish_layers makes them again: the exact scans and dists before a
    reorder (the norms exist) and after it (they must be the permuted rows')."""
    rng = np.random.default_rng(3000 + dim + int8)
    el = rw.prep(scan_forms.uniform_rows(rng, 3000, dim), int8)
    q = rw.prep(scan_forms.uniform_rows(rng, 24, dim), int8)
    oix = oracle.build_index(el, num_neighbors=20, max_search=20, layer_multiplier=rw.MULT, n_threads=4)
    gix = gpu_index(ga, oix)
    _assert_scans(oracle, gix, oix, q, form)
    hbm = gix.hbm_bytes()
    want = oix.compute_order()
    assert gix.reorder().tolist() == want.tolist()
    ore = oix.reordered(want)
    _assert_scans(oracle, gix, ore, q, form)
    assert gix.hbm_bytes() == hbm


@pytest.mark.parametrize("single_top", [False, True])
def test_reorder_by_keys_on_every_key_shape(ga, oracle, single_top):
    """All keys equal (the identity), descending keys (every layer reversed), keys that differ only above / only below
    bit 32, keys 0 and 2^64 - 1 -- against the oracle and against numpy's lexsort per layer; also on an index whose top
    layer has one row."""
    oix = rw.keys_world(single_top)
    assert (oix.layers[0].shape[0] == 1) == single_top
    rng = np.random.default_rng(9)
    q = rw.queries(rng, oix.elements, 16, False, drawn=11)
    for name, keys in rw.key_sets(len(oix)).items():
        want = oix.order_by_keys(keys)
        assert want.tolist() == rw.lexsort_order(oix, keys).tolist()
        gix = gpu_index(ga, oix)
        got = gix.reorder_by_keys(keys)
        assert got.tolist() == want.tolist(), name
        if name == "all_equal":
            assert got.tolist() == list(range(len(oix)))
        ore = oix.reordered(want)
        assert gix.index_bytes() == fileformat.write_index(ore.layers), name
        for i in range(0, len(ore), 13):
            assert gix.get_element(i).tobytes() == ore.elements[i].tobytes()
        assert_searches(gix, ore, q)
