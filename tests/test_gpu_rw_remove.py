"""RwGranneBuilder's removals on the GPU (remove / restore / removed_count / alive_filter / compact) against
tests/rw_remove_model.py: searches byte for byte with their counters, the layers row for row, the counts, the form that
ran, snapshots, compaction, threads and the error returns. tests/README_rw_remove.md says what each test pins.

Worlds: 600 places at multiplier 5 (layers of 2, 10, 120 and 600 rows), 50 elements built before the handle, 550 inserted
in the call pattern of tests/test_gpu_rw_builder.py -- 40 single inserts, a batch of 20, a large batch across the
promotion to the 600-row layer, then the rest and 20 rows too many. The model walks in Python, so every distance it needs
comes from one matrix per world (the library's Dist operator over a snapshot, checked against oracle/pyref.py on a
sample) and a (removed set, max_search) walk is modelled once."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyref  # noqa: E402
from tests import filter_model as fm  # noqa: E402
from tests.conftest import assert_counters, random_floats  # noqa: E402
from tests.rw_model import RwModel  # noqa: E402
from tests.rw_remove_model import RwRemoveModel  # noqa: E402

# dim, int8, num_neighbors, max_search of the config
CASES = [(32, False, 10, 20), (28, True, 10, 20), (100, False, 30, 40)]
# The worlds' seeds. The "nearest" state asserts that the answer is the former second; that holds for a query whenever
# the walk under the filter meets no alive element nearer than it, and need not otherwise: the filtered walk keeps fewer
# ids in `res`, so it stops later and evaluates every node the unfiltered walk evaluated and possibly more -- the answer
# is never farther than the former second, but it can be nearer (in the MODEL, 2 of 64 walks of the third world under
# seeds 4102 and 4103). These seeds are ones under which the model has the property for all 64; the test says so first.
SEEDS = [4100, 4101, 4104]
MULT, PLACES, START, NQ = 5.0, 600, 50, 16
U64_MAX = np.iinfo(np.uint64).max
# 64 and 65: the general walker's last one-list and first two-list size; 257: the exact walker
MAX_SEARCH = [20, 64, 65, 257]
STATES = ["nothing", "entry_point", "word_edge", "whole_word", "last", "inserted", "nearest", "half", "all_but_3", "everything"]
STEPS = [(i, i + 1) for i in range(40)] + [(40, 60), (60, PLACES - START - 5), (PLACES - START - 5, PLACES - START + 20)]


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _prepared(oracle, raw, int8):
    return oracle.quantize(raw) if int8 else oracle.normalize_f32(raw)


def _oracle_kw(nn, ms):
    return dict(num_neighbors=nn, max_search=ms, layer_multiplier=MULT, reinsert_elements=False, batch_max=65536, batch_div=8,
                n_threads=0)


def _start_layers(oracle, el, nn, ms, max_el, held_first):
    """The layers RwGranneBuilder::new finds, as tests/test_gpu_rw_builder.py's reference makes them: what a GranneBuilder
    that was built holds (held_first), then build() with expected_num_elements = max_elements."""
    kw = _oracle_kw(nn, ms)
    if not len(el):
        return []
    if held_first:
        held = oracle.build_index(el, **kw)
        return oracle.build_index(el, expected_num_elements=max_el, resume_from=held.layers, **kw).layers
    return oracle.build_index(el, expected_num_elements=max_el, **kw).layers


def _make_handle(ga, el, int8, nn, ms, start, build_first=True):
    b = ga.GranneBuilder("angular_int" if int8 else "angular", el[:start], num_neighbors=nn, max_search=ms, layer_multiplier=MULT,
                         reinsert_elements=False)
    if build_first:
        b.build()
        assert len(b) == start
    return ga.RwGranneBuilder(b, PLACES)


def _run_steps(target, el, steps, between=None):
    """The calls of `steps` (row ranges after the START built rows) on a handle or a model; the ids each returned."""
    out = []
    for call, (lo, hi) in enumerate(steps):
        rows = el[START + lo:START + hi]
        if hi - lo == 1:
            got = target.insert(rows[0])
            out.append([] if got is None else [int(got)])
        else:
            out.append([int(x) for x in target.insert_batch(rows)])
        if between:
            between(call)
    return out


def assert_layers_equal(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (l, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, "layer %d: %d rows differ, first %d: %s vs %s" % (l, bad.size, bad[0], g[bad[0]], w[bad[0]])


class World:
    """A full handle with nothing removed, the model of the same calls, NQ queries and their distances to every element."""

    def __init__(self, ga, oracle, ci, el=None, seed=None):
        dim, int8, nn, ms = CASES[ci]
        self.ga, self.int8, self.nn, self.ms = ga, int8, nn, ms
        rng = np.random.default_rng(SEEDS[ci] if seed is None else seed)
        self.el = _prepared(oracle, random_floats(rng, PLACES + 20, dim), int8) if el is None else el
        self.q = _prepared(oracle, random_floats(rng, NQ, dim), int8)
        self.cfg = {"num_neighbors": nn, "max_search": ms, "layer_multiplier": MULT}
        self.model = RwRemoveModel.new(_start_layers(oracle, self.el[:START], nn, ms, PLACES, True), self.el[:START], self.cfg, PLACES)
        self.ids = _run_steps(self.model, self.el, STEPS)
        self.layers = self.model.layers()
        # three previous layers: two as the builder of 50 made them, then the levels of 600 places
        assert [len(l) for l in self.layers] == [2, 10, 120, 600]
        self.rw = _make_handle(ga, self.el, int8, nn, ms, START)
        assert _run_steps(self.rw, self.el, STEPS) == self.ids and len(self.rw) == PLACES
        assert_layers_equal(self.rw.layers(), self.layers)
        snap = self.rw.get_index()
        self.D = snap.dists_many(self.q, np.tile(np.arange(PLACES, dtype=np.uint32), (NQ, 1)))
        snap.close()
        for qi, i in zip(rng.integers(0, NQ, 32), rng.integers(0, PLACES, 32)):  # the matrix is pyref's, on a sample
            assert np.float32(self.D[qi, i]).view(np.uint32) == np.float32(pyref.dist(self.el[i], self.q[qi])).view(np.uint32)
        self.cache, self.walks = [], {}
        # what a handle that never saw a remove answers
        self.clean = {ms_: self.rw.search_batch(self.q, ms_, 10, stats=True) for ms_ in MAX_SEARCH}

    def walk(self, alive, ms):
        """The modelled batch with num_neighbors = max_search (all of `res`): ids [NQ][ms], dists, counts, stats."""
        key = (alive.tobytes(), ms)
        if key not in self.walks:
            ids, ds = np.full((NQ, ms), U64_MAX, np.uint64), np.full((NQ, ms), np.inf, np.float32)
            cnt, st = np.zeros(NQ, np.uint32), np.zeros((NQ, 3), np.uint64)
            for i in range(NQ):
                r = fm.search_filtered(self.layers, self.el[:PLACES], self.q[i], alive, ms, ms, 0, self.D[i], self.cache)
                ids[i], ds[i] = r.padded(ms)
                cnt[i] = r.count
                st[i] = (r.counters["n_dist"], r.counters["n_expand"], r.counters["n_adj"])
            self.walks[key] = (ids, ds, cnt, st)
        return self.walks[key]

    def check(self, alive, ms, k, exact_stats=True, q_rows=slice(None)):
        """One live search_batch against the model under `alive`."""
        ids, ds, cnt, st = self.rw.search_batch(self.q[q_rows], ms, k, stats=True)
        mi, md, mc, mst = (a[q_rows] for a in self.walk(alive, ms))
        assert k <= ms
        want_ids, want_ds = mi[:, :k], md[:, :k]  # (the model's rows are filled beyond their counts as the library fills them)
        assert (cnt == np.minimum(mc, k)).all()
        assert (ids == want_ids).all()
        assert ds.tobytes() == want_ds.tobytes()
        if exact_stats:
            assert (st == mst).all()
        else:  # the unfiltered launch may be a register walker's: it keeps no visited set (tests/conftest.py)
            assert_counters(st, mst, exact=False)
        return ids, ds, cnt, st

    def state(self, name):
        """The ids to remove for one of STATES."""
        rng = np.random.default_rng(sum(map(ord, name)))
        if name == "nothing":
            return []
        if name == "entry_point":
            return [0]
        if name == "word_edge":
            return [31, 32, 33]
        if name == "whole_word":
            return list(range(64, 96))
        if name == "last":
            return [PLACES - 1]
        if name == "inserted":
            return [START + 123]
        if name == "nearest":
            return sorted({int(x) for ms in MAX_SEARCH for x in self.clean[ms][0][:, 0]})  # (at every max_search tested)
        if name == "half":
            return sorted(int(x) for x in np.nonzero(rng.random(PLACES) < 0.5)[0])
        if name == "all_but_3":
            return sorted(set(range(PLACES)) - {7, 300, PLACES - 1})
        assert name == "everything"
        return list(range(PLACES))


@pytest.fixture(scope="module")
def worlds(ga, oracle):
    made = {}

    def get(ci):
        if ci not in made:
            made[ci] = World(ga, oracle, ci)
        w = made[ci]
        assert w.rw.removed_count() == 0  # every test leaves it as it found it
        return w

    yield get
    for w in made.values():
        w.rw.close()


def _alive(removed):
    a = np.ones(PLACES, bool)
    a[list(removed)] = False
    return a


def _words(f):
    """A Filter's words with the bits at positions >= n cleared (the handle's bitmap holds ones there; every reader of a
    filter ignores them)."""
    w = f.words().copy()
    if f.n % 32:
        w[-1] &= np.uint32((1 << (f.n % 32)) - 1)
    return w


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("ci", range(len(CASES)))
def test_search_equals_the_model(worlds, ci, state):
    w = worlds(ci)
    removed = w.state(state)
    alive = _alive(removed)
    assert w.rw.remove(removed) == (len(removed), 0, 0) and w.rw.removed_count() == len(removed)
    try:
        for ms in MAX_SEARCH:
            for k in (10, ms):
                ids, _ds, cnt, _st = w.check(alive, ms, k, exact_stats=bool(removed))
                assert not np.isin(ids[ids != U64_MAX], removed).any()
                if state == "everything":
                    assert (cnt == 0).all() and (ids == U64_MAX).all()
                if state == "all_but_3":
                    assert (cnt <= 3).all() and cnt.max() > 0
                if state == "nearest" and k == 10:
                    # the answer is the former second -- the first of the former answers that is still alive
                    was, model_first = w.clean[ms][0], w.walk(alive, ms)[0][:, 0]
                    for qi in range(NQ):
                        survivors = [int(x) for x in was[qi] if int(x) not in removed]
                        assert int(was[qi, 0]) in removed and survivors
                        assert int(model_first[qi]) == survivors[0]  # the inputs have the property (SEEDS)
                        assert int(ids[qi, 0]) == survivors[0]
    finally:
        assert w.rw.restore(removed) == (len(removed), 0, 0)


@functools.lru_cache(maxsize=None)
def _tied_rows(seed):
    rng = np.random.default_rng(seed)
    raw = random_floats(rng, PLACES + 20, 32)
    raw[200:220] = raw[400:420] = raw[:20]  # 20 rows three times: ids i, i + 200, i + 400
    return raw


def test_ties_order_by_distance_bits_then_id(ga, oracle):
    el = oracle.normalize_f32(_tied_rows(7))
    w = World(ga, oracle, 0, el=el, seed=8)
    # queries next to the tripled rows, so that the copies lead the answers
    w.q = oracle.normalize_f32(el[:NQ] + np.float32(0.05) * random_floats(np.random.default_rng(9), NQ, 32))
    snap = w.rw.get_index()
    w.D = snap.dists_many(w.q, np.tile(np.arange(PLACES, dtype=np.uint32), (NQ, 1)))
    snap.close()
    middle = list(range(200, 220))
    assert w.rw.remove(middle) == (20, 0, 0)
    alive = _alive(middle)
    seen_pairs = 0
    for ms in (20, 65, 257):
        ids, ds, cnt, _ = w.check(alive, ms, ms)
        bits = ds.view(np.uint32)
        for qi in range(NQ):
            c = int(cnt[qi])
            keys = [(int(bits[qi, j]), int(ids[qi, j])) for j in range(c)]
            assert keys == sorted(keys) and len(set(keys)) == c
            got = [i for _, i in keys]
            assert not set(got) & set(middle)
            for j, i in enumerate(got):
                if i < 20 and i + 400 in got:  # the two surviving copies: equal distance bits, the lower id first
                    assert got[j + 1] == i + 400 and keys[j][0] == keys[j + 1][0]
                    seen_pairs += 1
    assert seen_pairs >= NQ
    w.rw.close()


def test_counts(ga, worlds):
    w = worlds(0)
    rw = w.rw
    ids = [5, 5, 7, len(rw), 2 ** 40]
    try:
        assert rw.remove(ids) == (2, 1, 2)
        assert rw.removed_count() == 2 == rw.get_option(ga.rw_builder.REMOVED)
        assert rw.remove(ids) == (0, 3, 2)
        assert rw.removed_count() == 2 == rw.get_option(ga.rw_builder.REMOVED)
        assert rw.remove([]) == (0, 0, 0)
        assert (_words(rw.alive_filter()) == fm.pack_bits(_alive([5, 7]))).all()
        assert rw.restore(ids) == (2, 1, 2)
        assert rw.removed_count() == 0 == rw.get_option(ga.rw_builder.REMOVED)
        assert rw.restore(ids) == (0, 3, 2)
        big = np.arange(100000, dtype=np.uint64) % 1000  # many blocks: ids 0..599 a hundred times, 600..999 out of range
        assert rw.remove(big) == (PLACES, 99 * PLACES, 400 * 100) and rw.removed_count() == PLACES
        assert rw.restore(big) == (PLACES, 99 * PLACES, 400 * 100)
        with pytest.raises(ga.GranneHipError):
            rw.set_option(ga.rw_builder.REMOVED, 1)  # read-only
    finally:
        rw.restore(np.arange(PLACES))
    assert rw.removed_count() == 0 and len(rw) == PLACES


def test_the_form_that_ran(ga, worlds):
    w = worlds(1)
    rw, opt = w.rw, ga.rw_builder.FILTERED_SEARCHES
    at = rw.get_option(opt)
    rw.search_batch(w.q, 20, 10)
    rw.search(w.q[0], 20, 10)
    assert rw.get_option(opt) == at  # nothing removed: the launch it always ran
    rw.remove([9])
    try:
        rw.search_batch(w.q, 20, 10)
        rw.search_batch(w.q, 257, 10)
        assert rw.get_option(opt) == at + 2
        rw.search(w.q[0], 20, 10)
        assert rw.get_option(opt) == at + 3
    finally:
        rw.restore([9])
    for ms in MAX_SEARCH:  # every id restored: the unfiltered launch again, and a never-removed handle's bytes
        for x, y in zip(rw.search_batch(w.q, ms, 10, stats=True), w.clean[ms]):
            assert x.tobytes() == y.tobytes()
    assert rw.get_option(opt) == at + 3


def test_inserts_are_blind_to_tombstones(ga, worlds):
    """The world's call pattern with removes and restores between the calls: the ids and every layer are the model's for
    the inserts alone, new ids are alive, and the bitmap is carried across the promotion."""
    w = worlds(0)
    rw = _make_handle(ga, w.el, w.int8, w.nn, w.ms, START)
    removed = set()

    def between(call):
        n = len(rw)
        if call % 3 == 0:
            ids = [call, n - 1, n + 5]  # an early id, the newest, one not there yet
            got = rw.remove(ids)
            fresh = {i for i in ids[:2] if i not in removed}
            assert got == (len(fresh), 2 - len(fresh), 1)
            removed.update(fresh)
        if call % 7 == 6:
            back = sorted(removed)[::2]
            assert rw.restore(back) == (len(back), 0, 0)
            removed.difference_update(back)
        assert rw.removed_count() == len(removed)

    layers_before = rw.num_layers()
    assert _run_steps(rw, w.el, STEPS, between) == w.ids
    assert rw.num_layers() == layers_before + 1 == 4  # the large batch crossed a promotion
    assert removed and len(rw) == PLACES
    assert_layers_equal(rw.layers(), w.layers)
    alive = _alive(removed)
    f = rw.alive_filter()
    assert (_words(f) == fm.pack_bits(alive)).all() and f.count() == PLACES - len(removed)
    ids, ds, _cnt, st = rw.search_batch(w.q, 20, 10, stats=True)
    mi, md, _mc, mst = w.walk(alive, 20)
    assert (ids == mi[:, :10]).all() and ds.tobytes() == md[:, :10].tobytes() and (st == mst).all()
    rw.close()


def test_snapshot_under_the_alive_filter_is_the_live_search(worlds):
    w = worlds(2)
    removed = w.state("half")
    w.rw.remove(removed)
    try:
        f = w.rw.alive_filter()
        assert f.n == PLACES and (f.ids() == np.nonzero(_alive(removed))[0]).all()
        snap = w.rw.get_index()
        for ms in (20, 65, 257):
            live = w.rw.search_batch(w.q, ms, 10, stats=True)
            still = snap.search_filtered_batch(w.q, f, ms, 10, stats=True)
            for x, y in zip(live, still):
                assert x.tobytes() == y.tobytes()
        snap.close()
        f.close()
    finally:
        w.rw.restore(removed)


@pytest.mark.parametrize("ci", [0, 1])
def test_compact(ga, oracle, ci):
    dim, int8, nn, ms = CASES[ci]
    rng = np.random.default_rng(900 + ci)
    el = _prepared(oracle, random_floats(rng, PLACES, dim), int8)
    q = _prepared(oracle, random_floats(rng, NQ, dim), int8)
    cfg = {"num_neighbors": nn, "max_search": ms, "layer_multiplier": MULT}
    steps = [(0, 200), (200, PLACES - START - 10)]  # ten places stay free
    model = RwModel.new(_start_layers(oracle, el[:START], nn, ms, PLACES, True), el[:START], cfg, PLACES)
    _run_steps(model, el, steps)
    rw = _make_handle(ga, el, int8, nn, ms, START)
    _run_steps(rw, el, steps)
    n = len(rw)
    assert n == PLACES - 10
    removed = np.nonzero(rng.random(n) < 1 / 3)[0]
    alive = np.ones(n, bool)
    alive[removed] = False
    assert rw.remove(removed) == (len(removed), 0, 0)
    before = rw.search_batch(q, 20, 10, stats=True)

    new, old_ids = rw.compact()
    m = int(alive.sum())
    assert old_ids.dtype == np.uint64 and (old_ids == np.nonzero(alive)[0]).all()
    assert len(new) == m and new.removed_count() == 0 and new.max_elements == PLACES
    for i in (0, 1, m // 2, m - 1):
        assert (new.get_element(i) == el[old_ids[i]]).all()
    got = new.layers()
    fresh = _make_handle(ga, el[old_ids], int8, nn, ms, m, build_first=False)
    assert_layers_equal(got, fresh.layers())
    fresh.close()
    assert_layers_equal(got, RwModel.new(_start_layers(oracle, el[old_ids], nn, ms, PLACES, False), el[old_ids], cfg, PLACES).layers())
    assert new.insert(el[0]) == m  # it is a live handle of its own
    new.close()

    # the source is as it was
    assert len(rw) == n and rw.removed_count() == len(removed)
    assert_layers_equal(rw.layers(), model.layers())
    for x, y in zip(rw.search_batch(q, 20, 10, stats=True), before):
        assert x.tobytes() == y.tobytes()
    assert rw.insert(el[n]) == n and model.insert(el[n]) == n
    assert_layers_equal(rw.layers(), model.layers())
    assert (_words(rw.alive_filter()) == fm.pack_bits(np.append(alive, True))).all()  # the new id is alive

    # no survivors: an empty handle of the same dimension that takes inserts
    rw.remove(np.arange(len(rw)))
    empty, none = rw.compact(100)
    assert len(empty) == 0 and len(none) == 0 and empty.max_elements == 100 and empty.dim == dim
    assert empty.insert(el[3]) == 0 and (empty.get_element(0) == el[3]).all()
    empty.close()
    rw.close()


def test_searches_from_threads_see_whole_remove_calls(worlds):
    """Four threads search 8 queries 30 times each while one thread makes 8 remove calls of 10 ids: every result is the
    model's for one of the 9 alive states, and per thread the state never goes back."""
    w = worlds(0)
    rw, q = w.rw, w.q[:8]
    lead = []
    # the ids these 8 queries' answers hold, nearest first (then anything): every remove call changes answers
    for i in list(w.clean[20][0][:8].T.reshape(-1)) + list(range(PLACES)):
        if int(i) not in lead and len(lead) < 80:
            lead.append(int(i))
    groups = [lead[10 * c:10 * c + 10] for c in range(8)]
    assert all(len(g) == 10 for g in groups)
    states, gone = [], []
    for c in range(9):
        if c:
            gone += groups[c - 1]
        mi, md, mc, _ = (a[:8] for a in w.walk(_alive(gone), 20))
        assert (mc >= 10).all()
        states.append((mi[:, :10].tobytes(), md[:, :10].tobytes(), np.full(8, 10, np.uint32).tobytes()))
    assert len(set(states)) == 9
    results, errors = [[] for _ in range(4)], []

    def remover():
        try:
            for g in groups:
                assert rw.remove(g) == (10, 0, 0)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def searcher(out):
        try:
            for _ in range(30):
                i, d, cnt = rw.search_batch(q, 20, 10)
                out.append((i.tobytes(), d.tobytes(), cnt.tobytes()))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=searcher, args=(r,)) for r in results] + [threading.Thread(target=remover)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=120)
            assert not t.is_alive()
        assert not errors, errors
        for out in results:
            assert len(out) == 30
            at = 0
            for r in out:
                while at <= 8 and states[at] != r:
                    at += 1
                assert at <= 8, "a search result that is no whole-call state of the model (or an earlier one)"
        i, d, cnt = rw.search_batch(q, 20, 10)
        assert (i.tobytes(), d.tobytes(), cnt.tobytes()) == states[8]
    finally:
        rw.restore(lead)


def test_errors_leave_usable_handles(ga, worlds):
    from granne_amd import _lib
    w = worlds(1)
    rw, lib = w.rw, _lib.lib()
    counts = (C.c_uint64 * 3)(9, 9, 9)
    ids = np.array([1, 2], np.uint64)
    p = ids.ctypes.data_as(C.c_void_p)
    for fn in (lib.granne_hip_rw_builder_remove, lib.granne_hip_rw_builder_restore):
        assert fn(rw._h, None, 2, counts) == _lib.ERR_INVALID and b"ids is null" in lib.granne_hip_last_error()
        assert list(counts) == [0, 0, 0]
        assert fn(rw._h, p, 2, None) == _lib.ERR_INVALID and b"out_counts is null" in lib.granne_hip_last_error()
        assert fn(rw._h, None, 0, counts) == _lib.OK  # nothing to do needs no ids
    assert rw.removed_count() == 0
    with pytest.raises(ga.GranneHipError) as e:
        rw.compact(0)
    assert e.value.code == _lib.ERR_INVALID and "max_elements" in str(e.value)
    with pytest.raises(ga.GranneHipError) as e:
        rw.compact(2 ** 32 - 1)
    assert e.value.code == _lib.ERR_INVALID
    out, n = C.c_void_p(), C.c_uint64(5)
    assert lib.granne_hip_rw_builder_compact(rw._h, 10, C.byref(out), None, C.byref(n)) == _lib.ERR_INVALID
    assert not out.value and n.value == 0
    assert lib.granne_hip_rw_builder_alive(rw._h, None, None) == _lib.ERR_INVALID
    closed = _make_handle(ga, w.el, w.int8, w.nn, w.ms, START)
    closed.close()
    for call in (lambda: closed.remove([1]), lambda: closed.restore([1]), closed.removed_count, closed.alive_filter, closed.compact):
        with pytest.raises(ValueError):
            call()
    # the handle still answers, and removes
    for x, y in zip(rw.search_batch(w.q, 20, 10, stats=True), w.clean[20]):
        assert x.tobytes() == y.tobytes()
    assert rw.remove([4]) == (1, 0, 0) and rw.restore([4]) == (1, 0, 0)
