"""RwGranneBuilder on the GPU (granne_amd.RwGranneBuilder over granne_hip_rw_builder_*) against the CPU model of the
batched Rw schedule (tests/rw_model.py): ids, every layer row for row, live searches bit for bit, files, snapshots,
threads and the error returns.

Every case follows one insert pattern: 40 single inserts, one batch of 20, one large batch that crosses the layer
promotions that are left, then the rest plus 100 rows too many. That is two promotions in case 0, which starts empty at
multiplier 5 and 1,500 places (60 -> 300 -> 1,500 rows); the other pyramids have fewer left after 60 inserts: one in
cases 2 and 3, none in case 1 (6, 80, 1,200 rows: its promotion falls among the single inserts). The large batch runs to the last five
places, so that its sub-batches lie on both sides of the small-path threshold: 2 x members x num_neighbors ops against
RW_SMALL_OPS = 2,048 -- at 10 neighbors more than 102 members, i.e. more than 820 nodes in the layer. Case 2 (900 places
at 10 neighbors) cannot get there (a sub-batch that starts beyond 820 nodes has fewer than 80 places left), so it runs
with the threshold set to 512 ops, the option's third kind of value. How many sub-batches take which path is computed
from the model's schedule and the GPU handle's two counters must say exactly that."""
import functools
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402
from tests.rw_model import RwModel  # noqa: E402

# dim, int8, num_neighbors, max_search, multiplier, max_elements, built elements the GranneBuilder holds, small-ops option
CASES = [
    (8, False, 10, 20, 5.0, 1500, 0, 1),
    (100, False, 30, 40, 15.0, 1200, 50, 1),
    (28, True, 10, 20, 5.0, 900, 0, 512),
    (6, False, 31, 40, 5.0, 800, 50, 1),  # full rows prune and refill
]
RW_SMALL_OPS = 2048
NQ = 32


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _steps(max_elements, start):
    """(lo, hi) row ranges of the calls, relative to the first inserted row; single inserts are ranges of one."""
    steps = [(i, i + 1) for i in range(40)] + [(40, 60)]
    big_end = max_elements - start - 5
    steps.append((60, big_end))
    steps.append((big_end, max_elements - start + 100))
    return steps


@functools.lru_cache(maxsize=None)
def reference(ci):
    """The model's run of case ci, computed once: elements, start layers, per-call ids, final layers, the schedule, and
    the model's searches at the checkpoints (call index -> results of NQ queries at (20, 10) and (1, 1))."""
    from oracle import oracle
    dim, int8, nn, ms, mult, max_el, start, _opt = CASES[ci]
    rng = np.random.default_rng(1000 + ci)
    raw = random_floats(rng, max_el + 100, dim)
    el = oracle.quantize(raw) if int8 else oracle.normalize_f32(raw)
    queries = random_floats(rng, NQ, dim)
    queries = oracle.quantize(queries) if int8 else oracle.normalize_f32(queries)
    cfg = {"num_neighbors": nn, "max_search": ms, "layer_multiplier": mult}
    if start:
        # what the GranneBuilder holds (built without expected_num_elements), then RwGranneBuilder::new's build() with it set
        kw = dict(num_neighbors=nn, max_search=ms, layer_multiplier=mult, reinsert_elements=False, batch_max=65536, batch_div=8,
                  n_threads=0)
        held = oracle.build_index(el[:start], **kw)
        start_layers = oracle.build_index(el[:start], expected_num_elements=max_el, resume_from=held.layers, **kw).layers
    else:
        start_layers = []
    m = RwModel.new(start_layers, el[:start], cfg, max_el)
    steps = _steps(max_el, start)
    first_cap = m.capacity()
    checkpoints = {}
    ids, promotions = [], []

    def snap(call):
        ix = m.index()
        res = {}
        for ef, k in ((20, 10), (1, 1)):
            if ix is None:
                res[(ef, k)] = None
            else:
                i, d, c, _ = ix.search_batch(queries, ef, k)
                res[(ef, k)] = (i, d, c)
        checkpoints[call] = (len(m), res)

    for call, (lo, hi) in enumerate(steps):
        before = len(m.prev)
        ids.append(m.insert_batch(el[start + lo:start + hi]))
        promotions.append(len(m.prev) - before)
        if not start and len(m) in (first_cap, first_cap + 1):  # the last call before the first promotion, the first after
            snap(call)
        if call in (40, len(steps) - 1):  # mid-way (after the batch of 20) and full
            snap(call)
    # self-recall at max_search 20 (rw/mod.rs:299-301), the model's share
    ix = m.index()
    found, _d, _c, _ = ix.search_batch(el[:max_el], 20, 1)
    share = float((found[:, 0] == np.arange(max_el)).mean())
    return dict(el=el, queries=queries, steps=steps, ids=ids, layers=m.layers(), subs=list(m.sub_batches), promotions=promotions,
                checkpoints=checkpoints, share=share, n=len(m))


def make_rw(ga, ci, small_ops=None):
    dim, int8, nn, ms, mult, max_el, start, opt = CASES[ci]
    ref = reference(ci)
    et = "angular_int" if int8 else "angular"
    b = ga.GranneBuilder(et, ref["el"][:start] if start else None, num_neighbors=nn, max_search=ms, layer_multiplier=mult,
                         reinsert_elements=False)
    if start:
        b.build()
        assert len(b) == start  # it holds 50 built elements
    rw = ga.RwGranneBuilder(b, max_el, dim=dim)
    assert b._h is None  # consumed
    rw.set_option(ga.rw_builder.SMALL_OPS, opt if small_ops is None else small_ops)
    return rw


def run_calls(rw, ref, start, upto=None, on_call=None):
    out = []
    for call, (lo, hi) in enumerate(ref["steps"][:upto]):
        rows = ref["el"][start + lo:start + hi]
        if hi - lo == 1:
            got = rw.insert(rows[0])
            out.append([] if got is None else [got])
        else:
            out.append([int(x) for x in rw.insert_batch(rows)])
        if on_call:
            on_call(call)
    return out


def assert_layers_equal(got, want):
    assert len(got) == len(want)
    for l, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (l, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, "layer %d: %d rows differ, first %d: %s vs %s" % (l, bad.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_layers_equal_the_models(ga, ci):
    dim, int8, nn, ms, mult, max_el, start, opt = CASES[ci]
    ref = reference(ci)
    rw = make_rw(ga, ci)
    got = run_calls(rw, ref, start)
    assert got == ref["ids"]
    assert got[-1] and got[-1][-1] == max_el - 1 and len(got[-1]) == 5  # the 100 rows too many were dropped
    assert len(rw) == ref["n"] == max_el
    assert rw.insert(ref["el"][0]) is None and len(rw.insert_batch(ref["el"][:7])) == 0
    assert ref["promotions"][41] == (2, 0, 1, 1)[ci] and sum(ref["promotions"]) >= 1  # what the large batch crossed
    assert_layers_equal(rw.layers(), ref["layers"])
    # both phase B paths ran, as often as the schedule says
    thr = RW_SMALL_OPS if opt == 1 else opt
    small = sum(1 for b in ref["subs"] if 2 * b * nn <= thr)
    sorted_ = len(ref["subs"]) - small
    assert small > 0 and sorted_ > 0
    assert rw.get_option(ga.rw_builder.SMALL_LAUNCHES) == small
    assert rw.get_option(ga.rw_builder.SORTED_LAUNCHES) == sorted_
    rw.close()


@pytest.mark.parametrize("ci", [0, 3])
def test_small_path_changes_nothing(ga, ci):
    start = CASES[ci][6]
    ref = reference(ci)
    layers = []
    for small_ops in (0, 1):
        rw = make_rw(ga, ci, small_ops)
        run_calls(rw, ref, start)
        if small_ops == 0:
            assert rw.get_option(ga.rw_builder.SMALL_LAUNCHES) == 0
        else:
            assert rw.get_option(ga.rw_builder.SMALL_LAUNCHES) > 0
        layers.append(rw.layers())
        rw.close()
    assert len(layers[0]) == len(layers[1])
    for a, b in zip(*layers):
        assert a.tobytes() == b.tobytes()


def assert_search_equal(got, want, nq=NQ):
    ids, dists, counts = got
    if want is None:  # no previous layer: nothing
        assert (counts == 0).all()
        return
    wi, wd, wc = want
    assert (counts == wc).all()
    for q in range(nq):
        c = int(wc[q])
        assert (ids[q, :c] == wi[q, :c]).all(), q
        assert (dists[q, :c].view(np.uint32) == wd[q, :c].view(np.uint32)).all(), q


@pytest.mark.parametrize("ci", [0, 2])
def test_live_search_equals_the_models(ga, ci):
    start = CASES[ci][6]
    ref = reference(ci)
    cps = ref["checkpoints"]
    assert len(cps) == 4
    lens = [cps[c][0] for c in sorted(cps)]
    assert [r is None for r in (cps[c][1][(20, 10)] for c in sorted(cps))] == [True, False, False, False]
    rw = make_rw(ga, ci)
    seen = []

    def on_call(call):
        if call in cps:
            assert len(rw) == cps[call][0]
            for (ef, k), want in cps[call][1].items():
                assert_search_equal(rw.search_batch(ref["queries"], ef, k), want)
            one = rw.search(ref["queries"][0], 20, 10)
            want = cps[call][1][(20, 10)]
            assert one == ([] if want is None else [(int(want[0][0, i]), float(want[1][0, i])) for i in range(int(want[2][0]))])
            seen.append(call)

    run_calls(rw, ref, start, on_call=on_call)
    assert seen == sorted(cps) and lens == sorted(lens)
    rw.close()


def test_self_recall(ga):
    """rw/mod.rs:299-301: every inserted element finds itself first at max_search 20 -- for at least the share of
    elements for which the model's search does."""
    ref = reference(0)
    max_el = CASES[0][5]
    rw = make_rw(ga, 0)
    run_calls(rw, ref, 0)
    ids, _d, counts = rw.search_batch(ref["el"][:max_el], 20, 1)
    assert (counts == 1).all()
    share = float((ids[:, 0] == np.arange(max_el)).mean())
    assert ref["share"] >= 0.9
    assert share >= ref["share"]
    rw.close()


def test_save_and_load(ga, tmp_path):
    ref = reference(2)
    rw = make_rw(ga, 2)
    run_calls(rw, ref, 0, upto=42)
    ip, ep = str(tmp_path / "index.granne"), str(tmp_path / "elements.bin")
    rw.save(ip, ep)
    ix = ga.Granne.from_files(ip, "angular_int", ep)
    assert len(ix) == len(rw) and ix.num_layers() == rw.num_layers()
    for ef, k in ((20, 10), (1, 1)):
        a, b = ix.search_batch(ref["queries"], ef, k), rw.search_batch(ref["queries"], ef, k)
        assert (a[2] == b[2]).all() and (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all()
    assert (ix.get_element(17) == rw.get_element(17)).all() and (rw.get_element(17) == ref["el"][17]).all()
    ix.close()
    rw.close()
    # an empty builder writes zero layers
    empty = ga.RwGranneBuilder(ga.GranneBuilder("angular", None, num_neighbors=10, max_search=20), 100, dim=8)
    assert len(empty) == 0 and empty.search(np.ones(8, np.float32), 20, 5) == []
    empty.save(ip, ep)
    ix = ga.Granne.from_files(ip, "angular", ep)
    assert ix.num_layers() == 0 and len(ix) == 0
    assert os.path.getsize(ep) == 8
    ix.close()
    empty.close()


def test_get_index_is_a_snapshot(ga):
    ref = reference(0)
    rw = make_rw(ga, 0)
    run_calls(rw, ref, 0, upto=41)
    snap = rw.get_index()
    live = rw.search_batch(ref["queries"], 20, 10)
    before = snap.search_batch(ref["queries"], 20, 10)
    assert len(snap) == len(rw) == 60
    assert_search_equal(before, live)
    rw.insert_batch(ref["el"][60:400])
    after = snap.search_batch(ref["queries"], 20, 10)
    assert len(snap) == 60
    assert_search_equal(after, before)
    assert (rw.search_batch(ref["queries"], 20, 10)[0] != live[0]).any()  # the live graph has moved on
    snap.close()
    rw.close()


def test_searches_from_threads_see_whole_insert_calls(ga, oracle):
    """One thread inserts 30 batches of 16 while three threads search 8 fixed queries in a loop: every result is the
    model's for one of the 31 graph states, and per thread the matched state never goes back."""
    dim, nn, ms, mult, max_el, start, calls = 8, 10, 20, 5.0, 600, 100, 30
    rng = np.random.default_rng(77)
    el = oracle.normalize_f32(random_floats(rng, start + calls * 16, dim))
    queries = oracle.normalize_f32(random_floats(rng, 8, dim))
    kw = dict(num_neighbors=nn, max_search=ms, layer_multiplier=mult, reinsert_elements=False, batch_max=65536, batch_div=8,
              n_threads=0)
    start_layers = oracle.build_index(el[:start], expected_num_elements=max_el, **kw).layers
    m = RwModel.new(start_layers, el[:start], {"num_neighbors": nn, "max_search": ms, "layer_multiplier": mult}, max_el)
    states = []
    for c in range(calls + 1):
        if c:
            m.insert_batch(el[start + (c - 1) * 16:start + c * 16])
        i, d, cnt, _ = m.index().search_batch(queries, 20, 10)
        states.append((i.tobytes(), d.tobytes(), cnt.tobytes()))

    b = ga.GranneBuilder("angular", el[:start], num_neighbors=nn, max_search=ms, layer_multiplier=mult, reinsert_elements=False,
                         expected_num_elements=max_el)
    rw = ga.RwGranneBuilder(b, max_el)
    done = threading.Event()
    results = [[] for _ in range(3)]
    errors = []

    def inserter():
        try:
            for c in range(calls):
                assert len(rw.insert_batch(el[start + c * 16:start + (c + 1) * 16])) == 16
        except Exception as e:  # noqa: BLE001
            errors.append(e)
        finally:
            done.set()

    def searcher(out):
        try:
            while True:
                last = done.is_set()
                i, d, cnt = rw.search_batch(queries, 20, 10)
                out.append((i.tobytes(), d.tobytes(), cnt.tobytes()))
                if last or len(out) > 100000:
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=inserter)] + [threading.Thread(target=searcher, args=(r,)) for r in results]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
        assert not t.is_alive()
    assert not errors, errors
    for out in results:
        assert out
        at = 0
        for r in out:
            while at <= calls and states[at] != r:
                at += 1
            assert at <= calls, "a search result that is no whole-call state of the model (or an earlier one)"
        assert out[-1] == states[calls]  # the search begun after the last insert sees all of it
    assert_layers_equal(rw.layers(), m.layers())
    rw.close()


def test_errors_leave_usable_handles(ga, oracle):
    from granne_amd import _lib
    import ctypes as C
    rng = np.random.default_rng(3)
    el = oracle.normalize_f32(random_floats(rng, 60, 8))
    b = ga.GranneBuilder("angular", el[:30], num_neighbors=10, max_search=20, layer_multiplier=5.0, reinsert_elements=False)
    with pytest.raises(ga.GranneHipError) as e:
        ga.RwGranneBuilder(b, 0)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ga.GranneHipError) as e:
        ga.RwGranneBuilder(b, 2 ** 32 - 1)
    assert e.value.code == _lib.ERR_INVALID
    b.build()  # the builder is still the caller's, and works
    assert len(b) == 30
    se = ga.SumEmbeddings(random_floats(rng, 20, 8), [[i % 20, (i * 7) % 20] for i in range(40)])
    sb = ga.GranneBuilder("embeddings", se, num_neighbors=10, max_search=20)
    with pytest.raises(ga.GranneHipError) as e:
        ga.RwGranneBuilder(sb, 100)
    assert e.value.code == _lib.ERR_INVALID and "SumEmbeddings" in str(e.value)
    sb.build()
    assert len(sb) == 40
    sb.close()
    rw = ga.RwGranneBuilder(b, 100)
    assert len(rw) == 30
    count = C.c_uint64(5)
    ids = np.zeros(4, np.uint64)
    rc = _lib.lib().granne_hip_rw_builder_insert_batch(rw._h, None, 4, ids.ctypes.data_as(C.c_void_p), C.byref(count))
    assert rc == _lib.ERR_INVALID and count.value == 0 and len(rw) == 30
    with pytest.raises(ValueError):
        rw.insert_batch(np.zeros((2, 9), np.float32))  # dimension mismatch, caught in the Python layer
    with pytest.raises(ValueError):
        rw.search(np.zeros(7, np.float32))
    assert [int(x) for x in rw.insert_batch(el[30:34])] == [30, 31, 32, 33]  # the handle still works
    assert rw.insert(el[34]) == 35 - 1 and len(rw) == 35
    rw.close()
