"""GRANNE_HIP_OPT_COALESCE on the GPU: host calls that are inside the library at the same moment share search launches
(granne_amd/csrc/combiner.h), and no caller can tell -- ids, distance bits, counts, counters and statuses are those of
the calls made alone, i.e. the oracle's.

Every thread is joined with a timeout and a thread still alive fails the test: a combiner bug must fail, not hang.

Run on the MI355X box: python -m pytest tests -m gpu
"""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import assert_counters, random_floats  # noqa: E402

JOIN_SECONDS = 60.0
WAIT_US = 5_000_000  # the issue's wait for the deterministic groups: a group that fills leaves long before it


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    from granne_amd import _lib, build
    assert os.path.exists(build.LIB_PATH), "libgranne_hip.so must be built in-tree (python -m granne_amd.build)"
    _lib.lib()
    return granne_amd


class Case:
    """One index shape: its elements, the oracle's index, a pool of queries and the oracle's answers, made once."""

    def __init__(self, oracle, element_type, n, dim, seed):
        rng = np.random.default_rng(seed)
        int8 = element_type == "angular_int"
        prep = oracle.quantize if int8 else oracle.normalize_f32
        self.element_type = element_type
        self.el = prep(random_floats(rng, n, dim))
        self.oix = oracle.build_index(self.el, num_neighbors=20, max_search=20, reinsert_elements=False, n_threads=0)
        self.q = prep(random_floats(rng, 300, dim))
        self._want = {}

    def want(self, max_search, k):
        """(ids, dists, counts, counters) of the whole pool; computed once per key and never written to."""
        key = (max_search, k)
        if key not in self._want:
            self._want[key] = self.oix.search_batch(self.q, max_search, k)
        return self._want[key]

    def index(self, ga, coalesce=False):
        gix = ga.Granne(self.element_type, self.el, self.oix.layers)
        gix.search_batch(self.q[:2], 40, 10)  # the walker's code is loaded before anything is timed or counted
        gix.coalesce = coalesce
        return gix


@pytest.fixture(scope="module")
def f32(oracle):
    """6,000 x 100-d f32, num_neighbors 20: the shape of test_concurrent_searches_on_a_shared_index"""
    return Case(oracle, "angular", 6000, 100, 19)


@pytest.fixture(scope="module")
def i8(oracle):
    return Case(oracle, "angular_int", 3000, 32, 23)


def run_threads(fns):
    """Runs every callable on a thread of its own; returns what each returned. A thread that raised, or that is still
    alive after JOIN_SECONDS, fails the test."""
    out, err = [None] * len(fns), [None] * len(fns)

    def body(i):
        try:
            out[i] = fns[i]()
        except BaseException as e:  # noqa: BLE001 (reported below, on the test's thread)
            err[i] = e

    th = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(fns))]
    deadline = time.monotonic() + JOIN_SECONDS
    [t.start() for t in th]
    for t in th:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in th), "a search call did not return: %s" % [t.is_alive() for t in th]
    for e in err:
        if e is not None:
            raise e
    return out


def raw_search(gix, q, max_search, k, stats=True, single=False):
    """The C ABI itself: (status, ids, dists, counts, stats or None). single=True: granne_hip_search (one query)."""
    from granne_amd._lib import lib
    nq = q.shape[0]
    ids = np.full((nq, max(k, 1)), 7, np.uint64)
    ds = np.full((nq, max(k, 1)), 7, np.float32)
    cnt = np.full(nq, 7, np.uint32)
    st = np.zeros((nq, 3), np.uint64) if stats else None
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if single:
        assert nq == 1
        rc = lib().granne_hip_search(gix._h, p(q), max_search, k, p(ids), p(ds), cnt.ctypes.data_as(C.POINTER(C.c_uint32)))
    else:
        rc = lib().granne_hip_search_batch(gix._h, p(q), nq, max_search, k, p(ids), p(ds), p(cnt), p(st) if stats else None)
    return rc, ids[:, :k], ds[:, :k], cnt, st


def assert_rows(case, first, got, max_search, k, exact_counters=None):
    """rows first .. of the pool: ids, distance bits, counts (and counters when asked) are the oracle's"""
    rc, ids, ds, cnt, st = got
    oi, od, oc, octr = case.want(max_search, k)
    assert rc == 0
    n = ids.shape[0]
    assert (cnt == oc[first:first + n]).all(), (cnt, oc[first:first + n])
    for i in range(n):
        c = int(cnt[i])
        assert ids[i, :c].tolist() == oi[first + i, :c].tolist(), (first + i, ids[i, :c], oi[first + i, :c])
        assert ds[i, :c].tobytes() == od[first + i, :c].tobytes(), (first + i, ds[i, :c], od[first + i, :c])
        assert (ids[i, c:] == np.iinfo(np.uint64).max).all() and np.isinf(ds[i, c:]).all()
    if exact_counters is not None and st is not None:
        assert_counters(st, octr[first:first + n], exact=exact_counters)


def counters(gix):
    from granne_amd import _lib
    return gix.get_option(_lib.OPT_COALESCED_LAUNCHES), gix.get_option(_lib.OPT_COALESCED_QUERIES)


def barrier_calls(gix, case, specs):
    """One thread per (first row, nq, max_search, k): all leave a barrier together, then each makes its one call."""
    bar = threading.Barrier(len(specs))

    def call(first, nq, max_search, k):
        bar.wait(JOIN_SECONDS)
        return raw_search(gix, case.q[first:first + nq], max_search, k)

    return run_threads([lambda s=s: call(*s) for s in specs])


def test_option_basics(ga, f32):
    """Off by default; set and read back; off means the two counters stay 0 whatever is searched."""
    from granne_amd import _lib
    from granne_amd._lib import GranneHipError
    gix = f32.index(ga)
    assert gix.get_option(_lib.OPT_COALESCE) == 0 and gix.coalesce is False
    assert gix.get_option(_lib.OPT_COALESCE_MAX) == 1024 == _lib.COALESCE_MAX
    assert gix.get_option(_lib.OPT_COALESCE_WAIT_US) == 0
    assert_rows(f32, 0, raw_search(gix, f32.q[:1], 40, 10), 40, 10)
    run_threads([lambda i=i: assert_rows(f32, i, raw_search(gix, f32.q[i:i + 1], 40, 10), 40, 10) for i in range(4)])
    assert counters(gix) == (0, 0)
    gix.coalesce = True
    assert gix.get_option(_lib.OPT_COALESCE) == 1 and gix.coalesce is True
    gix.set_option(_lib.OPT_COALESCE_MAX, 8)
    gix.set_option(_lib.OPT_COALESCE_WAIT_US, 123)
    assert gix.get_option(_lib.OPT_COALESCE_MAX) == 8 and gix.get_option(_lib.OPT_COALESCE_WAIT_US) == 123
    for opt, bad in ((_lib.OPT_COALESCE, 2), (_lib.OPT_COALESCE_MAX, 0), (_lib.OPT_COALESCE_MAX, 1025),
                     (_lib.OPT_COALESCED_LAUNCHES, 0), (_lib.OPT_COALESCED_QUERIES, 5)):
        with pytest.raises(GranneHipError) as e:
            gix.set_option(opt, bad)
        assert e.value.code == _lib.ERR_INVALID
    gix.coalesce = False
    assert gix.get_option(_lib.OPT_COALESCE) == 0
    kw = ga.Granne("angular", f32.el[:64], [], coalesce=True)
    assert kw.coalesce is True
    assert _lib.lib().granne_hip_abi_version() == 3


def deterministic_group(ga, case, force_slow):
    from granne_amd import _lib
    gix = case.index(ga, coalesce=True)
    gix.set_option(_lib.OPT_COALESCE_MAX, 8)
    gix.set_option(_lib.OPT_COALESCE_WAIT_US, WAIT_US)
    if force_slow:
        gix.set_option(_lib.OPT_FORCE_SLOW, 1)
    t0 = time.monotonic()
    got = barrier_calls(gix, case, [(11 * i, 1, 40, 10) for i in range(8)])
    wall = time.monotonic() - t0
    assert counters(gix) == (1, 8)
    for i in range(8):
        assert_rows(case, 11 * i, got[i], 40, 10)
    assert wall < WAIT_US / 1e6 / 2, wall  # the cap let the group go, not the timer
    return gix


def test_eight_callers_share_one_launch(ga, f32):
    """COALESCE_MAX 8 under a wait of 5 s: eight threads behind a barrier make one launch of eight queries."""
    deterministic_group(ga, f32, force_slow=False)


def test_exact_walker_serves_a_group(ga, i8):
    """The same group on the int8 index with FORCE_SLOW: the exact walker's scratch is the group's, and so is the
    count of queries it served."""
    from granne_amd import _lib
    gix = deterministic_group(ga, i8, force_slow=True)
    assert gix.last_slow_count() == 8
    assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_EXACT


def test_two_keys_never_share_a_launch(ga, f32):
    """Four callers of (40, 10) and four of (20, 5) under the same cap of 8 and wait of 5 s: each key gets a leader
    and a launch of its own. Neither group of four can reach the cap, so this test lasts as long as the wait (both
    leaders wait at the same time)."""
    from granne_amd import _lib
    gix = f32.index(ga, coalesce=True)
    gix.set_option(_lib.OPT_COALESCE_MAX, 8)
    gix.set_option(_lib.OPT_COALESCE_WAIT_US, WAIT_US)
    specs = [(7 * i, 1, 40, 10) if i % 2 == 0 else (7 * i, 1, 20, 5) for i in range(8)]
    got = barrier_calls(gix, f32, specs)
    for s, g in zip(specs, got):
        assert_rows(f32, s[0], g, s[2], s[3])
    launches, queries = counters(gix)
    assert queries == 8 and launches >= 2


def test_free_running_callers(ga, f32):
    """No wait: 16 threads x 50 calls of nq 1 and nq 3 mixed, every third without stats. Whatever groups form (that is
    timing, and not asserted), every call gets the oracle's rows; with the exact visited set n_dist is the oracle's too."""
    from granne_amd import _lib
    gix = f32.index(ga, coalesce=True)
    gix.set_option(_lib.OPT_VISITED16, 1)
    T, N = 16, 50
    issued = [0] * T

    def work(t):
        for j in range(N):
            c = t * N + j
            nq = 3 if c % 4 == 1 else 1
            first = (c * 5) % (f32.q.shape[0] - 3)
            assert_rows(f32, first, raw_search(gix, f32.q[first:first + nq], 40, 10, stats=c % 3 != 0), 40, 10, exact_counters=True)
            issued[t] += nq

    run_threads([lambda t=t: work(t) for t in range(T)])
    launches, queries = counters(gix)
    assert queries == sum(issued) and 1 <= launches <= T * N


def test_large_calls_bypass_the_combiner(ga, f32):
    from granne_amd import _lib
    gix = f32.index(ga, coalesce=True)
    before = counters(gix)
    assert_rows(f32, 0, raw_search(gix, f32.q[:300], 40, 10), 40, 10)
    assert_rows(f32, 0, raw_search(gix, f32.q[:_lib.COALESCE_CALL_MAX + 1], 40, 10), 40, 10)
    assert counters(gix) == before == (0, 0)
    assert_rows(f32, 0, raw_search(gix, f32.q[:_lib.COALESCE_CALL_MAX], 40, 10), 40, 10)  # the largest call that takes part
    assert counters(gix) == (1, _lib.COALESCE_CALL_MAX)


def test_one_bad_caller_among_good_ones(ga, f32):
    """Argument errors are decided before a call queues and belong to that caller alone: of eight callers one passes
    max_search = 0; the seven others fill a cap of 7 (the bad call never counts towards a group) and leave together."""
    from granne_amd import _lib
    gix = f32.index(ga, coalesce=True)
    gix.set_option(_lib.OPT_COALESCE_MAX, 7)
    gix.set_option(_lib.OPT_COALESCE_WAIT_US, WAIT_US)
    t0 = time.monotonic()
    got = barrier_calls(gix, f32, [(13 * i, 1, 0 if i == 3 else 40, 10) for i in range(8)])
    assert time.monotonic() - t0 < WAIT_US / 1e6 / 2
    for i in range(8):
        if i == 3:
            assert got[i][0] == _lib.ERR_INVALID and (got[i][3] == 7).all()  # nothing written
        else:
            assert_rows(f32, 13 * i, got[i], 40, 10)
    assert counters(gix) == (1, 7)
    rc, _ids, _ds, cnt, _st = raw_search(gix, f32.q[:2], 40, 0)  # .take(0): no launch, counts 0
    assert rc == 0 and (cnt == 0).all() and counters(gix) == (1, 7)
    null = _lib.lib().granne_hip_search_batch(gix._h, None, 1, 40, 10, None, None, None, None)
    assert null == _lib.ERR_INVALID and counters(gix) == (1, 7)


def test_single_query_entry_point(ga, f32):
    """granne_hip_search -- Granne::search itself, what granne.hpp's and the Rust wrapper's `search` call -- goes
    through the combiner: a lone caller is a group of one, with no wait."""
    gix = f32.index(ga, coalesce=True)
    for i in (0, 5):
        assert_rows(f32, i, raw_search(gix, f32.q[i:i + 1], 40, 10, stats=False, single=True), 40, 10)
    assert counters(gix) == (2, 2)
    assert [(int(a), float(b)) for a, b in zip(f32.want(40, 10)[0][9], f32.want(40, 10)[1][9])][:int(f32.want(40, 10)[2][9])] \
        == gix.search(f32.q[9], 40, 10)
    assert counters(gix) == (3, 3)
