"""The exact selection on a partitioned index (granne_hip_sharded_exact_topk*, ShardedHost.exact_topk / exact_topk_filtered)
against tests/sharded_filter_model.expected_exact: the oracle's scan over the allowed rows of the CONCATENATED set, which
knows nothing of shards -- ids, distance bytes, counts and the fill past the count. The shards are handles without layers
(the selection reads rows only). tests/README_sharded_filtered.md says what each test pins."""
import ctypes as C

import numpy as np
import pytest

from tests import exact_topk_filtered_model as etm
from tests import exact_topk_model as em
from tests import filter_model as fm
from tests import sharded_filter_model as sm

pytestmark = pytest.mark.gpu

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _host(el, lengths, int8, groups=None):
    import granne_amd
    from granne_amd.sharded import ShardedHost
    offs = sm.offsets(lengths)
    gixs = [granne_amd.Granne("angular_int" if int8 else "angular", np.ascontiguousarray(el[o:o + n]), []) for o, n in zip(offs, lengths)]
    return ShardedHost(gixs, offs, groups=groups)


@pytest.fixture(scope="module")
def worlds(oracle):
    made = {}

    def get(int8):
        if int8 not in made:
            el, q = sm.fixture_rows(oracle, int8)
            made[int8] = (el, q, _host(el, sm.LENGTHS, int8))
        return made[int8]

    return get


def assert_equal(got, want):
    assert (got[2] == want[2]).all()
    assert (got[0] == want[0]).all()
    assert got[1].tobytes() == want[1].tobytes()  # (the fill past the count included: UINT64_MAX / +inf)


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("k", [1, 17, 100, 819])  # 819: the largest k five shards can merge
def test_plain_and_shared_filters_equal_the_scan_over_the_whole_set(worlds, oracle, int8, k):
    el, q, h = worlds(int8)
    got = h.exact_topk(q, k, stats=True)
    assert_equal(got, sm.expected_exact(oracle, el, np.ones(sm.N, bool), q, k))
    assert got[3][0] == 0 and got[3][3] == 0
    for name, mask in etm.shared_filters(np.random.default_rng(k), sm.N, k).items():
        got = h.exact_topk_filtered(q, k, mask, stats=True)
        assert_equal(got, sm.expected_exact(oracle, el, mask, q, k))
        assert got[3][0] == 0 and got[3][3] == int(mask.sum()), name  # the allowed ids of the whole set


@pytest.mark.parametrize("int8", [False, True])
def test_per_query_filters(worlds, oracle, int8):
    el, q, h = worlds(int8)
    mask = np.random.default_rng(21).random((sm.NQ, sm.N)) < 0.3
    mask[0] = False
    mask[1] = False
    mask[1, [30, 31, 63, 64, 4036]] = True  # fewer than k, across word and shard borders
    got = h.exact_topk_filtered(q, 17, mask, stats=True)
    assert_equal(got, sm.expected_exact(oracle, el, mask, q, 17))
    assert got[2][0] == 0 and got[2][1] == 5 and got[3][0] == 0


@pytest.mark.parametrize("int8", [False, True])
def test_fewer_than_k_allowed_all_in_one_shard(worlds, oracle, int8):
    el, q, h = worlds(int8)
    mask = etm.only(sm.N, [1001, 1500, 1999, 2000, 1002])  # the fourth shard's first and last ids among them
    got = h.exact_topk_filtered(q, 17, mask, stats=True)
    assert_equal(got, sm.expected_exact(oracle, el, mask, q, 17))
    assert (got[2] == 5).all() and (got[0][:, 5:] == NONE).all() and np.isinf(got[1][:, 5:]).all() and got[3][3] == 5


@pytest.mark.parametrize("int8", [False, True])
def test_ties_across_shards_come_in_global_id_order(oracle, int8):
    el, q = sm.fixture_rows(oracle, int8)
    el = el.copy()
    el[40] = el[1500] = el[3000] = el[5]  # one row in four shards
    q = q.copy()
    q[0] = el[5]
    h = _host(el, sm.LENGTHS, int8)
    got = h.exact_topk(q, 17)
    assert list(got[0][0, :4]) == [5, 40, 1500, 3000] and len(set(got[1][0, :4].tobytes()[i:i + 4] for i in range(0, 16, 4))) == 1
    assert_equal(got, sm.expected_exact(oracle, el, np.ones(sm.N, bool), q, 17))
    mask = np.ones(sm.N, bool)
    mask[40] = False
    assert_equal(h.exact_topk_filtered(q, 17, mask), sm.expected_exact(oracle, el, mask, q, 17))
    h.close()


@pytest.mark.parametrize("groups", [[0, 0, 1, 1, 2], [0, 1, 2, 3, 4]])
def test_exchange_groups(worlds, oracle, groups):
    """the overflow flags travel with the block through the peer copies; the filter is copied and sliced per group"""
    el, q, _ = worlds(True)
    h = _host(el, sm.LENGTHS, True, groups)
    mask = np.random.default_rng(22).random(sm.N) < 0.5
    assert_equal(h.exact_topk_filtered(q, 17, mask), sm.expected_exact(oracle, el, mask, q, 17))
    assert_equal(h.exact_topk(q, 100), sm.expected_exact(oracle, el, np.ones(sm.N, bool), q, 100))
    pq = np.random.default_rng(23).random((sm.NQ, sm.N)) < 0.3
    assert_equal(h.exact_topk_filtered(q, 17, pq), sm.expected_exact(oracle, el, pq, q, 17))
    h.close()


def test_a_query_that_overflows_in_one_shard_is_voided_not_answered_in_part(oracle):
    """5,000 copies of one row in the middle shard, query 0 = that row, k 10: its selection overflows there (more than 4096
    rows inside one second-level bin at its k-th distance). The merged result must not be the other shards' rows."""
    import granne_amd
    from granne_amd import _lib
    rng = np.random.default_rng(31)
    lengths = [500, 5300, 700]
    el = oracle.normalize_f32((rng.random((sum(lengths), 32), dtype=np.float32) - np.float32(0.5)).astype(np.float32))
    el[600:5600] = el[600]
    q = oracle.normalize_f32((rng.random((8, 32), dtype=np.float32) - np.float32(0.5)).astype(np.float32))
    q[0] = el[600]
    q[1:] = oracle.normalize_f32(-q[0][None, :] + np.float32(0.3) * q[1:])  # far from the copies, in every shard
    # the model's verdict, shard by shard: only query 0 overflows, and only in the middle shard
    over = [[em.select(em.all_dists(oracle, el[o:o + n], qi), 10)[2] for qi in q] for o, n in zip(sm.offsets(lengths), lengths)]
    assert over[1][0] and sum(map(sum, over)) == 1
    h = _host(el, lengths, False)
    n = sum(lengths)
    for mask in (None, np.ones(n, bool)):
        got = h.exact_topk(q, 10, stats=True) if mask is None else h.exact_topk_filtered(q, 10, mask, stats=True)
        assert got[3][0] == 1
        assert got[2][0] == 0 and (got[0][0] == NONE).all() and np.isinf(got[1][0]).all()
        want = sm.expected_exact(oracle, el, np.ones(n, bool), q, 10)
        assert_equal(tuple(a[1:] for a in got[:3]), tuple(a[1:] for a in want))  # every other query is still right
        with pytest.raises(granne_amd.GranneHipError) as e:
            h.exact_topk(q, 10) if mask is None else h.exact_topk_filtered(q, 10, mask)
        assert e.value.code == _lib.ERR_OVERFLOW
    # the host form: ERR_OVERFLOW with the outputs written
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ids, ds, cnt, st = np.zeros((8, 10), np.uint64), np.zeros((8, 10), np.float32), np.ones(8, np.uint32), np.zeros(4, np.uint32)
    assert _lib.lib().granne_hip_sharded_exact_topk(h._h, p(q), 8, 10, p(ids), p(ds), p(cnt), p(st)) == _lib.ERR_OVERFLOW
    assert st[0] == 1 and cnt[0] == 0 and (ids[0] == NONE).all()
    assert_equal((ids[1:], ds[1:], cnt[1:]), tuple(a[1:] for a in want))
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_host_entries_and_refusals(worlds, oracle, int8):
    from granne_amd import _lib
    el, q, h = worlds(int8)
    lib = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    mask = np.random.default_rng(24).random(sm.N) < 0.1
    words = fm.pack_bits(mask)
    for nq in (sm.NQ, 3, sm.NQ):  # other batch sizes on one handle
        qq = np.ascontiguousarray(q[:nq])
        ids, ds, cnt, st = np.zeros((nq, 17), np.uint64), np.zeros((nq, 17), np.float32), np.zeros(nq, np.uint32), np.ones(4, np.uint32)
        _lib.check(lib.granne_hip_sharded_exact_topk_filtered(h._h, p(qq), nq, 17, p(words), 0, p(ids), p(ds), p(cnt), p(st)))
        assert_equal((ids, ds, cnt), sm.expected_exact(oracle, el, mask, qq, 17))
        assert st[0] == 0 and st[3] == int(mask.sum())
        _lib.check(lib.granne_hip_sharded_exact_topk(h._h, p(qq), nq, 17, p(ids), p(ds), p(cnt), None))
        assert_equal((ids, ds, cnt), sm.expected_exact(oracle, el, np.ones(sm.N, bool), qq, 17))
    ids, ds, cnt = np.zeros((sm.NQ, 1024), np.uint64), np.zeros((sm.NQ, 1024), np.float32), np.zeros(sm.NQ, np.uint32)
    assert lib.granne_hip_sharded_exact_topk(h._h, p(q), sm.NQ, 0, p(ids), p(ds), p(cnt), None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk(h._h, p(q), sm.NQ, 1025, p(ids), p(ds), p(cnt), None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk(h._h, p(q), sm.NQ, 820, p(ids), p(ds), p(cnt), None) == _lib.ERR_INVALID  # 5 x 820 > 4096
    assert b"4096" in lib.granne_hip_last_error()
    assert lib.granne_hip_sharded_exact_topk_filtered(h._h, p(q), sm.NQ, 17, None, 0, p(ids), p(ds), p(cnt), None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk_filtered(h._h, p(q), sm.NQ, 17, p(words), len(words) - 1, p(ids), p(ds), p(cnt),
                                                      None) == _lib.ERR_INVALID
    assert lib.granne_hip_sharded_exact_topk(h._h, p(q), 0, 17, None, None, None, None) == _lib.OK  # nq == 0 does nothing
