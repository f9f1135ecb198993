"""exact_topk_filtered (granne_amd/csrc/exact_topk_filtered.h) against the CPU oracle: every case compares the WHOLE ids
array, the distance bytes and the counts with the oracle's scan of the allowed subset -- oracle.Index(el[allowed],
[]).scan_topk, its ids mapped through the ascending allowed list (tests/exact_topk_filtered_model.py, which also holds the
shapes, the filters and the inputs shared with tests/test_exact_topk_filtered_model.py). No tolerance anywhere.

Shared filters run the list form (status[3] == the number of allowed ids, asserted every time), one Filter per query the
bit-tested form (status[3] stays 0). Filters are handed over as words with the bits at positions >= n SET
(Filter.from_words): such bits are never returned and never counted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_filtered_model as fm  # noqa: E402
from tests import exact_topk_model as m  # noqa: E402
from tests import high_ids  # noqa: E402

NONE = fm.NONE


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def _filter(ga, mask):
    return ga.Filter.from_words(fm.words(mask, garbage_past_n=True), len(mask))


def check_shared(ga, oracle, ix, el, q, k, mask, allowed=None):
    """exact_topk_filtered under one filter for all queries against the oracle's scan of the subset; returns the status"""
    ids, ds, cnt, st = ix.exact_topk_filtered(q, k, _filter(ga, mask) if allowed is None else allowed, stats=True)
    oi, od, oc = fm.oracle_subset(oracle, el, mask, q, k)
    t = min(k, int(mask.sum()))
    assert (cnt == oc).all() and (cnt == t).all()
    assert (ids == oi).all(), np.nonzero((ids != oi).any(axis=1))[0][:5]
    assert ds.tobytes() == od.tobytes()
    assert (ids[:, t:] == NONE).all() and np.isinf(ds[:, t:]).all()
    assert st[0] == 0 and st[3] == int(mask.sum()) and t <= st[2] <= m.CAP
    return st


@pytest.mark.parametrize("case", fm.CASES, ids=[fm.case_id(c) for c in fm.CASES])
def test_shared_filters_equal_the_oracle_on_the_subset(ga, oracle, case):
    int8, dim, n, nq, k = case
    el, q, filters = fm.case_input(oracle, case)
    ix = ga.Granne(_et(el), el, [])
    assert ix.num_elements() == n and len(ix) == 0  # a handle without layers: all rows are candidates
    for name, mask in filters.items():
        if name == "ones":  # exact_topk's answer bit for bit, with no oracle between them
            ids, ds, cnt, st = ix.exact_topk_filtered(q, k, _filter(ga, mask), stats=True)
            ei, ed, ec, est = ix.exact_topk(q, k, stats=True)
            assert (ids == ei).all() and ds.tobytes() == ed.tobytes() and (cnt == ec).all()
            assert st[3] == n and (st[:3] == est[:3]).all()
            if nq > 65:
                continue  # (the oracle's scan of all rows for 1100 queries: exact_topk's own tests compare it)
        st = check_shared(ga, oracle, ix, el, q, k, mask)
        if name == "none":
            assert st[2] == 0 and st[1] == 0
    ix.close()


def test_allowed_takes_what_search_filtered_takes(ga, oracle):
    rng = np.random.default_rng(41)
    el, q = m.unit_rows(oracle, rng, 4037, 100), m.unit_rows(oracle, rng, 3, 100)
    mask = fm.random_mask(rng, 4037, 0.1)
    ix = ga.Granne("angular", el, [])
    check_shared(ga, oracle, ix, el, q, 17, mask, allowed=mask)  # a bool array
    check_shared(ga, oracle, ix, el, q, 17, mask, allowed=np.nonzero(mask)[0])  # an id array
    check_shared(ga, oracle, ix, el, q, 17, mask, allowed=ga.Filter.from_mask(mask))
    ids, ds, cnt = ix.exact_topk_filtered(q[0], 17, mask)  # one query, no stats
    assert ids.shape == (1, 17) and (ids == fm.oracle_subset(oracle, el, mask, q[:1], 17)[0]).all()
    with pytest.raises(ValueError):
        ix.exact_topk_filtered(q, 17, mask[:-1])
    with pytest.raises(ValueError):
        ix.exact_topk_filtered(q, 17, ga.Filter.from_mask(mask[:-1]))
    with pytest.raises(ValueError):
        ix.exact_topk_filtered(q[:, :99], 17, mask)
    ix.close()


@pytest.mark.parametrize("int8", [False, True], ids=["f32", "i8"])
def test_stage_rule_under_a_device_side_count(ga, oracle, int8):
    """n = 40009: prefixes 16384, then n. m = 300 and m = 16384 exactly: the second stage is idle and the first is final;
    m = 16385 and 30000: both stages live; m = n - 1. status[3] == m each time."""
    rng = np.random.default_rng(42)
    n, dim, nq = 40009, 32, 5
    if int8:
        el = np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
        q = np.ascontiguousarray(el[rng.choice(n, nq)])
    else:
        el = m.unit_rows(oracle, rng, n, dim)
        q = m.unit_rows(oracle, rng, nq, dim)
    assert fm.prefixes(n) == [16384, n]
    ix = ga.Granne(_et(el), el, [])
    for count in (300, 16384, 16385, 30000, n - 1):
        mask = fm.exactly(rng, n, count)
        assert [s[1:] for s in fm.stages(n, count)] == ([(True, True), (False, False)] if count <= 16384 else [(True, False), (True, True)])
        for k in (17, 1024):
            st = check_shared(ga, oracle, ix, el, q, k, mask)
            assert st[3] == count
    ix.close()


def test_ties_come_in_global_id_order(ga, oracle):
    rng = np.random.default_rng(21)
    el = m.tripled(m.unit_rows(oracle, rng, 1200, 32))
    q = m.unit_rows(oracle, rng, 9, 32)
    q[8] = 0  # a zero query: every distance exactly 1.0
    mask = np.arange(3600) >= 1200  # copies 2 and 3 only
    ix = ga.Granne("angular", el, [])
    for k in (1, 17, 100, 1024):
        check_shared(ga, oracle, ix, el, q, k, mask)
    ids, ds, cnt = ix.exact_topk_filtered(q, 100, mask)
    assert (ids >= 1200).all()
    assert (ids[:8, 1::2] == ids[:8, 0::2] + 1200).all() and (ds[:, 0::2] == ds[:, 1::2]).all()
    assert (ids[8] == np.arange(1200, 1300)).all() and (ds[8] == 1.0).all()
    ix.close()
    el, q = m.copies_of_the_nearest(oracle, np.random.default_rng(22))
    mask = np.ones(len(el), bool)
    mask[501:3500:2] = False  # every second copy
    ix = ga.Granne("angular", el, [])
    st = check_shared(ga, oracle, ix, el, q, 100, mask)
    ids, _, _ = ix.exact_topk_filtered(q, 100, mask)
    assert (ids[0] == np.arange(500, 700, 2)).all()
    assert 1500 <= st[2] <= 1510 and st[1] == 0  # every allowed copy ranked, by the first level
    ix.close()


PER_QUERY = [(False, 32, 17), (False, 100, 100), (True, 100, 17), (True, 300, 1024), (False, 333, 17)]


@pytest.mark.parametrize("int8,dim,k", PER_QUERY, ids=["%s-%d-k%d" % ("i8" if c[0] else "f32", c[1], c[2]) for c in PER_QUERY])
def test_per_query_filters(ga, oracle, int8, dim, k):
    """65 queries at n = 40009 (a prefix of 16384 rows first), each under its own bitmap and compared with its own subset's
    oracle scan: a full one, an empty one, one whose ids all lie past row 16384, one with fewer than k ids inside the
    prefix and the rest after it, a single id, n - 1 alone, the last word alone, and random ones from 0.9 down to 0.0005.
    The f32 dim 32 case carries the designed priming trap (exact_topk_filtered_model.trap_input) as query 4."""
    rng = np.random.default_rng(43 + dim)
    n, nq = 40009, 65
    if int8:
        el = np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
        q = np.trunc(rng.uniform(-1.0, 1.0, (nq, dim)) * 127.0).astype(np.int8)
    else:
        el, q = m.unit_rows(oracle, rng, n, dim), m.unit_rows(oracle, rng, nq, dim)
    masks = [np.ones(n, bool), np.zeros(n, bool), np.arange(n) >= 16384 + 77,
             fm.only(n, np.concatenate([rng.choice(16384, 5, replace=False), 16384 + rng.choice(n - 16384, 200, replace=False)])),
             fm.only(n, [12345]), fm.only(n, [n - 1]), fm.only(n, np.arange((n - 1) & ~31, n)), fm.exactly(rng, n, k),
             fm.exactly(rng, n, max(k - 1, 1))]
    if not int8 and dim == 32:
        rows, tq, tmask = fm.trap_input(oracle, rng, n=n, dim=dim, k=17)
        el, q[4], masks[4] = rows, tq, tmask  # (the other queries see the same rows)
        assert len(fm.staged_select(m.all_dists(oracle, el, tq), tmask, 17, naive=True)[0]) < 17  # the trap is one
    sel = np.geomspace(0.9, 0.0005, nq - len(masks))
    masks += [fm.random_mask(rng, n, s) for s in sel]
    ix = ga.Granne(_et(el), el, [])
    filters = [_filter(ga, a) for a in masks]
    ids, ds, cnt, st = ix.exact_topk_filtered(q, k, filters, stats=True)
    assert st[0] == 0 and st[3] == 0  # the per-query form leaves status[3] alone
    for a in range(nq):
        oi, od, oc = fm.oracle_subset(oracle, el, masks[a], q[a:a + 1], k)
        assert cnt[a] == oc[0] == min(k, int(masks[a].sum())), a
        assert (ids[a] == oi[0]).all(), a
        assert ds[a].tobytes() == od[0].tobytes(), a
    assert cnt[1] == 0 and (ids[1] == NONE).all() and np.isinf(ds[1]).all()
    ei, ed, ec = ix.exact_topk(q[:1], k)  # the full filter: exact_topk's row
    assert (ids[0] == ei[0]).all() and ds[0].tobytes() == ed[0].tobytes()
    # more than one round of queries, each under one of the bitmaps
    nq2 = 1100
    pick = rng.integers(0, nq, nq2)
    q2 = np.ascontiguousarray(q[pick])
    ids2, ds2, cnt2 = ix.exact_topk_filtered(q2, k, [filters[a] for a in pick])
    assert (ids2 == ids[pick]).all() and ds2.tobytes() == ds[pick].tobytes() and (cnt2 == cnt[pick]).all()
    ix.close()


def _long_empty_stretches(n):
    a = np.zeros(n, bool)
    a[[0, n - 1]] = True
    if n > 300000:
        a[[65535, 65536, 200000, 200031, 200032]] = True  # whole blocks of 65536 ids count zero between them
    return a


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4037, 1_000_003])
def test_filter_ids_equals_nonzero(ga, n):
    rng = np.random.default_rng(44 + n)
    for mask in (fm.random_mask(rng, n, 0.3), np.ones(n, bool), np.zeros(n, bool), _long_empty_stretches(n), fm.random_mask(rng, n, 0.001)):
        for f in (ga.Filter.from_mask(mask), _filter(ga, mask)):
            got = f.ids()
            assert got.dtype == np.uint64 and (got == np.nonzero(mask)[0]).all(), n
            assert len(got) == f.count()
    ids = np.nonzero(fm.random_mask(rng, n, 0.5))[0].astype(np.uint64)
    assert (ga.Filter.from_ids(ids, n).ids() == ids).all()  # the inverse of from_ids


def test_refusals_and_degenerate_calls(ga, oracle):
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table, model_rows
    L = _lib.lib()
    rng = np.random.default_rng(45)
    el, q = m.unit_rows(oracle, rng, 300, 32), m.unit_rows(oracle, rng, 4, 32)
    mask = fm.random_mask(rng, 300, 0.5)
    w = fm.words(mask)
    f = ga.Filter.from_words(w, 300)
    out = np.zeros(8192, np.uint64)
    p, o, hw = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, nq=4, host_filter=hw, dev_filter=C.c_void_p(f.ptr), stride=0):
        for rc in (L.granne_hip_exact_topk_filtered(h, p, nq, k, host_filter, stride, o, o, o, None),
                   L.granne_hip_exact_topk_filtered_device(h, p, nq, k, dev_filter, stride, o, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])
    refused(f16._h, "F16")
    refused(f16._h, "F16", nq=0)  # the handle is refused before anything else is looked at
    with pytest.raises(ga.GranneHipError, match="F16"):
        f16.exact_topk_filtered(q, 5, mask)
    f16.close()
    tab, lists = make_table(rng, 100, 32), make_lists(rng, 300, 100)
    se = ga.SumEmbeddings(tab, lists)
    layer = np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))
    cix = ga.Granne("embeddings", se, [layer], compact=True)
    refused(cix._h, "needs dense rows")
    with pytest.raises(ga.GranneHipError, match="needs dense rows"):
        cix.exact_topk_filtered(q, 5, f)
    cix.close()
    mix = ga.Granne("embeddings", se, [])  # the materialised form is an f32 handle like any other
    rows = model_rows(oracle, tab, lists)
    for k in (1, 100, 1024):
        check_shared(ga, oracle, mix, rows, q, k, mask)
    mix.close()
    ix = ga.Granne("angular", el, [])
    refused(ix._h, "k must be in [1, 1024]", k=0)
    refused(ix._h, "k must be in [1, 1024]", k=1025)
    refused(ix._h, "the filter is null", host_filter=None, dev_filter=None)
    refused(ix._h, "filter_stride_words (9)", stride=9)  # ceil(300 / 32) = 10
    refused(None, "index is null")
    with pytest.raises(ga.GranneHipError):
        ix.exact_topk_filtered(q, 0, mask)
    out[:] = 7
    assert L.granne_hip_exact_topk_filtered(ix._h, p, 0, 5, hw, 0, o, o, o, None) == _lib.OK  # nq = 0: nothing happens
    assert L.granne_hip_exact_topk_filtered_device(ix._h, None, 0, 5, None, 0, None, None, None, None, None) == _lib.OK
    assert (out == 7).all()
    ids, ds, cnt = ix.exact_topk_filtered(q[:0], 5, mask)
    assert ids.shape == (0, 5) and cnt.shape == (0,)
    ix.close()


def test_host_entry(ga, oracle):
    """granne_hip_exact_topk_filtered: host buffers, the filter's words on the host, both forms; the status written"""
    from granne_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(46)
    n, nq, k = 4037, 5, 17
    el, q = m.unit_rows(oracle, rng, n, 100), m.unit_rows(oracle, rng, nq, 100)
    ix = ga.Granne("angular", el, [])
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    oid, ods = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32)
    ocnt, ost = np.full(nq, 77, np.uint32), np.full(4, 9, np.uint32)
    mask = fm.random_mask(rng, n, 0.05)
    w = fm.words(mask, garbage_past_n=True)
    assert L.granne_hip_exact_topk_filtered(ix._h, p(q), nq, k, p(w), 0, p(oid), p(ods), p(ocnt), p(ost)) == _lib.OK
    oi, od, oc = fm.oracle_subset(oracle, el, mask, q, k)
    assert (oid == oi).all() and ods.tobytes() == od.tobytes() and (ocnt == oc).all()
    assert ost[0] == 0 and ost[3] == mask.sum()
    none = fm.words(np.zeros(n, bool))
    assert L.granne_hip_exact_topk_filtered(ix._h, p(q), nq, k, p(none), 0, p(oid), p(ods), p(ocnt), p(ost)) == _lib.OK
    assert (ocnt == 0).all() and (oid == NONE).all() and np.isinf(ods).all() and (ost == 0).all()
    # per-query bitmaps, a stride longer than the bitmap
    masks = [fm.random_mask(rng, n, s) for s in (1.0, 0.5, 0.01, 0.0, 0.002)]
    stride = len(w) + 3
    packed = np.zeros((nq, stride), np.uint32)
    for a in range(nq):
        packed[a, :len(w)] = fm.words(masks[a], garbage_past_n=True)
        packed[a, len(w):] = 0xFFFFFFFF
    ost[:] = 9
    assert L.granne_hip_exact_topk_filtered(ix._h, p(q), nq, k, p(packed), stride, p(oid), p(ods), p(ocnt), p(ost)) == _lib.OK
    for a in range(nq):
        oi, od, oc = fm.oracle_subset(oracle, el, masks[a], q[a:a + 1], k)
        assert (oid[a] == oi[0]).all() and ods[a].tobytes() == od[0].tobytes() and ocnt[a] == oc[0]
    assert ost[0] == 0 and ost[3] == 0
    assert L.granne_hip_exact_topk_filtered(ix._h, p(q), nq, k, p(packed), len(w) - 1, p(oid), p(ods), p(ocnt), None) == _lib.ERR_INVALID
    ix.close()


def test_second_level_and_overflow_under_a_filter(ga, oracle):
    """exact_topk's second-level input: with every row allowed the 6000 rows of the band need the second level, with every
    second one allowed the 3050 rows up to the band's bin are within the 4096 ranked and the first level decides;
    duplicates_nearest with 4500 of the copies allowed overflows as exact_topk does, with 4000 it does not."""
    from granne_amd import _lib
    el, q = m.second_level_input(oracle)
    ix = ga.Granne("angular", el, [])
    mask = np.ones(len(el), bool)
    st = check_shared(ga, oracle, ix, el, q, 100, mask)
    assert st[1] == 1
    mask[50::2] = False
    assert not fm.select(m.all_dists(oracle, el, q[0]), mask, 100)[2]
    st = check_shared(ga, oracle, ix, el, q, 100, mask)
    assert st[1] == 0
    ix.close()
    rng = np.random.default_rng(24)
    el, q = m.duplicates_nearest(oracle, rng)
    ix = ga.Granne("angular", el, [])
    mask = np.ones(len(el), bool)
    mask[5500:6000] = False  # 4500 copies left
    d = m.all_dists(oracle, el, q[0])
    assert fm.select(d, mask, 100)[1:3] == (2, True)
    ids, ds, cnt, st = ix.exact_topk_filtered(q, 100, mask, stats=True)
    assert st[0] == 1 and cnt[0] == 0 and (ids[0] == NONE).all() and np.isinf(ds[0]).all()
    oi, od, _ = fm.oracle_subset(oracle, el, mask, q, 100)
    assert (ids[1:] == oi[1:]).all() and ds[1:].tobytes() == od[1:].tobytes()
    with pytest.raises(ga.GranneHipError) as e:
        ix.exact_topk_filtered(q, 100, mask)
    assert e.value.code == _lib.ERR_OVERFLOW
    mask[5000:5500] = False  # 4000 copies: ranked
    assert not fm.select(d, mask, 100)[2]
    check_shared(ga, oracle, ix, el, q, 100, mask)
    ix.close()


def test_past_4_gib(ga, oracle):
    """f32 rows of 1024 components are 4096 bytes apart: row 2^20 starts at byte 2^32. n = 2^20 + 4096 rows made on the
    device, a handle without layers, about 3,000 allowed ids on both sides of row 2^20 -- n - 1, 2^20 and 2^20 - 1 among
    them --, eight queries that are allowed rows, k = 100: the list form over a list far shorter than the first prefix (two
    idle stages), the memory form of the scan. The reference is oracle.dist over the allowed rows fetched by torch
    indexing: the subset needs no shortlist. A row product taken in 32 bits would read row id - 2^20 in place of an
    allowed row past the mark (high_ids.aliases_differ: other bytes), and the plants there would miss their own lists."""
    import torch
    from granne_amd import _lib
    dim, mark = 1024, 1 << 20
    n = mark + 4096
    seed = 0x6772616E6E65 + 78
    el = high_ids.synth(_lib, seed, 0, n, dim, "f32")
    R = high_ids.Range(n, high_ids.device_row_stride("f32", dim), "f32 rows of 1024 components")
    assert R.past and R.top0 == mark
    rng = np.random.default_rng(47)
    allowed = np.unique(np.concatenate([rng.choice(mark, 1500, replace=False), mark + rng.choice(n - mark, 1500, replace=False),
                                        [n - 1, mark, mark - 1, mark + 1000, n - 33, 5, mark - 4000]])).astype(np.int64)
    assert 3000 <= len(allowed) <= 3007 and (allowed >= mark).sum() >= 1500 and (allowed < mark).sum() >= 1500
    R.assert_covers(allowed)
    high_ids.aliases_differ(el, allowed, R)
    plants = [n - 1, mark, mark - 1, mark + 1000, n - 33, 5, mark - 4000, int(allowed[len(allowed) // 2])]
    q = high_ids.fetch(el, plants)
    torch.cuda.synchronize()
    ix = ga.Granne.from_device("angular", el.data_ptr(), n, dim, [], [], [])
    assert ix.num_elements() == n
    k = 100
    sub = high_ids.fetch(el, allowed)
    _, oi, od = oracle.Index(sub, []).scan_topk(q, k)
    assert od[0].tobytes() == np.sort(m.all_dists(oracle, sub, q[0]), kind="stable")[:k].tobytes()  # oracle.dist, one by one
    mask = fm.only(n, allowed)
    ids, ds, cnt, st = ix.exact_topk_filtered(q, k, _filter(ga, mask), stats=True)
    assert (cnt == k).all() and st[0] == 0 and st[3] == len(allowed)
    assert (ids == allowed.astype(np.uint64)[oi.astype(np.int64)]).all() and ds.tobytes() == od.tobytes()
    for a, i in enumerate(plants):
        assert ids[a, 0] == i, (a, i)
    print("  past-the-mark assertions ran: %d ids >= %d among the results" % (int((ids >= mark).sum()), mark))
    assert (ids >= mark).sum() > 100
    ix.close()
    del el
    torch.cuda.empty_cache()
