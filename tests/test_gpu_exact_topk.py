"""exact_topk (granne_amd/csrc/exact_topk.h) against the CPU oracle: every case compares the WHOLE ids array and the
distance bytes with oracle.Index(elements, []).scan_topk, the counts with min(k, n), the places past the count with
UINT64_MAX / +inf. No tolerance anywhere: the selection is by (distance bits, id) over distances in the reference's own
arithmetic. tests/exact_topk_model.py holds the selection's host model and the inputs shared with
tests/test_exact_topk_model.py.

Shapes: f32 dims 3, 32, 100, 200 (rows in registers: 1, 1, 4 and 8 blocks of 128 bytes) and 333 (the memory form), int8
dims 17, 100, 128, 300 (1, 1, 1 and 4 blocks) and 1500 (the memory form); n in 1, 7, 4037 (a partial eight-lane group: 4037 =
8 * 504 + 5; a partial tile of 32 rows), 20011 (several row ranges) and 40009 (two priming stages: a prefix of 16384 rows
first); nq in 1, 3, 65 (a partial query tile), 1100 (past one round of 1024 queries); k in 1, 16, 17, 100, 1024."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402
from tests import high_ids  # noqa: E402
from tests import value_edges as ve  # noqa: E402

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def _rows(oracle, rng, n, dim, int8):
    if int8:
        return np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
    return m.unit_rows(oracle, rng, n, dim)


def check(ga, oracle, el, q, ks, ix=None):
    """exact_topk of q at every k of ks against oracle.scan_topk: ids, distance bytes, counts; returns the status words of
    the last k"""
    own = ix is None
    if own:
        ix = ga.Granne(_et(el), el, [])
    oix = oracle.Index(el, [])
    st = None
    for k in ks:
        ids, ds, cnt, st = ix.exact_topk(q, k, stats=True)
        _, oi, od = oix.scan_topk(q, k)
        t = min(k, len(el))
        assert (cnt == t).all()
        assert (ids == oi).all(), (k, np.nonzero((ids != oi).any(axis=1))[0][:5])
        assert ds.tobytes() == od.tobytes(), k
        assert (ids[:, t:] == NONE).all() and np.isinf(ds[:, t:]).all()
        assert st[0] == 0 and st[3] == 0 and t <= st[2] <= m.CAP
    if own:
        ix.close()
    return st


# (int8, dim, n, nq, ks): between them every dim, n, nq and k of the module's docstring, n < k, n = 1
SHAPES = [
    (False, 3, 1, 3, (1, 16)),
    (False, 3, 7, 65, (1, 17, 1024)),
    (False, 32, 4037, 65, (1, 16, 17, 100, 1024)),
    (False, 100, 4037, 1100, (16,)),
    (False, 100, 20011, 65, (17, 100)),
    (False, 200, 4037, 3, (1, 100, 1024)),
    (False, 200, 20011, 1, (1024,)),
    (False, 333, 4037, 65, (1, 17, 1024)),
    (False, 32, 40009, 65, (1, 100, 1024)),
    (True, 17, 7, 3, (1, 16, 1024)),
    (True, 17, 4037, 65, (17, 1024)),
    (True, 100, 20011, 65, (16, 100)),
    (True, 100, 4037, 1100, (17,)),
    (True, 128, 4037, 3, (1, 100, 1024)),
    (True, 300, 4037, 65, (16, 1024)),
    (True, 300, 1, 1, (1, 17)),
    (True, 1500, 4037, 3, (1, 100)),
    (True, 100, 40009, 3, (16, 1024)),
]


@pytest.mark.parametrize("int8,dim,n,nq,ks", SHAPES, ids=["%s-%d-n%d-q%d" % ("i8" if s[0] else "f32", s[1], s[2], s[3]) for s in SHAPES])
def test_equals_the_oracle(ga, oracle, int8, dim, n, nq, ks):
    rng = np.random.default_rng(7000 + dim + n + nq + int(int8))
    el, q = _rows(oracle, rng, n, dim, int8), _rows(oracle, rng, nq, dim, int8)
    if n > 100:  # some queries are rows of the set: distance 0 or an ulp from it
        q[:2] = el[[n - 1, n // 2]][:min(2, nq)]
    st = check(ga, oracle, el, q, ks)
    if n <= 32768:  # one stage: the candidates ranked are the model's
        want = max(m.select(m.all_dists(oracle, el, q[a]), ks[-1])[3] for a in range(min(nq, 3)))
        assert st[2] >= want
        if nq <= 3:
            assert st[2] == want


def test_every_row_three_times(ga, oracle):
    rng = np.random.default_rng(21)
    el = m.tripled(m.unit_rows(oracle, rng, 1200, 32))
    q = m.unit_rows(oracle, rng, 9, 32)
    q[8] = 0  # a zero query: every distance exactly 1.0, ordered by id (3600 rows at one distance: within the 4096 ranked)
    ix = ga.Granne("angular", el, [])
    check(ga, oracle, el, q, (1, 17, 100, 1024), ix=ix)
    ids, ds, cnt = ix.exact_topk(q, 99)
    assert (ids[:8, 1::3] == ids[:8, 0::3] + 1200).all() and (ids[:8, 2::3] == ids[:8, 0::3] + 2400).all()
    assert (ds[:, 0::3] == ds[:, 1::3]).all() and (ds[:, 0::3] == ds[:, 2::3]).all()
    assert (ids[8] == np.arange(99)).all() and (ds[8] == 1.0).all()
    ix.close()


def test_copies_of_the_nearest_row_come_in_id_order(ga, oracle):
    rng = np.random.default_rng(22)
    el, q = m.copies_of_the_nearest(oracle, rng)
    ix = ga.Granne("angular", el, [])
    st = check(ga, oracle, el, q, (100,), ix=ix)
    ids, _, _ = ix.exact_topk(q, 100)
    assert (ids[0] == np.arange(500, 600)).all()
    assert 3000 <= st[2] <= 3010 and st[1] == 0  # every copy ranked, by the first level
    ix.close()


def test_int8_zero_row_and_zero_query(ga, oracle):
    rng = np.random.default_rng(23)
    el = _rows(oracle, rng, 1501, 17, True)
    el[100] = 0  # (about rank 750 of every query: inside k = 1024)
    q = _rows(oracle, rng, 5, 17, True)
    q[4] = 0
    ix = ga.Granne("angular_int", el, [])
    check(ga, oracle, el, q, (16, 1024), ix=ix)
    ids, ds, _ = ix.exact_topk(q, 1024)
    assert (ids[:4] == 100).any() and (ds[:4][ids[:4] == 100] == 1.0).all()  # the zero row: distance exactly 1
    assert (ids[4] == np.arange(1024)).all() and (ds[4] == 1.0).all()
    ix.close()


def test_second_level(ga, oracle):
    el, q = m.second_level_input(oracle)
    d = m.all_dists(oracle, el, q[0])
    m.second_level_precondition(d)
    assert m.select(d, 100)[1:3] == (2, False)
    nq = 5
    q = np.repeat(q, nq, axis=0)
    ix = ga.Granne("angular", el, [])
    st = check(ga, oracle, el, q, (100,), ix=ix)
    assert st[1] == nq and st[0] == 0 and st[2] == m.select(d, 100)[3]
    st = check(ga, oracle, el, q, (50,), ix=ix)  # the nearer rows alone: no second level
    assert st[1] == 0
    ix.close()


def test_overflow(ga, oracle):
    from granne_amd import _lib
    rng = np.random.default_rng(24)
    el, q = m.duplicates_nearest(oracle, rng)
    nq, k = len(q), 100
    assert m.select(m.all_dists(oracle, el, q[0]), k)[1:3] == (2, True)
    ix = ga.Granne("angular", el, [])
    with pytest.raises(ga.GranneHipError) as e:
        ix.exact_topk(q, k)
    assert e.value.code == _lib.ERR_OVERFLOW
    ids, ds, cnt, st = ix.exact_topk(np.repeat(q[:1], 3, axis=0), k, stats=True)  # every query of a batch
    assert st[0] == 3 and (cnt == 0).all() and (ids == NONE).all() and np.isinf(ds).all()
    ids, ds, cnt, st = ix.exact_topk(q, k, stats=True)
    assert st[0] == 1 and st[1] >= 1
    assert cnt[0] == 0 and (ids[0] == NONE).all() and np.isinf(ds[0]).all()
    _, oi, od = oracle.Index(el, []).scan_topk(q, k)  # the others, far from the copies, are exact
    assert (cnt[1:] == k).all() and (ids[1:] == oi[1:]).all() and ds[1:].tobytes() == od[1:].tobytes()
    assert not ((ids[1:] >= 1000) & (ids[1:] < 6000)).any()
    # the host entry: GRANNE_HIP_ERR_OVERFLOW, the outputs and the status still written
    oid, ods = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32)
    ocnt, ost = np.full(nq, 77, np.uint32), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _lib.lib().granne_hip_exact_topk(ix._h, p(q), nq, k, p(oid), p(ods), p(ocnt), p(ost))
    assert rc == _lib.ERR_OVERFLOW
    assert (oid == ids).all() and ods.tobytes() == ds.tobytes() and (ocnt == cnt).all() and (ost == st).all()
    rc = _lib.lib().granne_hip_exact_topk(ix._h, p(q[1:]), nq - 1, k, p(oid), p(ods), p(ocnt), None)  # no status asked for
    assert rc == _lib.OK and (oid[:nq - 1] == oi[1:]).all()
    ix.close()


@pytest.mark.parametrize("name", ["off_sphere_f32", "odd_i8", "one_sided_i8", "far_side_i8"])
def test_value_edges(ga, oracle, name):
    rng = np.random.default_rng(25)
    n, nq = 3000, 12
    if name == "off_sphere_f32":
        el, q = ve.off_sphere_f32(rng, n, 100), ve.off_sphere_f32(rng, nq, 100)
        d = np.array([m.all_dists(oracle, el, x) for x in q[:4]])
        assert (d > 2.0).any() and ((d == 0.0).sum(axis=1) > 100).any()  # beyond 2; many rows at exactly 0.0, by id
    elif name == "odd_i8":
        el, q = ve.odd_i8(rng, n, 100), ve.odd_i8(rng, nq, 100)
    else:
        el, q = getattr(ve, name)(rng, n, 100, nq=nq)
    check(ga, oracle, el, q, (16, 100, 1024))


def test_agrees_with_brute_force_and_leaves_last_scan_alone(ga, oracle):
    from granne_amd import _lib
    rng = np.random.default_rng(26)
    el, q = m.unit_rows(oracle, rng, 4000, 100), m.unit_rows(oracle, rng, 96, 100)
    # untied where brute_force SELECTS: it keeps min(k + 6, 16) = 16 candidates by a score good to ~4e-5 and re-ranks them
    # exactly, so its ids are the oracle's whenever ranks 16 and 17 lie further apart than that (chosen on the oracle alone)
    _, oi, od = oracle.Index(el, []).scan_topk(q, 17)
    q = np.ascontiguousarray(q[od[:, 16].astype(np.float64) - od[:, 15] > 1e-4])
    assert len(q) >= 64
    ix = ga.Granne("angular", el, [])
    assert ix.get_option(_lib.OPT_LAST_SCAN) == 0
    ids, ds, cnt = ix.exact_topk(q, 10)
    assert ix.get_option(_lib.OPT_LAST_SCAN) == 0
    bi, bd, bc = ix.brute_force(q, 10)
    word = ix.get_option(_lib.OPT_LAST_SCAN)
    assert word != 0
    assert (ids == bi).all() and ds.tobytes() == bd.tobytes() and (cnt == bc).all()
    ix.exact_topk(q, 1024)
    assert ix.get_option(_lib.OPT_LAST_SCAN) == word
    ix.close()


def test_refusals_and_degenerate_calls(ga, oracle):
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table, model_rows
    L = _lib.lib()
    rng = np.random.default_rng(27)
    el, q = m.unit_rows(oracle, rng, 300, 32), m.unit_rows(oracle, rng, 4, 32)
    out = np.zeros(8192, np.uint64)
    p, o = q.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(h, word, k=5, nq=4):
        for rc in (L.granne_hip_exact_topk(h, p, nq, k, o, o, o, None), L.granne_hip_exact_topk_device(h, p, nq, k, o, o, o, None, None)):
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])
    refused(f16._h, "F16")
    refused(f16._h, "F16", nq=0)  # the handle is refused before anything else is looked at
    with pytest.raises(ga.GranneHipError, match="F16"):
        f16.exact_topk(q, 5)
    f16.close()
    tab, lists = make_table(rng, 100, 32), make_lists(rng, 300, 100)
    se = ga.SumEmbeddings(tab, lists)
    layer = np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))
    cix = ga.Granne("embeddings", se, [layer], compact=True)
    refused(cix._h, "needs dense rows")
    cix.close()
    mix = ga.Granne("embeddings", se, [])  # the materialised form is an f32 handle like any other
    check(ga, oracle, model_rows(oracle, tab, lists), q, (1, 100, 1024), ix=mix)
    mix.close()
    ix = ga.Granne("angular", el, [])  # a layerless handle
    refused(ix._h, "k must be in [1, 1024]", k=0)
    refused(ix._h, "k must be in [1, 1024]", k=1025)
    refused(None, "index is null")
    with pytest.raises(ga.GranneHipError):
        ix.exact_topk(q, 0)
    with pytest.raises(ValueError):
        ix.exact_topk(q[:, :31], 5)
    out[:] = 7
    assert L.granne_hip_exact_topk(ix._h, p, 0, 5, o, o, o, None) == _lib.OK  # nq = 0: nothing happens
    assert L.granne_hip_exact_topk_device(ix._h, None, 0, 5, None, None, None, None, None) == _lib.OK
    assert (out == 7).all()
    check(ga, oracle, el, q, (5, 1024), ix=ix)
    ix.close()


def test_past_4_gib(ga, oracle):
    """f32 rows of 1024 components are 4096 bytes apart: row 2^20 starts at byte 2^32. n = 2^20 + 4096 rows made on the
    device (no host copy), a handle without layers, eight queries that are planted rows (ids n - 1 and 2^20 - 1 carry the
    same row: the smaller id stands first), k = 100; two priming stages and the memory form of the scan. The reference is
    high_ids.scan_reference's two stages with check_exact_scan's guard on its shortlist: the 256th float64 distance
    exceeds the oracle's k-th by 1e-3 at least (the oracle's f32 dot of unit rows is within dim * 2^-24 = 6.1e-5 of the
    exact one, so nothing outside the shortlist is among the oracle's k best). A row product taken in 32 bits would read
    rows id - 2^20 in place of the rows past the mark: the plants there would be missing from their own lists.
    (high_ids.Range.assert_covers asks for 1,003 distinct ids past the mark, more than 8 x 100 results can hold: the
    planted ids on both sides of the mark are asserted instead.)"""
    import torch
    from granne_amd import _lib
    dim, mark = 1024, 1 << 20
    n = mark + 4096
    seed = 0x6772616E6E65 + 77
    el = high_ids.synth(_lib, seed, 0, n, dim, "f32")
    dq = high_ids.synth(_lib, seed + 1, 0, 8, dim, "f32")
    plants = [(n - 1, 0), (mark, 1), (mark - 1, 0), (mark + 1000, 2), (mark + 2000, 3), (mark + 3000, 4), (mark + 4000, 5),
              (n - 33, 6)]  # (query 7 is no row of the set)
    assert len(plants) == 8
    for i, j in plants:
        el[i] = dq[j]
    q = dq.cpu().numpy()
    torch.cuda.synchronize()
    R = high_ids.Range(n, high_ids.device_row_stride("f32", dim), "f32 rows of 1024 components")
    assert R.past and R.top0 == mark
    high_ids.aliases_differ(el, [i for i, _ in plants], R)
    ix = ga.Granne.from_device("angular", el.data_ptr(), n, dim, [], [], [])
    assert ix.hbm_bytes() >= n * R.row_stride  # the handle's own copy of the rows, 4096 bytes apart
    k = 100
    ref_i, ref_d, d64 = high_ids.scan_reference(oracle, el, lambda r: r, q, "f32", keep=256)
    gap = d64[:, 255] - ref_d[:, k - 1]
    print("  shortlist guard: 256th float64 distance - oracle's %dth: min %.4g" % (k, gap.min()))
    assert (gap >= 1e-3).all()
    ids, ds, cnt, st = ix.exact_topk(q, k, stats=True)
    assert (cnt == k).all() and st[0] == 0
    assert (ids == ref_i[:, :k].astype(np.uint64)).all() and ds.tobytes() == ref_d[:, :k].tobytes()
    assert ids[0, 0] == mark - 1 and ids[0, 1] == n - 1 and ds[0, 0] == ds[0, 1]
    have = set(ids.reshape(-1).tolist())
    for i, _ in plants:
        assert i in have, i
    assert n - 1 in have and R.top0 in have and R.top0 - 1 in have
    print("  past-the-mark assertions ran: %d ids >= %d among the results" % (int((ids >= mark).sum()), mark))
    ix.close()
    del el
    torch.cuda.empty_cache()
