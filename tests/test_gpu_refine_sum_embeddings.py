"""Refined search over a SumEmbeddings CONTAINER on the GPU (granne_hip_refine_sum_embeddings_device,
granne_hip_search_refined_sum_embeddings_batch*, granne_hip_sum_embeddings_rows*) against tests/refine_model.py over
oracle.normalize_f32 of the numpy term sums, and against the materialised index over the same container: ids, distance
BYTES, counts and the dropped-candidate word; rows byte for byte. No tolerances. V = 300 table rows, n = 1500 elements,
16 queries; every world and every reference is made once per module.

The kernel keeps a row's sum in registers up to 8 full 32-float blocks (dim < 288) in four forms (up to 1, 3, 4, 8
blocks) and sums twice beyond: the dims below take every form and both sides of each boundary."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_model as model  # noqa: E402
from tests.conftest import assert_counters, random_floats  # noqa: E402

U64_MAX = model.U64_MAX
V, N, NQ = 300, 1500, 16
LENGTHS = (0, 1, 2, 5, 6, 9, 40)
# 3: tail only; 32: one block, no tail; 36, 63: the one-block form; 64, 100, 127: three blocks; 128, 159: four; 160, 200,
# 287: eight; 288, 300: two passes
DIMS = (3, 32, 36, 63, 64, 100, 127, 128, 159, 160, 200, 287, 288, 300)


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def term_sums(tab, lists):
    """create_embedding in numpy: no terms -> zeros, else a copy of the first term's row and `+=` in list order"""
    raw = np.zeros((len(lists), tab.shape[1]), np.float32)
    for i, t in enumerate(lists):
        if len(t):
            acc = tab[t[0]].copy()
            for x in t[1:]:
                acc += tab[x]
            raw[i] = acc
    return raw


def random_lists(rng, v, n, lengths=LENGTHS):
    return [[int(x) for x in rng.integers(0, v, int(rng.choice(lengths)))] for _ in range(n)]


_worlds = {}


def world(ga, oracle, dim):
    """table, term lists, the rows they stand for, prepared queries, the container and its materialised index (rows only)"""
    if dim not in _worlds:
        rng = np.random.default_rng(7000 + dim)
        tab = random_floats(rng, V, dim)
        lists = random_lists(rng, V, N)
        w = dict(tab=tab, lists=lists, rows=oracle.normalize_f32(term_sums(tab, lists)),
                 q=oracle.normalize_f32(random_floats(rng, NQ, dim)))
        w["se"] = ga.SumEmbeddings(tab, lists)
        w["mix"] = ga.Granne("embeddings", w["se"], [])
        _worlds[dim] = w
    return _worlds[dim]


def assert_result(got, want):
    ids, ds, cnt = got[:3]
    eids, eds, ecnt = want[:3]
    bad = np.nonzero((ids != eids).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], eids[bad[:1]])
    assert ds.tobytes() == eds.tobytes()
    assert (cnt == ecnt).all()


def assert_same(a, b):
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


# ---- 1. dims x list lengths ----------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_dims_and_list_lengths(ga, oracle, dim):
    """m = 70: two rounds of 32 candidates and a partial one; every query's list mixes the term-list lengths"""
    w = world(ga, oracle, dim)
    rng = np.random.default_rng(dim)
    m, k = 70, 10
    cand = np.stack([rng.permutation(N)[:m] for _ in range(NQ)]).astype(np.uint64)
    for i in range(NQ):
        assert len({len(w["lists"][int(c)]) for c in cand[i]}) >= 5
    got = w["se"].refine(w["q"], cand, k=k, dropped=True)
    assert_result(got, model.refine(oracle, w["rows"], w["q"], cand, None, k))
    assert got[3] == 0
    assert_same(got[:3], w["mix"].refine(w["q"], cand, k=k))
    full = w["se"].refine(w["q"], cand, k=m)  # every candidate's distance, not only the ten best
    assert_same(full, w["mix"].refine(w["q"], cand, k=m))


# ---- 2. value edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [36, 100, 300])
def test_value_edges(ga, oracle, dim):
    """terms that cancel to an all-zero sum (norm 0: no divide, distance 1), no terms, -0.0 components in a first and in a
    later term (block and tail positions), duplicate term ids"""
    rng = np.random.default_rng(50 + dim)
    tab = random_floats(rng, 12, dim)
    tab[1] = -tab[0]
    spots = [0, 5, 31, dim - 1, dim - 2]
    tab[2, spots] = -0.0
    tab[3, spots] = -0.0
    tab[4, spots] = 0.0
    lists = [[0, 1], [], [2], [2, 3], [3, 2], [4, 2], [2, 4], [5, 5, 5], [6, 7, 6, 7, 6], [0, 1, 0, 1], [0, 8, 1], [1, 0, 9, 9],
             [2, 2], [10], [11, 10, 11]]
    raw = term_sums(tab, lists)
    assert not raw[0].any() and not raw[9].any() and not raw[1].any()
    assert np.signbit(raw[2][spots]).all() and np.signbit(raw[3][spots]).all() and not np.signbit(raw[5][spots]).any()
    rows = oracle.normalize_f32(raw)
    q = oracle.normalize_f32(random_floats(rng, 5, dim))
    q[4] = 0
    se = ga.SumEmbeddings(tab, lists)
    mix = ga.Granne("embeddings", se, [])
    n = len(lists)
    cand = np.stack([rng.permutation(n) for _ in range(5)]).astype(np.uint64)
    got = se.refine(q, cand, k=n, dropped=True)
    assert_result(got, model.refine(oracle, rows, q, cand, None, n))
    assert_same(got[:3], mix.refine(q, cand, k=n))
    ids, ds = got[0], got[1]
    for i in range(5):
        for zero in (0, 1, 9):
            assert ds[i][np.nonzero(ids[i] == zero)[0][0]] == 1.0
    # the signs of the zeros are visible in the rows themselves
    assert se.to_rows("angular").tobytes() == rows.tobytes()
    assert np.signbit(se.to_rows("angular")[3][spots]).all()


# ---- 3. list shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 32, 33, 64, 65, 1024])
def test_list_lengths_counts_padding_and_dropped_ids(ga, oracle, m):
    """a round is 32 candidates (one per group of eight lanes): lists that end with a round, one entry into the next, and
    the longest list there is"""
    w = world(ga, oracle, 100)
    se, mix, rows = w["se"], w["mix"], w["rows"]
    nq = 6
    q = w["q"][:nq]
    rng = np.random.default_rng(m)
    cand = np.stack([rng.permutation(N)[:m] for _ in range(nq)]).astype(np.uint64)
    counts = np.array([0, m, m // 2, min(1, m), m, max(m - 1, 0)], np.uint32)
    for i in range(nq):
        cand[i, counts[i]:] = U64_MAX  # the padding a search leaves behind its results
    bad = [N, (1 << 32) + 3, int(U64_MAX), N + 12345]  # n itself, one whose LOW 32 bits name an element, UINT64_MAX
    for i in (1, 4):
        for t, pos in enumerate(rng.permutation(int(counts[i]))[:len(bad)]):
            cand[i, pos] = bad[t]
    if m >= 64:  # an id named twice keeps every entry, in list order (list 2 holds no bad id)
        cand[2, 20] = cand[2, 21] = cand[2, 3]
    inside = np.arange(m)[None, :] < counts[:, None]
    for k in (10, m + 3):  # k may exceed m: padded output
        got = se.refine(q, cand, counts, k=k, dropped=True)
        want = model.refine(oracle, rows, q, cand, counts, k)
        assert_result(got, want)
        assert got[3] == want[3] == int((cand[inside] >= N).sum()) == 2 * min(len(bad), m)
        assert (got[2] == np.minimum(k, want[2])).all() and got[2][0] == 0
        assert (got[0][0] == U64_MAX).all() and np.isinf(got[1][0]).all()  # an empty list: every slot unused
        assert_same(got[:3], mix.refine(q, cand, counts, k=k))
        if m >= 64 and k > m:
            twice = np.nonzero(got[0][2] == cand[2, 3])[0]
            assert twice.size == 3 and (np.diff(twice) == 1).all()
    got = se.refine(q, cand, None, k=10, dropped=True)  # no counts: all m entries, the padding dropped and counted
    want = model.refine(oracle, rows, q, cand, None, 10)
    assert_result(got, want)
    assert got[3] == want[3] == int((cand >= N).sum())


@pytest.mark.parametrize("nq", [0, 1, 1025])
def test_batch_sizes(ga, oracle, nq):
    w = world(ga, oracle, 100)
    rng = np.random.default_rng(nq)
    q = oracle.normalize_f32(random_floats(rng, nq, 100)) if nq else np.zeros((0, 100), np.float32)
    cand = rng.integers(0, N, (nq, 9)).astype(np.uint64)
    ids, ds, cnt = w["se"].refine(q, cand, k=4)
    assert ids.shape == (nq, 4) and ds.shape == (nq, 4) and cnt.shape == (nq,)
    if nq:
        assert_result((ids, ds, cnt), model.refine(oracle, w["rows"], q, cand, None, 4))
        assert_same((ids, ds, cnt), w["mix"].refine(q, cand, k=4))


# ---- 4. the fused call ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fused(ga, oracle):
    w = dict(world(ga, oracle, 100))
    rng = np.random.default_rng(4)
    w["qlists"] = random_lists(rng, V, NQ, lengths=(1, 2, 5, 6))
    w["fq"] = oracle.normalize_f32(term_sums(w["tab"], w["qlists"]))
    w["rows8"] = oracle.quantize(w["rows"])
    w["fq8"] = oracle.quantize(w["fq"])
    w["oix8"] = oracle.build_index(w["rows8"], num_neighbors=20, max_search=20, n_threads=8)
    w["oix"] = oracle.build_index(w["rows"], num_neighbors=10, max_search=20, n_threads=8)
    return w


def test_to_rows_gives_the_walk_index_its_rows(ga, oracle, fused):
    assert fused["se"].to_rows("angular_int").tobytes() == fused["rows8"].tobytes()


@pytest.mark.parametrize("ms,m,k", [(50, 50, 10), (30, 30, 30), (20, 7, 10), (1, 1, 1)])
def test_int8_walk_container_rerank(ga, oracle, fused, ms, m, k):
    w = fused
    g8 = ga.Granne("angular_int", w["se"].to_rows("angular_int"), w["oix8"].layers)
    got = ga.RefinedGranne(g8, w["se"]).search_batch((w["fq8"], w["fq"]), ms, k, refine_from=m, stats=True, dropped=True)
    want = model.search_refined(oracle, w["oix8"], w["rows"], w["fq8"], w["fq"], ms, m, k)
    assert_result(got, want)
    assert got[4] == 0 == want[3]
    assert_counters(got[3], want[4], exact=False)
    assert_same(got, ga.RefinedGranne(g8, w["mix"]).search_batch((w["fq8"], w["fq"]), ms, k, refine_from=m, stats=True, dropped=True))


def test_fused_device_entry_and_its_status_words(ga, oracle, fused):
    import torch
    w = fused
    nq, ms, m, k = NQ, 50, 50, 10
    g8 = ga.Granne("angular_int", w["rows8"], w["oix8"].layers)
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    tq8 = torch.from_numpy(w["fq8"].view(np.uint8)).to(dev)
    tq = torch.from_numpy(w["fq"]).to(dev)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_c = torch.empty(nq, dtype=torch.int32, device=dev)
    st = torch.zeros((nq, 3), dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rstatus = torch.zeros(1, dtype=torch.int32, device=dev)
    ga.RefinedGranne(g8, w["se"]).search_batch_device(tq8.data_ptr(), tq.data_ptr(), nq, ms, m, k, out_i.data_ptr(), out_d.data_ptr(),
                                                      out_c.data_ptr(), st.data_ptr(), status.data_ptr(), rstatus.data_ptr(), s)
    torch.cuda.synchronize(dev)
    want = model.search_refined(oracle, w["oix8"], w["rows"], w["fq8"], w["fq"], ms, m, k)
    assert_result((out_i.cpu().numpy().view(np.uint64), out_d.cpu().numpy(), out_c.cpu().numpy().view(np.uint32)), want)
    assert_counters(st.cpu().numpy(), want[4], exact=False)
    assert not status.cpu().numpy().any() and rstatus.cpu().numpy()[0] == 0
    L = ga._lib.lib()
    assert L.granne_hip_search_refined_sum_embeddings_batch_device(g8._h, w["se"]._h, None, None, 0, 50, 50, 10, None, None, None, None,
                                                                   None, None, None) == ga._lib.OK  # nq 0: nothing to do


def test_compact_index_walked_container_reranks(ga, oracle, fused):
    """the container twice: as the rows provider of the compact index that is walked, and as the re-ranking side. A
    compact index on the refine side is refused as before."""
    w = fused
    cix = ga.Granne("embeddings", w["se"], w["oix"].layers, compact=True)
    want = model.search_refined(oracle, w["oix"], w["rows"], w["fq"], w["fq"], 30, 30, 5)
    assert_result(ga.RefinedGranne(cix, w["se"]).search_batch((w["fq"], w["fq"]), 30, 5), want)
    with pytest.raises(ga.GranneHipError) as e:
        ga.RefinedGranne(cix, cix).search_batch((w["fq"], w["fq"]), 30, 5)
    assert e.value.code == ga._lib.ERR_INVALID


def test_term_list_queries(ga, oracle, fused):
    w = fused
    g8 = ga.Granne("angular_int", w["rows8"], w["oix8"].layers)
    rg = ga.RefinedGranne(g8, w["se"])
    want = model.search_refined(oracle, w["oix8"], w["rows"], w["fq8"], w["fq"], 40, 40, 10)
    assert_result(rg.search_batch(w["qlists"], 40, 10, prepared=False), want)
    one = rg.search(w["qlists"][3], 40, 5, prepared=False)
    assert one == [(int(i), float(d)) for i, d in zip(want[0][3, :5], want[1][3, :5])]
    # raw float rows: normalised, and quantised for the int8 walk
    raw = term_sums(w["tab"], w["qlists"])
    assert_result(rg.search_batch(raw, 40, 10, prepared=False), want)
    # the re-rank alone takes term lists too
    cand = np.stack([np.random.default_rng(i).permutation(N)[:20] for i in range(NQ)]).astype(np.uint64)
    assert_result(w["se"].refine(w["qlists"], cand, k=5, prepared=False), model.refine(oracle, w["rows"], w["fq"], cand, None, 5))


# ---- 5. to_rows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 100, 300])
def test_to_rows_in_every_element_type(ga, oracle, dim, monkeypatch):
    w = world(ga, oracle, dim)
    se, rows = w["se"], w["rows"]
    want = {"angular": rows, "angular_int": oracle.quantize(rows), "angular_f16": rows.astype(np.float16)}
    codes = {"angular": ga.F32, "angular_int": ga.I8, "angular_f16": ga.F16}
    for et, exp in want.items():
        for name in (et, codes[et]):  # the element type's name, or its GRANNE_HIP_* code
            got = se.to_rows(name)
            assert got.dtype == exp.dtype and got.shape == exp.shape and got.tobytes() == exp.tobytes(), name
    # a range that is no multiple of the chunk, the chunk shrunk so that 1,480 rows cross it 211 times
    monkeypatch.setenv("GRANNE_HIP_SE_ROWS_CHUNK", "7")
    for et, exp in want.items():
        assert se.to_rows(et, first=11, count=N - 20).tobytes() == exp[11:N - 9].tobytes(), et
        assert se.to_rows(et, first=N - 3).tobytes() == exp[N - 3:].tobytes(), et
        assert se.to_rows(et, first=5, count=7).tobytes() == exp[5:12].tobytes(), et


@pytest.mark.parametrize("chunk", [None, "5"])
def test_to_rows_device_with_a_stride_beyond_the_row(ga, oracle, chunk, monkeypatch):
    import torch
    if chunk:
        monkeypatch.setenv("GRANNE_HIP_SE_ROWS_CHUNK", chunk)
    w = world(ga, oracle, 100)
    se, rows = w["se"], w["rows"]
    first, count = 7, 83
    want = {"angular": rows, "angular_int": oracle.quantize(rows), "angular_f16": rows.astype(np.float16)}
    dev = torch.device("cuda", 0)
    for et, exp in want.items():
        row = 100 * exp.dtype.itemsize
        stride = row + 28
        buf = torch.full((count, stride), 0xAB, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        se.to_rows_device(et, buf.data_ptr(), first, count, stride_bytes=stride, stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        got = buf.cpu().numpy()
        assert got[:, :row].tobytes() == exp[first:first + count].tobytes(), et
        assert (got[:, row:] == 0xAB).all(), et  # the bytes between the rows are the caller's


# ---- 6. state and addressing ---------------------------------------------------------------------------
def test_extend_is_seen_by_the_next_call(ga, oracle):
    rng = np.random.default_rng(61)
    tab = random_floats(rng, V, 100)
    lists = random_lists(rng, V, 260)
    rows = oracle.normalize_f32(term_sums(tab, lists))
    q = oracle.normalize_f32(random_floats(rng, 4, 100))
    se = ga.SumEmbeddings(tab, lists[:200])
    cand = np.stack([rng.permutation(260)[:64] for _ in range(4)]).astype(np.uint64)
    cand[:, 0] = 230  # in the new range
    before = se.refine(q, cand, k=64, dropped=True)
    assert_result(before, model.refine(oracle, rows[:200], q, cand, None, 64))
    assert before[3] == int((cand >= 200).sum()) and not (before[0] == 230).any()
    se.extend(lists[200:])
    after = se.refine(q, cand, k=64, dropped=True)
    assert_result(after, model.refine(oracle, rows, q, cand, None, 64))
    assert after[3] == 0 and (after[0] == 230).sum() == 4
    assert se.to_rows("angular", first=200).tobytes() == rows[200:].tobytes()


def test_two_threads_make_the_first_device_use(ga, oracle):
    w = world(ga, oracle, 100)
    se = ga.SumEmbeddings(w["tab"], w["lists"])  # fresh: no device copy yet
    rng = np.random.default_rng(62)
    cand = np.stack([rng.permutation(N)[:50] for _ in range(NQ)]).astype(np.uint64)
    gate, out = threading.Barrier(2), [None, None]

    def run(t):
        gate.wait()
        out[t] = se.refine(w["q"], cand, k=10, dropped=True)

    threads = [threading.Thread(target=run, args=(t,)) for t in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    want = model.refine(oracle, w["rows"], w["q"], cand, None, 10)
    for got in out:
        assert got is not None
        assert_result(got, want)
        assert got[3] == 0


def test_table_rows_past_4gib(ga, oracle):
    """dim 128 (512-byte table rows), V just above 2^23: the rows of the highest term ids start past byte 2^32 of the
    table. The table is made on the device; the rows the model needs are fetched by torch indexing, and the row a product
    truncated to 32 bits would read instead (term - 2^23) is asserted to hold other bytes."""
    import torch
    from tests import high_ids
    from granne_amd import _lib
    dim, mark = 128, 1 << 23
    v, n, nq = mark + 1024, 400, 8
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tab = torch.empty((v, dim), dtype=torch.float32, device=dev)
    _lib.check(L.granne_hip_synth_rows_device(C.c_void_p(tab.data_ptr()), 99, 0, v, dim, 0, sp))
    rng = np.random.default_rng(63)
    lists = []
    for i in range(n):
        ln = int(rng.integers(1, 5))
        hi = rng.integers(mark, v, ln)
        lo = rng.integers(0, mark, ln)
        lists.append([int(x) for x in np.where(rng.random(ln) < 0.6, hi, lo)])
    lists[0], lists[1], lists[2] = [v - 1], [mark, 5], [mark - 1, v - 1, mark]
    from granne_amd.embeddings import csr_of
    off, terms = csr_of(lists)
    t_off = torch.from_numpy(off.view(np.int64)).to(dev)
    t_terms = torch.from_numpy(terms.view(np.int32)).to(dev)
    se = ga.SumEmbeddings.from_device(tab.data_ptr(), v, dim, t_off.data_ptr(), t_terms.data_ptr(), n, 0, sp.value)
    uniq = np.unique(terms.astype(np.int64))
    high = uniq[uniq >= mark]
    assert high.size >= 300 and v - 1 in high and mark in high and mark - 1 in uniq
    own, other = high_ids.fetch(tab, high), high_ids.fetch(tab, high - mark)  # (term * 512) mod 2^32 = (term - 2^23) * 512
    assert not (own == other).all(axis=1).any()
    fetched = dict(zip(uniq.tolist(), high_ids.fetch(tab, uniq)))
    del tab
    raw = np.zeros((n, dim), np.float32)
    for i, t in enumerate(lists):
        acc = fetched[t[0]].copy()
        for x in t[1:]:
            acc += fetched[x]
        raw[i] = acc
    rows = oracle.normalize_f32(raw)
    q = oracle.normalize_f32(random_floats(rng, nq, dim))
    cand = np.stack([rng.permutation(n)[:70] for _ in range(nq)]).astype(np.uint64)
    cand[:, :3] = 0, 1, 2
    got = se.refine(q, cand, k=70, dropped=True)
    assert_result(got, model.refine(oracle, rows, q, cand, None, 70))
    assert got[3] == 0
    assert se.to_rows("angular", first=0, count=3).tobytes() == rows[:3].tobytes()
    se.close()
