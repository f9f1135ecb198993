"""Refined search on the GPU (granne_hip_refine_device, granne_hip_search_refined_batch*) against tests/refine_model.py:
ids, distance BYTES, counts and the dropped-candidate word. Oracle graphs are small (n = 3000, num_neighbors 10-20, built
at max_search 20); every reference is computed once per module."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_model as model  # noqa: E402
from tests.conftest import assert_counters, random_floats  # noqa: E402

U64_MAX = model.U64_MAX
N, NQ = 3000, 64


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.fixture(scope="module")
def world(ga, oracle):
    """The same 3000 elements three ways -- f32 100-d, int8 100-d, f32 over the first 28 components -- each with an oracle
    graph and a GPU handle; f32 rows also as a rows-only handle (no layers)."""
    rng = np.random.default_rng(20240)
    rows = oracle.normalize_f32(random_floats(rng, N, 100))
    q = oracle.normalize_f32(random_floats(rng, NQ, 100))
    w = dict(rows=rows, rows8=oracle.quantize(rows), rows28=oracle.normalize_f32(rows[:, :28].copy()),
             q=q, q8=oracle.quantize(q), q28=oracle.normalize_f32(q[:, :28].copy()))
    w["oix"] = oracle.build_index(w["rows"], num_neighbors=20, max_search=20, n_threads=8)
    w["oix8"] = oracle.build_index(w["rows8"], num_neighbors=20, max_search=20, n_threads=8)
    w["oix28"] = oracle.build_index(w["rows28"], num_neighbors=10, max_search=20, n_threads=8)
    w["g"] = ga.Granne("angular", w["rows"], w["oix"].layers)
    w["g8"] = ga.Granne("angular_int", w["rows8"], w["oix8"].layers)
    w["g28"] = ga.Granne("angular", w["rows28"], w["oix28"].layers)
    w["r"] = ga.Granne("angular", w["rows"], [])        # rows only
    w["r8"] = ga.Granne("angular_int", w["rows8"], [])
    return w


def assert_result(got, want):
    ids, ds, cnt = got[:3]
    eids, eds, ecnt = want[:3]
    bad = np.nonzero((ids != eids).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], eids[bad[:1]])
    assert ds.tobytes() == eds.tobytes()
    assert (cnt == ecnt).all()


def check_fused(ga, oracle, walk, refine, oix, rows, qw, qr, ms, m, k):
    rg = ga.RefinedGranne(walk, refine)
    ids, ds, cnt, st, dropped = rg.search_batch((qw, qr), ms, k, refine_from=m, stats=True, dropped=True)
    want = model.search_refined(oracle, oix, rows, qw, qr, ms, m, k)
    assert_result((ids, ds, cnt), want)
    assert dropped == 0 == want[3]
    assert_counters(st, want[4], exact=False)


SHAPES = [(50, 50, 10), (30, 30, 30), (200, 200, 10), (20, 7, 10), (1, 1, 1)]


@pytest.mark.parametrize("ms,m,k", SHAPES)
def test_int8_walk_f32_rerank_equals_the_model(ga, oracle, world, ms, m, k):
    check_fused(ga, oracle, world["g8"], world["r"], world["oix8"], world["rows"], world["q8"], world["q"], ms, m, k)


@pytest.mark.parametrize("ms,m,k", SHAPES)
def test_f32_walk_int8_rerank_equals_the_model(ga, oracle, world, ms, m, k):
    check_fused(ga, oracle, world["g"], world["r8"], world["oix"], world["rows8"], world["q"], world["q8"], ms, m, k)


@pytest.mark.parametrize("ms,m,k", SHAPES)
def test_28d_walk_100d_rerank_equals_the_model(ga, oracle, world, ms, m, k):
    check_fused(ga, oracle, world["g28"], world["r"], world["oix28"], world["rows"], world["q28"], world["q"], ms, m, k)


def test_refine_from_defaults_to_max_search_and_unprepared_queries(ga, oracle, world):
    rg = ga.RefinedGranne(world["g8"], world["r"])
    a = rg.search_batch((world["q8"], world["q"]), 40, 10)
    b = rg.search_batch((world["q8"], world["q"]), 40, 10, refine_from=40)
    assert_result(a, b)
    # raw rows: normalised, and for the int8 walk the normalised rows quantised -- the library's kernels give the oracle's bytes
    raw = random_floats(np.random.default_rng(3), 16, 100)
    nrm = oracle.normalize_f32(raw)
    want = model.search_refined(oracle, world["oix8"], world["rows"], oracle.quantize(nrm), nrm, 40, 40, 10)
    assert_result(rg.search_batch(raw, 40, 10, prepared=False), want)
    one = rg.search(raw[3], 40, 5, prepared=False)
    assert one == [(int(i), float(d)) for i, d in zip(want[0][3, :5], want[1][3, :5])]


# ---- the re-rank alone -----------------------------------------------------------------------------
def prepared_rows(oracle, rng, n, dim, dtype):
    rows = oracle.normalize_f32(random_floats(rng, n, dim))
    return rows if dtype == "angular" else oracle.quantize(rows)


@pytest.mark.parametrize("et,dim", [("angular", d) for d in (3, 28, 97, 100, 200, 333)] + [("angular_int", d) for d in (32, 100, 130)])
def test_row_widths(ga, oracle, et, dim):
    """No full 32-float block, tails, the unrolled and the looped block counts; int8 rows of 32, 128 and 256 device bytes."""
    rng = np.random.default_rng(1000 + dim)
    n, nq, m, k = 300, 9, 37, 12
    rows, q = prepared_rows(oracle, rng, n, dim, et), prepared_rows(oracle, rng, nq, dim, et)
    cand = np.stack([rng.permutation(n)[:m] for _ in range(nq)]).astype(np.uint64)
    r = ga.Granne(et, rows, [])
    got = r.refine(q, cand, k=k, dropped=True)
    want = model.refine(oracle, rows, q, cand, None, k)
    assert_result(got, want)
    assert got[3] == 0
    # the same bits as the stand-alone Dist operator
    full = r.refine(q, cand, k=m)
    dd = r.dists_many(q, cand.astype(np.uint32))
    for i in range(nq):
        assert np.sort(dd[i].view(np.uint32)).tobytes() == full[1][i].view(np.uint32).tobytes()


@pytest.fixture(scope="module")
def rows2000(oracle):
    rng = np.random.default_rng(77)
    rows = oracle.normalize_f32(random_floats(rng, 2000, 100))
    q = oracle.normalize_f32(random_floats(rng, 6, 100))
    return {"angular": (rows, q), "angular_int": (oracle.quantize(rows), oracle.quantize(q))}


@pytest.mark.parametrize("et", ["angular", "angular_int"])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 1024])
def test_list_lengths_counts_padding_and_dropped_ids(ga, oracle, rows2000, et, m):
    rows, q = rows2000[et]
    n, nq = len(rows), len(q)
    rng = np.random.default_rng(m)
    cand = np.stack([rng.permutation(n)[:m] for _ in range(nq)]).astype(np.uint64)
    counts = np.array([0, m, m // 2, min(1, m), m, max(m - 1, 0)], np.uint32)
    for i in range(nq):
        cand[i, counts[i]:] = U64_MAX  # the padding a search leaves behind its results
    # ids the index does not hold, inside the counted part: n itself, one whose LOW 32 bits name an element, UINT64_MAX
    bad = [n, (1 << 32) + 3, int(U64_MAX), n + 12345]
    for i in (1, 4):
        for t, pos in enumerate(rng.permutation(int(counts[i]))[:len(bad)]):
            cand[i, pos] = bad[t]
    r = ga.Granne(et, rows, [])
    for k in (10, m + 3):  # k may exceed m
        got = r.refine(q, cand, counts, k=k, dropped=True)
        want = model.refine(oracle, rows, q, cand, counts, k)
        assert_result(got, want)
        assert got[3] == want[3] == 2 * min(len(bad), m)
        assert (got[2] == np.minimum(k, want[2])).all() and got[2][0] == 0
        assert (got[0][0] == U64_MAX).all() and np.isinf(got[1][0]).all()  # an empty list: every slot unused
    # no counts: all m entries of every list, the padding dropped and counted
    got = r.refine(q, cand, None, k=10, dropped=True)
    want = model.refine(oracle, rows, q, cand, None, 10)
    assert_result(got, want)
    assert got[3] == want[3] == int((cand >= n).sum())


@pytest.mark.parametrize("et", ["angular", "angular_int"])
def test_equal_distances_order_by_id(ga, oracle, et):
    """Groups of identical rows, two all-zero rows (distance 1.0 to everything), an all-zero query (distance 1.0 to every
    row: the whole list ties), and an id named twice in a list."""
    rng = np.random.default_rng(5)
    n, nq, m = 400, 8, 200
    base = prepared_rows(oracle, rng, 12, 100, et)
    rows = base[rng.integers(0, 12, n)].copy()
    rows[7] = 0
    rows[8] = 0
    q = prepared_rows(oracle, rng, nq, 100, et)
    q[2] = 0
    cand = np.stack([rng.permutation(n)[:m] for _ in range(nq)]).astype(np.uint64)
    cand[:, 10], cand[:, 11] = 7, 8
    cand[:, 5] = cand[:, 3]  # a duplicate id: kept twice
    cand[:, 150] = cand[:, 3]
    r = ga.Granne(et, rows, [])
    got = r.refine(q, cand, k=m)
    want = model.refine(oracle, rows, q, cand, None, m)
    assert_result(got, want)
    ids, ds, cnt = got
    assert (cnt == m).all()
    assert (ds[2] == 1.0).all() and (np.diff(ids[2].astype(np.int64)) >= 0).all()
    for i in range(nq):
        tie = ds[i][1:] == ds[i][:-1]
        assert tie.sum() > m // 2  # twelve distinct rows: most neighbours in the order tie
        assert (ids[i][1:][tie] >= ids[i][:-1][tie]).all()
        at = np.nonzero(ids[i] == 7)[0]
        assert at.size >= 1 and ds[i][at[0]] == 1.0


def test_fused_equals_the_composition_on_the_device(ga, world):
    """No oracle: the walk with k = m, then dists_device, then a sort by (distance bits, id) on the host."""
    import torch
    w = world
    nq, ms, m, k = NQ, 50, 50, 10
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream(dev).cuda_stream
    tq8 = torch.from_numpy(w["q8"].view(np.uint8)).to(dev)
    tq = torch.from_numpy(w["q"]).to(dev)
    cand = torch.empty((nq, m), dtype=torch.int64, device=dev)
    cd = torch.empty((nq, m), dtype=torch.float32, device=dev)
    cc = torch.empty(nq, dtype=torch.int32, device=dev)
    st = torch.zeros((nq, 3), dtype=torch.int64, device=dev)
    w["g8"].search_batch_device(tq8.data_ptr(), nq, ms, m, cand.data_ptr(), cd.data_ptr(), cc.data_ptr(), st.data_ptr(), 0, s)
    ids32 = cand.to(torch.int32)
    dd = torch.empty((nq, m), dtype=torch.float32, device=dev)
    w["r"].dists_device(tq.data_ptr(), nq, ids32.data_ptr(), m, dd.data_ptr(), 0, s)
    out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    out_c = torch.empty(nq, dtype=torch.int32, device=dev)
    st2 = torch.zeros((nq, 3), dtype=torch.int64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    rstatus = torch.zeros(1, dtype=torch.int32, device=dev)
    ga.RefinedGranne(w["g8"], w["r"]).search_batch_device(tq8.data_ptr(), tq.data_ptr(), nq, ms, m, k, out_i.data_ptr(), out_d.data_ptr(),
                                                         out_c.data_ptr(), st2.data_ptr(), status.data_ptr(), rstatus.data_ptr(), s)
    torch.cuda.synchronize(dev)
    ci, cb, cn = cand.cpu().numpy().view(np.uint64), dd.cpu().numpy().view(np.uint32), cc.cpu().numpy()
    eids = np.full((nq, k), U64_MAX, np.uint64)
    eds = np.full((nq, k), np.inf, np.float32)
    ecnt = np.zeros(nq, np.uint32)
    for i in range(nq):
        c = int(cn[i])
        order = np.lexsort((ci[i, :c], cb[i, :c]))[:k]
        ecnt[i] = order.size
        eids[i, :order.size] = ci[i, order]
        eds[i, :order.size] = cb[i, order].view(np.float32)
    assert_result((out_i.cpu().numpy().view(np.uint64), out_d.cpu().numpy(), out_c.cpu().numpy().view(np.uint32)), (eids, eds, ecnt))
    assert (st2.cpu().numpy() == st.cpu().numpy()).all()
    assert not status.cpu().numpy()[0] and rstatus.cpu().numpy()[0] == 0


def test_rows_only_handle_keeps_its_rows_and_equals_a_layered_one(ga, oracle, world):
    w = world
    assert w["r"].num_layers() == 0 and w["g"].num_layers() > 0
    for i in (0, 5, N - 1):
        assert w["r"].get_element(i).tobytes() == w["rows"][i].tobytes()
        assert w["r8"].get_element(i).tobytes() == w["rows8"][i].tobytes()
    rng = np.random.default_rng(8)
    cand = np.stack([rng.permutation(N)[:33] for _ in range(NQ)]).astype(np.uint64)
    assert w["r"].dists_many(w["q"], cand.astype(np.uint32)).tobytes() == w["g"].dists_many(w["q"], cand.astype(np.uint32)).tobytes()
    a, b = w["r"].refine(w["q"], cand, k=10), w["g"].refine(w["q"], cand, k=10)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert_result(a, model.refine(oracle, w["rows"], w["q"], cand, None, 10))
    # through the fused call too
    fa = ga.RefinedGranne(w["g8"], w["r"]).search_batch((w["q8"], w["q"]), 50, 10)
    fb = ga.RefinedGranne(w["g8"], w["g"]).search_batch((w["q8"], w["q"]), 50, 10)
    for x, y in zip(fa, fb):
        assert x.tobytes() == y.tobytes()


def test_sum_embeddings_handles(ga, oracle):
    """A compact SumEmbeddings index keeps no rows: ERR_INVALID as the re-ranking side, fine as the walked side."""
    from granne_amd import _lib
    rng = np.random.default_rng(12)
    v, n, dim, nq = 200, 1500, 32, 32
    tab = random_floats(rng, v, dim)
    lists = [[int(x) for x in rng.integers(0, v, int(rng.integers(1, 5)))] for _ in range(n + nq)]
    raw = np.zeros((n + nq, dim), np.float32)
    for i, t in enumerate(lists):
        acc = tab[t[0]].copy()
        for x in t[1:]:
            acc += tab[x]
        raw[i] = acc
    allrows = oracle.normalize_f32(raw)
    rows, q = allrows[:n], allrows[n:]
    oix = oracle.build_index(rows, num_neighbors=10, max_search=20, n_threads=8)
    se = ga.SumEmbeddings(tab, lists[:n])
    cix = ga.Granne("embeddings", se, oix.layers, compact=True)
    mix = ga.Granne("embeddings", se, oix.layers)
    cand = np.stack([rng.permutation(n)[:20] for _ in range(nq)]).astype(np.uint64)
    with pytest.raises(ga.GranneHipError) as e:
        cix.refine(q, cand, k=5)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ga.GranneHipError) as e:
        ga.RefinedGranne(mix, cix).search_batch((q, q), 30, 5)
    assert e.value.code == _lib.ERR_INVALID
    want = model.search_refined(oracle, oix, rows, q, q, 30, 30, 5)
    assert_result(ga.RefinedGranne(cix, mix).search_batch((q, q), 30, 5), want)
    assert_result(mix.refine(q, cand, k=5), model.refine(oracle, rows, q, cand, None, 5))


@pytest.mark.parametrize("nq", [0, 1, 1025])
def test_batch_sizes(ga, oracle, world, nq):
    rng = np.random.default_rng(nq)
    q = oracle.normalize_f32(random_floats(rng, nq, 100)) if nq else np.zeros((0, 100), np.float32)
    q8 = oracle.quantize(q) if nq else np.zeros((0, 100), np.int8)
    ids, ds, cnt = ga.RefinedGranne(world["g8"], world["r"]).search_batch((q8, q), 20, 10, refine_from=20)
    assert ids.shape == (nq, 10) and ds.shape == (nq, 10) and cnt.shape == (nq,)
    if nq:
        assert_result((ids, ds, cnt), model.search_refined(oracle, world["oix8"], world["rows"], q8, q, 20, 20, 10))


def test_arguments_on_live_handles(ga, world):
    from granne_amd import _lib
    rg = ga.RefinedGranne(world["g8"], world["r"])
    for ms, m, k in ((50, 0, 10), (2000, 1025, 10), (50, 50, 0), (20, 21, 10)):
        with pytest.raises(ga.GranneHipError) as e:
            rg.search_batch((world["q8"], world["q"]), ms, k, refine_from=m)
        assert e.value.code == _lib.ERR_INVALID
    L = _lib.lib()
    assert L.granne_hip_refine_device(world["r"]._h, None, 1, None, None, 8, 4, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.granne_hip_refine_device(world["r"]._h, None, 0, None, None, 8, 4, None, None, None, None, None) == _lib.OK  # nq 0: nothing to do
    assert L.granne_hip_search_refined_batch_device(world["g8"]._h, world["r"]._h, None, None, 0, 50, 50, 10, None, None, None, None,
                                                    None, None, None) == _lib.OK
