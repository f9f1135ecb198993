"""SumEmbeddings on the GPU against a host model of a few lines: raw = table[t0].copy(); raw += table[t] for the other
terms in list order (float32), then oracle.normalize_f32(raw) -- what embeddings/mod.rs:124-143 and :164-166 compute. A
walk over the container is a walk over those dense rows, so oracle.Index / oracle.build_index over the model's rows are
the reference for the materialised index, the compact index and the builder alike."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import assert_counters, random_floats  # noqa: E402

MAX_SEARCH = [1, 10, 50, 200, 1024]


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def make_table(rng, v, dim):
    """Rows uniform in [-0.5, 0.5) (src/test_helper.rs:3-6); row 1 is -row 0, so the list [0, 1] sums to zero."""
    tab = random_floats(rng, v, dim)
    tab[1] = -tab[0]
    return tab


def make_lists(rng, n, v, max_terms=40, dups=0):
    """Term lists of 0..max_terms ids, a skewed draw so that common words repeat; on purpose: empty lists, a term twice
    in one list, two lists that are permutations of each other, exact duplicate lists, and the pair that sums to zero."""
    lists = []
    for _ in range(n):
        k = int(rng.integers(0, max_terms + 1)) if rng.random() < 0.3 else int(rng.integers(1, 9))
        lists.append([int(x) for x in np.minimum((rng.random(k) ** 3 * v).astype(np.int64), v - 1)])
    lists[0] = []
    lists[1] = [5, 5]
    lists[2] = [7, 3, 7, 9, 3]
    lists[3] = [11, 12, 13, 14, 15, 16]
    lists[4] = [16, 15, 14, 13, 12, 11]  # a permutation of lists[3]: the sums differ in their last bits at most
    lists[5] = list(lists[3])            # an exact duplicate
    lists[6] = [0, 1]                    # row 1 = -row 0: the zero vector
    lists[7] = [1, 0]
    lists[n - 1] = []
    for i in range(dups):                # many exact duplicates: ties everywhere
        lists[8 + i] = list(lists[8 + (i % 5)])
    return lists


def model_rows(oracle, tab, lists, normalized=True):
    out = np.zeros((len(lists), tab.shape[1]), np.float32)
    for i, t in enumerate(lists):
        if len(t):
            raw = tab[t[0]].copy()
            for x in t[1:]:
                raw += tab[x]
            out[i] = raw
    return oracle.normalize_f32(out) if normalized else out


def assert_same(oix, gix, q, ms, k, exact):
    ids, ds, cnt, st = gix.search_batch(q, ms, k, stats=True)
    oi, od, oc, octr = oix.search_batch(q, ms, k)
    assert (ids == oi).all(), (ms, np.nonzero((ids != oi).any(axis=1))[0][:5])
    assert ds.tobytes() == od.tobytes() and (cnt == oc).all()
    assert_counters(st, octr, exact)
    return ids, ds, cnt


@pytest.mark.parametrize("dim", [1, 3, 31, 32, 33, 100, 200, 300])
def test_rows_have_the_host_models_bits(ga, oracle, dim):
    rng = np.random.default_rng(100 + dim)
    v, n = 300, 700
    tab = make_table(rng, v, dim)
    lists = make_lists(rng, n, v)
    se = ga.SumEmbeddings(tab, lists)
    raw, nrm = model_rows(oracle, tab, lists, False), model_rows(oracle, tab, lists, True)
    # the range entry: the whole container, a range inside it, single elements
    assert se.get_embeddings().tobytes() == raw.tobytes()
    assert se.get_embeddings(normalized=True).tobytes() == nrm.tobytes()
    assert se.get_embeddings(65, 130, normalized=True).tobytes() == nrm[65:195].tobytes()
    assert se.get_embedding(2).tobytes() == raw[2].tobytes() and se.get(6).tobytes() == nrm[6].tobytes()
    assert not se.get(6).any() and not se.get(0).any()  # the zero vector stays zero (norm > 0 guards the division)
    # the term-list entry (queries)
    assert se.create_embeddings(lists).tobytes() == raw.tobytes()
    assert se.create_embeddings(lists, normalized=True).tobytes() == nrm.tobytes()
    assert se.create_embedding(lists[2]).tobytes() == raw[2].tobytes()
    with pytest.raises(ga.GranneHipError):
        se.create_embedding([v])


def test_rows_into_strided_device_buffers(ga, oracle):
    import torch
    from granne_amd import _lib
    rng = np.random.default_rng(5)
    tab = make_table(rng, 100, 33)
    lists = make_lists(rng, 200, 100)
    se = ga.SumEmbeddings(tab, lists)
    nrm = model_rows(oracle, tab, lists, True)
    out = torch.full((50, 40), 7.0, dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().granne_hip_sum_embeddings_materialize_device(se._h, 20, 50, 1, C.c_void_p(out.data_ptr()), 40, None))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:, :33].tobytes() == nrm[20:70].tobytes() and (got[:, 33:] == 7.0).all()
    off, ids = ga.embeddings.csr_of(lists[:64])
    to, ti = torch.from_numpy(off.view(np.int64)).cuda(), torch.from_numpy(ids.view(np.int32)).cuda()
    out2 = torch.zeros((64, 33), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().granne_hip_sum_embeddings_embed_device(se._h, C.c_void_p(to.data_ptr()), C.c_void_p(ti.data_ptr()), 64, 1,
                                                                 C.c_void_p(out2.data_ptr()), 33, None))
    torch.cuda.synchronize()
    assert out2.cpu().numpy().tobytes() == nrm[:64].tobytes()
    assert _lib.lib().granne_hip_sum_embeddings_materialize_device(se._h, 190, 11, 1, C.c_void_p(out.data_ptr()), 40, None) == _lib.ERR_INVALID
    assert _lib.lib().granne_hip_sum_embeddings_materialize_device(se._h, 0, 1, 1, C.c_void_p(out.data_ptr()), 32, None) == _lib.ERR_INVALID


@pytest.fixture(scope="module", params=[(4000, 100, 0), (2500, 33, 0), (3000, 100, 1200)], ids=["100d", "33d", "duplicates"])
def world(request, ga, oracle):
    n, dim, dups = request.param
    rng = np.random.default_rng(n + dim + dups)
    v = 600
    tab = make_table(rng, v, dim)
    lists = make_lists(rng, n, v, dups=dups)
    rows = model_rows(oracle, tab, lists)
    oix = oracle.build_index(rows, num_neighbors=30, max_search=40, n_threads=8)
    qlists = make_lists(rng, 96, v, max_terms=12)
    q = model_rows(oracle, tab, qlists)
    se = ga.SumEmbeddings(tab, lists)
    return dict(se=se, rows=rows, oix=oix, q=q, qlists=qlists, dups=dups, dim=dim)


def test_materialised_index_equals_the_oracle(ga, world):
    from granne_amd import _lib
    gix = ga.Granne("embeddings", world["se"], world["oix"].layers)
    assert len(gix) == len(world["rows"]) and gix.get_element(3).tobytes() == world["rows"][3].tobytes()
    for ms in MAX_SEARCH:
        assert_same(world["oix"], gix, world["q"], ms, 10, exact=False)
    gix.set_option(_lib.OPT_VISITED16, 3)  # the exact visited set: n_dist is the reference's count
    for ms in MAX_SEARCH:
        assert_same(world["oix"], gix, world["q"], ms, 10, exact=True)
    # term-id queries are embedded on the device: the same answers
    ids, ds, cnt = gix.search_batch(world["qlists"], 50, 10)
    oi, od, oc, _ = world["oix"].search_batch(world["q"], 50, 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
    assert gix.search(world["qlists"][9], 50, 5) == [(int(i), float(d)) for i, d in zip(oi[9, :5], od[9, :5])]


def test_compact_index_equals_the_oracle_on_every_walker(ga, world):
    from granne_amd import _lib
    cix = ga.Granne("embeddings", world["se"], world["oix"].layers, compact=True)
    assert len(cix) == len(world["rows"])
    for i in (0, 3, 6, len(world["rows"]) - 1):
        assert cix.get_element(i).tobytes() == world["rows"][i].tobytes()
    for ms in MAX_SEARCH:
        assert_same(world["oix"], cix, world["q"], ms, 10, exact=True)
        want = _lib.WALKER_GENERAL if ms <= 256 else _lib.WALKER_EXACT
        assert cix.get_option(_lib.OPT_LAST_WALKER) == want
    # every query through the exact walker
    cix.set_option(_lib.OPT_FORCE_SLOW, 1)
    for ms in MAX_SEARCH:
        assert_same(world["oix"], cix, world["q"], ms, 10, exact=True)
        assert cix.last_slow_count() == len(world["q"])
    cix.set_option(_lib.OPT_FORCE_SLOW, 0)
    # hand-overs inside a launch: a visited table far too small and no overflow table (tests/test_gpu_parity.py,
    # test_visited_table_overflow_hands_over). Seen on the GPU: every one of these launches hands walks over.
    cix.set_option(_lib.OPT_VISITED_SLOTS, 256)
    cix.set_option(_lib.OPT_OVERFLOW_SLOTS, 1)
    for ms in (50, 100, 200):
        assert_same(world["oix"], cix, world["q"], ms, 10, exact=True)
        print("hand-overs at max_search %d: %d of %d" % (ms, cix.last_slow_count(), len(world["q"])))
        assert cix.last_slow_count() > 0
    cix.set_option(_lib.OPT_VISITED_SLOTS, 0)
    cix.set_option(_lib.OPT_OVERFLOW_SLOTS, 0)
    assert_same(world["oix"], cix, world["q"], 100, 10, exact=True)


def test_compact_and_materialised_results_are_equal_bytes(ga, world):
    rng = np.random.default_rng(9)
    se = world["se"]
    gix = ga.Granne("embeddings", se, world["oix"].layers)
    cix = ga.Granne("embeddings", se, world["oix"].layers, compact=True)
    for i in range(12):  # one query per call
        a, b = gix.search(world["q"][i], 50, 10), cix.search(world["q"][i], 50, 10)
        assert a == b and len(a) == 10
        assert cix.search(world["qlists"][i], 50, 10) == a
    q = world["rows"][rng.integers(0, len(world["rows"]), 1024)]  # a batch of 1024
    q = np.ascontiguousarray(q + np.float32(0.01) * random_floats(rng, 1024, world["dim"]))
    q = ga.normalize(q)
    for ms in (50, 200):
        a, b = gix.search_batch(q, ms, 10), cix.search_batch(q, ms, 10)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_compact_index_on_the_device_entry_points_and_as_a_shard(ga, world):
    import torch
    from granne_amd import _lib
    from granne_amd.sharded import ShardedHost
    cix = ga.Granne("embeddings", world["se"], world["oix"].layers, compact=True)
    q = world["q"]
    oi, od, oc, _ = world["oix"].search_batch(q, 50, 10)
    nq = len(q)
    tq = torch.from_numpy(q).cuda()
    ids = torch.zeros((nq, 10), dtype=torch.int64, device="cuda")
    ds = torch.zeros((nq, 10), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    t = cix.search_begin_device(tq.data_ptr(), nq, 50, 10, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), stream=s)
    cix.search_end_device(t, s)
    torch.cuda.synchronize()
    assert (ids.cpu().numpy().astype(np.uint64) == oi).all() and ds.cpu().numpy().tobytes() == od.tobytes()
    packed = torch.zeros(int(_lib.lib().granne_hip_packed_topk_bytes(nq, 10)), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().granne_hip_search_batch_packed_device(cix._h, C.c_void_p(tq.data_ptr()), nq, 50, 10,
                                                                C.c_void_p(packed.data_ptr()), None, C.c_void_p(s)))
    torch.cuda.synchronize()
    raw = packed.cpu().numpy()
    assert (raw[:nq * 80].view(np.uint64).reshape(nq, 10) == oi).all()
    assert raw[nq * 80:nq * 120].tobytes() == od.tobytes()
    sh = ShardedHost([cix], [0])
    si, sd, sc = sh.search_batch(q, 50, 10)
    assert (si == oi).all() and sd.tobytes() == od.tobytes() and (sc == oc).all()


def test_unsupported_calls_on_a_compact_index_are_invalid(ga, world):
    from granne_amd import _lib
    L = _lib.lib()
    cix = ga.Granne("embeddings", world["se"], world["oix"].layers, compact=True)
    q = world["q"][:4]
    p = q.ctypes.data_as(C.c_void_p)
    out = np.zeros(4096, np.uint64)
    o = out.ctypes.data_as(C.c_void_p)
    n = len(cix)
    calls = {
        "brute_force": lambda: L.granne_hip_brute_force(cix._h, p, 4, 5, o, o, o),
        "brute_force_device": lambda: L.granne_hip_brute_force_device(cix._h, p, 4, 5, o, o, o, None),
        "dists_device": lambda: L.granne_hip_dists_device(cix._h, p, 4, o, 2, o, None, None),
        "dist_pairs_device": lambda: L.granne_hip_dist_pairs_device(cix._h, p, o, o, 2, o, None),
        "dist_pairs": lambda: L.granne_hip_dist_pairs(cix._h, p, 4, o, o, 2, o),
        "reorder": lambda: L.granne_hip_index_reorder(cix._h, None),
        "reorder_by_keys": lambda: L.granne_hip_index_reorder_by_keys(cix._h, np.zeros(n, np.uint64).ctypes.data_as(C.c_void_p), None),
        "get_sketch": lambda: L.granne_hip_index_get_sketch(cix._h, 0, 1, o),
    }
    for name, call in calls.items():
        assert call() == _lib.ERR_INVALID, name
        assert b"MATERIALIZED" in L.granne_hip_last_error(), name
    # and the index is as good as before
    ids, ds, cnt = cix.search_batch(world["q"], 50, 10)
    oi, od, _, _ = world["oix"].search_batch(world["q"], 50, 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes()


def test_hbm_bytes_of_the_two_forms(ga):
    """n = 200,000, V = 5,000, dim 100, mean 6 terms: about 9 MB of container against 80 MB of rows (102 MB with the
    rows' 512-byte pitch). No search, only the byte counts."""
    rng = np.random.default_rng(1)
    n, v, dim = 200_000, 5_000, 100
    tab = make_table(rng, v, dim)
    cnt = rng.integers(0, 13, n)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(cnt)
    terms = rng.integers(0, v, int(off[-1])).astype(np.uint32)
    se = ga.SumEmbeddings(tab, offsets=off, terms=terms)
    layers = [np.full((n, 30), 0xFFFFFFFF, np.uint32)]
    cix = ga.Granne("embeddings", se, layers, compact=True)
    gix = ga.Granne("embeddings", se, layers)
    layer_bytes = n * 32 * 4
    row_pitch = 400  # 100 floats, a multiple of 16 bytes
    want = v * row_pitch + 8 * (n + 1) + 4 * len(terms)
    assert se.hbm_bytes() == want
    storage = cix.hbm_bytes() - layer_bytes
    assert want <= storage <= want + 3 * 256  # alignment slack of the three allocations at most
    assert gix.hbm_bytes() - layer_bytes >= n * dim * 4
    assert cix.hbm_bytes() < gix.hbm_bytes() and storage * 8 < gix.hbm_bytes() - layer_bytes


BUILDS = [(3000, 100, 30, 40, 256), (1500, 28, 20, 20, 64)]


@pytest.mark.parametrize("n,dim,nn,ms,bmax", BUILDS)
def test_builder_over_a_container_equals_the_builder_over_its_rows(ga, oracle, n, dim, nn, ms, bmax):
    rng = np.random.default_rng(n + dim)
    v = 500
    tab = make_table(rng, v, dim)
    lists = make_lists(rng, n, v)
    rows = model_rows(oracle, tab, lists)
    se = ga.SumEmbeddings(tab, lists)
    b = ga.GranneBuilder("embeddings", se, num_neighbors=nn, max_search=ms, batch_max=bmax, batch_div=8)
    b.build()
    assert len(b) == n and b.num_elements() == n
    oix = oracle.build_index(rows, num_neighbors=nn, max_search=ms, batch_max=bmax, batch_div=8, n_threads=0)
    assert b.num_layers() == len(oix.layers)
    for l, want in enumerate(oix.layers):
        got = b.get_layer(l)
        assert got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, (l, bad[:5], got[bad[:1]], want[bad[:1]])
    q = model_rows(oracle, tab, make_lists(rng, 32, v, max_terms=10))
    gix, cix = b.get_index(), b.get_index(compact=True)
    oi, od, oc, _ = oix.search_batch(q, 30, 10)
    for ix in (gix, cix):
        ids, ds, cnt = ix.search_batch(q, 30, 10)
        assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
    b.build()  # the builder is still whole after handing both out
    assert len(b) == n and b.get_layer(len(oix.layers) - 1).tobytes() == oix.layers[-1].tobytes()


def test_files_round_trip_in_both_modes(ga, world, tmp_path):
    se, oix, q = world["se"], world["oix"], world["q"]
    pi, pt, pe = str(tmp_path / "index.bin"), str(tmp_path / "table.bin"), str(tmp_path / "elements.bin")
    cix = ga.Granne("embeddings", se, oix.layers, compact=True)
    cix.save_index(pi)
    se.save_embeddings(pt)
    se.save_elements(pe)
    want = cix.search_batch(q, 50, 10)
    for compact in (False, True):
        ix = ga.Granne.from_files(pi, "embeddings", pe, embeddings_path=pt, compact=compact)
        assert len(ix) == len(cix) and ix.num_layers() == cix.num_layers()
        for x, y in zip(ix.search_batch(q, 50, 10), want):
            assert x.tobytes() == y.tobytes()
        for x, y in zip(ix.search_batch(world["qlists"], 50, 10), want):
            assert x.tobytes() == y.tobytes()
    with pytest.raises(ga.GranneHipError):
        cix.save_elements(str(tmp_path / "rows.bin"))
