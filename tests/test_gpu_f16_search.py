"""Searches of an "angular_f16" index on the GPU against the f32 oracle over R = normalize_f32(widen(rows16)) -- the
definition of the container: ids, distance BYTES and counts are equal, on the general walker
(max_search <= 256) and on the exact walker (beyond), through every kind of search entry, and for dists / dist_pairs.
Oracle graphs are small and built once per shape."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import assert_counters, random_floats  # noqa: E402

NQ = 24
SHAPES = [(2000, 100), (1500, 28), (700, 3), (1200, 200), (600, 768), (500, 1)]
GENERAL = [1, 10, 64, 65, 256]  # max_search on the general walker: one, two and four list slots
EXACT = 300                     # ... and on the exact walker


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


_worlds = {}


def world(ga, oracle, n, dim):
    """rows16, the f32 rows R they stand for, an oracle graph over R, the GPU F16 index over rows16 and that graph."""
    if (n, dim) not in _worlds:
        rng = np.random.default_rng(n * 13 + dim)
        rows16 = oracle.normalize_f32(random_floats(rng, n, dim)).astype(np.float16)
        R = oracle.normalize_f32(rows16.astype(np.float32))
        built = oracle.build_index(R, num_neighbors=12, max_search=20, reinsert_elements=False, n_threads=0)
        oix = oracle.Index(R, built.layers)
        gix = ga.Granne("angular_f16", rows16, built.layers)
        q = oracle.normalize_f32(random_floats(rng, NQ, dim))
        _worlds[(n, dim)] = dict(rows16=rows16, R=R, oix=oix, gix=gix, q=q)
    return _worlds[(n, dim)]


def assert_same(got, want):
    ids, ds, cnt = got[:3]
    oi, od, oc = want[:3]
    bad = np.nonzero((ids != oi).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], oi[bad[:1]])
    assert ds.tobytes() == od.tobytes()
    assert (cnt == oc).all()


@pytest.mark.parametrize("n,dim", SHAPES)
def test_search_batch_equals_the_f32_oracle_over_the_widened_rows(ga, oracle, n, dim):
    from granne_amd import _lib
    w = world(ga, oracle, n, dim)
    gix, oix, q = w["gix"], w["oix"], w["q"]
    assert gix.dtype_code == _lib.F16 and gix.get_element(3).tobytes() == w["rows16"][3].tobytes()
    for ms in GENERAL + [EXACT]:
        for k in sorted({10, ms}):
            ids, ds, cnt, st = gix.search_batch(q, ms, k, stats=True)
            walker = gix.get_option(_lib.OPT_LAST_WALKER)
            want = oix.search_batch(q, ms, k)
            assert_same((ids, ds, cnt), want)
            assert_counters(st, want[3], exact=True)  # both walkers keep an exact visited set
            assert walker == (_lib.WALKER_EXACT if ms > 256 else _lib.WALKER_GENERAL), (ms, walker)
            assert walker not in (_lib.WALKER_REGISTER, _lib.WALKER_REGISTER_WIDE)


def test_single_query_search(ga, oracle):
    w = world(ga, oracle, 2000, 100)
    for qi in range(4):
        got = w["gix"].search(w["q"][qi], 50, 10)
        want = w["oix"].search(w["q"][qi], 50, 10)
        assert [i for i, _ in got] == [i for i, _ in want]
        assert np.array([d for _, d in got], np.float32).tobytes() == np.array([d for _, d in want], np.float32).tobytes()
    # raw queries go through Vector::from, as for "angular"
    raw = w["q"][:3] * np.float32(3.0)
    ids, ds, cnt = w["gix"].search_batch(raw, 50, 10, prepared=False)
    assert_same((ids, ds, cnt), w["oix"].search_batch(oracle.normalize_f32(raw), 50, 10))


def test_several_batches_in_one_launch(ga, oracle):
    import torch
    w = world(ga, oracle, 1500, 28)
    gix, q = w["gix"], w["q"]
    nb, nq, ef, k = 3, NQ // 3, 40, 7
    dq = [torch.from_numpy(q[b * nq:(b + 1) * nq].copy()).cuda() for b in range(nb)]
    ids = [torch.full((nq, k), -7, dtype=torch.int64, device="cuda") for _ in range(nb)]
    ds = [torch.zeros((nq, k), dtype=torch.float32, device="cuda") for _ in range(nb)]
    cnt = [torch.full((nq,), 99, dtype=torch.int32, device="cuda") for _ in range(nb)]
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptrs = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    gix.search_batches_device(ptrs(dq), nq, ef, k, ptrs(ids), ptrs(ds), ptrs(cnt), None, status.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    oi, od, oc, _ = w["oix"].search_batch(q, ef, k)
    for b in range(nb):
        sl = slice(b * nq, (b + 1) * nq)
        assert (ids[b].cpu().numpy().astype(np.uint64) == oi[sl]).all()
        assert ds[b].cpu().numpy().tobytes() == od[sl].tobytes()
        assert (cnt[b].cpu().numpy().astype(np.uint32) == oc[sl]).all()
    assert status[0].item() == 0


def test_coalesced_single_queries(ga, oracle):
    from concurrent.futures import ThreadPoolExecutor
    from granne_amd import _lib
    w = world(ga, oracle, 1200, 200)
    gix, q = w["gix"], w["q"]
    want = w["oix"].search_batch(q, 30, 10)
    gix.coalesce = True
    try:
        with ThreadPoolExecutor(8) as pool:
            got = list(pool.map(lambda i: gix.search_batch(q[i:i + 1], 30, 10), range(NQ)))
    finally:
        gix.coalesce = False
    for i, (ids, ds, cnt) in enumerate(got):
        assert (ids[0] == want[0][i]).all() and ds[0].tobytes() == want[1][i].tobytes() and cnt[0] == want[2][i]
    assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_GENERAL


def test_a_walk_handed_to_the_exact_walker_keeps_its_bits(ga, oracle):
    """Every vector twice: tied distances hand walks of the general walker over to the exact one inside a launch."""
    rng = np.random.default_rng(99)
    raw = random_floats(rng, 1000, 28)
    raw[500:] = raw[:500]
    rows16 = oracle.normalize_f32(raw).astype(np.float16)
    R = oracle.normalize_f32(rows16.astype(np.float32))
    built = oracle.build_index(R, num_neighbors=12, max_search=20, reinsert_elements=False, n_threads=0)
    gix = ga.Granne("angular_f16", rows16, built.layers)
    q = oracle.normalize_f32(random_floats(rng, NQ, 28))
    assert_same(gix.search_batch(q, 30, 30), oracle.Index(R, built.layers).search_batch(q, 30, 30))


# 1 .. 100 and 128: rows of up to four full blocks, held in registers; 170, 230, 333, 256: rows read in rounds of four
# blocks with a last round of 1, 3, 2 and 0 blocks (every branch of f16_dist_group)
@pytest.mark.parametrize("dim", [1, 7, 32, 100, 128, 170, 230, 256, 333])
def test_dists_and_dist_pairs_have_the_oracles_bytes(ga, oracle, dim):
    rng = np.random.default_rng(500 + dim)
    n, nq, m = 300, 5, 37
    rows16 = (random_floats(rng, n, dim) * np.float32(3.0)).astype(np.float16)  # not unit rows: normalised on read
    rows16[11] = 0
    R = oracle.normalize_f32(rows16.astype(np.float32))
    q = oracle.normalize_f32(random_floats(rng, nq, dim))
    gix = ga.Granne("angular_f16", rows16, [])
    ids = rng.integers(0, n, (nq, m)).astype(np.uint32)
    ids[0, 0] = 11
    want = np.array([[oracle.dist(R[i], q[qi]) for i in ids[qi]] for qi in range(nq)], np.float32)
    assert gix.dists_many(q, ids).tobytes() == want.tobytes()
    qidx = np.repeat(np.arange(nq, dtype=np.uint32), m)
    assert gix.dists(q, qidx, ids.reshape(-1)).tobytes() == want.tobytes()
    # an id beyond the rows is +inf
    far = ids.copy()
    far[1, 2] = n + 5
    got = gix.dists_many(q, far)
    assert np.isinf(got[1, 2]) and got[1, 3].tobytes() == want[1, 3].tobytes()
