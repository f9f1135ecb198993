"""BASELINE.json's full sizes (configs[1]/[2]: 10M x 100-d, f32 and int8; one shard of configs[3]: 12.5M x 200-d f32,
batch 4096 -- the fully unrolled 200-d walker) on the graph bench.py measures
(GranneBuilder with the reference's BuildConfig::default(): max_search 200, reinsertion), checked against the
CPU oracle on the same index -- ids, distance bits and counters of 2048 queries -- and through
size-independent properties:
  * every returned distance equals the oracle's distance for that (query, id) pair, bit for bit;
  * results are ascending by (dist, id), ids are distinct and < n, counts == k;
  * the walk is repeatable and independent of batch composition (idempotence);
  * elements of the set, used as queries, find themselves (the reference's verify_search,
    src/index/tests.rs:50-62);
  * a larger max_search never returns a worse k-th distance on the same query.
The same fixtures serve the operators that read rows by id * row_stride at ids past byte offset 2^32 of the device rows
(the f32 indexes are 5.12 GB and 11.2 GB): element preparation at the high end, get_element / get_sketch, dists, refine,
the exact scan, and angular_f16 rows made from the 200-d set (tests/high_ids.py holds the checks). Audited before their
first run -- every kernel and host function they reach widens to 64 bits before it multiplies a row id, a row count
or an element count; nothing had to be fixed: row_sketch_kernel, relayout_rows_kernel, inline_tails_kernel,
synth_rows_kernel, normalize_rows_kernel, quantize_rows_kernel, dists_kernel, refine_kernel, f16_dist_group,
f32_to_f16_kernel, f16_to_f32_kernel, the bf_* scan kernels with inv_norm_rows_kernel / inv_gmax_kernel /
bf_narrow_ids_kernel / bf_final_kernel, merge_topk_kernel; on the host grid_for, upload_elements_from_device,
make_inline_tails, make_scan_norms, make_row_sketch, get_element / get_sketch, the *_device preparation and conversion
entries, dists_launch, refine_launch, plan_scan, ScanScratch, granne_hip_brute_force_device (tests/README.md has the
notes). With GRANNE_FULLSIZE_N shrunk below the mark these tests run on the top of the id range and print that the
past-the-mark assertions did not run.
Set GRANNE_FULLSIZE_N / GRANNE_FULLSIZE_N200 to run on fewer points (defaults 10,000,000 / 12,500,000)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import high_ids  # noqa: E402
from tests.conftest import assert_counters  # noqa: E402

pytestmark = pytest.mark.gpu

N100 = int(os.environ.get("GRANNE_FULLSIZE_N", "10000000"))
N200 = int(os.environ.get("GRANNE_FULLSIZE_N200", "12500000"))
SEED = 0x6772616E6E65
# measured on the default graph: 0.566 (f32), 0.559 (i8) at 100-d; see test_members_find_themselves
SELF_BAR = {("f32", 100): 0.5, ("i8", 100): 0.5, ("f32", 200): 0.05}
CASES = {"f32": ("f32", N100, 100, 1024), "i8": ("i8", N100, 100, 1024), "f32x200": ("f32", N200, 200, 4096)}


class Built(tuple):
    """(kind, elements, queries, index, layer sizes, host layers) + the case's n, dim and batch"""


@pytest.fixture(scope="module", params=["f32", "i8", "f32x200"])
def built(request):
    import torch
    import granne_amd
    from granne_amd import _lib
    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    kind, N, DIM, NQ = CASES[request.param]
    request_param = kind

    def synth(seed, rows):
        raw = torch.empty((rows, DIM), dtype=torch.float32, device="cuda")
        _lib.check(lib.granne_hip_synth_rows_device(C.c_void_p(raw.data_ptr()), seed, 0, rows, DIM, 0, sp))
        if request_param == "f32":
            _lib.check(lib.granne_hip_normalize_f32_device(C.c_void_p(raw.data_ptr()), rows, DIM, 0, sp))
            return raw
        q = torch.empty((rows, DIM), dtype=torch.int8, device="cuda")
        _lib.check(lib.granne_hip_quantize_f32_device(C.c_void_p(raw.data_ptr()), C.c_void_p(q.data_ptr()), rows, DIM, 0, sp))
        return q

    el = synth(SEED, N)
    q = synth(SEED + 1, NQ)
    torch.cuda.synchronize()
    et = "angular" if request_param == "f32" else "angular_int"
    # BuildConfig::default() (src/index/mod.rs:220-231): the graph of bench.py's headline run
    b = granne_amd.GranneBuilder.from_device(et, el.data_ptr(), N, DIM, num_neighbors=30, max_search=200,
                                             reinsert_elements=True)
    b.build()
    ix = b.get_index()
    sizes = [b.layer_len(l) for l in range(b.num_layers())]
    layers = b.layers()  # host copies, for the oracle
    b.close()
    out = Built((request_param, el, q.cpu().numpy(), ix, sizes, layers))
    out.n, out.dim, out.nq = N, DIM, NQ
    return out


def test_layer_pyramid(built, oracle):
    _, _, _, ix, sizes, _ = built
    N = built.n
    assert sizes == [oracle.num_elements_in_layer(N, 15.0, l) for l in range(len(sizes))]
    assert len(ix) == N


def test_results_are_wellformed_and_distances_are_the_oracles(built, oracle):
    kind, el, q, ix, _, _ = built
    N = built.n
    q = q[:1024]
    ids, ds, cnt, st = ix.search_batch(q, 50, 10, stats=True)
    assert (cnt == 10).all()
    assert (ids < N).all()
    for i in range(len(q)):
        assert len(set(ids[i].tolist())) == 10
        keys = list(zip(ds[i].tolist(), ids[i].tolist()))
        assert keys == sorted(keys)
    # oracle distance for every returned pair (rows fetched from the device copy)
    flat = ids.reshape(-1).astype(np.int64)
    import torch
    rows = el[torch.from_numpy(flat).cuda()].cpu().numpy()
    want = np.array([oracle.dist(rows[j], q[j // 10]) for j in range(len(flat))], np.float32)
    assert want.tobytes() == ds.reshape(-1).tobytes()
    assert (st[:, 0] >= st[:, 1]).all() and (st[:, 1] >= 50).all()  # >= max_search expansions at the bottom


def test_bit_exact_against_the_oracle_on_the_bench_graph(built, oracle):
    """The same index on the host, walked by the CPU oracle: ids, distance bits and the three counters of
    every query must agree -- at max_search 50 (the headline; the 200-d case: one batch of 4096), 200 (configs[4])
    and 1 with k = 1."""
    from concurrent.futures import ThreadPoolExecutor
    kind, el, q, ix, _, layers = built
    N, DIM = built.n, built.dim
    h_el = np.empty(tuple(el.shape), np.float32 if kind == "f32" else np.int8)
    parts = 16
    bounds = [N * i // parts for i in range(parts + 1)]

    def cp(i):
        h_el[bounds[i]:bounds[i + 1]] = el[bounds[i]:bounds[i + 1]].cpu().numpy()
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(cp, range(parts)))
    oix = oracle.Index(h_el, layers)
    import torch
    import ctypes as C
    from granne_amd import _lib
    extra = torch.empty((1024, DIM), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib().granne_hip_synth_rows_device(C.c_void_p(extra.data_ptr()), SEED + 2, 0, 1024, DIM, 0,
                                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    raw = extra.cpu().numpy()
    more = oracle.normalize_f32(raw) if kind == "f32" else oracle.quantize(raw)
    queries = np.concatenate([q, more])
    for ms, k in [(50, 10), (200, 10), (1, 1)]:
        nq = len(queries) if ms == 50 else 256
        ids, ds, cnt, st = ix.search_batch(queries[:nq], ms, k, stats=True)
        oi, od, oc, octr = oix.search_batch(queries[:nq], ms, k, n_threads=0)
        assert (cnt == oc).all()
        assert (ids == oi).all(), (ms, int((ids != oi).any(axis=1).sum()))
        assert ds.tobytes() == od.tobytes()
        assert_counters(st, octr, exact=False)  # the default walkers keep no visited set: n_dist counts evaluations
        if ms == 50:  # the same walk with the exact bucket tables: every counter the reference's
            ix.set_option(_lib.OPT_VISITED16, 3)
            ids3, ds3, cnt3, st3 = ix.search_batch(queries[:nq], ms, k, stats=True)
            ix.set_option(_lib.OPT_VISITED16, 0)
            assert (ids3 == oi).all() and ds3.tobytes() == od.tobytes()
            assert_counters(st3, octr, exact=True)
    assert ix.last_slow_count() == 0


def test_idempotent_and_batch_independent(built):
    _, _, q, ix, _, _ = built
    q = q[:1024]
    a = ix.search_batch(q, 50, 10)
    b = ix.search_batch(q, 50, 10)
    assert (a[0] == b[0]).all() and a[1].tobytes() == b[1].tobytes()
    perm = np.random.default_rng(0).permutation(len(q))
    c = ix.search_batch(q[perm], 50, 10)
    assert (c[0] == a[0][perm]).all() and c[1].tobytes() == a[1][perm].tobytes()
    d = ix.search_batch(q[:7], 50, 10)
    assert (d[0] == a[0][:7]).all()


def test_members_find_themselves(built):
    kind, el, _, ix, _, _ = built
    N = built.n
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(N, 512, replace=False))
    import torch
    rows = el[torch.from_numpy(pick).cuda()].cpu().numpy()
    ids, ds, cnt = ix.search_batch(rows, 50, 1)
    hit = (ids[:, 0] == pick.astype(np.uint64))
    # int8 rows can collide exactly (distance 0 ties broken by id), so allow distance-0 matches
    ok = hit | (ds[:, 0] <= 1e-6)
    print("self-query hit rate at n=%d (%s): %.3f" % (N, kind, ok.mean()))
    # the reference's bar is 0.95 on 500-1500 points (src/index/tests.rs:50-62); on 10M i.i.d.-uniform 100-d points
    # at max_search 50 the default graph finds 56 % of its own members (the CPU oracle finds the same ones: the
    # walk is bit-identical, test above) -- the bar sits a margin below what the graph achieves
    assert ok.mean() > SELF_BAR[(kind, built.dim)], ok.mean()


def test_larger_max_search_is_never_worse(built):
    _, _, q, ix, _, _ = built
    d50 = ix.search_batch(q[:256], 50, 10)[1]
    d200 = ix.search_batch(q[:256], 200, 10)[1]
    assert (d200[:, 0] <= d50[:, 0]).mean() > 0.99
    assert (d200[:, 9] <= d50[:, 9]).mean() > 0.99


# ---- the row-reading operators at ids past byte offset 2^32 of the device rows (tests/high_ids.py) ----------------
# At the default sizes the f32 index is 10M rows of 512 bytes (ids >= 8,388,608 lie past 4 GiB) and the 200-d one 12.5M
# rows of 896 bytes (ids >= 4,793,491); the int8 one is 1.28 GB, a full-size operator check (tests/test_gpu_past_4gib.py
# holds the int8 rows past the mark). Audit of the address computations: tests/README.md.
def _range(built, what):
    return high_ids.Range(built.n, high_ids.device_row_stride(built[0], built.dim), "%s[%s x %d]" % (what, built[0], built.dim))


def test_prepared_rows_at_the_high_end_are_the_oracles(built, oracle):
    """normalize_f32_device / quantize_f32_device wrote the fixture's rows; nothing read the high ones back. The last
    4,096 rows, regenerated (synth_rows' row0 form) and prepared by the oracle, are the fixture's bytes. The mark here is
    that of the DENSE buffer the two kernels write (dim x 4 or dim bytes a row): the 200-d window lies 5.7 GB past it
    (dense rows n - 4096 .. and their aliases 5,368,709 rows below hold different pseudo-random bytes), the 100-d ones
    end below it (4.0 GB and 1.0 GB) and are checks of the range's top.
    Device memory on top of the fixture: 3 MB; host: 7 MB."""
    from granne_amd import _lib
    kind, el = built[0], built[1]
    n, dim, w = built.n, built.dim, min(4096, built.n)
    R = high_ids.Range(n, dim * (4 if kind == "f32" else 1), "dense rows[%s x %d]" % (kind, dim))
    if R.past:
        assert n - w >= R.top0
        print("  past-the-mark assertion ran: the window starts %d rows past the mark" % (n - w - R.top0))
    raw = high_ids.synth(_lib, SEED, n - w, w, dim, None).cpu().numpy()
    assert raw.tobytes() == oracle.synth_rows(SEED, n - w, w, dim).tobytes()
    want = oracle.normalize_f32(raw) if kind == "f32" else oracle.quantize(raw)
    assert el[n - w:].cpu().numpy().tobytes() == want.tobytes()


def test_get_element_and_sketch_at_high_ids(built):
    """get_element (a copy from elements + idx * row_stride, on the host) at 1,200 ids, 1,100 of them past the mark with
    n - 1, first_high and first_high - 1; for the 100-d f32 index the sketch table's last 4,096 lines against the host
    model of tests/test_sketch_bound.py. Truncated to 32 bits, id reads row id - 8,388,608 (512-byte rows) or the bytes
    at (id * 896) mod 2^32 (200-d): other pseudo-random rows (high_ids.aliases_differ asserts it).
    Device memory on top of the fixture: < 1 MB; host: < 2 MB."""
    from tests.test_sketch_bound import row_sketch
    kind, el, _, ix = built[:4]
    n = built.n
    R = _range(built, "get_element")
    high_ids.check_get_element(ix, el, R, np.random.default_rng(11))
    if kind == "f32" and built.dim == 100:
        w = min(4096, n)
        tab = ix.get_sketch(n - w, w)
        assert tab is not None and tab.tobytes() == row_sketch(el[n - w:].cpu().numpy()).tobytes()


def test_dists_at_high_ids(built, oracle):
    """dists_kernel through dists_many (64 x 128 ids, status word) and the pair form (8,192 pairs): half the ids past the
    mark, with n - 1, first_high, first_high - 1 and one id >= n (+inf, status 1); bit-equal to oracle.dist over rows
    fetched by torch indexing. A row offset truncated to 32 bits reads row id - 2^32 / 512 (or the bytes at
    (id * 896) mod 2^32): other rows, other distances.
    Device memory on top of the fixture: < 1 MB; host: 10 MB."""
    kind, el, q, ix = built[:4]
    high_ids.check_dists(oracle, ix, el, lambda r: r, q, _range(built, "dists"), np.random.default_rng(12))


def test_refine_at_high_ids(built, oracle):
    """refine_kernel: 64 ragged lists of up to 257 candidates from the same id mix, k = 10, one candidate >= n (dropped
    and counted), against tests/refine_model.py: ids, distance bytes, counts, the dropped word. Truncation aliases as in
    test_dists_at_high_ids.
    Device memory on top of the fixture: < 1 MB; host: 15 MB."""
    kind, el, q, ix = built[:4]
    high_ids.check_refine(oracle, ix, el, lambda r: r, q, _range(built, "refine"), np.random.default_rng(13))


def test_exact_scan_over_the_whole_index(built, oracle):
    """brute_force (k = 10 and 16) over every row: 16 of the fixture's queries and 16 member rows with ids past the mark
    (n - 1 and first_high among them), against a reference made in two stages (high_ids.scan_reference: float64 scores
    of all rows on the device by torch, the oracle's distances on the shortlist), guarded on the reference alone, with
    the assertions and tolerances of tests/test_gpu_bruteforce.py. A member query's rank 0 is the member itself at the
    oracle's self-distance: a scan whose tile addresses were truncated to 32 bits would never score the rows past the
    mark -- it would score their aliases (id - 2^32 / 512, other bytes) twice -- and the members past the mark, whose
    nearest other row is ~0.5 away, would be missing from their own lists.
    Device memory on top of the fixture: 2.7 GB (a 1M-row chunk in float64, its [32, 1M] scores and ids); host: 20 MB."""
    kind, el, q, ix = built[:4]
    n = built.n
    R = _range(built, "exact scan")
    rng = np.random.default_rng(14)
    mem = np.concatenate([[n - 1, R.top0], rng.integers(R.top0, n, 14)]).astype(np.int64)
    queries = np.concatenate([q[:16], high_ids.fetch(el, mem)])
    ref_i, _ = high_ids.check_exact_scan(oracle, ix, el, lambda r: r, queries, kind, {16 + j: int(i) for j, i in enumerate(mem)})
    if R.past:  # the fixture's queries find neighbours on both sides of the mark
        assert (ref_i[:16, :16] >= R.top0).any() and (ref_i[:16, :16] < R.top0).any()
        print("  past-the-mark assertions ran: 16 member queries with ids >= %d, %d of the other queries' 256 results past it"
              % (R.top0, int((ref_i[:16, :16] >= R.top0).sum())))


def test_f16_rows_past_the_mark(built, oracle):
    """angular_f16 rows past 4 GiB: the fixture's 12.5M x 200 f32 rows (10 GB dense) converted by
    granne_hip_f32_to_f16_device (5 GB dense), a rows-only handle over them (512-byte rows: 6.4 GB, ids >= 8,388,608 past
    the mark), get_element / dists / refine on it against the f32 oracle over normalize_f32(widen(row)), and
    granne_hip_f16_to_f32_device back over the whole buffer. Windows of 4,096 rows at the end and around the 4 GiB marks
    of the f32 buffer (row 5,368,709.1: 800-byte rows) and of the halves' (row 10,737,418.2: 400-byte rows). A flat index
    truncated to 32 bits reads element t - 2^32 of the buffer, 5.4M (f32) or 10.7M (halves) rows lower: other
    pseudo-random rows; a truncated row offset on the handle reads row id - 8,388,608.
    Device memory on top of the fixture: 5 + 6.4 GB while the handle lives, 5 + 10 GB for the way back; host: 30 MB."""
    import torch
    import granne_amd
    from granne_amd import _lib
    kind, el, q, _ = built[:4]
    if built.dim != 200:
        pytest.skip("rows of halves past 4 GiB are made from the 200-d case's rows only (5 GB of halves)")
    n, dim = built.n, built.dim
    lib = _lib.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    marks = sorted({high_ids.first_high(dim * 4), high_ids.first_high(dim * 2)})
    windows = [(max(0, m - 2048), min(n, m + 2048)) for m in marks if m + 2048 <= n] + [(max(0, n - 4096), n)]
    if len(windows) == 3:
        print("f16 conversions: windows around rows %d and %d (the 4 GiB marks of the f32 and f16 buffers) and at the end; "
              "past-the-mark assertions ran" % tuple(marks))
    else:
        print("f16 conversions: %d rows end below a 4 GiB mark; windows %s" % (n, windows))
    el16 = torch.empty((n, dim), dtype=torch.float16, device="cuda")
    _lib.check(lib.granne_hip_f32_to_f16_device(C.c_void_p(el.data_ptr()), C.c_void_p(el16.data_ptr()), n, dim, 0, sp))
    torch.cuda.synchronize()
    for a, b in windows:
        assert el16[a:b].cpu().numpy().tobytes() == el[a:b].cpu().numpy().astype(np.float16).tobytes(), (a, b)
    ix = granne_amd.Granne.from_device("angular_f16", el16.data_ptr(), n, dim, [], [], [])
    try:
        stride = high_ids.device_row_stride("f16", dim)
        assert ix.hbm_bytes() == n * stride and stride == 512
        R = high_ids.Range(n, stride, "f16 handle")

        def prep(rows16):
            return oracle.normalize_f32(rows16.astype(np.float32))
        high_ids.check_get_element(ix, el16, R, np.random.default_rng(21))
        high_ids.check_dists(oracle, ix, el16, prep, q, R, np.random.default_rng(22))
        high_ids.check_refine(oracle, ix, el16, prep, q, R, np.random.default_rng(23))
    finally:
        ix.close()
    back = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.granne_hip_f16_to_f32_device(C.c_void_p(el16.data_ptr()), C.c_void_p(back.data_ptr()), n, dim, 1, 0, sp))
    torch.cuda.synchronize()
    for a, b in windows:
        want = oracle.normalize_f32(el16[a:b].cpu().numpy().astype(np.float32))
        assert back[a:b].cpu().numpy().tobytes() == want.tobytes(), (a, b)
    del back, el16
    torch.cuda.empty_cache()


def test_reorder_at_full_size(built):
    """Granne::reorder (src/index/reorder.rs) at BASELINE size, through its size-independent properties.
    LAST in this module: it reorders the fixture's index in place."""
    import torch
    kind, el, q, ix, sizes, _ = built
    N = built.n
    if built.dim != 100:
        pytest.skip("reorder at full size is covered by the 100-d cases")
    before = ix.search_batch(q, 50, 10)
    order = ix.reorder()
    assert order.shape == (N,)
    assert np.array_equal(np.sort(order), np.arange(N, dtype=np.uint64))  # a permutation
    lens = [0] + sizes
    for a, b in zip(lens[:-1], lens[1:]):  # layer preserving (reorder.rs:87-90)
        assert int(order[a:b].min()) == a and int(order[a:b].max()) == b - 1
    if len(sizes) >= 2:  # layer 0 keeps its order; layer 1's keys all map to 0 -> idx order (:136-137,159)
        assert np.array_equal(order[: lens[2]], np.arange(lens[2], dtype=np.uint64))
        assert not np.array_equal(order[lens[2]:], np.arange(lens[2], N, dtype=np.uint64))
    # the reference's own test (:311-320): same results modulo the permutation
    after = ix.search_batch(q, 50, 10)
    assert after[1].tobytes() == before[1].tobytes() and (after[2] == before[2]).all()
    distinct = (np.diff(before[1], axis=1) > 0).all(axis=1)  # a distance tie may swap with the new ids
    assert distinct.mean() > 0.99
    assert np.array_equal(order[after[0][distinct].astype(np.int64)], before[0][distinct])
    # elements moved with their ids; neighbor sets come out sorted (MultiSetVector::push)
    pick = np.random.default_rng(2).choice(N, 64, replace=False)
    rows = el[torch.from_numpy(order[pick].astype(np.int64)).cuda()].cpu().numpy()
    for j, i in enumerate(pick.tolist()):
        assert ix.get_element(i).tobytes() == rows[j].tobytes()
        nb = ix.get_neighbors(i)
        assert nb == sorted(nb) and len(set(nb)) == len(nb) and all(x < N for x in nb)


def test_c1_glove_example_shape(oracle):
    """BASELINE.json configs[0] = examples/glove.rs:46-60: ~400k x 100-d f32, `BuildConfig::default().max_search(10)`,
    then `index.search(&index.get_element(i), 200, 10)` for i in 0, 134, 5555, 37000 (one query per call, members of the
    set). GloVe is not in this image: the benchmark's synthetic rows stand in. Through the product: GranneBuilder ->
    get_index -> get_element -> search (granne_hip_search, host pointers), against the CPU oracle on the same graph."""
    import torch
    import granne_amd
    from granne_amd import _lib
    lib = _lib.lib()
    n, dim = 400_000, 100
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    el = torch.empty((n, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.granne_hip_synth_rows_device(C.c_void_p(el.data_ptr()), SEED + 50, 0, n, dim, 0, sp))
    _lib.check(lib.granne_hip_normalize_f32_device(C.c_void_p(el.data_ptr()), n, dim, 0, sp))
    torch.cuda.synchronize()
    b = granne_amd.GranneBuilder.from_device("angular", el.data_ptr(), n, dim, num_neighbors=30, max_search=10,
                                             reinsert_elements=True)
    b.build()
    assert [b.layer_len(l) for l in range(b.num_layers())] == [8, 119, 1778, 26667, 400000]  # src/index/tests.rs:314-334
    ix = b.get_index()
    oix = oracle.Index(el.cpu().numpy(), b.layers())
    for i in (0, 134, 5555, 37000):
        x = ix.get_element(i)
        res = ix.search(x, 200, 10)
        oi, od, oc, _ = oix.search_batch(x[None], 200, 10)
        assert len(res) == int(oc[0]) == 10
        assert [r[0] for r in res] == oi[0].tolist()
        assert np.array([r[1] for r in res], np.float32).tobytes() == od[0].tobytes()
        # whenever the walk reaches the member itself it is the nearest, at max(0, 1 - x.x) (a few ulps of 1 at most)
        if i in [r[0] for r in res]:
            assert res[0][0] == i and 0.0 <= res[0][1] <= 4e-7
    # 512 members in one call: same ids as the oracle; most find themselves (the graph was built with max_search 10)
    mem = np.arange(0, n, n // 512)[:512]
    q = el[torch.from_numpy(mem).cuda()].cpu().numpy()
    ids, ds, cnt = ix.search_batch(q, 200, 10)
    oi, od, oc, _ = oix.search_batch(q, 200, 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
    assert (ids[:, 0] == mem).mean() > 0.5


def test_c5_shard_shape_int8_max_search_200_batch_4096(oracle):
    """BASELINE.json configs[4] as one shard holds it: 100-d int8 rows, max_search 200 (four list slots of the register
    walker), batches of 4096, seven layers -- at 25M points (a shard of the real job has 125M and the same seven layers:
    bench.py's c5_shard sub-record measures that one; its host copy alone is 30 GB). 4,096 queries against the CPU oracle
    on the same index: ids, distance bits, counters. Set GRANNE_FULLSIZE_N_C5 for another size."""
    import torch
    import granne_amd
    from granne_amd import _lib
    from concurrent.futures import ThreadPoolExecutor
    lib = _lib.lib()
    n, dim, nq, ef, k = int(os.environ.get("GRANNE_FULLSIZE_N_C5", "25000000")), 100, 4096, 200, 10
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    el = torch.empty((n, dim), dtype=torch.int8, device="cuda")
    step = 12_500_000
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        raw = torch.empty((r1 - r0, dim), dtype=torch.float32, device="cuda")
        _lib.check(lib.granne_hip_synth_rows_device(C.c_void_p(raw.data_ptr()), SEED, r0, r1 - r0, dim, 0, sp))
        _lib.check(lib.granne_hip_quantize_f32_device(C.c_void_p(raw.data_ptr()), C.c_void_p(el[r0:r1].data_ptr()), r1 - r0, dim, 0, sp))
        torch.cuda.synchronize()
        del raw
    rawq = torch.empty((nq, dim), dtype=torch.float32, device="cuda")
    _lib.check(lib.granne_hip_synth_rows_device(C.c_void_p(rawq.data_ptr()), SEED + 1, 0, nq, dim, 0, sp))
    q = torch.empty((nq, dim), dtype=torch.int8, device="cuda")
    _lib.check(lib.granne_hip_quantize_f32_device(C.c_void_p(rawq.data_ptr()), C.c_void_p(q.data_ptr()), nq, dim, 0, sp))
    torch.cuda.synchronize()
    b = granne_amd.GranneBuilder.from_device("angular_int", el.data_ptr(), n, dim, num_neighbors=30, max_search=200,
                                             reinsert_elements=True)
    b.build()
    sizes = [b.layer_len(l) for l in range(b.num_layers())]
    assert sizes == [oracle.num_elements_in_layer(n, 15.0, l) for l in range(len(sizes))]
    if n == 25_000_000:
        assert len(sizes) == 7  # like the 125M shard (src/index/mod.rs:634-643)
    ix = b.get_index()
    layers = b.layers()
    b.close()
    h_el = np.empty((n, dim), np.int8)
    parts = 16
    bounds = [n * i // parts for i in range(parts + 1)]

    def cp(i):
        h_el[bounds[i]:bounds[i + 1]] = el[bounds[i]:bounds[i + 1]].cpu().numpy()
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(cp, range(parts)))
    oix = oracle.Index(h_el, layers)
    h_q = q.cpu().numpy()
    ids, ds, cnt, st = ix.search_batch(h_q, ef, k, stats=True)
    assert ix.get_option(_lib.OPT_LAST_WALKER) == 1  # the register walker
    oi, od, oc, octr = oix.search_batch(h_q, ef, k, n_threads=0)
    assert (cnt == oc).all() and (ids == oi).all(), int((ids != oi).any(axis=1).sum())
    assert ds.tobytes() == od.tobytes()
    assert_counters(st, octr, exact=False)
    assert ix.last_slow_count() == 0
    # the same batch as part of a launch of several (how bench.py hands batches over) and with the exact visited set
    ix.set_option(_lib.OPT_VISITED16, 3)
    ids3, ds3, cnt3, st3 = ix.search_batch(h_q[:1024], ef, k, stats=True)
    ix.set_option(_lib.OPT_VISITED16, 0)
    assert (ids3 == oi[:1024]).all() and ds3.tobytes() == od[:1024].tobytes()
    assert_counters(st3, octr[:1024], exact=True)


@pytest.mark.parametrize("data", ["latent", "mixture"])
def test_graph_quality_on_data_with_structure(data):
    """The reference's own quality bar (verify_search, src/index/tests.rs:50-62: members of the set, searched at
    (max_search, 1), find themselves more than 95 % of the time) holds on 10M-point graphs the GPU builder makes -- on data
    with structure (bench.py's two secondary generators at 1M points). On BASELINE's i.i.d.-uniform 100-d points no graph
    of this family reaches it (test_members_find_themselves states what it does reach), which is why a build gone wrong
    would not show there and must show here."""
    import types
    import torch
    import bench
    import granne_amd
    n, dim = 1_000_000, 100
    args = types.SimpleNamespace(gpus=1)
    os.environ.pop("WORLD_SIZE", None)
    B = bench.Bench(args)
    el = B.rows(data, SEED, 0, n, dim, "f32")
    torch.cuda.synchronize()
    b = granne_amd.GranneBuilder.from_device("angular", el.data_ptr(), n, dim, num_neighbors=30, max_search=200,
                                             reinsert_elements=True)
    b.build()
    ix = b.get_index()
    b.close()
    mem = torch.arange(0, n, n // 4096, device="cuda")[:4096]
    rows = el[mem].cpu().numpy()
    ids, ds, cnt = ix.search_batch(rows, 50, 1)
    hit = (ids[:, 0] == mem.cpu().numpy().astype(np.uint64)) | (ds[:, 0] <= 1e-6)
    print("self-query hit rate, %s, n=%d: %.4f" % (data, n, hit.mean()))
    assert hit.mean() > 0.95, hit.mean()
