"""Int8 rows past byte offset 2^32 of an index: 40,000,000 x 100-d int8 rows are 128-byte device rows, 5.12 GB, and the
ids >= 2^25 = 33,554,432 (16 % of the set) start past 4 GiB. The largest int8 index of the other modules ends just below
the mark (25M rows, 3.2 GB). The bottom layer's device copy (32 ids a node) is 5.12 GB too: nodes >= 2^25 have their
adjacency rows past the mark as well.

The walk is defined on any graph, so no 20-second build is made: the fixture writes a circulant graph on the device
with torch -- node i of a layer of length L has the neighbours (i + s) mod L for 16 fixed strides s -- two prefix-nested
layers [4096, n]. It copies rows and layers to the host once for the CPU oracle. Eight rows are overwritten with rows of
the query set before the index is made (PLANTS): the exact scan must find them.

What a row offset truncated to 32 bits would do: id >= 2^25 reads row id - 2^25 (2^32 / 128 exactly), another
pseudo-random row of the set (tests/high_ids.py aliases_differ asserts that the bytes differ), so every distance of such
an id, and with it the walk's order, the operators' results and the scan's lists, would change.

Audited before the first run (tests/README.md has the list): every address computation of the kernels and host
functions these tests reach widens to 64 bits before it multiplies a row id, a row count or an element count; nothing
had to be fixed. bf_i8_ring_kernel's tile base is `elements + e0 * 128` with a 64-bit e0 and its per-lane offsets stay
inside a tile (< 16 KB); its norm offsets are 32-bit by design for n < 2^29, the dispatch rule's bound.

Peaks, from the shapes. Device, fixture: dense rows 4.0 GB + one 4M-row f32 chunk 1.6 GB while the rows are made; then
the layer tensor 2.56 GB + 1 GB of int64 chunk; the index 5.12 GB rows + 5.12 GB bottom layer + 0.17 GB norms: 17 GB at
its peak (the index made, the fixture's layer tensor not yet freed), 14.4 GB afterwards. The scan's reference adds 2 GB
(a 1M-row chunk in float64, its [32, 1M] scores and ids). Host: rows 4.0 GB + layers 2.56 GB = 6.6 GB, the oracle reads
them in place."""
import ctypes as C

import numpy as np
import pytest

from tests import high_ids
from tests.conftest import assert_counters

pytestmark = pytest.mark.gpu

N, DIM = 40_000_000, 100
MARK_ID = 1 << 25  # 2^32 / 128
SEED = 0x6772616E6E65 + 40
TOP = 4096
# (i + s) mod L: distinct, 0 < s < L -- no self loop, no id twice in a row. Among them 1, L - 1, ~L/2 + 1, ~L/3, ~L/7.
# The bottom layer's other eleven lie one in each remaining sixteenth of the circle, so that EVERY node has two or three
# neighbours past the mark (strides bunched below L sent walks into the middle of the id range, where no neighbour
# is: on the CPU oracle 1 query in 256 then ranked no row past the mark at max_search 50; with these the fewest is 3).
STRIDES_TOP = [1, 4095, 2049, 1365, 585, 3, 4093, 17, 4001, 255, 3071, 1023, 777, 2500, 3333, 129]
STRIDES_BOTTOM = [1, N - 1, N // 2 + 1, N // 3, N // 7, 3750007, 8750011, 11250003, 16250009, 18750017, 23750021, 26250013,
                  28750003, 31250027, 33750001, 36250019]
# planted rows: (id, row of the query set). ids n - 1 and 2^25 - 1 carry the same row: the smaller id stands first.
PLANTS = [(N - 1, 0), (N - 33, 1), (MARK_ID, 2), (MARK_ID - 1, 0), (34567891, 3), (36000001, 4), (38123457, 5), (39999000, 6)]
CONFIGS = [(1, 1), (50, 10), (200, 10), (300, 40), (1024, 10)]


@pytest.fixture(scope="module")
def world(oracle):
    import torch
    import granne_amd
    from granne_amd import _lib
    from concurrent.futures import ThreadPoolExecutor
    assert len(set(STRIDES_TOP)) == 16 and all(0 < s < TOP for s in STRIDES_TOP)
    assert len(set(STRIDES_BOTTOM)) == 16 and all(0 < s < N for s in STRIDES_BOTTOM)
    el = torch.empty((N, DIM), dtype=torch.int8, device="cuda")
    for r0 in range(0, N, 4_000_000):  # (an f32 chunk of 1.6 GB at a time)
        rows = min(4_000_000, N - r0)
        el[r0:r0 + rows] = high_ids.synth(_lib, SEED, r0, rows, DIM, "i8")
    dq = high_ids.synth(_lib, SEED + 1, 0, 2048, DIM, "i8")
    for i, j in PLANTS:
        el[i] = dq[j]
    q = dq.cpu().numpy()

    def layer(L, strides):
        out = torch.empty((L, 16), dtype=torch.int32, device="cuda")
        s = torch.tensor(strides, dtype=torch.int64, device="cuda")
        for r0 in range(0, L, 4_000_000):
            i = torch.arange(r0, min(L, r0 + 4_000_000), dtype=torch.int64, device="cuda")
            out[r0:r0 + len(i)] = ((i[:, None] + s[None, :]) % L).to(torch.int32)
        return out
    d_layers = [layer(TOP, STRIDES_TOP), layer(N, STRIDES_BOTTOM)]
    torch.cuda.synchronize()
    ix = granne_amd.Granne.from_device("angular_int", el.data_ptr(), N, DIM, [TOP, N], [l.data_ptr() for l in d_layers], [16, 16])
    h_el = np.empty((N, DIM), np.int8)
    h_bottom = np.empty((N, 16), np.uint32)
    parts = 16
    bounds = [N * i // parts for i in range(parts + 1)]

    def cp(i):
        h_el[bounds[i]:bounds[i + 1]] = el[bounds[i]:bounds[i + 1]].cpu().numpy()
        h_bottom[bounds[i]:bounds[i + 1]] = d_layers[1][bounds[i]:bounds[i + 1]].cpu().numpy().view(np.uint32)
    with ThreadPoolExecutor(8) as ex:
        list(ex.map(cp, range(parts)))
    layers = [d_layers[0].cpu().numpy().view(np.uint32), h_bottom]
    del d_layers
    torch.cuda.empty_cache()
    w = {"el": el, "q": q, "ix": ix, "h_el": h_el, "oix": oracle.Index(h_el, layers),
         "R": high_ids.Range(N, high_ids.device_row_stride("i8", DIM), "int8 rows")}
    yield w
    ix.close()
    w.clear()
    del el, h_el, h_bottom, layers
    torch.cuda.empty_cache()


def _parity(w, q, ms, k, slow=None):
    """ids, distance bytes, counts, counters and the status the host entry reports (no overflow error; walks handed to
    the exact walker) against the oracle: without a visited set and with the exact tables"""
    from granne_amd import _lib
    ix = w["ix"]
    oi, od, oc, octr = w["oix"].search_batch(q, ms, k, n_threads=0)
    for mode in (0, 3):
        ix.set_option(_lib.OPT_VISITED16, mode)
        try:
            ids, ds, cnt, st = ix.search_batch(q, ms, k, stats=True)
        finally:
            ix.set_option(_lib.OPT_VISITED16, 0)
        assert (cnt == oc).all()
        assert (ids == oi).all(), (ms, k, mode, int((ids != oi).any(axis=1).sum()))
        assert ds.tobytes() == od.tobytes()
        if slow is None:
            assert ix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER and ix.last_slow_count() == 0
            assert ix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 0  # int8 launches stay one kernel, however many walks
            assert_counters(st, octr, exact=(mode == 3))
        else:
            assert ix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_EXACT and ix.last_slow_count() == slow
            assert_counters(st, octr, exact=True)
    return oi


def test_the_index_is_what_the_module_says(world):
    """128-byte rows, 128 bytes apart (hbm_bytes: rows + two layers of 32 ids + the scan's norms), and the rows past the
    mark are not their aliases'"""
    ix, R = world["ix"], world["R"]
    n_pad = (N + 31) & ~31
    assert ix.hbm_bytes() == N * 128 + (TOP + N) * 32 * 4 + (n_pad + n_pad // 16 + 1 + 16) * 4
    assert R.past and R.top0 == MARK_ID and len(ix) == N
    high_ids.aliases_differ(world["el"], np.arange(MARK_ID, N, 25_001), R)
    high_ids.check_get_element(ix, world["el"], R, np.random.default_rng(30))
    for i in (0, 5, TOP - 1):
        assert ix.get_neighbors(i, 0) == [(i + s) % TOP for s in STRIDES_TOP]
    for i in (0, MARK_ID - 1, MARK_ID, N - 1):  # the bottom layer's rows past ITS 4 GiB mark (node 2^25: 128 bytes a node)
        assert ix.get_neighbors(i) == [(i + s) % N for s in STRIDES_BOTTOM]


def test_walk_reads_rows_past_the_mark(world, oracle):
    """The int8 register walker on rows (and adjacency rows) past 4 GiB: 256 queries at (max_search, k) = (1, 1),
    (50, 10), (200, 10), (300, 40), (1024, 10), default options and OPT_VISITED16 = 3, and one call of 2,048 queries at
    (50, 10) (one kernel for int8: OPT_LAST_SPLIT_TAIL == 0), bit for bit against the CPU oracle on the same index. On the
    oracle's output alone: at each max_search >= 50 at least 10 % of the returned ids are >= 2^25, and every query's
    list of max_search nodes holds one (its walk expanded and ranked rows past the mark). Under a 32-bit row offset id
    and id - 2^25 alias; their rows differ (test_the_index_is_what_the_module_says), so the ranking would."""
    from granne_amd import _lib
    q = world["q"]
    for ms, k in CONFIGS:
        oi = _parity(world, q[:256], ms, k)
        if ms >= 50:
            share = float((oi >= MARK_ID).mean())
            full = world["oix"].search_batch(q[:256], ms, ms, n_threads=0)[0]
            per_query = (full >= MARK_ID).sum(axis=1)
            print("max_search %d: %.1f %% of the returned ids past the mark; ids past it in a query's list: min %d"
                  % (ms, 100 * share, per_query.min()))
            assert share >= 0.10 and (per_query >= 1).all()
    _parity(world, q, 50, 10)
    assert world["ix"].get_option(_lib.OPT_LAST_SPLIT_TAIL) == 0


def test_forced_exact_walker_past_the_mark(world):
    """OPT_FORCE_SLOW: slow_kernel.h reads rows and adjacency through its own path; 64 queries at (50, 10)."""
    from granne_amd import _lib
    ix = world["ix"]
    ix.set_option(_lib.OPT_FORCE_SLOW, 1)
    try:
        oi = _parity(world, world["q"][:64], 50, 10, slow=64)
    finally:
        ix.set_option(_lib.OPT_FORCE_SLOW, 0)
    assert (oi >= MARK_ID).any()


def test_operators_past_the_mark(world, oracle):
    """dists_many, the pair form and refine at ids on both sides of 2^25 (high_ids.check_dists / check_refine: n - 1,
    2^25, 2^25 - 1, thousands more past the mark, one id >= n), bit-equal to oracle.dist and tests/refine_model.py.
    Aliases under truncation: id and id - 2^25, rows of different bytes."""
    ix, el, q, R = world["ix"], world["el"], world["q"], world["R"]
    high_ids.check_dists(oracle, ix, el, lambda r: r, q, R, np.random.default_rng(31))
    high_ids.check_refine(oracle, ix, el, lambda r: r, q, R, np.random.default_rng(32))


def test_ring_scan_past_the_mark(world, oracle):
    """The exact scan on the LDS-DMA ring (bf_i8_ring_kernel builds its addresses by hand): rows are 128 bytes, 128 apart
    (hbm_bytes, test_the_index_is_what_the_module_says) and n < 2^29, which is what plan_scan (granne_hip.hip, "which
    scan kernel serves an index's rows") sends to the ring; no option reports the scan kernel. k = 1, 10 and 16, each
    twice, identical. Queries 0-6 are the planted rows (ids n - 1, n - 33, 2^25, 2^25 - 1 and four more past the mark):
    rank 0 is the planted id at the oracle's self-distance -- for query 0, planted at n - 1 AND at 2^25 - 1, the smaller id,
    then n - 1 at the same distance; queries 16-31 are member rows past the mark. A tile base truncated to 32 bits would
    score rows id - 2^25 in place of the rows past the mark: the plants and members there (other bytes than their
    aliases) would be missing from their own lists."""
    ix, el, q, R = world["ix"], world["el"], world["q"], world["R"]
    rng = np.random.default_rng(33)
    mem = np.concatenate([[N - 2, MARK_ID + 1], rng.integers(MARK_ID, N, 14)]).astype(np.int64)
    queries = np.concatenate([q[:16], high_ids.fetch(el, mem)])
    members = {0: N - 1, 1: N - 33, 2: MARK_ID, 3: 34567891, 4: 36000001, 5: 38123457, 6: 39999000}
    for qi, i in members.items():
        assert el[i].cpu().numpy().tobytes() == queries[qi].tobytes()
    members.update({16 + j: int(i) for j, i in enumerate(mem)})
    ref_i, ref_d = high_ids.check_exact_scan(oracle, ix, el, lambda r: r, queries, "i8", members, ks=(1, 10, 16))
    assert ref_i[0, 0] == MARK_ID - 1 and ref_i[0, 1] == N - 1 and ref_d[0, 0] == ref_d[0, 1]
    assert (ref_i[7:16, :16] >= MARK_ID).any() and (ref_i[7:16, :16] < MARK_ID).any()
    print("  past-the-mark assertions ran: 7 planted and 16 member queries past id %d" % MARK_ID)
