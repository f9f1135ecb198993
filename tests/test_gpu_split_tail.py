"""The split form of the sketched compacted f32 launches (walk_fast.h, fast_kernel's CR; slow_kernel.h, tail_kernel): two
kernels on the stream, the walkers alone and the exact walker's tail blocks behind them. Every compacted launch takes it,
so the launch searched here is one of 8,192 walks. It returns the oracle's ids, distance bits, counts, expansions and
adjacency entries, and the bits of the same queries searched in launches of 1,024, which are one kernel each;
GRANNE_HIP_OPT_FORCE_SLOW sends every query of it through the hand-over list and the tail kernel; the control words are
re-armed by the last tail block out, so searches follow each other on a stream with nothing in between; grouped calls
and the timed entry go the same way.

Indexes: 6,000 x 100-d, built by the oracle with num_neighbors 30 and max_search 40 (tests/test_gpu_walk_occupancy.py)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_walk_occupancy import _data  # noqa: E402

SEEDS = {"uniform": 51, "mixture": 52, "grid": 53}
PART = 1024
KNOBS = ("GRANNE_HIP_SEEN_MIN", "GRANNE_HIP_SKETCH", "GRANNE_HIP_COMPACT_ROWS")
SLOW_SLOTS = 16384  # the exact walker's containers: an index of 6,000 nodes fills no more than 6,000 of them


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.fixture(scope="module")
def split_nq():
    """Walks of the launch under test: 8 x 1,024, beyond GRANNE_HIP_OPT_SEEN_MIN, so the launch runs the compacted rows."""
    if any(os.environ.get(k) is not None for k in KNOBS):
        pytest.skip("an experiment knob overrides the launch forms this test is about")
    return 8 * PART


@pytest.fixture(scope="module")
def cases(ga, oracle, split_nq):
    """kind -> (queries, the oracle's index, ours); made once, searched by every test, never changed."""
    made = {}

    def get(kind):
        if kind not in made:
            rng = np.random.default_rng(SEEDS[kind])
            el = oracle.normalize_f32(_data(kind, rng, 6000))
            q = oracle.normalize_f32(_data(kind, rng, split_nq))
            oix = oracle.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
            made[kind] = (q, oix, ga.Granne("angular", el, oix.layers))
        return made[kind]

    yield get
    for _, _, gix in made.values():
        gix.close()


@pytest.fixture(scope="module")
def wanted():
    """(kind, max_search) -> the oracle's answer to the first split_nq queries; computed once."""
    return {}


def _oracle(wanted, kind, oix, q, ef):
    if (kind, ef) not in wanted:
        wanted[(kind, ef)] = oix.search_batch(q, ef, 10)
    return wanted[(kind, ef)]


def _is_oracles(got, want, what):
    ids, ds, cnt, st = got
    oi, od, oc, octr = want
    assert (cnt == oc).all(), what
    assert (ids == oi).all() and ds.tobytes() == od.tobytes(), what
    assert (st[:, 1:] == octr[:, 1:]).all(), (what, "n_expand / n_adj")


@pytest.mark.parametrize("kind", ["uniform", "mixture", "grid"])
def test_split_launch_is_the_oracle_and_the_one_kernel_form(cases, wanted, split_nq, kind):
    """max_search 1, 10, 50, 60 walk one slot of 64 keys, 100 two, 200 four. Sketch on: the launch splits and runs the
    compacted row stage. Sketch off: no compacted rows, so one kernel -- the same bits."""
    from granne_amd import _lib
    q, oix, gix = cases(kind)
    q = q[:split_nq]
    assert PART < gix.get_option(_lib.OPT_SEEN_MIN) <= split_nq
    for ef in (1, 10, 50, 60, 100, 200):
        want = _oracle(wanted, kind, oix, q, ef)
        for sketch in (1, 0):
            gix.set_option(_lib.OPT_SKETCH, sketch)
            one = gix.search_batch(q, ef, 10, stats=True)
            assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == sketch, (kind, ef, sketch)
            assert gix.get_option(_lib.OPT_LAST_COMPACT_ROWS) == sketch, (kind, ef, sketch)
            assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER
            _is_oracles(one, want, (kind, ef, sketch))
            if sketch:
                parts = []
                for i in range(0, split_nq, PART):
                    parts.append(gix.search_batch(q[i:i + PART], ef, 10))
                    assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 0
                for j, name in enumerate(("ids", "dists", "counts")):
                    assert one[j].tobytes() == np.concatenate([p[j] for p in parts]).tobytes(), (kind, ef, name)
    gix.set_option(_lib.OPT_SKETCH, 1)


@pytest.mark.parametrize("ef", [50, 200])
def test_force_slow_goes_through_the_tail_kernel(cases, wanted, split_nq, ef):
    """GRANNE_HIP_OPT_FORCE_SLOW on the launch that splits: every walker hands its query over, the tail kernel walks the
    whole list -- no query can be answered unless the list reached it."""
    from granne_amd import _lib
    q, oix, gix = cases("grid")
    q = q[:split_nq]
    gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
    gix.set_option(_lib.OPT_FORCE_SLOW, 1)
    try:
        got = gix.search_batch(q, ef, 10, stats=True)
        assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 1
        assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_EXACT
        assert gix.last_slow_count() == split_nq
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
    want = _oracle(wanted, "grid", oix, q, ef)
    _is_oracles(got, want, ("forced", ef))
    assert (got[3][:, 0] == want[3][:, 0]).all()  # (the exact walker keeps the reference's visited set: n_dist too)


def test_control_words_are_rearmed_between_searches(cases, split_nq):
    """Forced, plain, forced, plain on one stream with nothing between them: a forced search counts every query, the plain
    ones after it count the same hand-overs (tied distances: the grid data) as a plain search made alone, and no
    search reports exhausted containers."""
    import torch
    from granne_amd import _lib
    q, oix, gix = cases("grid")
    q = q[:split_nq]
    ef, k = 50, 10
    gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
    alone = gix.search_batch(q, ef, k)
    assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 1
    alone_slow = gix.last_slow_count()
    assert alone_slow < split_nq
    tq = torch.from_numpy(q).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    order = (1, 0, 1, 0)  # (the first forced search grows the stream's scratch block to the exact walker's many blocks)
    out = []
    for forced in order:
        ids = torch.full((split_nq, k), -7, dtype=torch.int64, device="cuda")
        ds = torch.zeros((split_nq, k), dtype=torch.float32, device="cuda")
        cnt = torch.full((split_nq,), 99, dtype=torch.int32, device="cuda")
        status = torch.zeros(4, dtype=torch.int32, device="cuda")
        out.append((ids, ds, cnt, status))
    for forced, (ids, ds, cnt, status) in zip(order, out):
        gix.set_option(_lib.OPT_FORCE_SLOW, forced)  # (read when the launch is planned, on the host)
        gix.search_batch_device(tq.data_ptr(), split_nq, ef, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), 0,
                                status.data_ptr(), stream)
        assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 1
    gix.set_option(_lib.OPT_FORCE_SLOW, 0)
    torch.cuda.synchronize()
    for forced, (ids, ds, cnt, status) in zip(order, out):
        st = status.cpu().numpy()
        assert st[0] == 0, forced
        assert st[1] == (split_nq if forced else alone_slow), (forced, st)
        assert ids.cpu().numpy().astype(np.uint64).tobytes() == alone[0].tobytes(), forced
        assert ds.cpu().numpy().tobytes() == alone[1].tobytes(), forced
        assert (cnt.cpu().numpy().astype(np.uint32) == alone[2]).all(), forced
    # and the host-pointer call after them reads what it read before them
    again = gix.search_batch(q, ef, k)
    assert gix.last_slow_count() == alone_slow
    assert again[0].tobytes() == alone[0].tobytes() and again[1].tobytes() == alone[1].tobytes()


@pytest.mark.parametrize("forced", [0, 1])
def test_grouped_calls_split_too(cases, forced):
    """granne_hip_search_batches_device, 8 batches of 1,024 in one launch of 8,192 walks: every batch's rows land in its
    own arrays, from the walkers' kernel and from the tail kernel alike."""
    import torch
    from granne_amd import _lib
    q, oix, gix = cases("grid")
    nb, nq, ef, k = 8, PART, 50, 10
    q = q[:nb * nq]
    gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
    want = gix.search_batch(q, ef, k)
    dq = [torch.from_numpy(q[b * nq:(b + 1) * nq].copy()).cuda() for b in range(nb)]
    ids = [torch.full((nq, k), -7, dtype=torch.int64, device="cuda") for _ in range(nb)]
    ds = [torch.zeros((nq, k), dtype=torch.float32, device="cuda") for _ in range(nb)]
    cnt = [torch.full((nq,), 99, dtype=torch.int32, device="cuda") for _ in range(nb)]
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ptrs = lambda ts: [t.data_ptr() for t in ts]  # noqa: E731
    gix.set_option(_lib.OPT_FORCE_SLOW, forced)
    try:
        gix.search_batches_device(ptrs(dq), nq, ef, k, ptrs(ids), ptrs(ds), ptrs(cnt), None, status.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 1
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
    torch.cuda.synchronize()
    for b in range(nb):
        sl = slice(b * nq, (b + 1) * nq)
        assert ids[b].cpu().numpy().astype(np.uint64).tobytes() == want[0][sl].tobytes(), (forced, b)
        assert ds[b].cpu().numpy().tobytes() == want[1][sl].tobytes(), (forced, b)
        assert (cnt[b].cpu().numpy().astype(np.uint32) == want[2][sl]).all(), (forced, b)
    assert status[0].item() == 0
    if forced:
        assert status[1].item() == nb * nq


def test_timed_entry_brackets_both_kernels(cases, wanted, split_nq):
    """granne_hip_search_batch_device_timed on the split shape: the oracle's results, a positive time between the events."""
    import torch
    from granne_amd import _lib
    q, oix, gix = cases("uniform")
    q = q[:split_nq]
    tq = torch.from_numpy(q).cuda()
    ids = torch.empty((split_nq, 10), dtype=torch.int64, device="cuda")
    ds = torch.empty((split_nq, 10), dtype=torch.float32, device="cuda")
    cnt = torch.empty(split_nq, dtype=torch.int32, device="cuda")
    lib = _lib.lib()
    e0, e1 = C.c_void_p(), C.c_void_p()
    _lib.check(lib.granne_hip_event_create(C.byref(e0)))
    _lib.check(lib.granne_hip_event_create(C.byref(e1)))
    gix.search_batch_device_timed(tq.data_ptr(), split_nq, 50, 10, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), 0, 0,
                                  torch.cuda.current_stream().cuda_stream, e0.value, e1.value)
    assert gix.get_option(_lib.OPT_LAST_SPLIT_TAIL) == 1
    torch.cuda.synchronize()
    ms = C.c_float(-1.0)
    _lib.check(lib.granne_hip_event_elapsed_ms(e0, e1, C.byref(ms)))
    assert 0.0 < ms.value < 1000.0
    lib.granne_hip_event_destroy(e0)
    lib.granne_hip_event_destroy(e1)
    want = _oracle(wanted, "uniform", oix, q, 50)
    assert (ids.cpu().numpy().astype(np.uint64) == want[0]).all() and ds.cpu().numpy().tobytes() == want[1].tobytes()
    assert (cnt.cpu().numpy().astype(np.uint32) == want[2]).all()
