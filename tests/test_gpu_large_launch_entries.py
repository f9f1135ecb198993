"""The launch forms of 2,048 walks and more (granne_hip.hip, plan_walk) through every entry that launches a walk. The
sketched 100-d launches are two kernels -- fast_kernel's CR, the walkers alone, and tail_kernel behind it on the stream --
and the other f32 dims skip revisits from an id cache in one kernel. tests/test_gpu_split_tail.py and its neighbours hold
these forms to the oracle through the host call, search_batch_device, search_batches_device and the timed entry; here the
same forms run through begin / end with batches in flight, caller streams beyond the scratch cache, host threads on one
handle, launches of alternating forms on one stream, the fused refined search, the packed and sharded entries, exhausted
containers, grouped batches that reach the threshold only together, and indexes from every maker. What these have in
common is the interplay of the two kernels, the per-(index, stream) scratch block and its control words.

Every comparison is bit for bit -- ids, distance bytes, counts, n_expand / n_adj where statistics are asked for -- and
every test asserts, after the call, the form it is about.

Indexes, made once per module and never changed: A, 6,000 x 100-d f32 ("clones": tied distances, walks are handed over
and the tail kernel has work; "uniform"), built by the oracle with num_neighbors 30 and max_search 40 (the shape of
tests/test_gpu_split_tail.py); B, 3,000 x 200-d and 3,000 x 96-d f32 on the clustered data of
test_revisits_skipped_before_their_rows_are_fetched (no sketch, no split: the unrolled and the streamed walker). The
oracle's answers are computed once per (index, max_search, k) over the index's whole pool of queries.

Why "clones" and not the "grid" or "duplicates" rows of the neighbouring modules: a register walker hands its walk over
when the key pushed off its list's end ties with the key at place max_search - 1 (walk_fast.h, merge_ranked), i.e. when
places max_search - 1 .. 64 S hold one distance -- 16 equal distances at max_search 50. Among 6,000 grid rows the longest
such run is 7, among rows drawn four times each 12 (a scan of either, any seed): no walk of theirs is ever handed over.
Sixty rows held 40 times each among 3,600 others give runs of 40, and about a quarter of the queries one across the
list's end."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_model as model  # noqa: E402
from tests.conftest import random_floats  # noqa: E402
from tests.test_gpu_sharded import _want as sharded_want  # noqa: E402  (per-shard oracle searches, oracle.merge.merge_topk_numpy)
from tests.test_gpu_walk_occupancy import _data  # noqa: E402
from tests.test_sketch_bound import row_sketch  # noqa: E402

NQ = 2048   # GRANNE_HIP_OPT_SEEN_MIN's default: the smallest launch that takes the forms
ODD = 2500  # no multiple of 64
K = 10
SLOW_SLOTS = 16384  # the exact walker's containers: an index of 6,000 nodes fills no more than 6,000 of them
KNOBS = ("GRANNE_HIP_SEEN_MIN", "GRANNE_HIP_SKETCH", "GRANNE_HIP_COMPACT_ROWS")
SEEDS = {"clones": 63, "uniform": 62}
POOL = {"clones": 4 * NQ, "uniform": ODD}
JOIN_SECONDS = 60.0


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _clones(rng, n, dim=100, groups=60, copies=40):
    """groups x copies rows that are exact copies of each other, the rest uniform, in random order."""
    base = random_floats(rng, groups, dim)
    rows = np.concatenate([np.repeat(base, copies, axis=0), random_floats(rng, n - groups * copies, dim)])
    return rows[rng.permutation(n)]


class Case:
    def __init__(self, name, el, q, oix, gix):
        self.name, self.el, self.q, self.oix, self.gix = name, el, q, oix, gix


class World:
    """The module's indexes, queries and oracle answers; everything is made on first use and kept."""

    def __init__(self, ga, orc):
        self.ga, self.orc = ga, orc
        self.cases, self._want, self._alone, self._tied, self.refiners, self.models = {}, {}, {}, None, {}, {}

    def a(self, kind):
        if kind not in self.cases:
            from granne_amd import _lib
            rng = np.random.default_rng(SEEDS[kind])
            el = self.orc.normalize_f32(_clones(rng, 6000) if kind == "clones" else _data(kind, rng, 6000))
            q = self.orc.normalize_f32(_data("uniform", rng, POOL[kind]))
            oix = self.orc.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
            gix = self.ga.Granne("angular", el, oix.layers)
            gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
            assert gix.get_option(_lib.OPT_SEEN_MIN) == NQ and gix.get_option(_lib.OPT_SKETCH) == 1
            self.cases[kind] = Case(kind, el, q, oix, gix)
        return self.cases[kind]

    def b(self, dim):
        name = "b%d" % dim
        if name not in self.cases:
            from granne_amd import _lib
            rng = np.random.default_rng(900 + dim)
            centers = random_floats(rng, 40, dim)

            def rows(n):
                return self.orc.normalize_f32((centers[rng.integers(0, 40, n)] + 0.05 * random_floats(rng, n, dim)).astype(np.float32))

            el, q = rows(3000), rows(3 * NQ if dim == 200 else NQ)
            oix = self.orc.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
            gix = self.ga.Granne("angular", el, oix.layers)
            gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
            assert gix.get_option(_lib.OPT_SEEN_MIN) == NQ and gix.get_sketch() is None
            self.cases[name] = Case(name, el, q, oix, gix)
        return self.cases[name]

    def want(self, case, ef, k=K):
        """The oracle's (ids, dists, counts, counters) for the case's whole pool of queries."""
        key = (case.name, ef, k)
        if key not in self._want:
            self._want[key] = case.oix.search_batch(case.q, ef, k)
        return self._want[key]

    def alone(self, case, lo, hi, ef):
        """Hand-overs of queries [lo, hi) searched by a plain host call, one launch of hi - lo walks."""
        key = (case.name, lo, hi, ef)
        if key not in self._alone:
            got = case.gix.search_batch(case.q[lo:hi], ef, K, stats=True)
            self._alone[key] = case.gix.last_slow_count()
            if case.name in SEEDS:
                (_is_split if hi - lo >= NQ else _is_one_kernel)(case.gix, key)
            _is_oracles(got, self.want(case, ef), slice(lo, hi), ("alone",) + key)
        return self._alone[key]

    def tied(self):
        """A on the data that hands walks over: some walks of a launch of NQ at max_search 50, not all."""
        if self._tied is None:
            case = self.a("clones")
            n = self.alone(case, 0, NQ, 50)
            assert 0 < n < NQ, "a launch of %d walks hands %d of them over" % (NQ, n)
            self._tied = case
        return self._tied

    def refiner(self, case, rkind):
        """The case's elements as a rows-only handle R (int8 rows / angular_f16 rows), the rows the model re-ranks by,
        and what prepares a batch of f32 queries for R."""
        key = (case.name, rkind)
        if key not in self.refiners:
            if rkind == "int8":
                rows = self.orc.quantize(case.el)
                self.refiners[key] = (self.ga.Granne("angular_int", rows, []), rows, self.orc.quantize)
            else:
                rows16 = case.el.astype(np.float16)
                rows = self.orc.normalize_f32(rows16.astype(np.float32))
                self.refiners[key] = (self.ga.Granne("angular_f16", rows16, []), rows, lambda q: q)
        return self.refiners[key]

    def close(self):
        for r, _, _ in self.refiners.values():
            r.close()
        for c in self.cases.values():
            c.gix.close()


@pytest.fixture(scope="module")
def world(ga, oracle):
    if any(os.environ.get(k) is not None for k in KNOBS):
        pytest.skip("an experiment knob overrides the launch forms this module is about")
    w = World(ga, oracle)
    yield w
    w.close()


# ---- what ran, and what came back ----------------------------------------------------------------------------------
def _form(gix):
    from granne_amd import _lib
    return (gix.get_option(_lib.OPT_LAST_SPLIT_TAIL), gix.get_option(_lib.OPT_LAST_COMPACT_ROWS), gix.get_option(_lib.OPT_LAST_WALKER))


def _is_split(gix, what=None, forced=False):
    """A's form: two kernels, the compacted row stage; forced: every walker hands its query to the tail kernel."""
    from granne_amd import _lib
    assert _form(gix) == (1, 1, _lib.WALKER_EXACT if forced else _lib.WALKER_REGISTER), (what, _form(gix))


def _is_one_kernel(gix, what=None, forced=False):
    from granne_amd import _lib
    assert _form(gix) == (0, 0, _lib.WALKER_EXACT if forced else _lib.WALKER_REGISTER), (what, _form(gix))


def _b_form(gix, run):
    """B's form: one kernel, no compacted rows, and run() -- the launches under test, which returns the rows they
    evaluated -- evaluates fewer than the same launches with the id cache out of reach."""
    from granne_amd import _lib
    with_cache = run()
    _is_one_kernel(gix)
    gix.set_option(_lib.OPT_SEEN_MIN, 0xFFFFFFFF)
    try:
        without = run()
        _is_one_kernel(gix)
    finally:
        gix.set_option(_lib.OPT_SEEN_MIN, NQ)
    assert with_cache < without, (with_cache, without)


def _is_oracles(got, want, sl, what):
    """Host results (ids, dists, counts[, stats]) against rows `sl` of the oracle's."""
    oi, od, oc, octr = want
    assert (got[2] == oc[sl]).all(), what
    assert got[0].tobytes() == oi[sl].tobytes() and got[1].tobytes() == od[sl].tobytes(), what
    if len(got) > 3:
        assert (got[3][:, 1:] == octr[sl][:, 1:]).all(), (what, "n_expand / n_adj")


class Out:
    """Device buffers of one search, filled with what no search writes."""

    def __init__(self, nq, k=K, stats=True):
        import torch
        self.ids = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
        self.ds = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        self.cnt = torch.full((nq,), 99, dtype=torch.int32, device="cuda")
        self.st = torch.zeros((nq, 3), dtype=torch.int64, device="cuda") if stats else None
        self.status = torch.zeros(4, dtype=torch.int32, device="cuda")

    def args(self):
        """d_ids, d_dists, d_counts, d_stats, d_status"""
        return (self.ids.data_ptr(), self.ds.data_ptr(), self.cnt.data_ptr(), self.st.data_ptr() if self.st is not None else 0,
                self.status.data_ptr())

    def host(self):
        got = (self.ids.cpu().numpy().view(np.uint64), self.ds.cpu().numpy(), self.cnt.cpu().numpy().view(np.uint32))
        return got + (self.st.cpu().numpy().view(np.uint64),) if self.st is not None else got

    def words(self):
        return self.status.cpu().numpy().view(np.uint32).tolist()

    def rows_evaluated(self):
        return int(self.st[:, 0].sum().item())


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def run_threads(fns):
    """Every callable on a thread of its own; a thread that raised, or is still alive after JOIN_SECONDS, fails the test."""
    err = [None] * len(fns)

    def body(i):
        try:
            fns[i]()
        except BaseException as e:  # noqa: BLE001 (reported below, on the test's thread)
            err[i] = e

    th = [threading.Thread(target=body, args=(i,), daemon=True) for i in range(len(fns))]
    deadline = time.monotonic() + JOIN_SECONDS
    [t.start() for t in th]
    for t in th:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in th), "a search call did not return: %s" % [t.is_alive() for t in th]
    for e in err:
        if e is not None:
            raise e


# ---- the fixtures' own premise ---------------------------------------------------------------------------------------
def test_the_tied_index_hands_walks_over(world):
    """A plain host call of NQ queries at max_search 50 hands some walks over, not all: the tail kernel of every test on
    this index has a list to walk."""
    case = world.tied()
    assert 0 < world.alone(case, 0, NQ, 50) < NQ


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tied", "uniform"])
def test_the_threshold(world, kind):
    """2,047, 2,048 and 2,049 of the same queries: one kernel, split, split -- and the oracle's rows from all three."""
    case = world.tied() if kind == "tied" else world.a("uniform")
    want = world.want(case, 50)
    for n in (NQ - 1, NQ, NQ + 1):
        got = case.gix.search_batch(case.q[:n], 50, K, stats=True)
        (_is_split if n >= NQ else _is_one_kernel)(case.gix, n)
        _is_oracles(got, want, slice(0, n), (kind, n))


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("efs", [(50, 50, 50), (50, 200, 100)])
@pytest.mark.parametrize("which", ["A", "B"])
def test_begin_end_with_large_launches_in_flight(world, which, efs):
    """Three batches of NQ distinct queries begun on the index's own streams before any is ended, ended in reverse order,
    each with its own status words: the oracle's results, no exhaustion, and the hand-overs of the batch searched alone.
    max_search 50 / 200 / 100: kernels of one, four and two list slots share the chip."""
    import torch
    from granne_amd import _lib
    case = world.tied() if which == "A" else world.b(200)
    gix = case.gix
    assert gix.get_option(_lib.OPT_SEARCH_DEPTH) == 3
    want = [world.want(case, ef) for ef in efs]
    alone = [world.alone(case, b * NQ, (b + 1) * NQ, efs[b]) for b in range(3)]
    dq = torch.from_numpy(case.q[:3 * NQ]).cuda()
    s = _stream()

    def run():
        outs = [Out(NQ) for _ in range(3)]
        tickets = []
        for b in range(3):
            tickets.append(gix.search_begin_device(dq[b * NQ:(b + 1) * NQ].data_ptr(), NQ, efs[b], K, *outs[b].args(), s))
            (_is_split if which == "A" else _is_one_kernel)(gix, (efs, b))
        for t in reversed(tickets):
            gix.search_end_device(t, s)
        torch.cuda.synchronize()
        for b in range(3):
            _is_oracles(outs[b].host(), want[b], slice(b * NQ, (b + 1) * NQ), (which, efs, b))
            assert outs[b].words()[:2] == [0, alone[b]], (which, efs, b, outs[b].words())
        return sum(o.rows_evaluated() for o in outs)

    if which == "A":
        run()
    else:
        _b_form(gix, run)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
def test_caller_streams_beyond_the_scratch_cache(world):
    """66 caller streams, more than the 64 that keep a scratch block: one split launch of NQ on each, twice round, one
    synchronisation at the end. The streams past the cache search with a block of the stream-ordered allocator."""
    import torch
    from granne_amd import _lib
    case = world.tied()
    gix = case.gix
    assert gix.get_option(_lib.OPT_SLOW_SLOTS) == SLOW_SLOTS
    want = world.want(case, 50)
    dq = [torch.from_numpy(case.q[b * NQ:(b + 1) * NQ].copy()).cuda() for b in range(4)]
    streams = [torch.cuda.Stream() for _ in range(66)]
    runs = [((i + rep) % 4, s_, Out(NQ, stats=False)) for rep in range(2) for i, s_ in enumerate(streams)]
    torch.cuda.synchronize()
    for b, s_, o in runs:
        gix.search_batch_device(dq[b].data_ptr(), NQ, 50, K, *o.args(), s_.cuda_stream)
        _is_split(gix)
    torch.cuda.synchronize()
    for i, (b, s_, o) in enumerate(runs):
        _is_oracles(o.host(), want, slice(b * NQ, (b + 1) * NQ), (i, b))
        assert o.words()[:2] == [0, world.alone(case, b * NQ, (b + 1) * NQ, 50)], (i, b, o.words())


# ---- 4 ---------------------------------------------------------------------------------------------------------------
def test_host_threads_on_one_handle(world):
    """Four threads, each with its own NQ queries, three host calls each: split launches on the streams of four call
    contexts of one index at the same time."""
    case = world.tied()
    want = world.want(case, 50)
    got = [[None] * 3 for _ in range(4)]

    def work(i):
        def body():
            for r in range(3):
                got[i][r] = case.gix.search_batch(case.q[i * NQ:(i + 1) * NQ], 50, K, stats=True)
                _is_split(case.gix, (i, r))
        return body

    run_threads([work(i) for i in range(4)])
    for i in range(4):
        for r in range(3):
            _is_oracles(got[i][r], want, slice(i * NQ, (i + 1) * NQ), (i, r))


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [(), (1, 3)])
def test_forms_alternate_on_one_stream(world, forced):
    """Launches of 2,048, 1,024, 2,500, 64 and 2,048 on one stream with nothing in between and no host synchronisation
    until the end: split, one kernel with tail blocks that spin, split with a longer hand-over list, the touch form,
    split. Every launch is the oracle's and counts the hand-overs of a launch of its size made alone. forced: the second
    and fourth run GRANNE_HIP_OPT_FORCE_SLOW -- the exact walker's kernel alone on many blocks, for whose containers the
    stream's scratch block grows between two split launches."""
    import torch
    from granne_amd import _lib
    case = world.tied()
    gix = case.gix
    sizes = (NQ, 1024, ODD, 64, NQ)
    los = [sum(sizes[:i]) for i in range(len(sizes))]
    assert los[-1] + sizes[-1] <= len(case.q)
    want = world.want(case, 50)
    alone = [n if i in forced else world.alone(case, lo, lo + n, 50) for i, (lo, n) in enumerate(zip(los, sizes))]
    dq = torch.from_numpy(case.q).cuda()
    outs = [Out(n) for n in sizes]
    stream = torch.cuda.Stream()  # (a stream the index has no scratch block for yet)
    torch.cuda.synchronize()
    try:
        for i, (lo, n) in enumerate(zip(los, sizes)):
            gix.set_option(_lib.OPT_FORCE_SLOW, 1 if i in forced else 0)  # (read when the launch is planned, on the host)
            gix.search_batch_device(dq[lo:lo + n].data_ptr(), n, 50, K, *outs[i].args(), stream.cuda_stream)
            (_is_split if n >= NQ else _is_one_kernel)(gix, (forced, i), forced=i in forced)
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
    torch.cuda.synchronize()
    for i, (lo, n) in enumerate(zip(los, sizes)):
        _is_oracles(outs[i].host(), want, slice(lo, lo + n), (forced, i))
        assert outs[i].words()[:2] == [0, alone[i]], (forced, i, outs[i].words())


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def _model_of(world, case, rkind, rows, prep):
    """refine_model.search_refined over the first 512 queries of the case's pool; computed once."""
    key = (case.name, rkind)
    if key not in world.models:
        q = case.q[:512]
        world.models[key] = model.search_refined(world.orc, case.oix, rows, q, prep(q), 50, 50, K)
    return world.models[key]


def _composition(case, R, prep, q):
    """The two steps apart: the walk with k = 50, then R's refine of its lists."""
    wi, _, wc = case.gix.search_batch(q, 50, 50)
    return R.refine(prep(q), wi, wc, k=K)


def _same_bytes(a, b, what):
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize("rkind", ["int8", "f16"])
def test_fused_refined_search_behind_a_split_walk(world, ga, rkind):
    """RefinedGranne(A, R): the walk's lists are written by fast_kernel and by tail_kernel, and refine_kernel follows both
    on the stream. The model's result on 512 queries, the composition's on all; then with GRANNE_HIP_OPT_FORCE_SLOW
    every list is the tail kernel's and the bytes are the same."""
    import torch
    from granne_amd import _lib
    case = world.tied()
    gix = case.gix
    R, rows, prep = world.refiner(case, rkind)
    rg = ga.RefinedGranne(gix, R)
    q0, q1 = case.q[:NQ], case.q[NQ:2 * NQ]
    fused = rg.search_batch((q0, prep(q0)), 50, K, refine_from=50, stats=True, dropped=True)
    _is_split(gix)
    want = _model_of(world, case, rkind, rows, prep)
    _same_bytes([x[:512] for x in fused[:3]], want, (rkind, "model"))
    assert fused[4] == 0 == want[3]
    assert (fused[3][:, 1:] == world.want(case, 50, 50)[3][:NQ, 1:]).all()
    _same_bytes(fused, _composition(case, R, prep, q0), (rkind, "composition"))
    # other queries through the same entry: whatever the stream-ordered scratch of the lists held, it is not q0's now
    other = rg.search_batch((q1, prep(q1)), 50, K, refine_from=50)
    _same_bytes(other, _composition(case, R, prep, q1), (rkind, "composition, other queries"))
    # the device entry, other queries first; then forced: all NQ lists come from the tail kernel
    dw = [torch.from_numpy(q).cuda() for q in (q1, q0)]
    dr = [torch.from_numpy(np.ascontiguousarray(prep(q))).cuda() for q in (q1, q0)]
    outs = [Out(NQ), Out(NQ)]
    rstatus = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = _stream()
    try:
        for i in (0, 1):
            gix.set_option(_lib.OPT_FORCE_SLOW, i)
            o = outs[i]
            rg.search_batch_device(dw[i].data_ptr(), dr[i].data_ptr(), NQ, 50, 50, K, o.ids.data_ptr(), o.ds.data_ptr(), o.cnt.data_ptr(),
                                   o.st.data_ptr(), o.status.data_ptr(), rstatus[i:].data_ptr(), s)
            _is_split(gix, (rkind, i), forced=bool(i))
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
    torch.cuda.synchronize()
    _same_bytes(outs[0].host(), other, (rkind, "device entry"))
    _same_bytes(outs[1].host(), fused, (rkind, "forced"))
    assert (outs[1].host()[3][:, 1:] == fused[3][:, 1:]).all()
    assert outs[0].words()[:2] == [0, world.alone(case, NQ, 2 * NQ, 50)] and outs[1].words()[:2] == [0, NQ]
    assert rstatus.tolist() == [0, 0]
    # and the handle answers as before
    again = rg.search_batch((q0, prep(q0)), 50, K, refine_from=50)
    _is_split(gix)
    _same_bytes(again, fused, (rkind, "after the forced search"))


def test_fused_refined_search_behind_a_one_kernel_walk(world, ga):
    """The same on B: a 200-d walk that skips revisits, one kernel, re-ranked by int8 rows."""
    case = world.b(200)
    R, rows, prep = world.refiner(case, "int8")
    rg = ga.RefinedGranne(case.gix, R)
    q0 = case.q[:NQ]
    res = []

    def run():
        res.append(rg.search_batch((q0, prep(q0)), 50, K, refine_from=50, stats=True, dropped=True))
        return int(res[-1][3][:, 0].sum())

    _b_form(case.gix, run)
    fused = res[0]
    want = _model_of(world, case, "int8", rows, prep)
    _same_bytes([x[:512] for x in fused[:3]], want, "model")
    assert fused[4] == 0 == want[3]
    assert (fused[3][:, 1:] == world.want(case, 50, 50)[3][:NQ, 1:]).all()
    _same_bytes(fused, _composition(case, R, prep, q0), "composition")
    _same_bytes(res[1], fused, "without the id cache")


# ---- 7 ---------------------------------------------------------------------------------------------------------------
class Shards:
    def __init__(self, world, ga, orc):
        from granne_amd import _lib, sharded
        self.case = world.tied()
        self.bounds = sharded.shard_bounds(len(self.case.el), 3)
        self.offsets = [b[0] for b in self.bounds]
        self.oixs, self.gixs, self._want = [], [], {}
        for lo, hi in self.bounds:
            part = np.ascontiguousarray(self.case.el[lo:hi])
            oix = orc.build_index(part, num_neighbors=30, max_search=40, n_threads=8)
            gix = ga.Granne("angular", part, oix.layers)
            gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
            self.oixs.append(oix)
            self.gixs.append(gix)

    def q(self, b):
        return self.case.q[b * NQ:(b + 1) * NQ]

    def want(self, b):
        """Per-shard oracle searches of batch b at max_search 50, merged by merge_topk_numpy."""
        if b not in self._want:
            self._want[b] = sharded_want(self.oixs, self.q(b), 50, K, self.offsets)
        return self._want[b]

    def all_split(self, what=None, forced=()):
        for s_, g in enumerate(self.gixs):
            _is_split(g, (what, s_), forced=s_ in forced)

    def handed_over(self, b):
        """Per shard: the hand-overs of batch b searched by a plain call on that shard alone."""
        out = []
        for g in self.gixs:
            g.search_batch(self.q(b), 50, K)
            out.append(g.last_slow_count())
        return out


@pytest.fixture(scope="module")
def shards(world, ga, oracle):
    sh = Shards(world, ga, oracle)
    yield sh
    for g in sh.gixs:
        g.close()


def _merged_is(got, want, what):
    ids, ds, cnt = got
    assert (cnt == want[2]).all(), what
    assert ids.tobytes() == want[0].tobytes() and ds.tobytes() == want[1].tobytes(), what


def test_packed_results_and_one_process_per_gpu(world, shards):
    """granne_hip_search_batch_packed_device on one shard holds the bytes of search_batch_device at its three offsets (and
    its status words behind them); sharded.ShardedGranne over the three shards returns the merged oracle searches."""
    import torch
    from granne_amd import _lib, sharded
    g, oix = shards.gixs[0], shards.oixs[0]
    pb = sharded.packed_bytes(NQ, K)
    dq = torch.from_numpy(shards.q(0)).cuda()
    packed = torch.zeros(pb + sharded.STATUS_BYTES, dtype=torch.uint8, device="cuda")
    s = _stream()
    _lib.check(_lib.lib().granne_hip_search_batch_packed_device(g._h, C.c_void_p(dq.data_ptr()), NQ, 50, K, C.c_void_p(packed.data_ptr()),
                                                                C.c_void_p(packed.data_ptr() + pb), C.c_void_p(s)))
    _is_split(g)
    o = Out(NQ, stats=False)
    g.search_batch_device(dq.data_ptr(), NQ, 50, K, *o.args(), s)
    torch.cuda.synchronize()
    raw = packed.cpu().numpy()
    ids, ds, cnt = o.host()
    assert raw[:NQ * K * 8].tobytes() == ids.tobytes()
    assert raw[NQ * K * 8:NQ * K * 12].tobytes() == ds.tobytes()
    assert raw[NQ * K * 12:NQ * K * 12 + NQ * 4].tobytes() == cnt.tobytes()
    assert raw[pb:pb + 16].view(np.uint32).tolist() == o.words()
    g.search_batch(shards.q(0), 50, K)
    assert o.words()[:2] == [0, g.last_slow_count()]  # (what the tail kernel counted lies in the packed buffer's words too)
    _is_oracles(o.host(), oix.search_batch(shards.q(0), 50, K), slice(0, NQ), "shard 0")
    sg = sharded.ShardedGranne(shards.gixs, shards.offsets)  # world 1: all shards are local
    m = sg.search_batch(shards.q(0), 50, K)
    torch.cuda.synchronize()
    shards.all_split("ShardedGranne")
    _merged_is((m[0].cpu().numpy().view(np.uint64), m[1].cpu().numpy(), m[2].cpu().numpy().view(np.uint32)), shards.want(0), "ShardedGranne")
    st = sg.status_of_last_batch().cpu().numpy().view(np.uint32)
    assert (st[:, 0] == 0).all() and st[:, 1].tolist() == shards.handed_over(0)


@pytest.mark.parametrize("exchange", ["peer", "rccl"])
def test_sharded_host_entries(world, shards, exchange):
    """The one-host-process handle over three shards of split launches: the device call, begin / end two deep over three
    batches, the pipelined host batches -- with peer copies and with the all-gather as the exchange step."""
    import torch
    from granne_amd import _lib, sharded
    sh = sharded.ShardedHost(shards.gixs, shards.offsets)
    try:
        if exchange == "rccl":
            sh.set_option(_lib.SHARDED_OPT_EXCHANGE, _lib.SHARDED_EXCHANGE_RCCL)
        assert sh.get_option(_lib.SHARDED_OPT_DEPTH) == 2
        nb = 3
        want = [shards.want(b) for b in range(nb)]
        handed = [sum(shards.handed_over(b)) for b in range(nb)]
        dq = torch.from_numpy(shards.case.q[:nb * NQ]).cuda()
        s = _stream()

        def check(outs, what):
            torch.cuda.synchronize()
            shards.all_split(what)
            for b in range(nb):
                _merged_is(outs[b].host(), want[b], (exchange, what, b))
                assert outs[b].words()[:2] == [0, handed[b]], (exchange, what, b, outs[b].words())

        outs = [Out(NQ, stats=False) for _ in range(nb)]
        for b in range(nb):  # one batch at a time, stream-ordered, no host synchronisation in between
            o = outs[b]
            sh.search_batch_device(dq[b * NQ:(b + 1) * NQ].data_ptr(), NQ, 50, K, o.ids.data_ptr(), o.ds.data_ptr(), o.cnt.data_ptr(),
                                   o.status.data_ptr(), s)
        check(outs, "device")
        outs = [Out(NQ, stats=False) for _ in range(nb)]
        tickets = []
        for b in range(nb):  # two in flight: batch b is begun before batch b - 1 is ended
            o = outs[b]
            tickets.append(sh.begin_device(dq[b * NQ:(b + 1) * NQ].data_ptr(), NQ, 50, K, o.ids.data_ptr(), o.ds.data_ptr(), o.cnt.data_ptr(),
                                           o.status.data_ptr(), s))
            if b >= 1:
                sh.end_device(tickets[b - 1], s)
        sh.end_device(tickets[-1], s)
        check(outs, "begin / end")
        h = sh.search_batches(shards.case.q[:2 * NQ].reshape(2, NQ, -1), 50, K)  # host buffers, pipelined inside the library
        shards.all_split("search_batches")
        for b in range(2):
            _merged_is((h[0][b], h[1][b], h[2][b]), want[b], (exchange, "search_batches", b))
    finally:
        sh.close()


def test_sharded_status_words_of_a_split_shard(world, shards):
    """Shard 1 with GRANNE_HIP_OPT_FORCE_SLOW: its tail kernel counts NQ hand-overs into the packed buffer's words, the
    results do not change. (status[1] sums over the shards: NQ, plus what shards 0 and 2 hand over of their own accord.)
    With 256 containers the launch is exhausted: status[0] from the device entry, GRANNE_HIP_ERR_OVERFLOW from the host
    entry. With both options restored the handle answers as before."""
    import torch
    from granne_amd import _lib, sharded
    sh = sharded.ShardedHost(shards.gixs, shards.offsets)
    g1 = shards.gixs[1]
    handed = shards.handed_over(0)
    want = shards.want(0)
    dq = torch.from_numpy(shards.q(0)).cuda()
    s = _stream()

    def device_call():
        o = Out(NQ, stats=False)
        sh.search_batch_device(dq.data_ptr(), NQ, 50, K, o.ids.data_ptr(), o.ds.data_ptr(), o.cnt.data_ptr(), o.status.data_ptr(), s)
        torch.cuda.synchronize()
        return o

    slots = g1.get_option(_lib.OPT_SLOW_SLOTS)
    try:
        g1.set_option(_lib.OPT_FORCE_SLOW, 1)
        o = device_call()
        shards.all_split("forced", forced=(1,))
        assert o.words()[:2] == [0, NQ + handed[0] + handed[2]], (o.words(), handed)
        _merged_is(o.host(), want, "forced")
        g1.set_option(_lib.OPT_SLOW_SLOTS, 256)  # far too few for a walk of max_search 50
        o = device_call()
        shards.all_split("exhausted", forced=(1,))
        assert o.words()[0] == 1, o.words()
        with pytest.raises(_lib.GranneHipError) as e:
            sh.search_batches(shards.q(0)[None], 50, K)
        assert e.value.code == _lib.ERR_OVERFLOW
    finally:
        g1.set_option(_lib.OPT_FORCE_SLOW, 0)
        g1.set_option(_lib.OPT_SLOW_SLOTS, slots)
    o = device_call()
    shards.all_split("restored")
    assert o.words()[:2] == [0, sum(handed)], (o.words(), handed)
    _merged_is(o.host(), want, "restored")
    h = sh.search_batches(shards.q(0)[None], 50, K)
    _merged_is((h[0][0], h[1][0], h[2][0]), want, "restored, host")
    sh.close()


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_exhaustion_in_the_split_form(world, ga):
    """GRANNE_HIP_OPT_FORCE_SLOW with 256 containers at max_search 200: every walk of the split launch outgrows them, and
    the host call reports it. With the options restored the next searches are the oracle's and count the hand-overs of a
    fresh index: the last tail block out re-armed the control words after the exhausted launch too."""
    import torch
    from granne_amd import _lib
    case = world.tied()
    gix = case.gix
    q = case.q[:NQ]
    fresh = ga.Granne("angular", case.el, case.oix.layers)
    fresh.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
    first = {}
    for ef in (200, 50):
        _is_oracles(fresh.search_batch(q, ef, K, stats=True), world.want(case, ef), slice(0, NQ), ("fresh", ef))
        first[ef] = fresh.last_slow_count()
    fresh.close()
    slots = gix.get_option(_lib.OPT_SLOW_SLOTS)
    try:
        gix.set_option(_lib.OPT_FORCE_SLOW, 1)
        gix.set_option(_lib.OPT_SLOW_SLOTS, 256)
        with pytest.raises(ga.GranneHipError) as e:
            gix.search_batch(q, 200, K)
        assert e.value.code == _lib.ERR_OVERFLOW
        _is_split(gix, "exhausted", forced=True)
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
        gix.set_option(_lib.OPT_SLOW_SLOTS, slots)
    for ef in (200, 50):
        got = gix.search_batch(q, ef, K, stats=True)
        _is_split(gix, ("restored", ef))
        _is_oracles(got, world.want(case, ef), slice(0, NQ), ("restored", ef))
        assert gix.last_slow_count() == first[ef], (ef, gix.last_slow_count(), first[ef])
    # the same on a caller's stream, where the status words report it: exhausted, then not
    dq = torch.from_numpy(q).cuda()
    outs = [Out(NQ), Out(NQ)]
    try:
        for i, o in enumerate(outs):
            gix.set_option(_lib.OPT_FORCE_SLOW, 1 - i)
            gix.set_option(_lib.OPT_SLOW_SLOTS, slots if i else 256)
            gix.search_batch_device(dq.data_ptr(), NQ, 200, K, *o.args(), _stream())
            _is_split(gix, i, forced=not i)
    finally:
        gix.set_option(_lib.OPT_FORCE_SLOW, 0)
        gix.set_option(_lib.OPT_SLOW_SLOTS, slots)
    torch.cuda.synchronize()
    assert outs[0].words()[0] == 1 and outs[1].words()[:2] == [0, first[200]], (outs[0].words(), outs[1].words())
    _is_oracles(outs[1].host(), world.want(case, 200), slice(0, NQ), "after the exhausted launch, on its stream")


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def _grouped(gix, q, nb, nq, ef):
    """One granne_hip_search_batches_device call over nb separate allocations of nq queries; returns the outputs."""
    import torch
    dq = [torch.from_numpy(q[b * nq:(b + 1) * nq].copy()).cuda() for b in range(nb)]
    outs = [Out(nq) for _ in range(nb)]
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    gix.search_batches_device([t.data_ptr() for t in dq], nq, ef, K, [o.ids.data_ptr() for o in outs], [o.ds.data_ptr() for o in outs],
                              [o.cnt.data_ptr() for o in outs], [o.st.data_ptr() for o in outs], status.data_ptr(), _stream())
    return outs, status, dq


@pytest.mark.parametrize("dim", [200, 96])
def test_grouped_batches_reach_the_threshold_together_one_kernel(world, dim):
    """2 x 1,024 on B: neither batch alone skips revisits, the launch of both does; every batch's rows land in its own arrays."""
    import torch
    case = world.b(dim)
    want = world.want(case, 50)

    def run():
        outs, status, _dq = _grouped(case.gix, case.q, 2, 1024, 50)
        torch.cuda.synchronize()
        for b, o in enumerate(outs):
            _is_oracles(o.host(), want, slice(b * 1024, (b + 1) * 1024), (dim, b))
        assert status.cpu().numpy().view(np.uint32).tolist()[:2] == [0, world.alone(case, 0, 2048, 50)]
        return sum(o.rows_evaluated() for o in outs)

    _b_form(case.gix, run)


def test_grouped_batches_reach_the_threshold_together_split(world):
    """3 x 700 on A: 2,100 walks in one launch, which splits."""
    import torch
    case = world.tied()
    outs, status, _dq = _grouped(case.gix, case.q, 3, 700, 50)
    _is_split(case.gix)
    torch.cuda.synchronize()
    want = world.want(case, 50)
    for b, o in enumerate(outs):
        _is_oracles(o.host(), want, slice(b * 700, (b + 1) * 700), b)
    assert status.cpu().numpy().view(np.uint32).tolist()[:2] == [0, world.alone(case, 0, 2100, 50)]


# ---- 10 --------------------------------------------------------------------------------------------------------------
def _sorted_layers(layers):
    """Layers as a written index holds them: every row's ids ascending (Layers::Compressed), UNUSED behind them."""
    return [np.sort(l, axis=1) for l in layers]  # (UNUSED is the largest uint32)


def _csr(layers):
    offsets, ids = [], []
    for layer in layers:
        deg = (layer != 0xFFFFFFFF).sum(axis=1)
        offsets.append(np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64))
        ids.append(np.concatenate([np.sort(r[:d]) for r, d in zip(layer, deg)]).astype(np.uint32))
    return offsets, ids


@pytest.mark.parametrize("maker", ["builder", "from_files", "from_bytes", "from_csr", "reorder", "reorder_by_keys"])
def test_every_maker_of_an_index(world, ga, oracle, tmp_path, maker):
    """However an index over A's rows came to be, it holds the row sketches of the host model over the rows in its own
    order, so a launch of NQ splits -- and is the oracle's over the same rows and layers."""
    from granne_amd import _lib
    from oracle import fileformat as off
    case = world.tied()
    el, oix, b = case.el, case.oix, None
    if maker == "builder":
        b = ga.GranneBuilder("angular", el, num_neighbors=30, max_search=40)
        b.build()
        gix = b.get_index()
        oix = oracle.Index(el, b.layers())
    elif maker in ("from_files", "from_bytes"):
        ib, eb = off.write_index(oix.layers), off.write_elements(el)
        if maker == "from_files":
            (tmp_path / "i.granne").write_bytes(ib)
            (tmp_path / "e.bin").write_bytes(eb)
            gix = ga.Granne.from_files(str(tmp_path / "i.granne"), "angular", str(tmp_path / "e.bin"))
        else:
            gix = ga.Granne.from_bytes(ib, "angular", eb)
        oix = oracle.Index(el, _sorted_layers(oix.layers))
    elif maker == "from_csr":
        gix = ga.Granne.from_csr("angular", el, *_csr(oix.layers))
        oix = oracle.Index(el, _sorted_layers(oix.layers))
    else:
        gix = ga.Granne("angular", el, oix.layers)
        if maker == "reorder":
            order = gix.reorder()
        else:
            keys = np.random.default_rng(64).integers(0, 60, len(el)).astype(np.uint64)
            order = gix.reorder_by_keys(keys)
            assert order.tolist() == oix.order_by_keys(keys).tolist()
        assert sorted(order.tolist()) == list(range(len(el)))
        oix = oix.reordered(order)
        el = oix.elements
    try:
        assert len(gix) == len(el) and gix.get_option(_lib.OPT_SKETCH) == 1
        tab = gix.get_sketch()
        assert tab is not None and tab.tobytes() == row_sketch(el).tobytes()
        gix.set_option(_lib.OPT_SLOW_SLOTS, SLOW_SLOTS)
        q = case.q[:NQ]
        got = gix.search_batch(q, 50, K, stats=True)
        _is_split(gix, maker)
        _is_oracles(got, oix.search_batch(q, 50, K), slice(0, NQ), maker)
    finally:
        gix.close()
        if b is not None:
            b.close()
