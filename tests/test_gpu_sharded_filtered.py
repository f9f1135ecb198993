"""Filtered search on a partitioned index (granne_hip_sharded_search_filtered_batch*, ShardedHost.search_filtered_batch)
against tests/sharded_filter_model.expected_filtered: every shard's modelled walk under mask[off : off + len], merged by
oracle.merge -- ids, distance bytes and counts, exactly. tests/README_sharded_filtered.md says what each test pins.

The model walks in Python, so a shard's distances come from one matrix per shard (the library's Dist operator, as in
tests/test_gpu_filtered.py) and a (filter, max_search, max_expand) batch is modelled once per shard, at max_search + 5
neighbors, and cut to the k a test asks for."""
import ctypes as C

import numpy as np
import pytest

from tests import exact_topk_filtered_model as etm
from tests import filter_model as fm
from tests import sharded_filter_model as sm

pytestmark = pytest.mark.gpu

MS = 70
U64_MAX = np.iinfo(np.uint64).max


class World:
    """The fixture's shards on the GPU and in the model."""

    def __init__(self, oracle, int8, lengths):
        import granne_amd
        self.int8, self.lengths = int8, list(lengths)
        self.el, self.q = sm.fixture_rows(oracle, int8)
        self.gixs, self.model_shards, at = [], [], 0
        for n in self.lengths:
            part = np.ascontiguousarray(self.el[at:at + n])
            at += n
            oix = oracle.build_index(part, num_neighbors=10, max_search=20, n_threads=0)
            layers = [np.ascontiguousarray(l) for l in oix.layers]
            gix = granne_amd.Granne("angular_int" if int8 else "angular", part, layers)
            D = gix.dists_many(self.q, np.tile(np.arange(n, dtype=np.uint32), (len(self.q), 1)))
            self.gixs.append(gix)
            self.model_shards.append((layers, part, D, []))
        self.walks = {}

    def host(self, gap=0, groups=None):
        from granne_amd.sharded import ShardedHost
        return ShardedHost(self.gixs, sm.offsets(self.lengths, gap), groups=groups)

    def local(self, mask, gap, s):
        o = sm.offsets(self.lengths, gap)[s]
        return np.asarray(mask, bool)[..., o:o + self.lengths[s]]

    def want(self, name, mask, k, gap=0, max_expand=0, ms=MS):
        """expected_filtered, the shards' walks remembered under `name` (the mask's, with whatever else tells two apart)"""
        key = (name, gap, max_expand, ms)
        if key not in self.walks:
            self.walks[key] = [sm.shard_walks(layers, part, self.q, self.local(mask, gap, s), ms, ms + 5, max_expand, D, cache)
                               for s, (layers, part, D, cache) in enumerate(self.model_shards)]
        parts = [(i[:, :k], d[:, :k], np.minimum(c, k).astype(np.uint32)) for i, d, c, _ in self.walks[key]]
        return sm.merge(parts, sm.offsets(self.lengths, gap), k) + (sum(w[3] for w in self.walks[key]),)

    def shard_status(self, mask, k, gap=0, max_expand=0, ms=MS):
        """what every shard's own filtered call reports under its slice, folded: | + + +"""
        import granne_amd
        st = np.zeros(4, np.uint64)
        for s, gix in enumerate(self.gixs):
            a = self.local(mask, gap, s)
            allowed = a if a.ndim == 1 else [granne_amd.Filter.from_mask(row) for row in a]
            one = gix.search_filtered_batch(self.q, allowed, ms, k, max_expand, status=True)[-1].astype(np.uint64)
            st[0] |= one[0]
            st[1:] += one[1:]
        return st


@pytest.fixture(scope="module")
def worlds(oracle):
    made = {}

    def get(int8, lengths=tuple(sm.LENGTHS)):
        if (int8, lengths) not in made:
            made[(int8, lengths)] = World(oracle, int8, lengths)
        return made[(int8, lengths)]

    return get


def masks(w, gap=0):
    """name -> bool mask over the global ids: the shared filters of the issue"""
    offs = sm.offsets(w.lengths, gap)
    span = sm.id_span(w.lengths, offs)
    rng = np.random.default_rng(11)
    one_shard = np.zeros(span, bool)
    one_shard[offs[3]:offs[3] + w.lengths[3]] = True
    ends = np.zeros(span, bool)
    for o, n in zip(offs, w.lengths):
        ends[[o, o + n - 1]] = True
    return {"ones": np.ones(span, bool), "half": rng.random(span) < 0.5, "selective": rng.random(span) < 0.05,
            "none": np.zeros(span, bool), "one_shard": one_shard, "ends": ends}


def assert_equal(got, want):
    assert (got[2] == want[2]).all()
    assert (got[0] == want[0]).all()
    assert got[1].tobytes() == want[1].tobytes()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("name", ["ones", "half", "selective", "none", "one_shard", "ends"])
def test_shared_filters_equal_the_model(worlds, int8, name):
    w = worlds(int8)
    mask = masks(w)[name]
    h = w.host()
    assert h.id_span() == sm.N
    for k in (1, 10):
        got = h.search_filtered_batch(w.q, mask, MS, k, status=True)
        assert_equal(got, w.want(name, mask, k))
        assert (got[3] == w.shard_status(mask, k)).all() and got[3][3] == 0
        if name == "ones":  # the unfiltered search, bit for bit
            assert_equal(got, h.search_batch(w.q, MS, k))
        if name == "none":
            assert (got[2] == 0).all()
        if name == "selective":  # walks that outgrow the bounded queues are handed to the exact walker: [1] is a sum over shards
            assert got[3][1] > 0
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_garbage_past_id_span_is_never_read(worlds, int8):
    import granne_amd
    w = worlds(int8)
    mask = masks(w)["half"]
    h = w.host()
    f = granne_amd.Filter.from_words(etm.words(mask, garbage_past_n=True), sm.N)
    assert_equal(h.search_filtered_batch(w.q, f, MS, 10), w.want("half", mask, 10))
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_k_64_over_8_equal_shards(worlds, int8):
    from granne_amd.sharded import shard_bounds
    lengths = tuple(hi - lo for lo, hi in shard_bounds(sm.N, 8))
    w = worlds(int8, lengths)
    mask = np.random.default_rng(12).random(sm.N) < 0.5
    h = w.host()
    assert_equal(h.search_filtered_batch(w.q, mask, MS, 64), w.want("half8", mask, 64))
    h.close()


def _device_call(h, w, words, stride, k, max_expand=0, ms=MS, nq=None):
    """the device entry on buffers of the test's own: words [rows][stride or word count] u32; returns ids, dists, counts, status"""
    from granne_amd import _lib
    from granne_amd.filters import _DeviceBlock
    q = w.q if nq is None else w.q[:nq]
    nq = len(q)
    d_q = _DeviceBlock(q.nbytes, h.device).upload(q)
    d_f = _DeviceBlock(words.nbytes, h.device).upload(words)
    d_ids, d_ds, d_cnt = _DeviceBlock(nq * k * 8, h.device), _DeviceBlock(nq * k * 4, h.device), _DeviceBlock(nq * 4, h.device)
    d_st = _DeviceBlock(16, h.device).upload(np.zeros(4, np.uint32))
    h.search_filtered_batch_device(d_q.ptr, nq, ms, k, d_f.ptr, stride, max_expand, d_ids.ptr, d_ds.ptr, d_cnt.ptr, d_st.ptr)
    _lib.check(_lib.lib().granne_hip_stream_synchronize(None, h.device))
    return (d_ids.download(np.uint64, nq * k).reshape(nq, k), d_ds.download(np.float32, nq * k).reshape(nq, k),
            d_cnt.download(np.uint32, nq), d_st.download(np.uint32, 4))


@pytest.mark.parametrize("int8", [False, True])
def test_per_query_filters(worlds, int8):
    w = worlds(int8)
    mask = np.random.default_rng(13).random((sm.NQ, sm.N)) < 0.3
    mask[0] = False
    want = w.want("per_query", mask, 10)
    h = w.host()
    assert_equal(h.search_filtered_batch(w.q, mask, MS, 10), want)  # stride = the word count
    words = np.stack([fm.pack_bits(row) for row in mask])
    padded = np.full((sm.NQ, words.shape[1] + 3), 0xFFFFFFFF, np.uint32)
    padded[:, :words.shape[1]] = words
    got = _device_call(h, w, padded, padded.shape[1], 10)
    assert_equal(got, want)
    assert (got[3].astype(np.uint64) == w.shard_status(mask, 10)).all()
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_max_expand_caps_every_shards_walk(worlds, int8):
    w = worlds(int8)
    mask = masks(w)["half"]
    h = w.host()
    got = h.search_filtered_batch(w.q, mask, MS, 10, max_expand=3, status=True)
    want = w.want("half", mask, 10, max_expand=3)
    assert_equal(got, want)
    assert got[3][3] == want[3] > 0  # walks cut, summed over the shards
    assert (got[3] == w.shard_status(mask, 10, max_expand=3)).all()
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_offsets_with_gaps(worlds, int8):
    w = worlds(int8)
    gap = 13
    offs = sm.offsets(w.lengths, gap)
    span = sm.id_span(w.lengths, offs)
    h = w.host(gap=gap)
    assert h.id_span() == span
    mask = np.random.default_rng(14).random(span) < 0.5
    for o, n in zip(offs[:-1], w.lengths[:-1]):
        mask[o + n:o + n + gap] = True  # ids no shard holds: ignored
    got = h.search_filtered_batch(w.q, mask, MS, 10)
    assert_equal(got, w.want("gaps", mask, 10, gap=gap))
    assert not np.isin(got[0][got[0] != U64_MAX], np.concatenate([np.arange(o + n, o + n + gap) for o, n in zip(offs, w.lengths)])).any()
    h.close()


@pytest.mark.parametrize("int8", [False, True])
@pytest.mark.parametrize("groups", [[0, 0, 1, 1, 2], [0, 1, 2, 3, 4]])
def test_exchange_groups_copy_and_slice_the_filter(worlds, int8, groups):
    """shards of another group take their bits by a copy of the covering words (offset 64: the copy is the slice) and a slice
    launch behind it (offsets 1001, 2001; 31 when every shard is a group of its own)"""
    w = worlds(int8)
    h = w.host(groups=groups)
    mask = masks(w)["half"]
    assert_equal(h.search_filtered_batch(w.q, mask, MS, 10), w.want("half", mask, 10))
    pq = np.random.default_rng(13).random((sm.NQ, sm.N)) < 0.3
    pq[0] = False
    assert_equal(h.search_filtered_batch(w.q, pq, MS, 10), w.want("per_query", pq, 10))  # one strided copy per shard
    h.close()


@pytest.mark.parametrize("int8", [False, True])
def test_host_and_device_entries_twice_and_with_other_batch_sizes(worlds, int8):
    from granne_amd import _lib
    w = worlds(int8)
    mask = masks(w)["half"]
    want = w.want("half", mask, 10)
    words = fm.pack_bits(mask)
    h = w.host()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for nq in (sm.NQ, sm.NQ, 7, 1, sm.NQ):  # two calls in a row, then other batch sizes on the same handle
        ids, ds, cnt, st = np.empty((nq, 10), np.uint64), np.empty((nq, 10), np.float32), np.zeros(nq, np.uint32), np.ones(4, np.uint32)
        q = np.ascontiguousarray(w.q[:nq])
        _lib.check(_lib.lib().granne_hip_sharded_search_filtered_batch(h._h, p(q), nq, MS, 10, p(words), 0, 0, p(ids), p(ds), p(cnt), p(st)))
        assert_equal((ids, ds, cnt), tuple(a[:nq] for a in want[:3]))
        assert st[0] == 0 and st[3] == 0
        got = _device_call(h, w, words, 0, 10, nq=nq)
        assert_equal(got, tuple(a[:nq] for a in want[:3]))
    # nq == 0 does nothing; num_neighbors == 0 gives empty results
    _lib.check(_lib.lib().granne_hip_sharded_search_filtered_batch(h._h, None, 0, MS, 10, None, 0, 0, None, None, None, None))
    cnt = np.ones(sm.NQ, np.uint32)
    _lib.check(_lib.lib().granne_hip_sharded_search_filtered_batch(h._h, p(w.q), sm.NQ, MS, 0, p(words), 0, 0, None, None, p(cnt), None))
    assert (cnt == 0).all()
    h.close()


def test_refusals(worlds):
    from granne_amd import _lib
    w = worlds(False)
    lib, h = _lib.lib(), w.host()
    words = fm.pack_bits(np.ones(sm.N, bool))
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = 10
    ids, ds, cnt = np.empty((sm.NQ, 820), np.uint64), np.empty((sm.NQ, 820), np.float32), np.zeros(sm.NQ, np.uint32)

    def call(ms=MS, k=k, filt=p(words), stride=0):
        return lib.granne_hip_sharded_search_filtered_batch(h._h, p(w.q), sm.NQ, ms, k, filt, stride, 0, p(ids), p(ds), p(cnt), None)

    assert call(ms=0) == _lib.ERR_INVALID and b"max_search" in lib.granne_hip_last_error()
    assert call(filt=None) == _lib.ERR_INVALID and b"filter is null" in lib.granne_hip_last_error()
    assert call(stride=len(words) - 1) == _lib.ERR_INVALID and b"filter_stride_words" in lib.granne_hip_last_error()
    assert call(k=820) == _lib.ERR_INVALID and b"4096" in lib.granne_hip_last_error()  # 5 shards x 820 = 4100
    assert lib.granne_hip_sharded_search_filtered_batch_device(h._h, None, sm.NQ, MS, k, p(words), 0, 0, None, None, None, None,
                                                               None) == _lib.ERR_INVALID
    assert call() == _lib.OK  # and the handle still works
    h.close()
