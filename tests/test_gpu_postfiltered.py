"""Post-filtered search on the GPU (granne_hip_search_postfiltered_batch*, granne_amd/csrc/postfilter.h) against the model
over the CPU oracle (tests/postfilter_model.py): every case compares the WHOLE ids array, the distance BYTES, the counts,
out_stage and status[3]. No tolerance anywhere. Filters are handed over as words with the bits at positions >= n SET.
What each test pins: tests/README_postfiltered.md."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_filtered_model as efm  # noqa: E402
from tests import postfilter_model as pm  # noqa: E402

NONE = pm.NONE
DENSE = ["f32-8", "i8-8", "i8-100", "f32-200"]
ALL = DENSE + ["f16-100"]
_gix, _answers = {}, {}


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def gix(ga, oracle, name):
    if name not in _gix:
        w = pm.world(oracle, name)
        _gix[name] = ga.Granne(w["et"], w["rows"], w["oix"].layers)
    return _gix[name]


def shared_filter(ga, mask):
    return ga.Filter.from_words(pm.words(mask), len(mask))


def model(oracle, name, key, masks, k, min_allowed, stages, fallback, nq=pm.NQ):
    """the model's answer, computed once per (world, filter, arguments) and left unchanged"""
    key = (name, key, k, min_allowed, tuple(stages), fallback, nq)
    if key not in _answers:
        w = pm.world(oracle, name)
        m = masks if np.ndim(masks) == 1 else masks[:nq]
        _answers[key] = pm.postfiltered(oracle, w["oix"], w["q"][:nq], m, k, min_allowed, stages, fallback)
    return _answers[key]


def assert_equals_model(got, a):
    ids, ds, cnt, stage, st = got
    bad = np.nonzero((ids != a.ids).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], a.ids[bad[:1]], stage[bad[:5]], a.stage[bad[:5]])
    assert ds.tobytes() == a.dists.tobytes()
    assert (cnt == a.counts).all()
    assert (stage == a.stage).all(), np.nonzero(stage != a.stage)[0][:5]
    assert st[0] == 0 and st[3] == a.unfinished, (st, a.unfinished)


def run(ga, oracle, name, allowed, k, min_allowed, stages, fallback, nq=pm.NQ, scratch_bytes=0):
    w = pm.world(oracle, name)
    return gix(ga, oracle, name).search_postfiltered_batch(w["q"][:nq], k, allowed, min_allowed, stages, fallback, scratch_bytes,
                                                           return_stage=True, status=True)


@pytest.mark.parametrize("name", ALL)
def test_all_ones_one_stage_is_the_plain_search(ga, oracle, name):
    """All bits set: every query ends at stage 0 and the answer is search_batch(E_0, k) -- the library's own and the
    oracle's -- bit for bit. On the dense 100-d / 200-d handles the walker is a register walker: the point of the feature."""
    from granne_amd import _lib
    w = pm.world(oracle, name)
    ix = gix(ga, oracle, name)
    ones = shared_filter(ga, np.ones(w["n"], bool))
    for E0, k, min_allowed in ((50, 10, 50), (16, 10, 16), (64, 64, 64)):
        ids, ds, cnt, stage, st = run(ga, oracle, name, ones, k, min_allowed, [E0], "exact" if name != "f16-100" else "short")
        walker = ix.get_option(_lib.OPT_LAST_WALKER)
        if name in ("i8-100", "f32-200"):
            assert walker in (_lib.WALKER_REGISTER, _lib.WALKER_REGISTER_WIDE), walker
        si, sd, sc = ix.search_batch(w["q"], E0, k)
        assert (ids == si).all() and ds.tobytes() == sd.tobytes() and (cnt == sc).all()
        oi, od, oc, _ = w["oix"].search_batch(w["q"], E0, k)
        assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
        assert (stage == 0).all() and st[3] == 0 and st[0] == 0


@pytest.mark.parametrize("fallback", ["exact", "short"])
@pytest.mark.parametrize("name", ["f32-8", "i8-8"])
def test_a_shared_filter_of_varying_density_holds_every_outcome(ga, oracle, name, fallback):
    w = pm.world(oracle, name)
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    stages = [16, 64, 256]
    a = model(oracle, name, "density", mask, 10, 16, stages, fallback)
    assert min(a.outcome_counts(3)) >= 4, a.outcome_counts(3)  # a condition on the inputs, from the model
    assert_equals_model(run(ga, oracle, name, shared_filter(ga, mask), 10, 16, stages, fallback), a)


@pytest.mark.parametrize("fallback", ["exact", "short"])
@pytest.mark.parametrize("name", DENSE)
def test_one_filter_per_query(ga, oracle, name, fallback):
    w = pm.world(oracle, name)
    masks = pm.per_query_masks(np.random.default_rng(101), w["n"], pm.NQ)
    stages = [16, 64, 256, 1024]
    a = model(oracle, name, "per-query", masks, 10, 16, stages, fallback)
    assert min(a.outcome_counts(4)) >= 4, a.outcome_counts(4)
    filters = [shared_filter(ga, m) for m in masks]
    assert_equals_model(run(ga, oracle, name, filters, 10, 16, stages, fallback), a)


@pytest.mark.parametrize("name", ["f32-8", "i8-8"])
def test_the_exhausted_rule(ga, oracle, name):
    """A stage beyond len ([16, 4096] on n = 3000): the walk runs out of graph and the stage answers. A filter allowing one
    id finishes at stage 1 with count 1, not in the fallback; so does one allowing nothing, with count 0. A stage in the
    two-level-list range: [16, 256, 2048]."""
    w = pm.world(oracle, name)
    nq = 65
    for key, mask in (("one", efm.only(w["n"], [1234])), ("none", np.zeros(w["n"], bool)),
                      ("sparse", np.random.default_rng(102).random(w["n"]) < 0.004)):
        a = model(oracle, name, key, mask, 10, 16, [16, 4096], "exact", nq)
        assert (a.stage >= 1).any() and a.unfinished == 0
        got = run(ga, oracle, name, shared_filter(ga, mask), 10, 16, [16, 4096], "exact", nq)
        assert_equals_model(got, a)
        if key == "one":
            assert (got[3] == 1).all() and (got[2] == 1).all() and (got[0][:, 0] == 1234).all()
        if key == "none":
            assert (got[3] == 1).all() and (got[2] == 0).all() and (got[0] == NONE).all() and np.isinf(got[1]).all()
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    for fallback in ("exact", "short"):
        a = model(oracle, name, "density", mask, 10, 16, [16, 256, 2048], fallback)
        assert (a.stage == 2).sum() >= 4
        assert_equals_model(run(ga, oracle, name, shared_filter(ga, mask), 10, 16, [16, 256, 2048], fallback), a)


def test_nothing_allowed_without_an_exhausting_stage(ga, oracle):
    none = np.zeros(3000, bool)
    for fallback, code in (("exact", pm.STAGE_EXACT), ("short", pm.STAGE_SHORT)):
        ids, ds, cnt, stage, st = run(ga, oracle, "f32-8", shared_filter(ga, none), 10, 16, [16, 64], fallback, 65)
        assert (cnt == 0).all() and (ids == NONE).all() and np.isinf(ds).all() and (stage == code).all() and st[3] == 65


def test_ties_come_in_id_order(ga, oracle):
    """Every row stored twice (ids i and i + 1500): equal distances straddle the k-th allowed place for odd k, and a filter
    that allows only one copy of some pairs moves the straddle about. The order is by (distance, id)."""
    w = pm.world(oracle, "ties-8")
    rng = np.random.default_rng(103)
    for key, mask in (("ones", np.ones(3000, bool)), ("some", rng.random(3000) < 0.6)):
        for k, fallback in ((9, "exact"), (10, "short"), (1, "exact")):
            a = model(oracle, "ties-8", key, mask, k, 16, [16, 64, 256], fallback, 65)
            assert_equals_model(run(ga, oracle, "ties-8", shared_filter(ga, mask), k, 16, [16, 64, 256], fallback, 65), a)
    a = model(oracle, "ties-8", "ones", np.ones(3000, bool), 9, 16, [16, 64, 256], "exact", 65)
    assert (a.dists[:, 0::2][:, :4] == a.dists[:, 1::2][:, :4]).all() and (a.ids[:, 0] + 1500 == a.ids[:, 1]).all()  # the world has ties


@pytest.mark.parametrize("nq", [1, 65, 300])
def test_launch_sizes(ga, oracle, nq):
    w = pm.world(oracle, "f32-8")
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    a = model(oracle, "f32-8", "density", mask, 10, 16, [16, 64, 256], "exact", nq)
    assert_equals_model(run(ga, oracle, "f32-8", shared_filter(ga, mask), 10, 16, [16, 64, 256], "exact", nq), a)
    w = pm.world(oracle, "i8-100")  # one filter per query: the fallback gathers the pending queries' bitmaps
    masks = pm.per_query_masks(np.random.default_rng(101), w["n"], pm.NQ)[:nq]
    a = model(oracle, "i8-100", "per-query", masks, 10, 16, [16, 64, 256, 1024], "exact", nq)
    assert_equals_model(run(ga, oracle, "i8-100", [shared_filter(ga, m) for m in masks], 10, 16, [16, 64, 256, 1024], "exact", nq), a)


def test_chunking_gives_the_same_bytes(ga, oracle):
    """scratch_bytes small enough for at least three chunks at every stage (a list is 12 * E bytes per pending query; the
    last stage has at least 12 pending queries here), down to one query per chunk: the same bytes."""
    for name, kind in (("f32-8", "density"), ("i8-8", "per-query")):
        w = pm.world(oracle, name)
        stages = [16, 64, 256]
        if kind == "density":
            masks = pm.density_mask(np.random.default_rng(100), w["rows_f"])
            allowed = shared_filter(ga, masks)
        else:
            masks = pm.per_query_masks(np.random.default_rng(101), w["n"], pm.NQ)
            allowed = [shared_filter(ga, m) for m in masks]
        for fallback in ("exact", "short"):
            a = model(oracle, name, kind, masks, 10, 16, stages, fallback)
            assert a.per_stage[2] >= 12
            for scratch in (4 * 12 * 256, 100 * 12 * 16, 1):
                assert_equals_model(run(ga, oracle, name, allowed, 10, 16, stages, fallback, scratch_bytes=scratch), a)


def test_device_pointer_entry_and_status_accumulation(ga, oracle):
    import torch
    from granne_amd import _lib
    name = "f32-8"
    w = pm.world(oracle, name)
    ix = gix(ga, oracle, name)
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    a = model(oracle, name, "density", mask, 10, 16, [16, 64, 256], "exact")
    f = shared_filter(ga, mask)
    nq, k = pm.NQ, 10
    dq = torch.from_numpy(w["q"].copy()).cuda()
    ids = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    ds = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.full((nq,), 99, dtype=torch.int32, device="cuda")
    stage = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    for call in (1, 2):
        ix.search_postfiltered_batch_device(dq.data_ptr(), nq, k, 16, [16, 64, 256], _lib.PF_FALLBACK_EXACT, f.ptr, 0, ids.data_ptr(),
                                            ds.data_ptr(), cnt.data_ptr(), stage.data_ptr(), status.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        got = (ids.cpu().numpy().astype(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32),
               stage.cpu().numpy().astype(np.uint32), np.array([0, 0, 0, a.unfinished]))
        assert_equals_model(got, a)
        assert status.cpu().numpy()[3] == call * a.unfinished and status.cpu().numpy()[0] == 0  # accumulated, not written
    # no out_stage, no status
    ids.fill_(-7)
    ix.search_postfiltered_batch_device(dq.data_ptr(), nq, k, 16, [16, 64, 256], _lib.PF_FALLBACK_SHORT, f.ptr, 0, ids.data_ptr(),
                                        ds.data_ptr(), cnt.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    s = model(oracle, name, "density", mask, 10, 16, [16, 64, 256], "short")
    assert (ids.cpu().numpy().astype(np.uint64) == s.ids).all() and (cnt.cpu().numpy().astype(np.uint32) == s.counts).all()


def test_host_entry_and_single_query(ga, oracle):
    from granne_amd import _lib
    L = _lib.lib()
    name = "i8-8"
    w = pm.world(oracle, name)
    ix = gix(ga, oracle, name)
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    a = model(oracle, name, "density", mask, 10, 16, [16, 64, 256], "exact")
    nq, k = pm.NQ, 10
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    oid, ods = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32)
    ocnt, osg, ost = np.full(nq, 77, np.uint32), np.full(nq, 77, np.uint32), np.full(4, 9, np.uint32)
    st = (C.c_uint32 * 3)(16, 64, 256)
    q = np.ascontiguousarray(w["q"])
    assert L.granne_hip_search_postfiltered_batch(ix._h, p(q), nq, k, 16, st, 3, 1, p(pm.words(mask)), 0, 0, p(oid), p(ods), p(ocnt), p(osg),
                                                  p(ost)) == _lib.OK
    assert_equals_model((oid, ods, ocnt, osg, ost), a)
    # one query through the Python wrapper, a bool array as the filter, default stages from the filter's count
    got = ix.search_postfiltered(w["q"][0], 10, mask, min_allowed=16, stages=[16, 64, 256])
    assert [i for i, _ in got] == [int(i) for i in a.ids[0, :a.counts[0]]]
    ids, ds, cnt, stage = ix.search_postfiltered_batch(w["q"][:20], 10, mask, return_stage=True)
    assert mask[ids[ids != NONE].astype(np.int64)].all() and (cnt == 10).all()
    with pytest.raises(ValueError):
        ix.search_postfiltered_batch(w["q"][:, :7], 10, mask)


def test_f16_handle_and_refusals(ga, oracle):
    """An angular_f16 handle: fallback SHORT equals the model over R = normalize_f32(widen(rows16)); fallback EXACT is
    refused by a message naming F16 (before anything is enqueued), and the device still answers afterwards. The refusals
    that need a handle: a null filter, a short stride."""
    from granne_amd import _lib
    L = _lib.lib()
    name = "f16-100"
    w = pm.world(oracle, name)
    ix = gix(ga, oracle, name)
    masks = pm.per_query_masks(np.random.default_rng(101), w["n"], pm.NQ)
    stages = [16, 64, 256, 1024]
    a = model(oracle, name, "per-query", masks, 10, 16, stages, "short")
    assert min(a.outcome_counts(4)) >= 4, a.outcome_counts(4)
    filters = [shared_filter(ga, m) for m in masks]
    assert_equals_model(run(ga, oracle, name, filters, 10, 16, stages, "short"), a)
    f = filters[1]
    with pytest.raises(ga.GranneHipError, match="F16"):
        run(ga, oracle, name, f, 10, 16, stages, "exact")
    assert_equals_model(run(ga, oracle, name, filters, 10, 16, stages, "short"), a)  # the device still answers
    mask = masks[1]  # one filter for all queries
    a1 = model(oracle, name, "half", mask, 10, 16, [16, 64], "short")
    assert_equals_model(run(ga, oracle, name, f, 10, 16, [16, 64], "short"), a1)
    p = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    st = (C.c_uint32 * 2)(16, 64)
    dix = gix(ga, oracle, "f32-8")
    for flt, stride, word in ((None, 0, "the filter is null"), (C.c_void_p(f.ptr), 93, "filter_stride_words (93)")):  # ceil(3000 / 32) = 94
        for rc in (L.granne_hip_search_postfiltered_batch_device(dix._h, p, 1, 10, 16, st, 2, 1, flt, stride, 0, p, p, p, None, None, None),
                   L.granne_hip_search_postfiltered_batch(dix._h, p, 1, 10, 16, st, 2, 1, None if flt is None else p, stride, 0, p, p, p, None, None)):
            assert rc == _lib.ERR_INVALID and word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()
    assert L.granne_hip_search_postfiltered_batch_device(dix._h, None, 0, 10, 16, st, 2, 1, C.c_void_p(f.ptr), 0, 0, None, None, None, None, None,
                                                         None) == _lib.OK  # nq == 0 does nothing
