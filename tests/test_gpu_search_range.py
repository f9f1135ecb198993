"""Range search by the walk on the GPU (granne_hip_search_range_batch*, granne_amd/csrc/range.h) against the staged model
over the CPU oracle (tests/range_model.py): every case compares the WHOLE ids array, the distance BYTES, the counts, found,
stage and status[3]. No tolerance anywhere. What each test pins: tests/README_range.md."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import range_model as rm  # noqa: E402

STAGES = [16, 64, 256]
DENSE = ["f32-100", "i8-100"]
_gix, _answers = {}, {}


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def gix(ga, oracle, name):
    if name not in _gix:
        w = rm.world(oracle, name)
        _gix[name] = ga.Granne(w["et"], w["rows"], w["oix"].layers)
    return _gix[name]


def model(oracle, name, cap, stages, fallback, radii=None):
    """the model's answer under the issue's radii, computed once per (world, arguments) and left unchanged"""
    key = (name, cap, tuple(stages), fallback, None if radii is None else radii.tobytes())
    if key not in _answers:
        w = rm.world(oracle, name)
        _answers[key] = rm.search_range(oracle, w["oix"], w["q"], rm.issue_radii(w) if radii is None else radii, cap, stages, fallback)
    return _answers[key]


def assert_equals_model(got, a):
    ids, ds, cnt, found, stage, st = got
    assert (stage == a.stage).all(), (np.nonzero(stage != a.stage)[0][:5], stage[:12], a.stage[:12])
    assert (found == a.found).all(), np.nonzero(found != a.found)[0][:5]
    assert (cnt == a.counts).all()
    bad = np.nonzero((ids != a.ids).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], a.ids[bad[:1]])
    assert ds.tobytes() == a.dists.tobytes()
    assert st[0] == 0 and st[3] == a.unfinished, (st, a.unfinished)


@pytest.mark.parametrize("fallback", ["exact", "short"])
@pytest.mark.parametrize("name", DENSE)
def test_equals_the_staged_model(ga, oracle, name, fallback):
    """the issue's radii under stages [16, 64, 256]: every stage code and the fallback's occur (asserted first, on the
    model); cap 3 lies below, at and above `within` (asserted), 50 between the stages' lists, 1024 above every list"""
    w = rm.world(oracle, name)
    code = rm.STAGE_EXACT if fallback == "exact" else rm.STAGE_SHORT
    for cap in (3, 50, 1024):
        a = model(oracle, name, cap, STAGES, fallback)
        assert set(a.stage.tolist()) == {0, 1, 2, code}
        if cap == 3:
            assert (a.found < cap).any() and (a.found == cap).any() and (a.found > cap).any()
        got = gix(ga, oracle, name).search_range_batch(w["q"], rm.issue_radii(w), cap, STAGES, fallback, stats=True)
        assert_equals_model(got, a)


def test_f16_with_the_short_fallback_and_its_exact_refusal(ga, oracle):
    from granne_amd import _lib
    w = rm.world(oracle, "f16-100")
    ix = gix(ga, oracle, "f16-100")
    a = model(oracle, "f16-100", 50, STAGES, "short")
    assert set(a.stage.tolist()) == {0, 1, 2, rm.STAGE_SHORT}
    assert_equals_model(ix.search_range_batch(w["q"], rm.issue_radii(w), 50, STAGES, "short", stats=True), a)
    with pytest.raises(ga.GranneHipError, match="GRANNE_HIP_RG_FALLBACK_EXACT has no form for GRANNE_HIP_F16") as e:
        ix.search_range_batch(w["q"], 0.5, 50, STAGES, "exact")
    assert e.value.code == _lib.ERR_INVALID
    assert_equals_model(ix.search_range_batch(w["q"], rm.issue_radii(w), 50, STAGES, "short", stats=True), a)  # the device answers afterwards


def test_a_graph_shorter_than_the_first_stage(ga, oracle):
    w = rm.world(oracle, "tiny-f32")
    a = model(oracle, "tiny-f32", 50, STAGES, "exact", radii=np.full(rm.NQ, np.inf, np.float32))
    assert (a.stage == 0).all() and (a.found == w["n"]).all()
    assert_equals_model(gix(ga, oracle, "tiny-f32").search_range_batch(w["q"], np.inf, 50, STAGES, "exact", stats=True), a)


@pytest.mark.parametrize("name", DENSE + ["f16-100"])
def test_one_stage_infinite_radius_short_is_the_plain_search(ga, oracle, name):
    w = rm.world(oracle, name)
    ix = gix(ga, oracle, name)
    for cap in (10, 50):
        ids, ds, cnt, found, stage, st = ix.search_range_batch(w["q"], np.inf, cap, [50], "short", stats=True)
        si, sd, sc = ix.search_batch(w["q"], 50, 50)
        assert (ids == si[:, :cap]).all() and ds.tobytes() == np.ascontiguousarray(sd[:, :cap]).tobytes()
        assert (cnt == np.minimum(sc, cap)).all() and (found == sc).all()
        assert (stage == rm.STAGE_SHORT).all() and st[3] == rm.NQ


def test_more_queries_than_one_scratch_chunk(ga, oracle):
    """scratch_bytes for 7 lists of the first stage (and fewer of the later ones): the same result for any value"""
    w = rm.world(oracle, "i8-100")
    a = model(oracle, "i8-100", 50, STAGES, "exact")
    got = gix(ga, oracle, "i8-100").search_range_batch(w["q"], rm.issue_radii(w), 50, STAGES, "exact", scratch_bytes=7 * 12 * 16, stats=True)
    assert_equals_model(got, a)


def test_the_host_entry_and_single_queries(ga, oracle):
    from granne_amd import _lib
    w = rm.world(oracle, "f32-100")
    ix = gix(ga, oracle, "f32-100")
    a = model(oracle, "f32-100", 50, STAGES, "exact")
    q, radii, nq, cap = w["q"], rm.issue_radii(w), rm.NQ, 50
    oid, ods = np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32)
    ocnt, ofound, ostage, ost = (np.full(nq, 77, np.uint32) for _ in range(4))
    ost = np.full(4, 77, np.uint32)
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    stages = (C.c_uint32 * 3)(*STAGES)
    rc = _lib.lib().granne_hip_search_range_batch(ix._h, p(q), nq, p(radii), cap, stages, 3, _lib.RG_FALLBACK_EXACT, 0, p(oid), p(ods), p(ocnt),
                                                  p(ofound), p(ostage), p(ost))
    assert rc == _lib.OK
    assert_equals_model((oid, ods, ocnt, ofound, ostage, ost), a)
    for qi in (0, 1, 2, 3, 4):
        one = ix.search_range(q[qi], radii[qi], cap, STAGES, "exact")
        assert [i for i, _ in one] == a.ids[qi, :a.counts[qi]].tolist()
        assert np.array([d for _, d in one], np.float32).tobytes() == a.dists[qi, :a.counts[qi]].tobytes()
    bad = radii.copy()
    bad[7] = np.nan
    rc = _lib.lib().granne_hip_search_range_batch(ix._h, p(q), nq, p(bad), cap, stages, 3, 1, 0, p(oid), p(ods), p(ocnt), None, None, None)
    assert rc == _lib.ERR_INVALID and b"the radius of query 7 is NaN" in _lib.lib().granne_hip_last_error()
