"""exact_range (granne_amd/csrc/exact_range.h) against its model over the CPU oracle (tests/range_model.py): every case
compares the WHOLE ids array, the distance bytes, the counts and the totals. No tolerance anywhere. The shapes, the radii
and the tie inputs are range_model's and exact_topk_model's; tests/test_range_model.py asserts on the host that they reach
what these tests mean to reach (every border total, phase B, the second level, the overflow)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import exact_topk_model as m  # noqa: E402
from tests import range_model as rm  # noqa: E402

NONE = rm.NONE


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def same(got, ans, what=""):
    """(ids, dists, counts, totals[, status]) of the GPU against a range_model.Exact"""
    ids, ds, cnt, tot = got[:4]
    assert (tot == ans.totals).all(), (what, np.nonzero(tot != ans.totals)[0][:5], tot[:8], ans.totals[:8])
    assert (cnt == ans.counts).all(), (what, np.nonzero(cnt != ans.counts)[0][:5])
    assert (ids == ans.ids).all(), (what, np.nonzero((ids != ans.ids).any(axis=1))[0][:5])
    assert ds.tobytes() == ans.dists.tobytes(), what


@pytest.mark.parametrize("shape", rm.SHAPES, ids=rm.shape_id)
def test_equals_the_model(ga, oracle, shape):
    el, q, scan = rm.shape_input(oracle, shape)
    ix = ga.Granne(_et(el), el, [])
    for j, cap in enumerate(shape[4]):
        radii = rm.mixed_radii(scan, cap, start=j * 5)
        ans = rm.exact_range(scan, radii, cap)
        got = ix.exact_range(q, radii, cap, stats=True)
        same(got, ans, cap)
        st = got[4]
        dense = int((ans.totals > rm.ET_CAP).sum())
        assert st[0] == 0 and st[1] == dense and st[3] == 0
        assert st[2] >= ans.ranked and (dense or st[2] == ans.ranked)
    ix.close()


def test_an_infinite_radius_is_exact_topk(ga, oracle):
    shape = rm.SHAPES[3]
    assert shape[2] == 20011
    el, q, scan = rm.shape_input(oracle, shape)
    ix = ga.Granne(_et(el), el, [])
    ids, ds, cnt, tot, st = ix.exact_range(q, np.inf, 1024, stats=True)
    ti, td, tc = ix.exact_topk(q, 1024)
    assert (tot == 20011).all() and st[1] == len(q)  # phase B for every query
    assert (ids == ti).all() and ds.tobytes() == td.tobytes() and (cnt == tc).all()
    same((ids, ds, cnt, tot), rm.exact_range(scan, np.inf, 1024))
    ids, ds, cnt, tot = ix.exact_range(q[:3], 2.0, 17)  # a scalar radius; every pair a hit
    same((ids, ds, cnt, tot), rm.exact_range((scan[0][:3], scan[1][:3]), 2.0, 17))
    ix.close()


def test_ties_come_in_id_order_across_the_cap(ga, oracle):
    rng = np.random.default_rng(21)
    el = m.tripled(m.unit_rows(oracle, rng, 1200, 32))
    q = m.unit_rows(oracle, rng, 9, 32)
    q[8] = 0  # a zero query: every distance exactly 1.0 -- 3,600 rows at the radius, answered by phase A in id order
    scan = rm.full_scan(oracle, el, q)
    ix = ga.Granne("angular", el, [])
    for cap in (1, 17, 100, 1024):  # 17 and 100 cut inside a triple
        radii = np.array([scan[1][a, 3 * (a + 1) * 40 - 1] for a in range(8)] + [1.0], np.float32)
        ans = rm.exact_range(scan, radii, cap)
        assert (ans.totals[:8] % 3 == 0).all() and ans.totals[8] == 3600
        got = ix.exact_range(q, radii, cap, stats=True)
        same(got, ans, cap)
        assert got[4][1] == 0 and got[4][2] == 3600
        assert (got[0][8] == np.arange(cap)).all() and (got[1][8] == 1.0).all()
    ix.close()


def test_phase_b_through_the_second_level(ga, oracle):
    el, q = m.second_level_input(oracle)
    d = m.all_dists(oracle, el, q[0])
    m.second_level_precondition(d)
    q = np.repeat(q, 3, axis=0)
    scan = rm.full_scan(oracle, el, q)
    radii = np.array([d.max(), d.max(), scan[1][0, 49]], np.float32)  # 6,050 rows twice; the 50 nearer rows alone
    ans = rm.exact_range(scan, radii, 100)
    assert ans.totals.tolist() == [6050, 6050, 50] and not ans.voided.any()
    ix = ga.Granne("angular", el, [])
    got = ix.exact_range(q, radii, 100, stats=True)
    same(got, ans)
    assert got[4][0] == 0 and got[4][1] == 2
    ix.close()


def test_overflow_voids_the_query_and_keeps_its_total(ga, oracle):
    from granne_amd import _lib
    el, q = m.duplicates_nearest(oracle, np.random.default_rng(24))
    scan = rm.full_scan(oracle, el, q)
    nq, cap = len(q), 100
    radii = np.array([scan[1][0, 4999]] + [scan[1][a, 29] for a in range(1, nq)], np.float32)
    ans = rm.exact_range(scan, radii, cap)
    assert ans.voided.tolist() == [True] + [False] * (nq - 1) and ans.totals[0] == 5000
    ix = ga.Granne("angular", el, [])
    with pytest.raises(ga.GranneHipError) as e:
        ix.exact_range(q, radii, cap)
    assert e.value.code == _lib.ERR_OVERFLOW
    got = ix.exact_range(q, radii, cap, stats=True)
    same(got, ans)
    assert got[4][0] == 1 and got[4][1] == 1
    assert got[2][0] == 0 and (got[0][0] == NONE).all() and np.isinf(got[1][0]).all() and got[3][0] == 5000
    # the host entry: GRANNE_HIP_ERR_OVERFLOW, the outputs and the status still written
    oid, ods = np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32)
    ocnt, otot, ost = np.full(nq, 77, np.uint32), np.full(nq, 77, np.uint32), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = _lib.lib().granne_hip_exact_range(ix._h, p(q), nq, p(radii), cap, None, 0, p(oid), p(ods), p(ocnt), p(otot), p(ost))
    assert rc == _lib.ERR_OVERFLOW
    same((oid, ods, ocnt, otot), ans)
    assert (ost == got[4]).all()
    rc = _lib.lib().granne_hip_exact_range(ix._h, p(q[1:]), nq - 1, p(radii[1:]), cap, None, 0, p(oid), p(ods), p(ocnt), p(otot), None)
    assert rc == _lib.OK and (oid[:nq - 1] == ans.ids[1:]).all() and (otot[:nq - 1] == ans.totals[1:]).all()
    ix.close()


def test_filters(ga, oracle):
    """shared and per-query bitmaps: all bits set equals no filter byte for byte, nothing allowed, allowed ids across word
    borders, and a filtered W past 4096 -- phase B under both filter forms"""
    from granne_amd.filters import Filter
    shape = rm.SHAPES[3]
    el, q, scan = rm.shape_input(oracle, shape)
    n, nq, cap = len(el), 10, 17
    q, scan = q[:nq], (scan[0][:nq], scan[1][:nq])
    rng = np.random.default_rng(5)
    ix = ga.Granne("angular", el, [])
    border = np.zeros(n, bool)
    border[[0, 31, 32, 33, 63, 64, 4095, 4096, n - 33, n - 1]] = True
    masks = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "half": rng.random(n) < 0.5, "border": border, "few": rng.random(n) < 0.01}
    radii = rm.mixed_radii(scan, cap)
    plain = ix.exact_range(q, radii, cap, stats=True)
    for name, mask in masks.items():
        for r in (radii, np.float32(2.0)):
            ans = rm.exact_range(scan, r, cap, mask)
            got = ix.exact_range(q, r, cap, allowed=mask, stats=True)
            same(got, ans, name)
            assert got[4][3] == mask.sum() and got[4][1] == int((ans.totals > rm.ET_CAP).sum()), name
            if name == "half":
                assert (ans.totals > rm.ET_CAP).any() or r is radii  # 2.0: about 10,000 allowed rows within: phase B, list form
            if name == "all" and r is radii:
                for a, b in zip(got[:4], plain[:4]):
                    assert a.tobytes() == b.tobytes()
            if name == "none":
                assert (got[3] == 0).all() and (got[2] == 0).all()
    # one bitmap per query: query a under masks[a % 5]; 2.0 under "all" and "half" passes 4096: phase B, bits form
    names = list(masks)
    per = np.stack([masks[names[a % 5]] for a in range(nq)])
    filters = [Filter.from_mask(per[a]) for a in range(nq)]
    for r in (radii, np.float32(2.0)):
        ans = rm.exact_range(scan, r, cap, per)
        got = ix.exact_range(q, r, cap, allowed=filters, stats=True)
        same(got, ans, "per query")
        assert got[4][1] == int((ans.totals > rm.ET_CAP).sum()) and got[4][3] == 0
    assert int((rm.exact_range(scan, 2.0, cap, per).totals > rm.ET_CAP).sum()) >= 4
    all_set = [Filter.from_mask(masks["all"]) for _ in range(nq)]
    got = ix.exact_range(q, radii, cap, allowed=all_set, stats=True)
    for a, b in zip(got[:4], plain[:4]):
        assert a.tobytes() == b.tobytes()
    ix.close()


def test_the_device_entry_on_a_stream_equals_the_host_entry(ga, oracle):
    import torch
    from granne_amd import _lib
    shape = rm.SHAPES[8]
    el, q, scan = rm.shape_input(oracle, shape)
    nq, cap = len(q), 17
    radii = rm.mixed_radii(scan, cap)
    ix = ga.Granne(_et(el), el, [])
    oid, ods = np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32)
    ocnt, otot, ost = np.zeros(nq, np.uint32), np.zeros(nq, np.uint32), np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert _lib.lib().granne_hip_exact_range(ix._h, p(q), nq, p(radii), cap, None, 0, p(oid), p(ods), p(ocnt), p(otot), p(ost)) == _lib.OK
    same((oid, ods, ocnt, otot), rm.exact_range(scan, radii, cap))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        tq, tr = torch.from_numpy(q.view(np.uint8)).to(dev), torch.from_numpy(radii).to(dev)
        ids = torch.empty((nq, cap), dtype=torch.int64, device=dev)
        ds = torch.empty((nq, cap), dtype=torch.float32, device=dev)
        cnt, tot = torch.empty(nq, dtype=torch.int32, device=dev), torch.empty(nq, dtype=torch.int32, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        ix.exact_range_device(tq.data_ptr(), nq, tr.data_ptr(), cap, 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), tot.data_ptr(),
                              st.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert (ids.cpu().numpy().view(np.uint64) == oid).all() and ds.cpu().numpy().tobytes() == ods.tobytes()
    assert (cnt.cpu().numpy().view(np.uint32) == ocnt).all() and (tot.cpu().numpy().view(np.uint32) == otot).all()
    assert (st.cpu().numpy().view(np.uint32) == ost).all()
    ix.close()


def test_refusals_and_degenerate_calls(ga, oracle):
    from granne_amd import _lib
    from tests.test_gpu_sum_embeddings import make_lists, make_table
    L = _lib.lib()
    rng = np.random.default_rng(27)
    el, q = m.unit_rows(oracle, rng, 300, 32), m.unit_rows(oracle, rng, 4, 32)
    radii = np.full(4, 0.9, np.float32)
    out = np.zeros(8192, np.uint64)
    p, r, o = q.ctypes.data_as(C.c_void_p), radii.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)

    def refused(h, word, cap=5, nq=4, rr=r, host_only=False):
        calls = [L.granne_hip_exact_range(h, p, nq, rr, cap, None, 0, o, o, o, o, None)]
        if not host_only:
            calls.append(L.granne_hip_exact_range_device(h, p, nq, rr, cap, None, 0, o, o, o, o, None, None))
        for rc in calls:
            assert rc == _lib.ERR_INVALID
            assert word in L.granne_hip_last_error().decode(), L.granne_hip_last_error()

    f16 = ga.Granne("angular_f16", el.astype(np.float16), [])
    refused(f16._h, "F16")
    refused(f16._h, "F16", nq=0)  # the handle is refused before anything else is looked at
    with pytest.raises(ga.GranneHipError, match="F16"):
        f16.exact_range(q, 0.9, 5)
    f16.close()
    tab, lists = make_table(rng, 100, 32), make_lists(rng, 300, 100)
    se = ga.SumEmbeddings(tab, lists)
    layer = np.tile(np.arange(1, 9, dtype=np.uint32), (300, 1))
    cix = ga.Granne("embeddings", se, [layer], compact=True)
    refused(cix._h, "needs dense rows")
    cix.close()
    ix = ga.Granne("angular", el, [])
    refused(ix._h, "cap (0) must be in [1, 1024]", cap=0)
    refused(ix._h, "cap (1025) must be in [1, 1024]", cap=1025)
    refused(ix._h, "null buffer", rr=None)
    refused(None, "index is null")
    nan = np.array([0.5, 0.5, np.nan, np.nan], np.float32)
    refused(ix._h, "the radius of query 2 is NaN", rr=nan.ctypes.data_as(C.c_void_p), host_only=True)
    with pytest.raises(ga.GranneHipError, match="query 2 is NaN"):
        ix.exact_range(q, nan, 5)
    with pytest.raises(ValueError):
        ix.exact_range(q[:, :31], 0.9, 5)
    with pytest.raises(ValueError):
        ix.exact_range(q, radii[:3], 5)
    out[:] = 7
    assert L.granne_hip_exact_range(ix._h, p, 0, r, 5, None, 0, o, o, o, o, None) == _lib.OK  # nq = 0: nothing happens
    assert L.granne_hip_exact_range_device(ix._h, None, 0, None, 5, None, 0, None, None, None, None, None, None) == _lib.OK
    assert (out == 7).all()
    # the device entry cannot see a NaN radius: the compare is false, the answer empty
    import torch
    dev = torch.device("cuda", 0)
    tq, tr = torch.from_numpy(q).to(dev), torch.from_numpy(nan).to(dev)
    ids, ds = torch.empty((4, 5), dtype=torch.int64, device=dev), torch.empty((4, 5), dtype=torch.float32, device=dev)
    cnt, tot = torch.empty(4, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ix.exact_range_device(tq.data_ptr(), 4, tr.data_ptr(), 5, 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), tot.data_ptr())
    torch.cuda.synchronize(dev)
    assert tot.cpu().tolist()[2:] == [0, 0] and cnt.cpu().tolist()[2:] == [0, 0] and (ids.cpu().numpy()[2:] == -1).all()
    # the device answers afterwards
    scan = rm.full_scan(oracle, el, q)
    same(ix.exact_range(q, radii, 5), rm.exact_range(scan, radii, 5))
    ix.close()
