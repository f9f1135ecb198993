"""The models of range search (tests/range_model.py) checked on the host, and the preconditions the GPU tests
(tests/test_gpu_exact_range.py, tests/test_gpu_search_range.py) rely on, asserted on the CPU oracle alone. No GPU."""
import numpy as np
import pytest

from tests import exact_topk_model as m
from tests import range_model as rm


def test_exact_model_equals_a_scalar_scan(oracle):
    """the full-scan model against oracle.dist of every pair, compared and sorted here"""
    rng = np.random.default_rng(1)
    for int8 in (False, True):
        el, q = rm.rows_of(oracle, rng, 300, 17, int8), rm.rows_of(oracle, rng, 7, 17, int8)
        scan = rm.full_scan(oracle, el, q)
        mask = rng.random(300) < 0.4
        radii = np.array([-1.0, 0.0, 0.7, 0.9, 1.0, 2.0, np.inf], np.float32)
        for masks in (None, mask):
            ans = rm.exact_range(scan, radii, 17, masks)
            for a in range(7):
                d = m.all_dists(oracle, el, q[a])
                ok = d <= radii[a]
                if masks is not None:
                    ok &= mask
                w = np.nonzero(ok)[0]
                w = w[np.lexsort((w, d[w].view(np.uint32)))]
                assert ans.totals[a] == len(w)
                t = min(len(w), 17)
                assert ans.counts[a] == t and (ans.ids[a, :t] == w[:t]).all() and ans.dists[a, :t].tobytes() == d[w[:t]].tobytes()
                assert (ans.ids[a, t:] == rm.NONE).all() and np.isinf(ans.dists[a, t:]).all()


def test_radius_for_total_includes_the_row_and_nextafter_excludes_it():
    ds = np.array([0.1, 0.2, 0.2, 0.3, 0.5], np.float32)
    assert rm.radius_for_total(ds, 1) == ds[0] and rm.radius_for_total(ds, 2) is None and rm.radius_for_total(ds, 3) == ds[2]
    assert rm.radius_for_total(ds, 5) == ds[4] and rm.radius_for_total(ds, 6) is None
    r0 = rm.radius_for_total(ds, 0)
    assert (ds <= r0).sum() == 0 and (ds <= np.nextafter(r0, np.float32(1))).sum() == 1


@pytest.mark.parametrize("shape", [s for s in rm.SHAPES if s[2] == 20011 and s[3] == 65], ids=rm.shape_id)
def test_every_border_total_occurs(oracle, shape):
    """what tests/test_gpu_exact_range.py relies on: at n = 20011, nq = 65 the mixed radii produce totals of 0, 1, cap - 1,
    cap, cap + 1, 4096 and 4097, a row excluded by nextafter, and every row (+inf and 2.0)"""
    el, q, scan = rm.shape_input(oracle, shape)
    for cap in shape[4]:
        ans = rm.exact_range(scan, rm.mixed_radii(scan, cap), cap)
        have = set(ans.totals.tolist())
        assert set(rm.border_totals(cap)) <= have, (cap, sorted(have))
        assert len(el) in have and not ans.voided.any()
        assert (ans.totals[7::12] <= 5).all()  # the 6th nearest row is excluded by the radius one ulp below it


def test_the_tie_inputs_are_what_the_gpu_tests_assume(oracle):
    rng = np.random.default_rng(21)
    el = m.tripled(m.unit_rows(oracle, rng, 1200, 32))
    zero = np.zeros((1, 32), np.float32)
    ans = rm.exact_range(rm.full_scan(oracle, el, zero), 1.0, 1024)
    assert ans.totals[0] == 3600 and (ans.ids[0] == np.arange(1024)).all() and (ans.dists[0] == 1.0).all()
    # 6,050 rows within the radius, 6,000 of them inside one first-level bin: phase B through the second level
    el, q = m.second_level_input(oracle)
    d = m.all_dists(oracle, el, q[0])
    m.second_level_precondition(d)
    assert m.select(d, 100)[1:3] == (2, False)
    ans = rm.exact_range(rm.full_scan(oracle, el, q), d.max(), 100)
    assert ans.totals[0] == 6050 and ans.counts[0] == 100 and not ans.voided[0]
    # 5,000 identical rows: the selection overflows, the query is voided, the total stays exact
    el, q = m.duplicates_nearest(oracle, np.random.default_rng(24))
    scan = rm.full_scan(oracle, el, q)
    ans = rm.exact_range(scan, np.array([scan[1][0, 4999]] + [0.5] * 3, np.float32), 100)
    assert ans.voided.tolist() == [True, False, False, False] and ans.totals[0] == 5000 and ans.counts[0] == 0
    assert (ans.totals[1:] <= rm.ET_CAP).all()


STAGES = [16, 64, 256]


@pytest.mark.parametrize("name", ["f32-100", "i8-100", "f16-100"])
def test_every_stage_code_occurs(oracle, name):
    """what tests/test_gpu_search_range.py relies on: with stages [16, 64, 256] and the issue's radii every stage code and
    the fallback's occur, with both fallbacks"""
    w = rm.world(oracle, name)
    radii = rm.issue_radii(w)
    for fallback, code in ((rm.EXACT, rm.STAGE_EXACT), (rm.SHORT, rm.STAGE_SHORT)):
        ans = rm.search_range(oracle, w["oix"], w["q"], radii, 50, STAGES, fallback)
        assert set(ans.stage.tolist()) == {0, 1, 2, code}, sorted(set(ans.stage.tolist()))
        assert ans.unfinished == int((ans.stage == code).sum()) > 0
        assert (ans.counts == np.minimum(ans.found, 50)).all()
        assert (ans.found[4::6] == 0).all() and (ans.stage[4::6] == 0).all()  # a negative radius ends at stage 0, empty
        if fallback == rm.EXACT:
            assert (ans.found[5::6] == w["n"]).all()  # +inf: every row, by the scan
        inside = np.isfinite(ans.dists)
        assert (ans.dists[inside] <= np.repeat(radii[:, None], 50, axis=1)[inside]).all()


def test_a_graph_shorter_than_the_first_stage_ends_at_stage_0(oracle):
    w = rm.world(oracle, "tiny-f32")
    ans = rm.search_range(oracle, w["oix"], w["q"], np.inf, 50, STAGES, rm.EXACT)
    assert (ans.stage == 0).all() and ans.unfinished == 0 and (ans.found == w["n"]).all()


def test_exact_fallback_model_is_the_exact_model(oracle):
    w = rm.world(oracle, "f32-100")
    radii = rm.issue_radii(w)
    ans = rm.search_range(oracle, w["oix"], w["q"], radii, 50, STAGES, rm.EXACT)
    ex = rm.exact_range(w["scan"], radii, 50)
    fb = ans.stage == rm.STAGE_EXACT
    assert (ans.ids[fb] == ex.ids[fb]).all() and (ans.found[fb] == ex.totals[fb]).all()
    assert (ans.found <= ex.totals).all()  # a walk never finds more than there is
