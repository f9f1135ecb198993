"""The model of post-filtered search (tests/postfilter_model.py) and granne_amd.filters.postfilter_stages on the host: what
the model pins before any GPU compares itself with it. No GPU."""
import numpy as np
import pytest

from tests import exact_topk_filtered_model as efm
from tests import postfilter_model as pm


def test_all_ones_is_the_plain_search(oracle):
    """All bits set: every query ends at stage 0, and the answer is search_batch(E_0, k) bit for bit."""
    for name in ("f32-8", "i8-8"):
        w = pm.world(oracle, name)
        q = w["q"][:40]
        for E0, k in ((16, 10), (64, 64), (20, 1)):
            a = pm.postfiltered(oracle, w["oix"], q, np.ones(w["n"], bool), k, min(E0, 16), [E0, 4 * E0], pm.EXACT)
            oi, od, oc, _ = w["oix"].search_batch(q, E0, k)
            assert (a.ids == oi).all() and a.dists.tobytes() == od.tobytes() and (a.counts == oc).all()
            assert (a.stage == 0).all() and a.unfinished == 0 and a.per_stage == [40, 0]


def test_nothing_allowed(oracle):
    w = pm.world(oracle, "f32-8")
    q = w["q"][:10]
    for fallback in (pm.EXACT, pm.SHORT):
        a = pm.postfiltered(oracle, w["oix"], q, np.zeros(w["n"], bool), 10, 16, [16, 64], fallback)
        assert (a.counts == 0).all() and (a.ids == pm.NONE).all() and np.isinf(a.dists).all()
        assert a.unfinished == 10 and (a.stage == (pm.STAGE_EXACT if fallback == pm.EXACT else pm.STAGE_SHORT)).all()
    # ... unless a stage exhausts the graph: then that stage answers, with count 0
    a = pm.postfiltered(oracle, w["oix"], q, np.zeros(w["n"], bool), 10, 16, [16, 4096], pm.EXACT)
    assert (a.counts == 0).all() and (a.stage == 1).all() and a.unfinished == 0


def test_the_exhausted_rule(oracle):
    """A stage beyond len: the walk runs out of graph (len(L) < E), so the stage answers whatever it holds. One allowed id:
    count 1 at stage 1, not in the fallback -- and the id is the one the exact scan would give."""
    w = pm.world(oracle, "f32-8")
    q = w["q"][:10]
    one = efm.only(w["n"], [1234])
    a = pm.postfiltered(oracle, w["oix"], q, one, 10, 16, [16, 4096], pm.EXACT)
    assert (a.stage == 1).all() and (a.counts == 1).all() and (a.ids[:, 0] == 1234).all() and a.unfinished == 0
    oi, od, _ = efm.oracle_subset(oracle, w["R"], one, q, 10)
    assert (a.ids == oi).all() and a.dists.tobytes() == od.tobytes()
    # the same filter without such a stage goes to the fallback
    a = pm.postfiltered(oracle, w["oix"], q, one, 10, 16, [16, 256], pm.EXACT)
    assert (a.stage == pm.STAGE_EXACT).all() and a.unfinished == 10 and (a.ids == oi).all()
    a = pm.postfiltered(oracle, w["oix"], q, one, 10, 16, [16, 256], pm.SHORT)
    assert (a.stage == pm.STAGE_SHORT).all() and (a.counts <= 1).all()


@pytest.mark.parametrize("name", ["f32-8", "i8-8"])
def test_the_density_filter_holds_every_outcome(oracle, name):
    """The input condition the GPU test asserts again: one shared filter, nq = 300, stages [16, 64, 256]: every outcome --
    stage 0, 1, 2 and the fallback -- holds at least 4 queries. The answer is allowed, ascending, and count = min(k, |A|)."""
    w = pm.world(oracle, name)
    mask = pm.density_mask(np.random.default_rng(100), w["rows_f"])
    a = pm.postfiltered(oracle, w["oix"], w["q"], mask, 10, 16, [16, 64, 256], pm.EXACT)
    print(name, a.outcome_counts(3), a.per_stage)
    assert min(a.outcome_counts(3)) >= 4 and sum(a.outcome_counts(3)) == pm.NQ
    s = pm.postfiltered(oracle, w["oix"], w["q"], mask, 10, 16, [16, 64, 256], pm.SHORT)
    done = a.stage < 3
    assert (s.stage[done] == a.stage[done]).all() and (s.stage[~done] == pm.STAGE_SHORT).all() and s.unfinished == a.unfinished
    assert (s.ids[done] == a.ids[done]).all() and (s.counts[~done] <= a.counts[~done]).all()
    for qi in range(pm.NQ):
        c = int(a.counts[qi])
        assert mask[a.ids[qi, :c].astype(np.int64)].all() and (a.ids[qi, c:] == pm.NONE).all()
        key = list(zip(a.dists[qi, :c].tolist(), a.ids[qi, :c].tolist()))
        assert key == sorted(key)


def test_per_query_filters_hold_every_outcome(oracle):
    w = pm.world(oracle, "f32-8")
    masks = pm.per_query_masks(np.random.default_rng(101), w["n"], pm.NQ)
    a = pm.postfiltered(oracle, w["oix"], w["q"], masks, 10, 16, [16, 64, 256, 1024], pm.EXACT)
    print(a.outcome_counts(4))
    assert min(a.outcome_counts(4)) >= 4
    assert (a.counts[4::5] == 0).all() and (a.stage[4::5] == pm.STAGE_EXACT).all()  # nothing allowed
    assert (a.stage[0::5] == 0).all()  # everything allowed


def test_postfilter_stages_properties():
    from granne_amd.filters import PF_DEFAULT_MARGIN, postfilter_stages
    for m in (1, 10, 50, 64, 200, 9000):
        for sel in (None, 1.0, 0.5, 0.1, 0.01, 0.001, 1e-9, 0.0):
            for e_max in (64, 1000, 8192):
                for n_stages in (1, 2, 4, 8, 20):
                    for margin in (1.0, 1.25, 2.0):
                        st = postfilter_stages(m, sel, e_max, n_stages, margin)
                        assert 1 <= len(st) <= min(n_stages, 8)
                        assert all(isinstance(e, int) for e in st)
                        assert all(a < b for a, b in zip(st, st[1:]))
                        assert st[0] >= m and st[-1] <= max(e_max, m)
    assert postfilter_stages(50) == [50, 200, 800, 3200]
    assert postfilter_stages(50, e_max=1000) == [50, 200, 800, 1000]
    assert postfilter_stages(50, 0.1, margin=1.0) == [512, 1024, 2048, 4096]  # roundup64(500)
    assert postfilter_stages(50, 0.01, margin=1.0) == [5056, 8192]
    assert postfilter_stages(50, 1.0, margin=1.0) == [64, 128, 256, 512]
    assert postfilter_stages(200, 1.0, margin=0.5) == [200, 400, 800, 1600]  # roundup64(100) = 128: never below min_allowed
    assert postfilter_stages(50, 0.0) == [8192]
    assert postfilter_stages(50, 0.1) == postfilter_stages(50, 0.1, margin=PF_DEFAULT_MARGIN)
    for bad in (dict(min_allowed=0), dict(min_allowed=5, selectivity=1.5), dict(min_allowed=5, n_stages=0), dict(min_allowed=5, margin=0)):
        with pytest.raises(ValueError):
            postfilter_stages(**bad)
