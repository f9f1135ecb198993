"""tests/exact_topk_filtered_model.py on the host: the selection over a subset gives what the oracle's scan of the allowed
rows gives -- oracle.Index(el[allowed], []).scan_topk, its ids mapped through the ascending allowed list -- on every shape
and shared filter of tests/test_gpu_exact_topk_filtered.py, and no chosen input overflows the selection (the GPU tests
never rest on an input the reference itself cannot rank); the stage rule under a count known only on the device; the
per-query form's priming rule, with the trap that defeats the naive one."""
import numpy as np
import pytest

from tests import exact_topk_filtered_model as fm
from tests import exact_topk_model as m


@pytest.mark.parametrize("case", fm.CASES, ids=[fm.case_id(c) for c in fm.CASES])
def test_model_equals_the_oracle_on_the_allowed_subset(oracle, case):
    int8, dim, n, nq, k = case
    el, q, filters = fm.case_input(oracle, case)
    q = q[:2]  # (every query's distances to every row, one oracle.dist at a time)
    d = [m.all_dists(oracle, el, x) for x in q]
    assert {"ones", "half", "percent", "one", "none", "last", "last_word"} <= set(filters)
    for name, mask in filters.items():
        oi, od, oc = fm.oracle_subset(oracle, el, mask, q, k)
        t = min(k, int(mask.sum()))
        assert (oc == t).all()
        for a in range(len(q)):
            got, level, over, ranked = fm.select(d[a], mask, k)
            assert not over, (name, a)
            assert (got == oi[a, :t]).all(), (name, a)
            assert d[a][got.astype(np.int64)].tobytes() == od[a, :t].tobytes(), (name, a)
            assert mask[got.astype(np.int64)].all()
            assert (oi[a, t:] == fm.NONE).all() and np.isinf(od[a, t:]).all()
            if name == "ones":
                assert (got == m.select(d[a], k)[0]).all()
            if name == "none":
                assert len(got) == 0 and ranked == 0


def test_shared_filters_hold_what_their_names_say():
    rng = np.random.default_rng(1)
    n, k = 4037, 17
    f = fm.shared_filters(rng, n, k)
    assert f["ones"].all() and not f["none"].any() and f["one"].sum() == 1
    assert np.nonzero(f["last"])[0].tolist() == [n - 1]
    lw = np.nonzero(f["last_word"])[0]
    assert lw[0] == 4032 and lw[-1] == n - 1 and n & 31  # only the last, partial word
    b = np.nonzero(f["block"])[0]
    assert (np.diff(b) == 1).all() and b[0] & 31 and (b[-1] + 1) & 31  # starts and ends mid-word
    assert 0.45 < f["half"].mean() < 0.55 and 0.004 < f["percent"].mean() < 0.02
    assert [int(f[x].sum()) for x in ("k-1", "k", "k+1")] == [16, 17, 18]
    # the words: bit (id & 31) of word (id >> 5); the bits past n set on request and nowhere else
    w, g = fm.words(f["half"]), fm.words(f["half"], garbage_past_n=True)
    assert (w[:-1] == g[:-1]).all() and g[-1] == w[-1] | np.uint32(0xFFFFFFE0) and w[-1] < 32
    assert fm.allowed_ids(f["last"]).dtype == np.uint64


def test_prefixes_and_the_stage_rule():
    assert fm.prefixes(7) == [7] and fm.prefixes(32768) == [32768]
    assert fm.prefixes(40009) == [16384, 40009]
    assert fm.prefixes(1_000_000) == [16384, 62500, 1_000_000]
    P = fm.prefixes(2**32 - 1)
    assert P[0] == 16384 and P[-1] == 2**32 - 1 and len(P) <= 16 and all(a < b for a, b in zip(P, P[1:]))
    assert all(p >= fm.PRIME_MIN > m.KMAX for p in P[:-1])  # a non-final prefix of the list holds k rows
    # n = 40009: (entries scanned, live, final) per stage
    assert fm.stages(40009, 0) == [(0, True, True), (0, False, False)]
    assert fm.stages(40009, 300) == [(300, True, True), (0, False, False)]
    assert fm.stages(40009, 16384) == [(16384, True, True), (0, False, False)]
    assert fm.stages(40009, 16385) == [(16384, True, False), (16385, True, True)]
    assert fm.stages(40009, 30000) == [(16384, True, False), (30000, True, True)]
    assert fm.stages(40009, 40009) == [(16384, True, False), (40009, True, True)]
    assert fm.stages(1_000_000, 10_000) == [(10_000, True, True), (0, False, False), (0, False, False)]
    assert fm.stages(1_000_000, 100_000) == [(16384, True, False), (62500, True, False), (100_000, True, True)]
    for n in (1, 7, 40009, 1_000_000, 2**32 - 1):
        for count in (0, 1, 16383, 16384, 16385, n // 2, n):
            st = fm.stages(n, min(count, n))
            assert sum(f for _, _, f in st) == 1 and st[0][1]  # exactly one final stage; stage 0 is always live
            last_live = max(i for i, s in enumerate(st) if s[1])
            assert st[last_live][2] and all(s[1] for s in st[:last_live])  # the live stages are a prefix, the last one final


def test_narrowing_rule():
    assert fm.narrow_target(5, 17, final=False) is None  # too few allowed rows yet: the bound stays
    assert fm.narrow_target(16, 17, final=False) is None
    assert fm.narrow_target(17, 17, final=False) == 17 and fm.narrow_target(9000, 17, final=False) == 17
    assert fm.narrow_target(5, 17, final=True) == 5 and fm.narrow_target(40, 17, final=True) == 17
    assert fm.narrow_target(0, 17, final=True) is None and fm.narrow_target(0, 17, final=False) is None
    assert fm.narrow_target(5, 17, final=False, naive=True) == 5


def test_the_priming_trap_defeats_the_naive_rule_only(oracle):
    rng = np.random.default_rng(31)
    k = 17
    rows, q, mask = fm.trap_input(oracle, rng, k=k)
    early = int(mask[:fm.PRIME_MIN].sum())
    assert 0 < early < k and mask.sum() == early + 200
    d = m.all_dists(oracle, rows, q)
    want, _, over, _ = fm.select(d, mask, k)
    assert not over and len(want) == k
    assert (want[:8] >= fm.PRIME_MIN).all()  # its nearest allowed rows lie after the first prefix
    assert set(np.nonzero(mask[:fm.PRIME_MIN])[0]) <= set(want.astype(np.int64))
    got, over = fm.staged_select(d, mask, k)
    assert not over and (got == want).all()
    oi, _, _ = fm.oracle_subset(oracle, rows, mask, q[None, :], k)
    assert (oi[0] == want).all()
    naive, _ = fm.staged_select(d, mask, k, naive=True)
    assert len(naive) < k  # a bound from the prefix's five rows cuts the answer short
    # an ordinary filter: both rules agree with the subset's selection, at every k
    mask = fm.random_mask(rng, len(rows), 0.3)
    for kk in (1, 100, 1024):
        want = fm.select(d, mask, kk)[0]
        assert (fm.staged_select(d, mask, kk)[0] == want).all()
    # empty, and fewer than k allowed in all
    assert len(fm.staged_select(d, np.zeros(len(rows), bool), k)[0]) == 0
    few = fm.only(len(rows), [3, 20000, 40008])
    assert (fm.staged_select(d, few, k)[0] == fm.select(d, few, k)[0]).all()


def test_tie_inputs_do_not_overflow(oracle):
    rng = np.random.default_rng(21)
    base = m.unit_rows(oracle, rng, 1200, 32)
    el = m.tripled(base)
    q = m.unit_rows(oracle, rng, 9, 32)
    q[8] = 0
    mask = np.arange(3600) >= 1200  # copies 2 and 3 only
    for a in (0, 8):
        d = m.all_dists(oracle, el, q[a])
        got, _, over, _ = fm.select(d, mask, 100)
        assert not over and (got >= 1200).all()
        if a == 0:
            assert (got[1::2] == got[0::2] + 1200).all()  # equal distances in id order
        else:
            assert (got == np.arange(1200, 1300)).all()  # a zero query: every distance exactly 1
    el, q = m.copies_of_the_nearest(oracle, np.random.default_rng(22))
    mask = np.ones(len(el), bool)
    mask[501:3500:2] = False  # every second copy
    got, _, over, _ = fm.select(m.all_dists(oracle, el, q[0]), mask, 100)
    assert not over and (got == np.arange(500, 700, 2)).all()
