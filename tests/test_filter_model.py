"""tests/filter_model.py -- the model the filtered GPU walk is compared with -- against the oracle and against a scan.
No GPU. The fixtures are the golden indexes (tests/golden/*.npz); a handful of queries each: the model is plain Python."""
import os

import numpy as np
import pytest

from tests import filter_model as fm

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["f32_d28", "f32_d100", "i8_d32"]
NQ = 4


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request, oracle):
    z = np.load(os.path.join(HERE, "golden", request.param + ".npz"))
    layers = [z["layer%d" % i] for i in range(int(z["n_layers"]))]
    el, q = z["elements"], z["queries"][:NQ]
    # every query's distance to every element, once, by the oracle's scalar function (the model's default computes the
    # same numbers pair by pair through oracle/pyref.py; test_default_distance_path ties the two)
    drow = np.array([[oracle.dist(el[i], qq) for i in range(len(el))] for qq in q], np.float32)
    return {"name": request.param, "layers": layers, "el": el, "q": q, "drow": drow, "oix": oracle.Index(el, layers)}


def _bits(d):
    return np.asarray(d, np.float32).view(np.uint32)


def test_all_allowed_is_the_oracles_search(fx):
    """Every bit set, max_expand = 0: ids, distance bits, count and the three counters of Granne::search."""
    n = len(fx["el"])
    for ms, k in ((1, 1), (10, 10), (50, 10), (70, 75)):
        for qi, q in enumerate(fx["q"]):
            want, ctr = fx["oix"].search(q, ms, k, counters=True)
            got = fm.search_filtered(fx["layers"], fx["el"], q, np.ones(n, bool), ms, k, dist_row=fx["drow"][qi])
            assert got.ids == [i for i, _ in want]
            assert got.dist_bits() == list(_bits([d for _, d in want]))
            assert got.count == len(want) and not got.cut
            assert (got.counters["n_dist"], got.counters["n_expand"], got.counters["n_adj"]) == tuple(int(c) for c in ctr)


def test_default_distance_path(fx):
    """Without dist_row the model computes distances through oracle/pyref.py: the same result (one query, small max_search)."""
    n = len(fx["el"])
    rng = np.random.default_rng(3)
    allowed = rng.random(n) < 0.5
    a = fm.search_filtered(fx["layers"], fx["el"], fx["q"][0], allowed, 5, 5)
    b = fm.search_filtered(fx["layers"], fx["el"], fx["q"][0], allowed, 5, 5, dist_row=fx["drow"][0])
    assert (a.ids, a.dist_bits(), a.counters, a.cut) == (b.ids, b.dist_bits(), b.counters, b.cut)


@pytest.mark.parametrize("sel", [0.5, 0.2, 0.05])
def test_results_are_allowed_and_ascending(fx, sel):
    n = len(fx["el"])
    allowed = np.random.default_rng(int(sel * 100)).random(n) < sel
    for qi, q in enumerate(fx["q"]):
        r = fm.search_filtered(fx["layers"], fx["el"], q, allowed, 20, 25, dist_row=fx["drow"][qi])
        assert all(allowed[i] for i in r.ids)
        keys = list(zip(r.dist_bits(), r.ids))
        assert keys == sorted(keys) and len(set(r.ids)) == len(r.ids)
        assert r.count <= 20
        assert [fx["drow"][qi][i] for i in r.ids] == r.dists


def test_max_search_beyond_n_is_the_scan_over_the_allowed_rows(fx):
    """max_search >= n on a connected graph: nothing is ever rejected, the walk visits every node, and `res` is the
    top-k over the allowed rows by (distance bits, id)."""
    n = len(fx["el"])
    allowed = np.random.default_rng(11).random(n) < 0.3
    for qi, q in enumerate(fx["q"][:2]):
        r = fm.search_filtered(fx["layers"], fx["el"], q, allowed, n + 5, 40, dist_row=fx["drow"][qi])
        assert r.counters["n_expand"] >= n  # (the bottom layer alone expands every node: the graph is connected)
        ids = np.nonzero(allowed)[0]
        order = np.lexsort((ids, _bits(fx["drow"][qi][ids])))[:40]
        assert r.ids == [int(i) for i in ids[order]]
        assert r.dist_bits() == [int(b) for b in _bits(fx["drow"][qi][ids[order]])]


def test_max_expand_returns_what_res_held(fx):
    """max_expand = m: the walk's first m pops are the uncapped walk's (the cap changes nothing before it strikes), so
    `res` after m pops is the allowed ones among them, best max_search by (dist, id)."""
    n = len(fx["el"])
    allowed = np.random.default_rng(5).random(n) < 0.5
    ms = 10
    for qi, q in enumerate(fx["q"]):
        full = fm.search_filtered(fx["layers"], fx["el"], q, allowed, ms, ms, dist_row=fx["drow"][qi])
        upper = fm.search_filtered(fx["layers"][:-1], fx["el"], q, np.ones(n, bool), 1, 1, dist_row=fx["drow"][qi]).counters["n_expand"]
        total = full.counters["n_expand"] - upper  # bottom-layer pops of the uncapped walk
        assert total > 3
        for m in (1, 3, total - 1, total, total + 1):
            r = fm.search_filtered(fx["layers"], fx["el"], q, allowed, ms, ms, max_expand=m, dist_row=fx["drow"][qi])
            assert r.counters["n_expand"] - upper == min(m, total)
            assert all(allowed[i] for i in r.ids)
            if m >= total:
                # the cap strikes only if the uncapped walk would have popped again
                assert (r.ids, r.dist_bits()) == (full.ids, full.dist_bits())
            else:
                assert r.cut
            if m == 1:
                ep = fm.bottom_entrypoint(fx["layers"], fx["el"], q, dist_row=fx["drow"][qi])
                assert r.ids == ([ep] if allowed[ep] else [])


def test_empty_filter(fx):
    n = len(fx["el"])
    r = fm.search_filtered(fx["layers"], fx["el"], fx["q"][0], np.zeros(n, bool), 10, 10, dist_row=fx["drow"][0])
    assert r.count == 0 and r.ids == [] and not r.cut
    ids, ds = r.padded(3)
    assert (ids == np.iinfo(np.uint64).max).all() and np.isinf(ds).all()


def test_pack_bits_layout():
    a = np.zeros(70, bool)
    a[[0, 31, 32, 69]] = True
    w = fm.pack_bits(a)
    assert w.tolist() == [1 | 1 << 31, 1, 1 << 5]
