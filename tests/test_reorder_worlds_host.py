"""tests/reorder_worlds.py held, on the CPU oracle alone, to the conditions that make its inputs worth reordering on the
GPU (tests/test_gpu_reorder_forms.py): the tied rows tie across layers, the oracle's order on tied and zero rows is its
Python restatement's, a ring's trail walks outgrow a visited table of 256 slots (some, not all), and the hand-made rows
hold what their docstrings say."""
import numpy as np
import pytest

from oracle import pyref
from tests import reorder_worlds as rw
from tests.scan_forms import structured_rows


@pytest.mark.parametrize("name", ["duplicates_f32", "duplicates_i8", "clones_f32", "clones_i8"])
def test_tied_rows_have_copies_in_the_layer_above(oracle, name):
    """A row whose copy sits in the layer above ends its trail on a node at distance 0 (or at the clamp), and so does
    every other copy: their trails are equal and only idx orders them. Observed: 674 of 1,280 (duplicates), 1,918 of
    2,400 (clones)."""
    oix, _ = rw.tied(name)
    below, tied = rw.copies_above(oix)
    print("%s: %d of %d bottom-layer rows have a copy above" % (name, tied, below))
    assert 4 * tied >= below


@pytest.mark.parametrize("name", ["duplicates_i8", "zero7_f32", "duplicates_f32_400"])
def test_oracle_order_is_the_restatement_s_on_tied_and_zero_rows(oracle, name):
    """oracle.compute_order (C) against pyref.compute_order (src/index/reorder.rs:135-208 restated from the Rust source
    on its own) where trails tie: copies of a row, zero rows (every distance to them is 1.0). f32 100-d is kept to 400
    rows: the restatement's ordered f32 dot product is slow."""
    if name == "duplicates_f32_400":
        rng = np.random.default_rng(400)
        el = rw.prep(structured_rows("duplicates", rng, 400), False)
        oix = oracle.build_index(el, num_neighbors=20, max_search=20, layer_multiplier=rw.MULT)
    else:
        oix, _ = rw.tied(name)
    assert len(oix.layers) >= 3
    want = pyref.compute_order([l for l in oix.layers], oix.elements)
    assert oix.compute_order().tolist() == want
    order = np.array(want, np.uint64)
    ore = oix.reordered(order)
    restated = pyref.reorder_layers(oix.layers, want)
    for rows, sets in zip(ore.layers, restated):
        assert [pyref.get_neighbors(rows, i) for i in range(rows.shape[0])] == sets


@pytest.mark.parametrize("name", sorted(rw.RING))
def test_ring_walks_outgrow_256_slots_some_not_all(oracle, name):
    """Observed: 1,200 walks, n_dist 17 .. 516 (median 262), lo 606, hi 943; with +-20 links 41 .. 540 (286), 670, 997."""
    oix, _ = rw.ring(name)
    int8, dim, links, _w = rw.RING[name]
    assert [l.shape for l in oix.layers] == [(rw.RING_NODES, 2 * links), (rw.RING_ALL, 2 * links)]
    top = oix.layers[0]
    for i in (0, 1, 499, 999):
        assert sorted(top[i].tolist()) == sorted((i + s) % rw.RING_NODES for s in range(-links, links + 1) if s)
    walks, lo, hi, n_dist = rw.ring_bounds(oix)
    print("%s: %d walks, n_dist %d .. %d (median %d), lo %d, hi %d" % (name, walks, n_dist.min(), n_dist.max(), np.median(n_dist), lo, hi))
    assert walks == rw.RING_ALL - rw.RING_NODES
    assert 0 < lo <= hi < walks


def test_edge_rows_hold_what_they_say(oracle):
    oix, _ = rw.edge_rows()
    assert tuple(l.shape[1] for l in oix.layers) == rw.EDGE_WIDTHS and tuple(l.shape[0] for l in oix.layers) == rw.EDGE_LENS
    for rows in oix.layers:
        L, W = rows.shape
        used = rows != rw.UNUSED
        assert (rows[used] < L).all()
        assert not used[rw.EDGE_EMPTY].any()
        assert used[rw.EDGE_FULL].all() and len(set(rows[rw.EDGE_FULL].tolist())) == W
        twice = pyref.get_neighbors(rows, rw.EDGE_TWICE)
        assert len(twice) == W - 3 and sorted(np.unique(twice, return_counts=True)[1].tolist())[-2:] == [1, 2]
        thrice = pyref.get_neighbors(rows, rw.EDGE_THRICE)
        assert len(thrice) == W and np.unique(thrice, return_counts=True)[1].max() == 3
        after = rows[rw.EDGE_AFTER_UNUSED]
        assert pyref.get_neighbors(rows, rw.EDGE_AFTER_UNUSED) == after[:5].tolist() and used[rw.EDGE_AFTER_UNUSED, 6:].all()
        assert len(pyref.get_neighbors(rows, 0)) >= 8
    # the oracle's reordered layers are the restatement's: sets sorted, repeats kept, the ids after an UNUSED dropped
    order = oix.compute_order()
    ore = oix.reordered(order)
    for rows, sets in zip(ore.layers, pyref.reorder_layers(oix.layers, order.astype(np.int64).tolist())):
        assert [pyref.get_neighbors(rows, i) for i in range(rows.shape[0])] == sets
    assert any(len(s) != len(set(s)) for sets in pyref.reorder_layers(oix.layers, order.astype(np.int64).tolist()) for s in sets)


def test_wide_rows_and_built_cases_are_as_wide_as_they_say(oracle):
    oix, _ = rw.wide_rows()
    assert [l.shape for l in oix.layers] == [(12, 100), (600, 100)]
    assert int((oix.layers[1] != rw.UNUSED).sum(axis=1).max()) == 100
    for name, (int8, dim, n, nn, walker) in rw.BUILT.items():
        oix, q = rw.built(name)
        assert len(oix) == n and oix.elements.dtype == (np.int8 if int8 else np.float32) and len(oix.layers) >= 4
        assert all(l.shape[1] == nn for l in oix.layers)
        # 64 device ids or more, or int8 rows beyond 512 bytes: the general walker
        assert (walker == "general") == (nn > 32 or (int8 and dim > 512))


def test_key_orders_are_numpy_s(oracle):
    for single_top in (False, True):
        oix = rw.keys_world(single_top)
        assert (oix.layers[0].shape[0] == 1) == single_top
        for name, keys in rw.key_sets(len(oix)).items():
            want = rw.lexsort_order(oix, keys)
            assert oix.order_by_keys(keys).tolist() == want.tolist(), name
            if name == "all_equal":
                assert want.tolist() == list(range(len(oix)))
            if name == "descending":
                lo = 0
                for l in oix.layers:
                    assert want[lo:l.shape[0]].tolist() == list(range(l.shape[0] - 1, lo - 1, -1))
                    lo = l.shape[0]
    keys = rw.key_sets(4000)
    assert len(set((keys["above_bit_32"] & np.uint64(0xFFFFFFFF)).tolist())) == 1 and len(set((keys["above_bit_32"] >> np.uint64(32)).tolist())) > 1
    assert len(set((keys["below_bit_32"] >> np.uint64(32)).tolist())) == 1 and len(set((keys["below_bit_32"] & np.uint64(0xFFFFFFFF)).tolist())) > 1
    assert set(keys["extremes"].tolist()) == {0, 2 ** 64 - 1}
