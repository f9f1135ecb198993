"""tests/rw_remove_model.py on the CPU: what tests/test_gpu_rw_remove.py holds the GPU handle against is a sound
statement of "removed elements stay in the graph and are never returned" (tests/README_rw_remove.md)."""
import numpy as np
import pytest

from tests.conftest import random_floats
from tests.rw_model import RwModel
from tests.rw_remove_model import RwRemoveModel

CFG = {"num_neighbors": 10, "max_search": 20, "layer_multiplier": 5.0}


@pytest.fixture(scope="module")
def world(oracle):
    rng = np.random.default_rng(21)
    el = oracle.normalize_f32(random_floats(rng, 300, 8))
    q = oracle.normalize_f32(random_floats(rng, 12, 8))
    return el, q


def _filled(el, removes=()):
    """300 places filled in four calls; `removes`: (after call, ids) pairs applied in between."""
    m = RwRemoveModel.new([], np.zeros((0, 8), np.float32), CFG, 300)
    calls = [(0, 1), (1, 40), (40, 41), (41, 300)]
    for c, (lo, hi) in enumerate(calls):
        assert m.insert_batch(el[lo:hi]) == list(range(lo, hi))
        for after, ids in removes:
            if after == c:
                m.remove(ids)
    return m


def test_layers_do_not_depend_on_removes(world):
    el, _q = world
    plain = _filled(el)
    marked = _filled(el, [(0, [0]), (1, [3, 4, 39, 500]), (2, list(range(10, 30))), (3, [299])])
    assert marked.removed_count() == 1 + 3 + 20 + 1
    a, b = plain.layers(), marked.layers()
    assert len(a) == len(b) >= 3
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all()


def test_nothing_removed_is_the_plain_search(world):
    el, q = world
    m = _filled(el)
    plain = RwModel.new([], np.zeros((0, 8), np.float32), CFG, 300)
    plain.insert_batch(el[:1]), plain.insert_batch(el[1:40]), plain.insert_batch(el[40:41]), plain.insert_batch(el[41:300])
    for x in q:
        want = plain.search(x, 20, 10)
        assert m.search(x, 20, 10) == want
        got, st = m.search(x, 20, 10, stats=True)  # the filtered walk under all ones: the same pairs
        assert [i for i, _ in got] == [i for i, _ in want]
        assert [np.float32(d).view(np.uint32) for _, d in got] == [np.float32(d).view(np.uint32) for _, d in want]
        assert st[0] >= st[1] > 0


def test_removed_ids_never_appear_and_restore_brings_them_back(world):
    el, q = world
    m = _filled(el)
    before = [m.search(x, 20, 10) for x in q]
    nearest = sorted({r[0][0] for r in before})
    assert m.remove(nearest + nearest[:1] + [300, 2 ** 40]) == (len(nearest), 1, 2)
    assert m.remove(nearest) == (0, len(nearest), 0)
    for x, was in zip(q, before):
        got = m.search(x, 20, 10)
        assert not {i for i, _ in got} & set(nearest)
        assert len(got) == 10
        survivors = [p for p in was if p[0] not in nearest]
        assert got[: len(survivors)][0] == survivors[0]  # the former second (or first alive) leads
    assert m.restore(nearest + [301]) == (len(nearest), 0, 1)
    assert m.removed_count() == 0
    assert [m.search(x, 20, 10) for x in q] == before
    # everything removed: nothing to return; all but three: at most three
    m.remove(range(300))
    assert all(m.search(x, 20, 10) == [] for x in q)
    m.restore([7, 150, 299])
    for x in q:
        got = m.search(x, 20, 10)
        assert 0 < len(got) <= 3 and {i for i, _ in got} <= {7, 150, 299}


def test_search_without_a_previous_layer_is_empty(world):
    el, _q = world
    m = RwRemoveModel.new([], np.zeros((0, 8), np.float32), CFG, 300)
    m.insert_batch(el[:m.m.capacity()])  # the first layer, full: elements, but no previous layer yet
    assert m.remove([1]) == (1, 0, 0)
    assert len(m) > 1 and not m.m.prev and m.search(el[0], 20, 5) == [] and m.search(el[0], 20, 5, stats=True) == ([], (0, 0, 0))
