"""The reference's own RwGranneBuilder properties (src/index/rw/mod.rs:226-366) on the CPU model of the batched Rw
schedule (tests/rw_model.py) that tests/test_gpu_rw_builder.py holds the GPU handle against."""
import numpy as np
import pytest

from tests.conftest import random_floats
from tests.rw_model import RwModel


def _config(nn=30, ms=50, mult=15.0):
    return {"num_neighbors": nn, "max_search": ms, "layer_multiplier": mult}


@pytest.mark.parametrize("multiplier", [10.0, 15.0, 25.0])
@pytest.mark.parametrize("max_elements", [13, 66, 199, 719])
def test_layer_counts(oracle, multiplier, max_elements):
    """rw/mod.rs:304-341: after max_elements single inserts the layers are as long as a builder's over the same
    elements."""
    rng = np.random.default_rng(max_elements)
    el = oracle.normalize_f32(random_floats(rng, max_elements, 2))
    rw = RwModel.new([], np.zeros((0, 2), np.float32), _config(mult=multiplier), max_elements)
    for i in range(max_elements):
        assert rw.insert(el[i]) == i
    b = oracle.Builder(el, num_neighbors=30, max_search=50, layer_multiplier=multiplier, reinsert_elements=False)
    b.build()
    lens = b.layer_lens()
    assert len(lens) == len(rw.prev) + 1
    assert [len(l) for l in rw.prev] == lens[:-1]
    assert rw.capacity() == lens[-1] and len(rw) == max_elements


@pytest.fixture(scope="module")
def filled(oracle):
    """rw/mod.rs:260-297: 1,500 places, 1,600 rows offered in the reference's five calls."""
    rng = np.random.default_rng(5)
    el = oracle.normalize_f32(random_floats(rng, 1600, 5))
    rw = RwModel.new([], np.zeros((0, 5), np.float32), _config(10, 20, 5.0), 1500)
    returned = [rw.insert_batch(el[:100]), rw.insert_batch(el[100:120]), rw.insert(el[120]),
                rw.insert_batch(el[121:1421]), rw.insert_batch(el[1421:])]
    return rw, el, returned


def test_insert_batch_ids(filled):
    rw, _el, returned = filled
    assert returned[0] == list(range(100))
    assert returned[1] == list(range(100, 120))
    assert returned[2] == 120
    assert returned[3] == list(range(121, 1421))
    assert returned[4] == list(range(1421, 1500))  # nothing past max_elements
    assert len(rw) == 1500
    assert rw.insert_batch(_el[:3]) == [] and rw.insert(_el[0]) is None
    lens = [len(l) for l in rw.layers()]
    assert lens == sorted(lens) and lens[-1] == 1500
    for layer in rw.layers():  # every link stays inside its layer, no row names itself
        used = layer != 0xFFFFFFFF
        assert (layer[used] < layer.shape[0]).all()
        assert not (layer == np.arange(layer.shape[0], dtype=np.uint32)[:, None]).any()


def test_most_elements_find_themselves(filled):
    """rw/mod.rs:299-301 asserts this for every element under the sequential schedule; under the batched one the model's
    own share is what the GPU test asks of the GPU handle -- here only that the graph is a sound one."""
    rw, el, _ = filled
    ids, _d, cnt, _ = rw.index().search_batch(el[:1500], 20, 1)
    assert (cnt == 1).all()
    assert (ids[:, 0] == np.arange(1500)).mean() >= 0.95


def test_search_without_a_previous_layer_is_empty(oracle):
    rng = np.random.default_rng(9)
    el = oracle.normalize_f32(random_floats(rng, 40, 4))
    rw = RwModel.new([], np.zeros((0, 4), np.float32), _config(10, 20, 5.0), 200)
    assert rw.search(el[0], 20, 5) == []  # an empty builder
    first_layer = rw.capacity()
    rw.insert_batch(el[:first_layer])
    assert len(rw) == first_layer and not rw.prev
    assert rw.search(el[0], 20, 5) == []  # elements, but no previous layer: index.search(..).first() is None
    rw.insert(el[first_layer])
    assert len(rw.prev) == 1
    assert rw.search(el[0], 20, 1)[0][0] == 0


def test_oracle_backed_model_equals_pyref_model(oracle):
    """fast=True (searches, select_neighbors and distances in the C oracle) and fast=False (pyref alone) give the same
    layers, ids and searches over a whole insert sequence that starts from a built index and crosses promotions."""
    rng = np.random.default_rng(11)
    el = oracle.normalize_f32(random_floats(rng, 150, 8))
    cfg = {"num_neighbors": 6, "max_search": 10, "layer_multiplier": 3.0, "batch_max": 16, "batch_div": 4}
    start = oracle.build_index(el[:20], num_neighbors=6, max_search=10, layer_multiplier=3.0, reinsert_elements=False,
                               expected_num_elements=120, batch_max=16, batch_div=4)
    models = [RwModel.new(start.layers, el[:20], cfg, 120, fast=f) for f in (True, False)]
    for m in models:
        got = [m.insert(el[20 + i]) for i in range(10)]
        got += m.insert_batch(el[30:55]) + m.insert_batch(el[55:150])
        assert got == list(range(20, 120))
    a, b = (m.layers() for m in models)
    assert len(a) == len(b) >= 3
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x == y).all()
    for q in el[120:130]:
        assert models[0].search(q, 10, 5) == models[1].search(q, 10, 5)
