"""The compacted row stage of the sketched f32 walkers (walk_fast.h, FastWalker::compact_rows): the launches that use the
index's row sketch read and evaluate only the neighbors that survive the look-up of evaluated ids and the sketch,
several lanes to a row. The same index with GRANNE_HIP_OPT_SKETCH 0 runs the walker that keeps two lanes per neighbor
slot: ids, distance bits, counts and all three counters are the same, and the oracle's.

Every walk's first bottom expansions have no finite max_search-th distance yet, so up to 30 neighbors survive there
(three or four passes of 8 rows); max_search 1 has a finite one from the first expansion on."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402
from tests.test_gpu_sketch import _index  # noqa: E402

SEEDS = {"uniform": 11, "latent": 12, "mixture": 13, "duplicates": 14, "grid": 15}
KNOBS = ("GRANNE_HIP_SEEN_MIN", "GRANNE_HIP_SKETCH", "GRANNE_HIP_COMPACT_ROWS")


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def _knobs_set():
    return any(os.environ.get(k) is not None for k in KNOBS)


@pytest.mark.parametrize("kind", ["uniform", "latent", "mixture", "duplicates", "grid"])
def test_compacted_is_the_two_lane_walker(ga, oracle, kind):
    """n = 6000 x 100-d, 300 queries, every launch skips revisits (SEEN_MIN 0). max_search 1 .. 60 walk one slot of 64
    keys, 61 and 124 two, 252 four."""
    if _knobs_set():
        pytest.skip("an experiment knob overrides the options this test switches")
    from granne_amd import _lib
    el, q, oix, gix = _index(ga, oracle, kind, SEEDS[kind])
    gix.set_option(_lib.OPT_SEEN_MIN, 0)
    for ef in (1, 10, 50, 60, 61, 124, 252):
        gix.set_option(_lib.OPT_SKETCH, 0)
        r0 = gix.search_batch(q, ef, 10, stats=True)
        assert gix.get_option(_lib.OPT_LAST_COMPACT_ROWS) == 0
        gix.set_option(_lib.OPT_SKETCH, 1)
        r1 = gix.search_batch(q, ef, 10, stats=True)
        assert gix.get_option(_lib.OPT_LAST_COMPACT_ROWS) == 1, (kind, ef)
        for a, b in zip(r0, r1):
            assert a.tobytes() == b.tobytes(), (kind, ef)
        oi, od, oc, octr = oix.search_batch(q, ef, 10)
        ids, ds, cnt, st = r1
        assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes(), (kind, ef)
        assert (st[:, 1:] == octr[:, 1:]).all(), (kind, ef)
    gix.close()


def test_every_survivor_count(ga, oracle):
    """One hand-made layer of 128 nodes whose rows hold 0 .. 32 valid ids: node i's row names (i + 1) % 33 neighbors (not
    i % 33: every walk starts at node 0, whose row must not be empty), so rows of 0, 1, 8, 9, 16, 17, 31 and 32 ids are
    all there. max_search 64 keeps every new neighbor a survivor until the list holds 64 entries; with and without the
    neighbors' tails next to the ids (GRANNE_HIP_OPT_INLINE_TAILS)."""
    if _knobs_set():
        pytest.skip("an experiment knob overrides the options this test switches")
    from granne_amd import _lib
    rng = np.random.default_rng(41)
    n = 128
    el = oracle.normalize_f32(random_floats(rng, n, 100))
    q = oracle.normalize_f32(random_floats(rng, 96, 100))
    layer = np.full((n, 32), 0xFFFFFFFF, np.uint32)
    counts = set()
    for i in range(n):
        m = (i + 1) % 33
        counts.add(m)
        others = np.delete(np.arange(n, dtype=np.uint32), i)
        layer[i, :m] = rng.permutation(others)[:m]
    assert {0, 1, 8, 9, 16, 17, 31, 32} <= counts
    oix = oracle.Index(el, [layer])
    gix = ga.Granne("angular", el, [layer])
    gix.set_option(_lib.OPT_SEEN_MIN, 0)
    for tails in (1, 0):
        gix.set_option(_lib.OPT_INLINE_TAILS, tails)
        assert gix.get_option(_lib.OPT_INLINE_TAILS) == tails
        for ef in (64, 60):  # two slots of 64 keys, and one
            ids, ds, cnt, st = gix.search_batch(q, ef, 10, stats=True)
            assert gix.get_option(_lib.OPT_LAST_COMPACT_ROWS) == 1
            oi, od, oc, octr = oix.search_batch(q, ef, 10)
            assert (cnt == oc).all() and (ids == oi).all() and ds.tobytes() == od.tobytes(), (tails, ef)
            assert (st[:, 1:] == octr[:, 1:]).all(), (tails, ef)
            assert (octr[:, 1] >= ef).all()  # (every walk expands at least max_search of the 128 nodes)
    gix.close()
