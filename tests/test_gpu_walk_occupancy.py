"""Where the short list's f32 query lives (walk_fast.h, fast_query_in_regs): the launches of many walks read it from LDS
and run four waves per SIMD, the launches of fewer keep it in registers. The arithmetic and its order are the same, so
the same queries searched as one launch of 4,096 (query in LDS) and as four launches of 1,024 (query in registers)
return the same ids, distance bits, counts, expansions and adjacency entries -- row sketches on and off -- and the
large launch returns the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import assert_counters, random_floats  # noqa: E402

NQ, PART = 4096, 1024
SEEDS = {"uniform": 41, "mixture": 42, "grid": 43}


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def _data(kind, rng, n, dim=100):
    if kind == "uniform":
        return random_floats(rng, n, dim)
    if kind == "mixture":
        centers = random_floats(rng, 64, dim)
        return (centers[rng.integers(0, 64, n)] + 0.05 * random_floats(rng, n, dim)).astype(np.float32)
    if kind == "grid":  # few distinct values per component: many equal distances
        return (rng.integers(-1, 2, (n, dim)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["uniform", "mixture", "grid"])
def test_one_launch_equals_four(ga, oracle, kind):
    from granne_amd import _lib
    rng = np.random.default_rng(SEEDS[kind])
    el = oracle.normalize_f32(_data(kind, rng, 6000))
    q = oracle.normalize_f32(_data(kind, rng, NQ))
    oix = oracle.build_index(el, num_neighbors=30, max_search=40, n_threads=8)
    gix = ga.Granne("angular", el, oix.layers)
    # the launch shapes this test is about: 4,096 walks skip revisits (query in LDS), 1,024 do not (query in registers)
    assert PART < gix.get_option(_lib.OPT_SEEN_MIN) <= NQ
    for ef in (1, 10, 50, 60):
        oi, od, oc, octr = oix.search_batch(q, ef, 10)
        for sketch in (1, 0):
            gix.set_option(_lib.OPT_SKETCH, sketch)
            one = gix.search_batch(q, ef, 10, stats=True)
            assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER
            parts = [gix.search_batch(q[i:i + PART], ef, 10, stats=True) for i in range(0, NQ, PART)]
            assert gix.get_option(_lib.OPT_LAST_WALKER) == _lib.WALKER_REGISTER
            four = [np.concatenate([p[j] for p in parts]) for j in range(4)]
            for name, a, b in zip(("ids", "dists", "counts"), one, four):
                assert a.tobytes() == b.tobytes(), (kind, ef, sketch, name)
            assert (one[3][:, 1:] == four[3][:, 1:]).all(), (kind, ef, sketch, "n_expand / n_adj")
            # the large launch against the oracle, as tests/test_gpu_parity.py compares
            ids, ds, cnt, st = one
            assert (cnt == oc).all(), (kind, ef, sketch)
            for i in range(NQ):
                c = int(cnt[i])
                assert ids[i, :c].tolist() == oi[i, :c].tolist(), (kind, ef, sketch, i)
                assert ds[i, :c].tobytes() == od[i, :c].tobytes(), (kind, ef, sketch, i)
                assert (ids[i, c:] == np.iinfo(np.uint64).max).all() and np.isinf(ds[i, c:]).all()
            assert_counters(st, octr, exact=False)
    gix.close()
