"""What has no form for "angular_f16" rows says so -- GRANNE_HIP_ERR_INVALID with a message that names F16 -- and leaves
the device usable: the exact scan, reorder, the live builder, the sharded build and a partitioned handle over F16 indexes, and halves as a SumEmbeddings table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


@pytest.fixture(scope="module")
def world(ga, oracle):
    rng = np.random.default_rng(5)
    rows = oracle.normalize_f32(random_floats(rng, 800, 32))
    rows16 = rows.astype(np.float16)
    R = oracle.normalize_f32(rows16.astype(np.float32))
    oix = oracle.build_index(R, num_neighbors=10, max_search=20, reinsert_elements=False, n_threads=0)
    q = oracle.normalize_f32(random_floats(rng, 8, 32))
    return dict(rows=rows, rows16=rows16, R=R, oix=oix, q=q, gix=ga.Granne("angular_f16", rows16, oix.layers))


def refused(ga, call):
    from granne_amd import _lib
    with pytest.raises(ga.GranneHipError) as e:
        call()
    assert e.value.code == _lib.ERR_INVALID
    assert "F16" in str(e.value), str(e.value)


def test_brute_force(ga, world):
    refused(ga, lambda: world["gix"].brute_force(world["q"], 10))


def test_reorder(ga, world):
    refused(ga, lambda: world["gix"].reorder())
    refused(ga, lambda: world["gix"].reorder_by_keys(np.arange(800, dtype=np.uint64)))


def test_rw_builder(ga, world):
    b = ga.GranneBuilder("angular_f16", world["rows16"][:200], num_neighbors=10, max_search=20)
    refused(ga, lambda: ga.RwGranneBuilder(b, 400))
    b.close()


def test_sharded_build(ga, world):
    from granne_amd.sharded import ShardedHost
    refused(ga, lambda: ShardedHost.build("angular_f16", world["rows16"], 2, devices=(0,), num_neighbors=10, max_search=20))


def test_sharded_create_over_f16_indexes(ga, world):
    from granne_amd.sharded import ShardedHost
    refused(ga, lambda: ShardedHost([world["gix"]], [0]))


def test_sum_embeddings_table(ga, world):
    refused(ga, lambda: ga.SumEmbeddings(world["rows16"][:50], [[0, 1], [2]]))
    refused(ga, lambda: ga.SumEmbeddings.from_bytes(world["rows16"][:50], b""))


def test_the_device_still_answers_afterwards(ga, oracle, world):
    for call in (lambda: world["gix"].brute_force(world["q"], 10), lambda: world["gix"].reorder()):
        with pytest.raises(ga.GranneHipError):
            call()
    oix32 = oracle.build_index(world["rows"], num_neighbors=10, max_search=20, reinsert_elements=False, n_threads=0)
    g32 = ga.Granne("angular", world["rows"], oix32.layers)
    ids, ds, cnt = g32.search_batch(world["q"], 30, 10)
    oi, od, oc, _ = oix32.search_batch(world["q"], 30, 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
    # and so does the F16 index itself
    ids, ds, cnt = world["gix"].search_batch(world["q"], 30, 10)
    oi, od, oc, _ = oracle.Index(world["R"], world["oix"].layers).search_batch(world["q"], 30, 10)
    assert (ids == oi).all() and ds.tobytes() == od.tobytes() and (cnt == oc).all()
