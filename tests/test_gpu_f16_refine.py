"""Re-ranking by "angular_f16" rows on the GPU (refine_kernel<F16>) against tests/refine_model.py over
R = normalize_f32(widen(rows16)): ids, distance BYTES, counts and the dropped-candidate word; the fused int8 walk + f16
re-rank equals the walk followed by refine of its lists; a rows-only handle is enough."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import refine_model as model  # noqa: E402
from tests.conftest import random_floats  # noqa: E402

U64_MAX = model.U64_MAX


@pytest.fixture(scope="module")
def ga():
    import granne_amd
    return granne_amd


def assert_result(got, want):
    ids, ds, cnt = got[:3]
    eids, eds, ecnt = want[:3]
    bad = np.nonzero((ids != eids).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], ids[bad[:1]], eids[bad[:1]])
    assert ds.tobytes() == eds.tobytes()
    assert (cnt == ecnt).all()


def rows_for(oracle, rng, n, dim):
    rows16 = oracle.normalize_f32(random_floats(rng, n, dim)).astype(np.float16)
    return rows16, oracle.normalize_f32(rows16.astype(np.float32))


# (170 and 230: rows of five and seven full blocks, a last round of one and of three -- with 768's none and the held rows
# of 100, 97 and 8 every branch of the eight-lane routine, with two rows to a group)
@pytest.mark.parametrize("dim", [100, 97, 768, 8, 170, 230])
@pytest.mark.parametrize("m", [1, 50, 1024])
def test_refine_equals_the_model(ga, oracle, dim, m):
    rng = np.random.default_rng(dim * 1000 + m)
    n, nq = 400, 3 if m == 1024 else 6
    rows16, R = rows_for(oracle, rng, n, dim)
    rows16[17] = 0  # a zero row: distance 1 to everything
    R[17] = 0
    r = ga.Granne("angular_f16", rows16, [])  # rows only (n_layers == 0)
    q = oracle.normalize_f32(random_floats(rng, nq, dim))
    cand = rng.integers(0, n, (nq, m)).astype(np.uint64)
    cand[0, 0] = 17
    counts = None
    if m > 1:
        cand[0, 1] = cand[0, 0]            # an id named twice stays twice
        cand[1, m // 2] = n                # ids the rows do not hold are dropped ...
        cand[1, m - 1] = n + 12345
        cand[2, 0] = U64_MAX               # ... the padding of search results included
        cand[2, m // 3] = U64_MAX
        counts = np.full(nq, m, np.uint32)
        counts[nq - 1] = m // 2            # a list shorter than m
    for k in sorted({1, 10, m, m + 5}):    # k > m included
        got = r.refine(q, cand, counts, k, dropped=True)
        want = model.refine(oracle, R, q, cand, counts, k)
        assert_result(got, want)
        assert got[3] == want[3], (got[3], want[3])
    if m > 1:
        assert want[3] == 4


@pytest.fixture(scope="module")
def pair(ga, oracle):
    """2000 elements of 100 dims as int8 rows with an oracle graph (walked) and as halves without a graph (re-ranked)."""
    rng = np.random.default_rng(4242)
    rows = oracle.normalize_f32(random_floats(rng, 2000, 100))
    rows8 = oracle.quantize(rows)
    rows16 = rows.astype(np.float16)
    R = oracle.normalize_f32(rows16.astype(np.float32))
    oix8 = oracle.build_index(rows8, num_neighbors=16, max_search=20, n_threads=8)
    q = oracle.normalize_f32(random_floats(rng, 32, 100))
    return dict(R=R, oix8=oix8, q=q, q8=oracle.quantize(q), g8=ga.Granne("angular_int", rows8, oix8.layers),
                r16=ga.Granne("angular_f16", rows16, []))


@pytest.mark.parametrize("ms,m,k", [(50, 50, 10), (200, 200, 10), (20, 7, 10), (1, 1, 1)])
def test_fused_int8_walk_f16_rerank(ga, oracle, pair, ms, m, k):
    rg = ga.RefinedGranne(pair["g8"], pair["r16"])
    ids, ds, cnt, dropped = rg.search_batch((pair["q8"], pair["q"]), ms, k, refine_from=m, dropped=True)
    # the model: the oracle's int8 walk, its lists re-ranked by R
    want = model.search_refined(oracle, pair["oix8"], pair["R"], pair["q8"], pair["q"], ms, m, k)
    assert_result((ids, ds, cnt), want)
    assert dropped == 0
    # ... and the two steps apart on the GPU: the walk, then refine of its lists
    wi, _, wc = pair["g8"].search_batch(pair["q8"], ms, m)
    assert_result(pair["r16"].refine(pair["q"], wi, wc, k), (ids, ds, cnt))


def test_unprepared_queries_and_refine_and_dists_agree(ga, oracle, pair):
    rg = ga.RefinedGranne(pair["g8"], pair["r16"])
    raw = pair["q"][:8] * np.float32(2.5)
    got = rg.search_batch(raw, 50, 10, prepared=False)
    qn = oracle.normalize_f32(raw)
    want = model.search_refined(oracle, pair["oix8"], pair["R"], oracle.quantize(qn), qn, 50, 50, 10)
    assert_result(got, want)
    # the distances refine reports are those of dists, bit for bit
    d = pair["r16"].dists_many(qn, got[0].astype(np.uint32))
    assert d.tobytes() == got[1].tobytes()
