"""tests/exact_topk_model.py on the host: the bins are monotone over all of [0, +inf] (random values, every float next
to a bin edge, 0, denormals, 2.0, beyond 2, +inf), the kernels' one-word key is the two bins side by side, the two-level
rule gives oracle.scan_topk's answer on the tie, second-level and off-sphere inputs of tests/test_gpu_exact_topk.py, and
the overflow rule fires exactly where include/granne_hip.h says."""
import numpy as np
import pytest

from tests import exact_topk_model as m
from tests import value_edges as ve


def _next(x, up=True):
    x = np.ascontiguousarray(x, np.float32)
    return np.nextafter(x, np.float32(np.inf if up else -np.inf)).astype(np.float32)


def _assert_monotone(d):
    d = np.unique(np.ascontiguousarray(d, np.float32))  # ascending
    assert (d >= 0).all()
    b1 = m.bin1(d)
    assert (np.diff(b1) >= 0).all() and b1.min() >= 0 and b1.max() < m.BINS1
    b2 = m.bin2(d, b1)
    assert b2.min() >= 0 and b2.max() < m.BINS2
    same = np.diff(b1) == 0
    assert (np.diff(b2)[same] >= 0).all()
    k = m.key(d)
    assert (np.diff(k) >= 0).all()
    assert (k >> 11 == b1).all() and (k & 2047 == b2).all()
    return b1, b2


def test_bins_are_monotone_on_random_distances():
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 0x7F800001, 2_000_000).astype(np.uint32)  # every non-negative float up to +inf
    _assert_monotone(bits.view(np.float32))
    _assert_monotone(rng.random(1_000_000, dtype=np.float32) * np.float32(2.5))
    _assert_monotone(np.float32(1.0) + (rng.random(1_000_000, dtype=np.float32) - np.float32(0.5)) * np.float32(1e-3))


def test_bins_at_every_first_level_edge():
    lin = (np.arange(0, 2049) / 1024.0).astype(np.float32)  # exact
    log = (np.arange(1024, 2041, dtype=np.uint32) << np.uint32(20)).view(np.float32)  # 2.0 .. +inf
    edges = np.concatenate([lin, log])
    assert np.isinf(edges[-1]) and edges[2048] == 2.0
    d = np.concatenate([edges, _next(edges[:-1]), _next(edges[1:], up=False)])
    _assert_monotone(d)
    assert (m.bin1(lin[:-1]) == np.arange(2048)).all() and (m.bin1(_next(lin[1:], up=False)) == np.arange(2048)).all()
    assert (m.bin1(log) == 2048 + np.arange(len(log))).all()
    assert (m.bin1(_next(log[1:], up=False)) == 2048 + np.arange(len(log) - 1)).all()
    assert m.bin1(np.float32(np.inf)) == 3064 < m.BINS1


@pytest.mark.parametrize("B1", [0, 1, 255, 256, 1023, 1024, 2046, 2047])
def test_second_level_edges_below_two(B1):
    edges = ((B1 + np.arange(0, 2049) / 2048.0) / 1024.0).astype(np.float32)
    assert ((edges.astype(np.float64) * 1024 - B1) * 2048 == np.arange(2049)).all()  # exact in float32
    d = np.concatenate([edges, _next(edges[:-1]), _next(edges[1:], up=False)])
    d = d[d >= 0]
    _assert_monotone(d)
    inside = edges[:-1]
    assert (m.bin1(inside) == B1).all() and (m.bin2(inside, B1) == np.arange(2048)).all()
    below = _next(edges[1:], up=False)
    ok = below >= inside  # (bin 0 of B1 = 0 starts at 0.0 and holds the denormals)
    assert (m.bin2(below[ok], B1) == np.arange(2048)[ok]).all()


@pytest.mark.parametrize("B1", [2048, 2049, 2100, 3000, 3063])
def test_second_level_edges_from_two_on(B1):
    base = np.uint32((B1 - 2048 + 1024) << 20)
    edges = (base + (np.arange(0, 2048, dtype=np.uint32) << np.uint32(9))).view(np.float32)
    d = np.concatenate([edges, _next(edges), _next(edges[1:], up=False)])
    _assert_monotone(d)
    assert (m.bin1(edges) == B1).all() and (m.bin2(edges, B1) == np.arange(2048)).all()
    assert (m.bin2(_next(edges[1:], up=False), B1) == np.arange(2047)).all()


def test_bins_of_the_special_values():
    tiny = np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, 1.17549435e-38], np.float32)  # 0, denormals, the first normal
    assert (m.bin1(tiny) == 0).all() and (m.bin2(tiny, 0) == 0).all() and (m.key(tiny) == 0).all()
    d = np.array([1.9999999, 2.0, 2.0000002, 3.0, 4.0, 47.5, 1e10, 3.4028235e38, np.inf], np.float32)
    b1, _ = _assert_monotone(np.concatenate([tiny, d]))
    assert m.bin1(np.float32(2.0)) == 2048 and m.bin2(np.float32(2.0), 2048) == 0
    assert m.bin1(np.float32(1.9999999)) == 2047 and m.bin2(np.float32(1.9999999), 2047) == 2047
    assert m.bin1(np.float32(4.0)) == 2048 + 8  # eight bins per binade


def test_model_equals_the_oracle_on_ties(oracle):
    rng = np.random.default_rng(11)
    rows = m.tripled(m.unit_rows(oracle, rng, 700, 32))
    q = m.unit_rows(oracle, rng, 3, 32)
    q[2] = 0  # a zero query: every distance is exactly 1
    for k in (1, 17, 100, 1024):
        m.check_against_oracle(oracle, rows, q, k)
    _, ids, _ = oracle.Index(rows, []).scan_topk(q[2:], 100)
    assert (ids[0] == np.arange(100)).all()
    rows, q = m.copies_of_the_nearest(oracle, rng)
    out = m.check_against_oracle(oracle, rows, q, 100)
    assert out[0][:2] == (1, False) and 3000 <= out[0][2] <= 3010
    got, _, _, _ = m.select(m.all_dists(oracle, rows, q[0]), 100)
    assert (got == np.arange(500, 600)).all()
    el = np.trunc(rng.uniform(-1, 1, (900, 17)) * 127).astype(np.int8)
    el[100] = 0  # an int8 zero row: distance exactly 1
    qi = np.trunc(rng.uniform(-1, 1, (2, 17)) * 127).astype(np.int8)
    m.check_against_oracle(oracle, el, qi, 900)
    assert oracle.dist(el[100], qi[0]) == 1.0


def test_model_equals_the_oracle_on_the_second_level_input(oracle):
    rows, q = m.second_level_input(oracle)
    d = m.all_dists(oracle, rows, q[0])
    m.second_level_precondition(d)
    out = m.check_against_oracle(oracle, rows, q, 100)
    level, over, ranked = out[0]
    assert level == 2 and not over and 100 <= ranked <= 50 + 50 + 4
    assert m.select(d, 50)[1] == 1  # the nearer rows alone: the first level is enough


def test_model_equals_the_oracle_off_the_sphere(oracle):
    rng = np.random.default_rng(12)
    el, q = ve.off_sphere_f32(rng, 3000, 32), ve.off_sphere_f32(rng, 6, 32)
    d = np.array([m.all_dists(oracle, el, x) for x in q])
    assert (d > 2.0).any() and ((d == 0.0).sum(axis=1) > 100).any()
    for k in (16, 1024):
        m.check_against_oracle(oracle, el, q, k)
    for make in (ve.one_sided_i8, ve.far_side_i8):
        el, q = make(rng, 3000, 100, nq=4)
        m.check_against_oracle(oracle, el, q, 100)
    el = ve.odd_i8(rng, 3000, 100)
    m.check_against_oracle(oracle, el, ve.odd_i8(rng, 4, 100), 100)


def test_the_overflow_rule_fires_exactly_where_stated():
    far = np.linspace(0.5, 1.5, 3000).astype(np.float32)
    same = np.float32(0.3)

    def run(n_same, n_near, k):
        near = np.linspace(0.01, 0.2, n_near).astype(np.float32)
        return m.select(np.concatenate([np.full(n_same, same), near, far]), k)

    ids, level, over, ranked = run(m.CAP, 0, 10)  # CAP rows up to the first bin: the first level holds them
    assert (level, over, ranked) == (1, False, m.CAP) and (ids == np.arange(10)).all()
    ids, level, over, ranked = run(m.CAP + 1, 0, 10)  # one more, all in one second-level bin
    assert (level, over, ranked) == (2, True, 0) and len(ids) == 0
    ids, level, over, ranked = run(m.CAP - 50, 50, 60)  # 50 nearer rows + CAP - 50 copies: CAP candidates
    assert (level, over, ranked) == (1, False, m.CAP)
    ids, level, over, ranked = run(m.CAP - 49, 50, 60)  # CAP + 1: second level, the copies' bin still holds too many
    assert (level, over) == (2, True)
    ids, level, over, ranked = run(m.CAP - 49, 50, 50)  # k within the nearer rows: the copies are never reached
    assert (level, over, ranked) == (1, False, 50)
    # CAP + 1 rows inside one first-level bin but spread over its second-level bins: the second level decides, no overflow
    spread = (np.float32(0.25) + (np.arange(m.CAP + 1) + 0.5) / (m.CAP + 1) / 1024.0).astype(np.float32)
    assert (m.bin1(spread) == 256).all()
    ids, level, over, ranked = m.select(np.concatenate([spread, far]), 10)
    assert level == 2 and not over and 10 <= ranked <= 16 and (ids == np.arange(10)).all()
    # n < k: every row, in order
    ids, level, over, ranked = m.select(np.array([0.5, 0.25, 3.0, 0.25], np.float32), 1024)
    assert ids.tolist() == [1, 3, 0, 2] and not over
