"""The compacted row stage of the sketched f32 walkers (walk_fast.h, FastWalker::compact_rows): a numpy float32 model of
its schedule -- G = 8 or 4 lanes to a 100-d row, lane t feeding accumulators 32 t / G .. 32 (t + 1) / G - 1 chunk by
chunk with fused multiply-adds, the ordered sum handed up the group one lane per step (DPP row_shr:1 inside a row of 16
lanes, the group's first lane taking +0.0 whatever its lower neighbor holds), the tail and `1 - r` in the last lane --
gives the oracle's distance bits (src/math.rs:17-39, src/elements/angular.rs)."""
import numpy as np
import pytest

from tests.conftest import random_floats

DIM, NB = 100, 3


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def _fma32(a, b, c):
    """fmaf on float32 arrays, exactly: a * b is exact in double; the double sum with c is taken with its rounding error
    (TwoSum) and, where it is inexact, moved to the neighbor with an odd mantissa (rounding to odd) -- rounding that to
    float32 is the single rounding of the exact a * b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)  # the exact sum lies further from zero than s
    away = np.where(s == 0, True, away)
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(np.float32)


def model_dists(rows, q, G):
    """Distances of `rows` [m, 100] to q [100] by the G-lane schedule, 16 / G groups side by side in each DPP row."""
    m = len(rows)
    per = 32 // G  # accumulators per lane
    groups = 16 // G
    out = np.empty(m, np.float32)
    for r0 in range(0, m, groups):
        batch = rows[r0:r0 + groups]
        nb = len(batch)
        # lane l of the DPP row: group l // G, lane t = l % G (groups past the batch hold stale garbage)
        acc = np.full((16, per), np.float32(1e30), np.float32)
        for g in range(nb):
            for t in range(G):
                a = np.zeros(per, np.float32)
                for b in range(NB):
                    sl = slice(32 * b + per * t, 32 * b + per * (t + 1))
                    a = _fma32(batch[g][sl], q[sl], a)
                acc[g * G + t] = a
        s = np.zeros(16, np.float32)
        for step in range(G):
            if step:
                shifted = np.concatenate([np.zeros(1, np.float32), s[:-1]])  # row_shr:1, lane 0 of the row: 0
                s = np.where(np.arange(16) % G == 0, np.float32(0.0), shifted)  # a group's first lane: +0.0, forced
            for j in range(per):
                s = (s + acc[:, j]).astype(np.float32)
        for g in range(nb):
            r = s[g * G + G - 1:g * G + G]
            for i in range(32 * NB, DIM):
                r = _fma32(batch[g][i:i + 1], q[i:i + 1], r)
            d = np.float32(1.0) - r[0]
            out[r0 + g] = d if np.float32(0.0) <= d else np.float32(0.0)
    return out


def _rows(oracle):
    rng = np.random.default_rng(77)
    q = oracle.normalize_f32(random_floats(rng, DIM))
    rows = [oracle.normalize_f32(random_floats(rng, 40, DIM))]
    rows.append(random_floats(rng, 8, DIM) * np.float32(3.0))  # off the sphere: distances clamp at 0
    rows.append(np.zeros((2, DIM), np.float32))
    rows.append(np.full((2, DIM), -0.0, np.float32))
    sub = (random_floats(rng, 4, DIM) * np.float32(1e-38)).astype(np.float32)  # subnormal components
    assert (np.abs(sub[sub != 0]) < np.finfo(np.float32).tiny).any()
    rows.append(sub)
    # partial sums that cancel to zero: within an accumulator (chunk 1 undoes chunk 0), between the accumulators of one
    # lane, and between two lanes of a group -- the exact zeros take their sign from the order of the adds
    c = np.zeros((4, DIM), np.float32)
    c[0, 0], c[0, 32] = q[32], -q[0]    # accumulator 0: fma(-q0, q32, q32 q0) = the rounding error of the product alone
    c[1, 0], c[1, 1] = q[1], -q[0]      # acc[0] + acc[1] = q0 q1 - q1 q0 = 0
    c[2, 3], c[2, 4] = q[4], -q[3]      # 8 lanes: the last accumulator of lane 0 against the first of lane 1
    c[3, 7], c[3, 8] = q[8], -q[7]      # 4 lanes: ... of lane 0 against lane 1; 8 lanes: lane 1 against lane 2
    c[3, 96:] = -0.0
    rows.append(c)
    return q, np.concatenate(rows).astype(np.float32)


@pytest.mark.parametrize("G", [8, 4])
def test_schedule_gives_the_oracles_bits(oracle, G):
    q, rows = _rows(oracle)
    want = np.array([oracle.dist(r, q) for r in rows], np.float32)
    got = model_dists(rows, q, G)
    assert got.tobytes() == want.tobytes()
    assert (want == 0.0).any() and (want == 1.0).any()
    # the zero query, and a query of -0.0: every distance is 1.0 - (+0.0)
    for z in (np.zeros(DIM, np.float32), np.full(DIM, -0.0, np.float32)):
        want = np.array([oracle.dist(r, z) for r in rows], np.float32)
        assert model_dists(rows, z, G).tobytes() == want.tobytes()


def test_fma_model_rounds_once():
    """The double sum alone rounds twice: a case where that differs from fmaf."""
    a = np.array([1.0 + 2.0 ** -23], np.float32)
    b = np.array([1.0 + 2.0 ** -23], np.float32)  # a b = 1 + 2^-22 + 2^-46
    c = np.array([2.0 ** -24], np.float32)        # a b + c = 1 + 2^-22 + 2^-24 + 2^-46: just above a float32 midpoint
    assert _fma32(a, b, c)[0] == np.float32(1.0 + 2.0 ** -22 + 2.0 ** -23)
    b = np.array([1.0 - 2.0 ** -23], np.float32)  # a b = 1 - 2^-46
    c = np.array([2.0 ** 24 + 2.0], np.float32)   # a b + c = 2^24 + 3 - 2^-46: the double sum is the midpoint 2^24 + 3,
    assert _fma32(a, b, c)[0] == np.float32(2.0 ** 24 + 2.0)  # which alone would round to the even 2^24 + 4
    assert (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)[0] == np.float32(2.0 ** 24 + 4.0)
