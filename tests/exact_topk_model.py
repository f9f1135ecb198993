"""The selection of exact_topk (granne_amd/csrc/exact_topk.h) restated on the host (test infrastructure, a plain module
like tests/refine_model.py): the two binning levels as include/granne_hip.h states them, the kernels' 32-bit key, the
two-level rule with its overflow, and the seeded inputs the host and the GPU tests share.

Distances are non-negative float32 (+inf included). First level, 3072 bins: d < 2 -> uint32(d * 1024), d >= 2 ->
2048 + ((bits(d) >> 20) - 1024). Second level, 2048 bins inside first-level bin B1: below 2 ->
uint32((d * 1024 - B1) * 2048) clamped to 2047, from 2 on -> (bits(d) >> 9) & 2047. Every product is by a power of two
and the difference removes leading bits only: all of it is exact in float32."""
import numpy as np

KMAX = 1024
CAP = 4096
BINS1, BINS2 = 3072, 2048


def _f32(d):
    return np.ascontiguousarray(d, np.float32)


def bin1(d):
    d = _f32(d)
    bits = d.view(np.uint32).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        lin = np.floor(np.where(d < 2, d, 0) * np.float32(1024.0)).astype(np.int64)
    return np.where(d < 2, lin, 2048 + ((bits >> 20) - 1024))


def bin2(d, b1):
    d = _f32(d)
    bits = d.view(np.uint32).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        lin = (np.where(d < 2, d, 0) * np.float32(1024.0) - np.asarray(b1).astype(np.float32)).astype(np.float32) * np.float32(2048.0)
        lin = np.minimum(np.floor(lin).astype(np.int64), 2047)
    return np.where(d < 2, lin, (bits >> 9) & 2047)


def key(d):
    """et_key: one monotone word whose upper bits are bin1 and whose low 11 bits are bin2 inside it"""
    d = _f32(d)
    bits = d.view(np.uint32).astype(np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        lin = np.floor(np.where(d < 2, d, 0) * np.float32(2097152.0)).astype(np.int64)
    return np.where(d < 2, lin, (bits >> 9) + (1024 << 11))


def _first_reaching(hist, target):
    cum = np.cumsum(hist)
    b = int(np.searchsorted(cum, target, side="left"))
    return b, int(cum[b] - hist[b]), int(hist[b])


def select(dists, k):
    """The k nearest of one query's distances by the two-level rule: (ids ascending by (distance bits, id), the level that
    decided (1 or 2), overflow, the number of candidates ranked). An overflowed query has no ids and ranks nothing."""
    d = _f32(dists)
    n = len(d)
    t = min(k, n)
    bits = d.view(np.uint32).astype(np.int64)
    b1 = bin1(d)
    B1, below1, pop1 = _first_reaching(np.bincount(b1, minlength=BINS1), t)
    level = 1
    if below1 + pop1 <= CAP:
        cand = np.nonzero(b1 <= B1)[0]
    else:
        level = 2
        inside = b1 == B1
        b2 = np.full(n, -1, np.int64)
        b2[inside] = bin2(d[inside], B1)
        B2, below2, pop2 = _first_reaching(np.bincount(b2[inside], minlength=BINS2), t - below1)
        if below1 + below2 + pop2 > CAP:
            return np.zeros(0, np.uint64), 2, True, 0
        cand = np.nonzero((b1 < B1) | (inside & (b2 <= B2)))[0]
    order = np.lexsort((cand, bits[cand]))
    return cand[order][:t].astype(np.uint64), level, False, len(cand)


def all_dists(oracle, el, q):
    """oracle.dist of every row to one query"""
    return np.array([oracle.dist(r, q) for r in el], np.float32)


def check_against_oracle(oracle, el, queries, k):
    """select() on oracle.dist values against oracle.scan_topk: ids and, through them, the distance bytes. Returns the
    (level, overflow, n_ranked) of every query."""
    _, ids, ds = oracle.Index(el, []).scan_topk(queries, k)
    t = min(k, len(el))
    out = []
    for a, q in enumerate(queries):
        d = all_dists(oracle, el, q)
        got, level, over, ranked = select(d, k)
        assert not over
        assert (got == ids[a, :t]).all(), a
        assert d[got.astype(np.int64)].tobytes() == ds[a, :t].tobytes(), a
        assert (ids[a, t:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and np.isinf(ds[a, t:]).all()
        out.append((level, over, ranked))
    return out


# ---- the inputs the host and the GPU tests share ---------------------------------------------------------------
def unit_rows(oracle, rng, n, dim):
    return oracle.normalize_f32((rng.random((n, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32))


def tripled(rows):
    """every row present three times (ids i, i + n, i + 2 n): equal distances, ordered by id"""
    return np.ascontiguousarray(np.concatenate([rows, rows, rows]))


def copies_of_the_nearest(oracle, rng, n=4000, dim=32, first=500, count=3000):
    """(rows, queries): `count` copies of query 0's nearest row at ids first .. first + count - 1 (the original, wherever
    it was, is overwritten by a far row unless it lies inside the block); the other queries are ordinary"""
    rows = unit_rows(oracle, rng, n, dim)
    q = unit_rows(oracle, rng, 3, dim)
    d = all_dists(oracle, rows, q[0])
    best = int(np.argmin(d))
    near = rows[best].copy()
    rows[best] = -near
    rows[first:first + count] = near
    return rows, q


def second_level_input(oracle, dim=32, n_band=6000, n_near=50):
    """(rows, query e0): n_band rows at distances 0.25 + (i + 0.5) / n_band / 1024 -- all inside first-level bin 256, a few
    per second-level bin -- after n_near nearer rows"""
    def at(d):
        c = 1.0 - np.asarray(d, np.float64)
        x = np.zeros((len(c), dim), np.float64)
        x[:, 0], x[:, 1] = c, np.sqrt(1.0 - c * c)
        return oracle.normalize_f32(x.astype(np.float32))
    near = at(0.05 + 0.002 * np.arange(n_near))
    band = at(0.25 + (np.arange(n_band) + 0.5) / n_band / 1024.0)
    q = np.zeros((1, dim), np.float32)
    q[0, 0] = 1.0
    return np.ascontiguousarray(np.concatenate([near, band])), q


def second_level_precondition(d, n_band=6000, n_near=50):
    """what the second-level tests rely on, asserted on oracle.dist values of second_level_input"""
    d = _f32(d)
    band = d[n_near:]
    assert (bin1(d[:n_near]) < 256).all() and (bin1(band) == 256).all()
    assert len(np.unique(band)) == n_band
    assert np.bincount(bin2(band, 256), minlength=BINS2).max() <= 4


def duplicates_nearest(oracle, rng, n=7000, dim=32, first=1000, count=5000, nq=4):
    """(rows, queries): `count` identical rows at ids first .. first + count - 1, equal to query 0 (distance 0 or an ulp
    from it: nothing is nearer); queries 1 .. nq - 1 are the negatives of other rows' neighbourhoods: far from the copies"""
    rows = unit_rows(oracle, rng, n, dim)
    q = unit_rows(oracle, rng, nq, dim)
    rows[first:first + count] = q[0]
    q[1:] = oracle.normalize_f32(-q[0][None, :] + np.float32(0.3) * q[1:])
    return rows, np.ascontiguousarray(q)
