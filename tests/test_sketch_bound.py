"""Row sketches (GRANNE_HIP_OPT_SKETCH, walk_fast.h FastWalker::sketch_rejects): a host model of the 128-byte row line
(util_kernels.h row_sketch_kernel, byte for byte), of the query's sketch (FastWalker::load_query_sketch) and of the lower
bound LB the walker rejects a neighbor by, in the device's f32 operations. The walker drops a neighbor when LB > theta, so
LB must never exceed the distance it would have computed: checked here against the oracle's f32 distance over millions of
random pairs and on adversarial ones."""
import numpy as np
import pytest

from oracle import oracle as orc

LINE, META = 128, 112
F32MAX = float(np.finfo(np.float32).max)


def _ceil_sqrt(S):
    """util_kernels.h sketch_ceil_sqrt: the smallest float f with f * f >= S (1 + 2^-40), +inf beyond the float range."""
    T = np.asarray(S, np.float64) * (1.0 + 2.0 ** -40)
    big = ~(T <= F32MAX * F32MAX)
    T = np.where(big, 0.0, T)
    f = np.sqrt(T).astype(np.float32)
    while True:
        up = f.astype(np.float64) ** 2 < T
        if not up.any():
            break
        f = np.where(up, (f.view(np.uint32) + 1).view(np.float32), f)
    while True:
        g = np.where(f > 0, (f.view(np.uint32) - np.uint32(1)).view(np.float32), f)
        down = (f > 0) & (g.astype(np.float64) ** 2 >= T)
        if not down.any():
            break
        f = np.where(down, g, f)
    return np.where(big, np.float32(np.inf), f).astype(np.float32)


def row_sketch(x):
    """The device table: uint8 [n][128] of f32 rows x [n][dim] (dim <= 112)."""
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    assert dim <= META
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        finite = np.isfinite(x).all(axis=1)
        m = np.where(finite, np.abs(np.where(np.isfinite(x), x, 0)).max(axis=1, initial=0), 0).astype(np.float32)
        s = np.where(finite, (m.astype(np.float64) / 127.0).astype(np.float32), np.float32(0)).astype(np.float32)
        s64 = s.astype(np.float64)
        se, sc, sx = np.zeros(n), np.zeros(n), np.zeros(n)
        out = np.zeros((n, LINE), np.uint8)
        for i in range(dim):
            xd = x[:, i].astype(np.float64)
            c = np.where(s > 0, np.clip(np.rint(np.where(s > 0, xd / np.where(s > 0, s64, 1.0), 0.0)), -127, 127), 0.0)
            pc = s64 * c
            e = xd - pc
            se = se + e * e
            sc = sc + pc * pc
            sx = sx + xd * xd
            out[:, i] = c.astype(np.int64).astype(np.int8).view(np.uint8)
    inf = np.float32(np.inf)
    meta = np.stack([s, np.where(finite, _ceil_sqrt(se), inf), np.where(finite, _ceil_sqrt(sc), inf),
                     np.where(finite, _ceil_sqrt(sx), inf)], axis=1).astype(np.float32)
    out[:, META:] = meta.view(np.uint8).reshape(n, 16)
    return out


def _f(v):
    return np.float32(v)


def _fma32(a, b, c):
    """fmaf of float32 arrays: a * b is exact in double and, for the operands here (|c| and |a b| within a few
    binades of each other, or c = 0), so is a * b + c -- one rounding to f32, as fmaf."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def query_sketch(q):
    """FastWalker::load_query_sketch: (codes int8 [128], s, R, N, finite). Sums taken in the host's order (the device's
    butterfly order differs; the bound holds for any order)."""
    q = np.ascontiguousarray(q, np.float32)
    dim = q.size
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = np.abs(q)
        fin = bool(np.isfinite(q).all())
        m = _f(a[np.isfinite(a)].max(initial=0)) if dim else _f(0)
        s = _f(m / _f(127))
        inv = _f(_f(127) / m) if m > 0 else _f(0)
        c = np.clip(np.rint((q * inv).astype(np.float32)), -127, 127).astype(np.float32)
        e = _fma32(np.full(dim, -s, np.float32), c, q)
        ee, nn = _f(0), _f(0)
        for i in range(dim):
            ee = _f(ee + _f(e[i] * e[i]))
            nn = _f(nn + _f(q[i] * q[i]))
        r = _f(_f(np.sqrt(ee) * _f(1 + 2.0 ** -8)) + _f(2.0 ** -58))
        nrm = _f(_f(np.sqrt(nn) * _f(1 + 2.0 ** -8)) + _f(2.0 ** -58))
    codes = np.zeros(LINE, np.int8)
    if fin:
        codes[:dim] = c.astype(np.int64).astype(np.int8)
    return codes, s, r, nrm, fin


def lower_bound(qs, sk):
    """FastWalker::sketch_rejects' LB (float32 [n]) and whether the pair may be rejected at all, for one query sketch qs
    against table lines sk [n][128]."""
    codes, sq, rq, nq, fin = qs
    cx = sk[:, :META].view(np.int8).astype(np.int64)
    ip = cx @ codes[:META].astype(np.int64)
    meta = np.ascontiguousarray(sk[:, META:]).view(np.float32)
    sx, rx, xx, nx = meta[:, 0], meta[:, 1], meta[:, 2], meta[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((sq * sx).astype(np.float32) * ip.astype(np.float32)).astype(np.float32)
        nqnx = (nq * nx).astype(np.float32)
        b = ((rq * xx).astype(np.float32) + (nq * rx).astype(np.float32)).astype(np.float32)
        b = (b + (nqnx * _f(2.0 ** -17)).astype(np.float32)).astype(np.float32)
        m = ((np.abs(t) * _f(2.0 ** -20)).astype(np.float32) + (b * _f(1.0001)).astype(np.float32)).astype(np.float32)
        m = (m + _f(2.0 ** -20)).astype(np.float32)
        U = (t + m).astype(np.float32)
        lb = (_f(1) - U).astype(np.float32)
    usable = fin & (nqnx < _f(2.0 ** 100))
    return lb, usable


def _check_pairs(qs_rows, xs, exact_all=False):
    """LB <= the oracle's f32 distance for every usable pair. Pairs whose LB is far below the float64 distance cannot
    fail (the f32 dot of these rows is within 1e-4 of the exact one); the rest go through the oracle."""
    sk = row_sketch(xs)
    x64 = xs.astype(np.float64)
    worst = -np.inf
    n_checked = 0
    for q in qs_rows:
        lb, usable = lower_bound(query_sketch(q), sk)
        with np.errstate(invalid="ignore", over="ignore"):
            d64 = 1.0 - x64 @ q.astype(np.float64)
        near = usable & ((lb.astype(np.float64) > d64 - 1e-4) | exact_all | ~np.isfinite(d64))
        for j in np.nonzero(near)[0]:
            d = orc.dist(q, xs[j])
            n_checked += 1
            assert not (lb[j] > d), (float(lb[j]), d, j)
        with np.errstate(invalid="ignore"):
            gap = lb.astype(np.float64) - d64
        if usable.any() and np.isfinite(gap[usable]).any():
            worst = max(worst, float(np.nanmax(gap[usable])))
    return worst, n_checked


@pytest.fixture(scope="module")
def built():
    orc.build()


def test_ceil_sqrt_is_the_smallest_upper_float():
    rng = np.random.default_rng(1)
    S = np.concatenate([rng.random(10000) * 4, rng.random(1000) * 1e-40, [0.0, 1.0, 4.0, 2.0 ** -300, 1e300, np.inf]])
    f = _ceil_sqrt(S).astype(np.float64)
    T = S * (1 + 2.0 ** -40)
    ok = np.isfinite(f)
    assert (f[ok] ** 2 >= T[ok]).all()
    g = np.nextafter(f[ok].astype(np.float32), np.float32(0)).astype(np.float64)
    assert ((g ** 2 < T[ok]) | (f[ok] == 0)).all()
    assert np.isinf(f[-2:]).all()


def test_row_sketch_layout():
    x = orc.normalize_f32(np.random.default_rng(2).random((50, 100), dtype=np.float32) - 0.5)
    sk = row_sketch(x)
    codes = sk[:, :100].view(np.int8).astype(np.float64)
    meta = np.ascontiguousarray(sk[:, META:]).view(np.float32).astype(np.float64)
    assert (sk[:, 100:META] == 0).all()
    assert (np.abs(codes).max(axis=1) == 127).all()
    s = meta[:, 0:1]
    e = np.linalg.norm(x - s * codes, axis=1)
    assert (meta[:, 1] >= e).all() and (meta[:, 1] <= e * (1 + 1e-6) + 1e-30).all()
    assert (meta[:, 2] >= np.linalg.norm(s * codes, axis=1)).all()
    assert (meta[:, 3] >= np.linalg.norm(x.astype(np.float64), axis=1)).all()
    assert meta[:, 1].mean() < 0.006  # a few thousandths of a unit row: the sketch is tight enough to reject by


def test_lower_bound_random_pairs(built):
    """Two million pairs of normalised uniform and latent rows, 100-d: LB never exceeds the walker's distance."""
    rng = np.random.default_rng(3)
    xs = orc.normalize_f32(rng.random((10000, 100), dtype=np.float32) - 0.5)
    qs = orc.normalize_f32(rng.random((100, 100), dtype=np.float32) - 0.5)
    worst, _ = _check_pairs(qs, xs)
    assert worst < 0
    # near neighbours (small distances, the ones walks compare against theta) and a low-rank set
    base = rng.standard_normal((8, 100)).astype(np.float32)
    lat = orc.normalize_f32((rng.standard_normal((10000, 8)).astype(np.float32) @ base)
                            + 0.05 * rng.standard_normal((10000, 100)).astype(np.float32))
    worst, _ = _check_pairs(lat[:100] + np.float32(1e-3) * rng.standard_normal((100, 100)).astype(np.float32), lat)
    assert worst < 0


def test_lower_bound_adversarial(built):
    rng = np.random.default_rng(4)
    x = orc.normalize_f32(rng.random((6, 100), dtype=np.float32) - 0.5)
    rows = [x[0], -x[0], x[1], np.zeros(100, np.float32), -np.zeros(100, np.float32)]
    one = np.zeros(100, np.float32); one[7] = 1.0
    rows += [one, -one]
    dom = np.full(100, 1e-4, np.float32); dom[3] = 1.0
    rows += [orc.normalize_f32(dom)]
    sub = np.full(100, 1e-40, np.float32); sub[::2] = -1e-41
    rows += [sub, np.float32(1e-30) * x[2], np.float32(1e15) * x[3]]
    bad = x[4].copy(); bad[5] = np.inf
    nan = x[5].copy(); nan[9] = np.nan
    rows += [bad, nan]
    ties = np.round(x[1] * 8) / 8
    rows += [ties.astype(np.float32), orc.normalize_f32(ties.astype(np.float32))]
    X = np.stack(rows).astype(np.float32)
    sk = row_sketch(X)
    meta = np.ascontiguousarray(sk[:, META:]).view(np.float32)
    assert np.isinf(meta[-4:-2, 1:]).all() and (meta[-4:-2, 0] == 0).all() and (sk[-4:-2, :META] == 0).all()
    assert (sk[3:5] == np.concatenate([np.zeros(META, np.uint8), np.zeros(16, np.uint8)])).all()
    worst, n = _check_pairs(X, X, exact_all=True)
    assert n > 0
    # a non-finite query disables the sketch for its walk
    assert not lower_bound(query_sketch(bad), sk)[1].any()
    # q == x: the bound is below the distance 0 (nothing at theta >= 0 is ever rejected)
    lb, ok = lower_bound(query_sketch(x[0]), row_sketch(x[:1]))
    assert ok[0] and lb[0] <= 0
