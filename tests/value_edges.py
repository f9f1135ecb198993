"""Seeded generators of the values the rest of the suite never draws (test infrastructure, a plain module like
tests/refine_model.py): f32 rows off the unit sphere, int8 rows at the type's extremes and with norms that differ by
more than 40 x inside a 32-row block, one-sided int8 sets (every dot <= 0) and raw rows over every decade of the float
range. Every value is finite: no generator holds a NaN or an infinity.

The distance is max(0, 1 - x.q) whatever the norms (src/elements/angular.rs:63-74, angular_int.rs:47-60): rows whose dot
with the query exceeds 1 all sit at distance exactly 0.0 and are ordered by id alone.

scan_input(name) makes the inputs of the exact-scan tests: tests/test_value_edges_host.py caps their share of near-tied
ranks on the oracle alone, tests/test_gpu_value_edges.py scans exactly these."""
import numpy as np

from oracle import oracle as orc

LOW_AMPLITUDES = (3, 8, 20, 60)


def _uniform(rng, *shape):
    """src/test_helper.rs:3-6: uniform in [-0.5, 0.5)."""
    return (rng.random(shape, dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def unit_f32(rng, n, dim):
    return orc.normalize_f32(_uniform(rng, n, dim))


def off_sphere_f32(rng, n, dim, lo=-1.3, hi=1.3):
    """Unit rows, each times 10^U(lo, hi); about 3 % of the rows at scale 1e-25 (every product with them is below half
    an ulp of 1: distance exactly 1.0) and about 1 % at scale 1e-20 (their products with each other are sub-normal);
    rows n // 3 and n - 1 are zero (n >= 4). The largest dot is 10^(2 hi): nowhere near the float range."""
    rows = unit_f32(rng, n, dim)
    scale = np.power(10.0, rng.uniform(lo, hi, n))
    kind = rng.random(n)
    scale[kind < 0.03] = 1e-25
    scale[(kind >= 0.03) & (kind < 0.04)] = 1e-20
    rows = (rows * scale.astype(np.float32)[:, None]).astype(np.float32)
    if n >= 4:
        rows[n // 3] = 0
        rows[n - 1] = 0
    assert np.isfinite(rows).all()
    return rows


def odd_i8(rng, n, dim):
    """trunc(amplitude * U(-1, 1)) per component: amplitude 127 for most rows, one of LOW_AMPLITUDES for about one row in
    40 (norms 40 x apart inside many 32-row blocks); in every seventh row the
    components <= -100 become -128; the last three rows (n >= 4) are all zero, all -128 and all 127."""
    amp = np.full(n, 127.0)
    low = rng.random(n) < 1.0 / 40.0
    amp[low] = rng.choice(LOW_AMPLITUDES, int(low.sum()))
    rows = np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * amp[:, None]).astype(np.int8)
    seventh = rows[6::7]
    seventh[seventh <= -100] = -128
    if n >= 4:
        rows[n - 3] = 0
        rows[n - 2] = -128
        rows[n - 1] = 127
    return rows


def one_sided_i8(rng, n, dim, nq=64):
    """(elements [n, dim], queries [nq, dim]): every element component >= 0, every query component <= 0, amplitude 127,
    so every dot is <= 0 and every distance >= 1; element n // 2 is zero: distance exactly 1.0, the nearest of all."""
    el = np.trunc(rng.uniform(0.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
    el[:, 0] = np.maximum(el[:, 0], 1)  # no second zero row, whatever the dimension
    el[n // 2] = 0
    q = (-np.trunc(rng.uniform(0.0, 1.0, (nq, dim)) * 127.0)).astype(np.int8)
    q[:, 0] = np.minimum(q[:, 0], -1)
    return el, q


def far_side_i8(rng, n, dim, nq=64):
    """(elements, queries): 15 rows in 16 have every component <= 0 at amplitude 127, the others every component >= 0 at an
    amplitude from 3, 8, 20, 60, 127; the queries are >= 0 at amplitude 127. A query's nearest rows are the few positive
    ones, most of them of a small norm, many in a 16-row lane half whose other rows -- and whose 32-row block's other
    half -- score below zero: the exact scan's block bound (largest dot of the half times ITS largest 1 / |x|) is all
    that lets such a block through once the lists' thresholds are positive."""
    el = (-np.trunc(rng.uniform(0.0, 1.0, (n, dim)) * 127.0)).astype(np.int8)
    pos = np.nonzero(rng.random(n) < 1.0 / 16.0)[0]
    amp = rng.choice(LOW_AMPLITUDES + (127,), len(pos)).astype(np.float64)
    el[pos] = np.trunc(rng.uniform(0.0, 1.0, (len(pos), dim)) * amp[:, None]).astype(np.int8)
    el[pos, 0] = np.maximum(el[pos, 0], 1)  # no zero row among them
    q = np.trunc(rng.uniform(0.0, 1.0, (nq, dim)) * 127.0).astype(np.int8)
    q[:, 0] = np.maximum(q[:, 0], 1)
    return el, q


def scaled_raw(rng, dim, top=19):
    """One raw f32 row per decade 1e-44 .. 10^top, components uniform in [-1, 1) times the scale: squares that underflow
    (norm 0: normalize keeps the row), sub-normal components, squares that overflow (norm +inf: the row becomes +-0).
    top = 19 for normalize; up to 30 for quantize, where x * 127 stays finite."""
    exps = np.arange(-44, top + 1)
    rows = (rng.uniform(-1.0, 1.0, (len(exps), dim)) * np.power(10.0, exps)[:, None]).astype(np.float32)
    assert np.isfinite(rows).all()
    return rows


def sketch_adversarial_f32(rng, n, nq, dim=100):
    """(rows, queries) on which the row sketch's error is nearly the whole of its margin N_q R_x (walk_fast.h,
    sketch_rejects). Queries are a power of two times integer codes (no quantisation residual: R_q = 0) that share one
    sign pattern, norms 7.6 / 3.8 / 1.9 / 0.95 in turn. Rows are s (c + 0.45 sign), c integer codes, s a power of two that
    puts the norm in [1, 4) (every row is indexed): the residual x - s c is 0.45 s in every component and points along
    the queries' signs, so q.(x - s c) > 0.97 |q| R_x. A bound whose margin misses the factor N_q rejects true neighbours
    of the queries longer than 1."""
    sign = np.where(rng.random(dim) < 0.5, -1.0, 1.0)
    u = rng.integers(64, 128, (nq, dim)).astype(np.float64)
    u[:, 0] = 127
    q = (np.exp2(-7.0 - np.arange(nq) % 4)[:, None] * sign * u).astype(np.float32)
    x = rng.integers(-126, 127, (n, dim)).astype(np.float64) + 0.45 * sign
    x[:, 1] = 127.0 * np.where(rng.random(n) < 0.5, -1.0, 1.0)  # the row's largest component: its scale is s exactly
    target = np.power(10.0, rng.uniform(0.0, 0.3, n))
    s = np.exp2(np.ceil(np.log2(target / np.linalg.norm(x, axis=1))))
    return (x * s[:, None]).astype(np.float32), q


# ---- the exact scan's inputs ---------------------------------------------------------------------------
SCAN_TOL_I8 = 2e-6   # tests/test_gpu_bruteforce.py TOL
SCAN_TOL_F32 = 4e-5  # tests/test_gpu_bruteforce.py TOL_F32
SCAN_KS = (1, 10, 16)

# name -> (kind, dim, n, nq, seed)
SCAN_INPUTS = {
    "odd_i8_17": ("odd_i8", 17, 3001, 70, 1),
    "odd_i8_100": ("odd_i8", 100, 5000, 70, 2),
    "odd_i8_128": ("odd_i8", 128, 3000, 70, 3),
    "odd_i8_200": ("odd_i8", 200, 2000, 70, 4),
    "odd_i8_300": ("odd_i8", 300, 1500, 70, 5),
    "one_sided_i8_100": ("one_sided_i8", 100, 3001, 70, 6),
    "one_sided_i8_128": ("one_sided_i8", 128, 3001, 70, 7),
    # 512 rows per list: the lists fill with positive scores, then the block bound decides (rows of 32 and of 128 bytes)
    "far_side_i8_17": ("far_side_i8", 17, 65_600, 70, 14),
    "far_side_i8_100": ("far_side_i8", 100, 65_600, 70, 15),
    "short_f32_100": ("short_f32", 100, 5000, 70, 8),
    "short_f32_300": ("short_f32", 300, 1300, 70, 9),
    "unit_f32_100": ("unit_f32", 100, 5000, 70, 10),
    # the smallest sizes (and 32 rows: a last tile of 33) at which the priming pass and the shared threshold run at every k of
    # SCAN_KS on the ring: 122,881 rows with four query tiles (64 ranges), 245,761 with fewer (128 ranges)
    "odd_i8_128_primed": ("odd_i8_planted", 128, 122_913, 1540, 11),
    "odd_i8_100_primed": ("odd_i8_planted", 100, 245_793, 200, 12),
    # rows shorter than 128 bytes keep the first int8 kernel: primed, its thresholds are sharp enough for its block bound to cut
    "odd_i8_17_primed": ("odd_i8_planted", 17, 150_000, 100, 13),
}
# name -> what the scan runs (GRANNE_HIP_OPT_LAST_SCAN): the kernel form, the ranges, and the k of SCAN_KS at which the priming
# pass runs. far_side_i8_17's first range holds 9 tiles: enough for kk = 7 alone.
SCAN_RAN = {
    "odd_i8_17": ("I8", 24, ()), "odd_i8_100": ("RING", 40, ()), "odd_i8_128": ("RING", 24, ()),
    "odd_i8_200": ("I8_CHUNKED", 16, ()), "odd_i8_300": ("I8_CHUNKED", 12, ()),
    "one_sided_i8_100": ("RING", 24, ()), "one_sided_i8_128": ("RING", 24, ()),
    "far_side_i8_17": ("I8", 64, (1,)), "far_side_i8_100": ("RING", 128, ()),
    "short_f32_100": ("B16_7_4", 40, ()), "short_f32_300": ("B16_CHUNKED", 21, ()), "unit_f32_100": ("B16_7_4", 40, ()),
    "odd_i8_128_primed": ("RING", 64, (1, 10, 16)), "odd_i8_100_primed": ("RING", 128, (1, 10, 16)),
    "odd_i8_17_primed": ("I8", 64, (1, 10, 16)),
}
PLANTED = 32


def planted_at(j, n):
    """Where query j's planted row stands: spread over the set, each in a 32-row block of its own."""
    return (17 + j * (n // PLANTED // 32) * 32 + 5 * j) % (n - 3)


def scan_input(name):
    """(elements, queries, tolerance) of one exact-scan case."""
    kind, dim, n, nq, seed = SCAN_INPUTS[name]
    rng = np.random.default_rng(7000 + seed)
    if kind == "odd_i8":
        return odd_i8(rng, n, dim), odd_i8(rng, nq + 3, dim)[:nq], SCAN_TOL_I8  # (queries: without the three fixed rows)
    if kind == "odd_i8_planted":
        el, q = odd_i8(rng, n, dim), odd_i8(rng, nq + 3, dim)[:nq]
        for j in range(PLANTED):
            # amplitude 3 along query j: its nearest neighbour, among rows of 40 x its norm
            q[j] = np.trunc(rng.uniform(-1.0, 1.0, dim) * 127.0).astype(np.int8)
            el[planted_at(j, n)] = np.trunc(q[j].astype(np.float64) * (3.0 / 127.0)).astype(np.int8)
        return el, q, SCAN_TOL_I8
    if kind == "one_sided_i8":
        el, q = one_sided_i8(rng, n, dim, nq)
        return el, q, SCAN_TOL_I8
    if kind == "far_side_i8":
        el, q = far_side_i8(rng, n, dim, nq)
        return el, q, SCAN_TOL_I8
    if kind == "short_f32":  # norms 10^U(-0.6, 0) against unit queries: no dot reaches 1, score order = distance order
        el = unit_f32(rng, n, dim)
        el = (el * np.power(10.0, rng.uniform(-0.6, 0.0, n)).astype(np.float32)[:, None]).astype(np.float32)
        return el, unit_f32(rng, nq, dim), SCAN_TOL_F32
    if kind == "unit_f32":
        return unit_f32(rng, n, dim), unit_f32(rng, nq, dim), SCAN_TOL_F32
    raise ValueError(kind)


def near_tie_share(dists, k, tol):
    """dists [nq, >= k + 1]: an exact scan's distances, ascending. The share of positions (query, rank j < k) whose
    distance to rank j + 1 lies within tol -- the positions at which a scan in tolerance mode may name another id."""
    d = np.asarray(dists, np.float64)
    return float((d[:, 1:k + 1] - d[:, :k] <= tol).mean())
