"""The exact scan (granne_hip_brute_force_device, granne_amd/csrc/brute_force.h) held to its contract on every kernel form
(test infrastructure, a plain module like tests/value_edges.py; tests/test_gpu_scan_forms.py runs it, and so do the child
processes that test starts for the two environment knobs).

structured_rows() are the row kinds every walker module draws from. scan_rule() restates on the host which launch
granne_hip_brute_force_device makes (ranges, priming sub-ranges, whether the priming pass runs): the tests assert the
library's GRANNE_HIP_OPT_LAST_SCAN word against literals, and this restatement explains the literals.

The contract (brute_force.h's header): the scan selects kk = min(k + 6, 16) candidates per query by a matrix-core score
whose error is eps, recomputes their distances in the reference's arithmetic and returns the k best by (distance, id).
With want_d the oracle's scan and 2 eps <= tol, for every query
    cnt == min(k, n); the distances are oracle.dist's bytes for the returned ids; a list ascends by (distance, id) and
    holds no id twice; |d[j] - want_d[j]| <= tol at every rank; every oracle id with want_d < want_d[k - 1] - tol is
    returned; every returned distance is <= want_d[k - 1] + tol.
None of this needs a cap on near-tied ranks, so clustered rows and exact ties are allowed."""
import functools

import numpy as np

TOL_I8 = 2e-6   # tests/test_gpu_bruteforce.py TOL
TOL_F32 = 4e-5  # tests/test_gpu_bruteforce.py TOL_F32

# form -> (rows per tile, most ranges). The ring takes up to 128 ranges while its query tiles of 512 number at most 3.
FORMS = {
    "RING": (128, 64), "I8": (128, 64), "I8_CHUNKED": (128, 64),
    "B16_7_4": (128, 64), "B16_13_2": (64, 64), "B16_16_1": (32, 64), "B16_CHUNKED": (64, 64),
    "F32_52_4": (128, 64), "F32_100_2": (64, 64), "F32_128_1": (32, 64),
}


def uniform_rows(rng, n, dim):
    """src/test_helper.rs:3-6: uniform in [-0.5, 0.5)."""
    return (rng.random((n, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def structured_rows(kind, rng, n, dim=100):
    """Raw f32 rows: i.i.d. uniform; 8 latent directions plus noise; 64 clusters; every row held about four times; a grid of
    three values per component (many equal distances)."""
    if kind == "uniform":
        return uniform_rows(rng, n, dim)
    if kind == "latent":
        base = rng.standard_normal((8, dim)).astype(np.float32)
        return (rng.standard_normal((n, 8)).astype(np.float32) @ base + 0.05 * uniform_rows(rng, n, dim)).astype(np.float32)
    if kind == "mixture":
        centers = uniform_rows(rng, 64, dim)
        return (centers[rng.integers(0, 64, n)] + 0.05 * uniform_rows(rng, n, dim)).astype(np.float32)
    if kind == "duplicates":
        base = uniform_rows(rng, n // 4, dim)
        return base[rng.integers(0, n // 4, n)].copy()
    if kind == "grid":  # few distinct values per component: many equal distances
        return (rng.integers(-1, 2, (n, dim)).astype(np.float32) * np.float32(0.25)).astype(np.float32)
    raise ValueError(kind)


def scan_rule(form, n, nq, k):
    """granne_hip_brute_force_device's launch, restated: dict(ranges, prime_ranges, primed, kk). The set is cut into
    G = min(tiles, most ranges) ranges of a whole number of tiles; with G >= 32 the first range is cut into up to 64
    sub-ranges (Gs), and the priming pass runs when Gs >= kk."""
    tile, most = FORMS[form]
    if form == "RING" and (nq + 511) // 512 * 64 < 256:
        most = 128
    kk = min(k + 6, 16)
    G = max(1, min((n + tile - 1) // tile, most))
    per_range = max(tile, ((n + G - 1) // G + tile - 1) // tile * tile)
    Gs = 0
    if G >= 32:
        first = min(per_range, n)
        Gs = min((first + tile - 1) // tile, 64)
        sub = ((first + Gs - 1) // Gs + tile - 1) // tile * tile
        Gs = (first + sub - 1) // sub
    return {"ranges": G, "prime_ranges": Gs, "primed": G >= 32 and Gs >= kk, "kk": kk}


def reported(ix):
    """what the index's last scan ran (GRANNE_HIP_OPT_LAST_SCAN), the form by its name"""
    from granne_amd import _lib
    r = _lib.last_scan(ix.get_option(_lib.OPT_LAST_SCAN))
    names = {getattr(_lib, "SCAN_" + name): name for name in FORMS}
    r["form"] = names.get(r["form"], r["form"])
    return r


def assert_reported(ix, form, ranges, primed, prime_ranges, k, where=None):
    r = reported(ix)
    assert r == {"form": form, "ranges": ranges, "primed": primed, "prime_ranges": prime_ranges, "kk": min(k + 6, 16)}, (where, r)
    return r


def _et(a):
    return "angular" if a.dtype == np.float32 else "angular_int"


def assert_contract(oracle, el, q, k, got, sub, want_i, want_d, tol, dist_rows, where):
    """One scan's lists against the contract. `sub`: the queries the oracle scanned (want_i, want_d [len(sub), >= k]);
    `dist_rows`: the queries whose returned distances are recomputed by oracle.dist. Returns (largest |d - true d|, share
    of positions whose id is the oracle's)."""
    ids, ds, cnt = got
    n, nq = len(el), len(q)
    m = min(k, n)
    assert ids.shape == (nq, k) and ds.shape == (nq, k)
    assert (cnt == m).all(), where
    ids, ds = ids[:, :m], ds[:, :m]
    assert (ids < n).all(), where
    for qi in dist_rows:
        want = np.array([oracle.dist(el[int(e)], q[qi]) for e in ids[qi]], np.float32)
        assert want.tobytes() == ds[qi].tobytes(), (where, qi)
    if m > 1:  # ascending by (distance, id): which also says that no id is held twice
        up = (ds[:, 1:] > ds[:, :-1]) | ((ds[:, 1:] == ds[:, :-1]) & (ids[:, 1:] > ids[:, :-1]))
        assert up.all(), (where, np.argwhere(~up)[:3])
    srt = np.sort(ids, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), where
    wi, wd = want_i[:, :m], want_d[:, :m].astype(np.float64)
    d = ds[sub].astype(np.float64)
    err = np.abs(d - wd)
    assert err.max() <= tol, (where, float(err.max()), np.unravel_index(err.argmax(), err.shape))
    assert (d <= wd[:, -1:] + tol).all(), where
    for r, qi in enumerate(sub):
        must = wi[r][wd[r] < wd[r, -1] - tol]
        missing = set(must.tolist()) - set(ids[qi].tolist())
        assert not missing, (where, qi, sorted(missing)[:4])
    return float(err.max()), float((ids[sub] == wi).mean())


class World:
    """Rows, queries and the oracle's scan of them, made once and scanned on the GPU at several k."""

    def __init__(self, oracle, el, q, tol, sub=None, members=None):
        self.oracle, self.el, self.q, self.tol = oracle, el, q, tol
        n, nq = len(el), len(q)
        self.sub = np.arange(nq) if sub is None else np.asarray(sub)
        self.members = members or {}  # query index -> the row it is
        _, self.want_i, self.want_d = oracle.Index(el, []).scan_topk(np.ascontiguousarray(q[self.sub]), min(16, n))
        # distance bytes: every query below 10,000 rows, a fixed sample of 32 and more above
        self.dist_rows = list(range(nq)) if n < 10_000 else sorted(set(np.linspace(0, nq - 1, min(nq, 40)).astype(int).tolist())
                                                                 | set(self.members))

    def scan(self, ix, k, expect, name, ids_repeat=True):
        """Two runs at k, each held to the contract and to `expect` = (form, ranges, primed, prime_ranges); the same
        distance bytes both times, the same ids unless the rows hold exact ties (ids_repeat=False)."""
        where = (name, len(self.el), len(self.q), k)
        rule = scan_rule(expect[0], len(self.el), len(self.q), k)  # the literal is what the restated rule gives
        assert (rule["ranges"], rule["primed"], rule["prime_ranges"]) == tuple(expect[1:]), (where, rule)
        first = ix.brute_force(self.q, k)
        assert_reported(ix, *expect, k, where=where)
        err, same = assert_contract(self.oracle, self.el, self.q, k, first, self.sub, self.want_i, self.want_d, self.tol,
                                    self.dist_rows, where)
        again = ix.brute_force(self.q, k)
        assert_reported(ix, *expect, k, where=where)
        assert first[1].tobytes() == again[1].tobytes() and (first[2] == again[2]).all(), where
        if ids_repeat:
            assert (first[0] == again[0]).all(), where
        else:  # (the distances are the first run's: what is left to hold is the ids' side of the contract)
            assert_contract(self.oracle, self.el, self.q, k, again, self.sub, self.want_i, self.want_d, self.tol, self.dist_rows, where)
        for qi, row in self.members.items():  # a member's nearest is itself, or a copy of it with a smaller id
            assert self.el[int(first[0][qi, 0])].tobytes() == self.el[row].tobytes(), (where, qi)
            assert self.el[int(again[0][qi, 0])].tobytes() == self.el[row].tobytes(), (where, qi)
        r = reported(ix)
        print("%s n=%d nq=%d k=%d %s G=%d Gs=%d primed=%d: largest |d - true d| %.3g, ids equal %.4f"
              % (name, len(self.el), len(self.q), k, r["form"], r["ranges"], r["prime_ranges"], r["primed"], err, same))
        return first


def prepare(oracle, raw, int8):
    return oracle.quantize(raw) if int8 else oracle.normalize_f32(raw)


@functools.lru_cache(maxsize=2)
def uniform_world_rows(int8, dim, n, nq, seed):
    """Prepared i.i.d. uniform rows and queries, made once per case."""
    from oracle import oracle
    oracle.build()
    rng = np.random.default_rng(seed)
    el = prepare(oracle, uniform_rows(rng, n, dim), int8)
    q = prepare(oracle, uniform_rows(rng, nq, dim), int8)
    return el, q


def uniform_world(oracle, int8, dim, n, nq, seed, n_max=None, oracle_queries=64):
    """The first n of n_max uniform rows (the sizes of one case share their rows), queries of which two are members of
    the first 1,000 rows; the oracle scans all queries up to 257 of them, a fixed 64 (the members among them) beyond."""
    el, q = uniform_world_rows(int8, dim, n_max or n, nq, seed)
    el, q = el[:n], q.copy()
    members = {}
    if nq >= 5:
        members = {3: 11, nq - 1: min(n, 1000) - 3}
        for qi, row in members.items():
            q[qi] = el[row]
    sub = None
    if nq > 257:
        sub = sorted(set(np.linspace(0, nq - 1, oracle_queries).astype(int).tolist()) | set(members))
    return World(oracle, el, q, TOL_I8 if int8 else TOL_F32, sub, members)


PLANTED_QUERIES = 8


def planted_world(oracle, int8, dim, n, tile, seed, nq=64):
    """The priming pass's threshold at its edge. Uniform rows whose first range is 16 sub-ranges of one tile each
    (n = ranges * tile * 15 + 1, kk = 16). Query j < PLANTED_QUERIES gets its nearest rows planted there, one per
    sub-range: 15 of them for even j, 16 for odd j, row s at the query's direction plus 0.04 (s + 1) of a unit noise vector
    (distances 0.0008 .. 0.14, the drawn rows' from 0.4 up). The 16th-largest sub-range maximum is then the score of
    an ordinary row (even j) or of the 16th nearest itself (odd j); the 15th-largest is a score that only 15 rows of the
    whole set reach: a threshold taken one place too high returns 15 rows at k = 16."""
    el, q = uniform_world_rows(int8, dim, n, nq, seed)
    el, q = el.copy(), q.copy()
    rng = np.random.default_rng(seed + 7)
    planted = {}
    for j in range(PLANTED_QUERIES):
        unit = q[j].astype(np.float64) / np.linalg.norm(q[j].astype(np.float64))
        rows = []
        for s in range(15 + j % 2):
            noise = rng.standard_normal(dim)
            noise -= (noise @ unit) * unit  # across the query: the distance is 1 - 1 / sqrt(1 + (0.04 (s + 1))^2)
            row = s * tile + (5 * j + 3 * s) % tile
            el[row] = prepare(oracle, (unit + 0.04 * (s + 1) * noise / np.linalg.norm(noise)).astype(np.float32)[None], int8)[0]
            rows.append(row)
        planted[j] = rows
    w = World(oracle, el, q, TOL_I8 if int8 else TOL_F32)
    for j, rows in planted.items():  # by the oracle alone: the planted rows are the nearest, in the order planted, well apart
        assert w.want_i[j, :len(rows)].tolist() == rows, (j, w.want_i[j], rows)
        assert (np.diff(w.want_d[j].astype(np.float64)) > 20 * w.tol).all(), (j, w.want_d[j])
    w.planted = planted
    return w


def structured_world(oracle, kind, int8, n, seed, nq=64, n_members=16):
    """Rows and queries of one kind from the same generator, then n_members member rows as queries."""
    rng = np.random.default_rng(seed)
    el = prepare(oracle, structured_rows(kind, rng, n), int8)
    q = prepare(oracle, structured_rows(kind, rng, nq), int8)
    rows = rng.choice(n, n_members, replace=False)
    q = np.concatenate([q, el[rows]])
    members = {nq + j: int(r) for j, r in enumerate(rows)}
    return World(oracle, el, q, TOL_I8 if int8 else TOL_F32, None, members)


# ---- the cases, shared by the GPU module and the knobs' child processes -----------------------------------
KS_BOUNDARY = (1, 9, 10, 13, 16)  # kk = 7, 15, 16, 16, 16
# Sub-ranges of the first range at the six sizes of a boundary case: one tile below the threshold of kk = 7, at it, and
# the same for kk = 15 and kk = 16. A size primes at k when its figure is at least min(k + 6, 16).
BOUNDARY_GS = (6, 7, 14, 15, 15, 16)


def boundary_sizes(tile, ranges):
    """ranges * tile * (kk - 1) + 1 rows are the fewest whose first range holds kk tiles; one tile fewer: kk - 1."""
    out = []
    for kk in (7, 15, 16):
        at = ranges * tile * (kk - 1) + 1
        out += [at - tile, at]
    return tuple(out)


def run_boundary(ga, oracle, form, int8, dim, nq, ranges, sizes, seed, which=range(6), ks=KS_BOUNDARY):
    """A form at the priming boundary: sizes[i] rows give BOUNDARY_GS[i] sub-ranges. The last size also runs with each of
    eight queries' nearest rows planted one per sub-range (planted_world)."""
    tile = FORMS[form][0]
    assert tuple(sizes) == boundary_sizes(tile, ranges)  # the literals are these
    for i in which:
        n = sizes[i]
        w = uniform_world(oracle, int8, dim, n, nq, seed, n_max=sizes[-1])
        ix = ga.Granne(_et(w.el), w.el, [])
        for k in ks:
            assert scan_rule(form, n, nq, k) == {"ranges": ranges, "prime_ranges": BOUNDARY_GS[i], "kk": min(k + 6, 16),
                                                 "primed": BOUNDARY_GS[i] >= min(k + 6, 16)}
            w.scan(ix, k, (form, ranges, BOUNDARY_GS[i] >= min(k + 6, 16), BOUNDARY_GS[i]), "%s_%d" % (form, dim))
        ix.close()
        if i == 5 and nq == 64:  # kk = 16 sub-ranges of a tile each: the threshold is the 16th-largest of 16 maxima
            w = planted_world(oracle, int8, dim, n, tile, seed)  # (the same drawn rows)
            ix = ga.Granne(_et(w.el), w.el, [])
            for k in (16, 10, 1):
                ids = w.scan(ix, k, (form, ranges, True, 16), "%s_%d_planted" % (form, dim))[0]
                for j, rows in w.planted.items():
                    assert ids[j, :min(k, len(rows))].tolist() == rows[:k], (form, dim, k, j)
            ix.close()


def run_unprimed(ga, oracle, form, int8, dim, seed, part, ring_wide=True):
    """One form below every threshold, in three parts. "tiles": 31, 32, 64 and 65 tiles (the last one short) -- fewer than
    32 ranges, exactly 32, the cap, and past it, where the ring with up to three query tiles goes on to 65 ranges and
    merges in two steps. "every_k": k = 1 .. 16 at 3,001 rows. "nq": query counts around the blocks' 256 (the ring's 512,
    and 1,537: four query tiles) at 3,001 rows."""
    tile = FORMS[form][0]
    name = "%s_%d" % (form, dim)
    if part == "tiles":
        for tiles in (31, 32, 64, 65):
            n = tiles * tile - 5
            ranges = tiles if tiles <= 64 or (form == "RING" and ring_wide) else 64
            gs = 0 if tiles < 32 else 2 if ranges == 64 and tiles == 65 else 1
            w = uniform_world(oracle, int8, dim, n, 70, seed, n_max=65 * tile - 5)
            ix = ga.Granne(_et(w.el), w.el, [])
            for k in (1, 10, 16):
                w.scan(ix, k, (form, ranges, False, gs), name)
            ix.close()
        return
    n = 3001
    ranges = (n + tile - 1) // tile  # 24, 47 or 94 tiles: one range each up to the cap
    ranges, gs = (ranges, 0) if ranges < 32 else (min(ranges, 64), 1 if ranges <= 64 else 2)
    if part == "every_k":
        w = uniform_world(oracle, int8, dim, n, 70, seed + 1)
        ix = ga.Granne(_et(w.el), w.el, [])
        for k in range(1, 17):
            w.scan(ix, k, (form, ranges, False, gs), name)
        ix.close()
        return
    assert part == "nq"
    ix = None
    for nq in (1, 31, 33, 255, 256, 257) + ((511, 512, 513, 1537) if form == "RING" else ()):
        w = uniform_world(oracle, int8, dim, n, nq, seed + 2, oracle_queries=96)
        ix = ix or ga.Granne(_et(w.el), w.el, [])  # (the rows are the seed's, whatever nq)
        for k in (10, 16):
            w.scan(ix, k, (form, ranges, False, gs), name)
    ix.close()


# ---- the forms behind an environment knob: run in a child process that has the knob set -------------------
def knob_main(knob):
    """GRANNE_HIP_BF_B16=0: f32 rows on the f32 matrix path at 100, 200 and 256 dims, unprimed and around the threshold of
    kk = 16 (at it, k = 1 runs primed with kk = 7 as well); 300 dims stay on the chunked bf16 kernel.
    GRANNE_HIP_BF_RING=0: 128-byte int8 rows through bf_i8_kernel at 3,000 and 122,881 rows."""
    import granne_amd as ga
    from oracle import oracle
    oracle.build()
    if knob == "GRANNE_HIP_BF_B16":
        for form, dim, sizes, seed in (("F32_52_4", 100, (49_025, 49_153, 114_561, 114_689, 122_753, 122_881), 801),
                                       ("F32_100_2", 200, (24_513, 24_577, 57_281, 57_345, 61_377, 61_441), 802),
                                       ("F32_128_1", 256, (12_257, 12_289, 28_641, 28_673, 30_689, 30_721), 803)):
            w = uniform_world(oracle, False, dim, 3001, 70, seed)
            ix = ga.Granne("angular", w.el, [])
            ranges = -(-3001 // FORMS[form][0])
            for k in (1, 10, 16):
                w.scan(ix, k, (form, min(ranges, 64), False, 0 if ranges < 32 else 1 if ranges <= 64 else 2), "%s_%d" % (form, dim))
            ix.close()
            run_boundary(ga, oracle, form, False, dim, 64, 64, sizes, seed + 10, which=(4, 5), ks=(1, 10, 16))
        w = uniform_world(oracle, False, 300, 3001, 70, 804)
        ix = ga.Granne("angular", w.el, [])
        for k in (1, 16):
            w.scan(ix, k, ("B16_CHUNKED", 47, False, 1), "B16_CHUNKED_300")
        ix.close()
    elif knob == "GRANNE_HIP_BF_RING":
        w = uniform_world(oracle, True, 128, 3000, 70, 811)
        ix = ga.Granne("angular_int", w.el, [])
        for k in (1, 10, 16):
            w.scan(ix, k, ("I8", 24, False, 0), "I8_128")
        ix.close()
        run_boundary(ga, oracle, "I8", True, 128, 64, 64, (49_025, 49_153, 114_561, 114_689, 122_753, 122_881), 812,
                     which=(4, 5), ks=(1, 10, 16))
    else:
        raise ValueError(knob)
    print("scan knob ok")
