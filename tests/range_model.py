"""The models of range search (TEST INFRASTRUCTURE, a plain module like tests/postfilter_model.py): the pseudo-code of
include/granne_hip.h ("range search") over the CPU oracle.

    exact_range(q, r, cap[, allowed]):
        W      = { i : allowed(q, i) and dist(i, q) <= r }          # dist: the oracle's, compared in float32
        total  = |W|
        answer = the first min(total, cap) members of W by (distance bits, id)
        total > 4096: the answer is exact_topk[_filtered](cap)'s -- the same ids unless that selection overflows
        (exact_topk_model.select), which voids the query: count 0, a filled row, the total kept

    search_range(q, r, cap, stages, fallback):
        for s, E in enumerate(stages):
            L = Granne::search(q, E, E)                              # oracle.Index.search_batch
            within = number of entries of L with distance <= r
            if within < len(L) or len(L) < E: return L[:min(within, cap)], found = within, stage = s
        EXACT: exact_range(q, r, cap), found = total, stage = STAGE_EXACT
        SHORT: the last L[:min(within, cap)], found = within, stage = STAGE_SHORT

The exact model works on a FULL SCAN: every row of every query sorted by (distance, id), which is
oracle.Index(el, []).scan_topk(q, n) -- computed once per input and shared by the tests that cut it at different radii."""
import numpy as np

from tests import exact_topk_model as m
from tests.conftest import random_floats

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
CAP_MAX = 1024  # GRANNE_HIP_RANGE_CAP_MAX
ET_CAP = m.CAP  # 4096: the keys phase A ranks
STAGE_EXACT, STAGE_SHORT = 0xFFFFFFFF, 0xFFFFFFFE  # GRANNE_HIP_RG_STAGE_*
EXACT, SHORT = "exact", "short"


def full_scan(oracle, el, q, chunk=512):
    """(ids [nq, n] u64, dists [nq, n] f32): every row of every query, ascending by (distance bits, id) -- what
    oracle.Index(el, []).scan_topk(q, n) returns. That scan keeps a sorted list of k entries by insertion, n * k work per
    query, so the rows are scanned `chunk` at a time (scan_topk(q, chunk) over each slice: all of its distances, the
    oracle's own values) and sorted here."""
    n, nq = len(el), len(q)
    d = np.empty((nq, n), np.float32)
    for lo in range(0, n, chunk):
        part = np.ascontiguousarray(el[lo:lo + chunk])
        _, ids, ds = oracle.Index(part, []).scan_topk(q, len(part))
        np.put_along_axis(d[:, lo:lo + len(part)], ids.astype(np.int64), ds, axis=1)
    ids = np.broadcast_to(np.arange(n, dtype=np.uint64), (nq, n))
    order = np.lexsort((ids, d.view(np.uint32)), axis=1)
    return np.take_along_axis(ids, order, axis=1), np.take_along_axis(d, order, axis=1)


class Exact:
    def __init__(self, nq, cap):
        self.ids = np.full((nq, cap), NONE, np.uint64)
        self.dists = np.full((nq, cap), np.inf, np.float32)
        self.counts = np.zeros(nq, np.uint32)
        self.totals = np.zeros(nq, np.uint32)
        self.voided = np.zeros(nq, bool)
        self.ranked = 0  # status[2] of a call no query of which is dense: the largest total


def exact_range(scan, radii, cap, masks=None):
    """The model on a full scan. radii: f32 [nq]; masks: None, bool [n] or bool [nq, n]."""
    ids, ds = scan
    nq = len(ids)
    radii = np.broadcast_to(np.asarray(radii, np.float32), (nq,))
    ans = Exact(nq, cap)
    for a in range(nq):
        row_ids, row_ds = ids[a], ds[a]
        if masks is not None:
            mask = masks if np.ndim(masks) == 1 else masks[a]
            ok = np.asarray(mask, bool)[row_ids.astype(np.int64)]
            row_ids, row_ds = row_ids[ok], row_ds[ok]
        with np.errstate(invalid="ignore"):
            total = int((row_ds <= radii[a]).sum())  # a prefix: the scan ascends
        assert total == 0 or (row_ds[:total] <= radii[a]).all()
        ans.totals[a] = total
        if total > ET_CAP and m.select(row_ds, cap)[2]:
            ans.voided[a] = True
            continue
        t = min(total, cap)
        ans.ids[a, :t], ans.dists[a, :t], ans.counts[a] = row_ids[:t], row_ds[:t], t
        if total <= ET_CAP:
            ans.ranked = max(ans.ranked, total)
    return ans


def radius_for_total(row_ds, t):
    """a radius with exactly t rows of the (ascending) distances within it, or None where a tie at the border or the
    length forbids it; t = 0: just below the nearest"""
    n = len(row_ds)
    if t > n:
        return None
    if t == 0:
        return np.float32(-1.0) if row_ds[0] == 0 else np.nextafter(row_ds[0], np.float32(-np.inf))
    if t < n and row_ds[t] == row_ds[t - 1]:
        return None
    return row_ds[t - 1]


# ---- the walk -------------------------------------------------------------------------------------------------------
class Walked:
    def __init__(self, nq, cap):
        self.ids = np.full((nq, cap), NONE, np.uint64)
        self.dists = np.full((nq, cap), np.inf, np.float32)
        self.counts = np.zeros(nq, np.uint32)
        self.found = np.zeros(nq, np.uint32)
        self.stage = np.zeros(nq, np.uint32)
        self.unfinished = 0
        self.per_stage = []


def _take(ans, qi, row_ids, row_ds, within, cap, stage):
    ans.ids[qi], ans.dists[qi] = NONE, np.inf
    t = min(within, cap)
    ans.ids[qi, :t], ans.dists[qi, :t] = row_ids[:t], row_ds[:t]
    ans.counts[qi], ans.found[qi], ans.stage[qi] = t, within, stage


def search_range(oracle, oix, q, radii, cap, stages, fallback):
    """The staged model over oracle.Index `oix`. Escalation is per query."""
    nq = len(q)
    radii = np.broadcast_to(np.asarray(radii, np.float32), (nq,))
    ans = Walked(nq, cap)
    pending = np.arange(nq)
    for s, E in enumerate(stages):
        ans.per_stage.append(len(pending))
        if len(pending) == 0:
            break
        ids, ds, cnt, _ = oix.search_batch(np.ascontiguousarray(q[pending]), E, E)
        left = []
        for r, qi in enumerate(pending):
            L = int(cnt[r])
            row_ids, row_ds = ids[r, :L], ds[r, :L]
            within = int((row_ds <= radii[qi]).sum())
            assert (row_ds[:within] <= radii[qi]).all()  # a prefix
            if within < L or L < E:
                _take(ans, qi, row_ids, row_ds, within, cap, s)
            else:
                left.append(qi)
                if s + 1 == len(stages) and fallback == SHORT:
                    _take(ans, qi, row_ids, row_ds, within, cap, STAGE_SHORT)
        pending = np.array(left, np.int64)
    ans.unfinished = len(pending)
    if fallback == EXACT and len(pending):
        ex = exact_range(full_scan(oracle, oix.elements, np.ascontiguousarray(q[pending])), radii[pending], cap)
        assert not ex.voided.any()
        ans.ids[pending], ans.dists[pending], ans.counts[pending], ans.found[pending] = ex.ids, ex.dists, ex.counts, ex.totals
        ans.stage[pending] = STAGE_EXACT
    return ans


# ---- worlds for the walk: name -> (n, dim, kind, seed), as tests/postfilter_model.py builds its own ---------------------
WORLDS = {
    "f32-100": (3000, 100, "f32", 41),
    "i8-100": (2000, 100, "i8", 42),
    "f16-100": (2000, 100, "f16", 43),
    "tiny-f32": (11, 8, "f32", 44),  # a graph shorter than the first stage
}
NQ = 96
RANKS = (3, 40, 200, 900)  # the radii of the issue: the distance to these exact neighbours, then one negative, one +inf
_worlds = {}


def world(oracle, name):
    """dict(rows: what the GPU index is made from, R: the oracle's rows, oix, q: NQ prepared queries, et, n, scan: the full
    scan of q over R), built once per session"""
    if name not in _worlds:
        n, dim, kind, seed = WORLDS[name]
        rng = np.random.default_rng(seed)
        rows_f = oracle.normalize_f32(random_floats(rng, n, dim))
        qf = oracle.normalize_f32(random_floats(rng, NQ, dim))
        if kind == "i8":
            rows, q, et = oracle.quantize(rows_f), oracle.quantize(qf), "angular_int"
            R = rows
        elif kind == "f16":
            rows = rows_f.astype(np.float16)
            R, q, et = oracle.normalize_f32(rows.astype(np.float32)), qf, "angular_f16"
        else:
            rows, R, q, et = rows_f, rows_f, qf, "angular"
        built = oracle.build_index(R, num_neighbors=20, max_search=50, reinsert_elements=False, n_threads=1)  # (one thread: the same graph everywhere)
        _worlds[name] = dict(rows=rows, R=R, oix=oracle.Index(R, built.layers), q=q, et=et, n=n, scan=full_scan(oracle, R, q))
    return _worlds[name]


def issue_radii(w):
    """query a: the oracle's distance to its RANKS[a % 6]-th exact neighbour (ranks that exist), a negative radius for
    a % 6 == 4, +inf for a % 6 == 5"""
    _, ds = w["scan"]
    r = np.zeros(len(ds), np.float32)
    for a in range(len(ds)):
        j = a % 6
        r[a] = -0.5 if j == 4 else np.inf if j == 5 else ds[a, min(RANKS[j], w["n"]) - 1]
    return r


# ---- the radii and inputs of the exact scan's tests, shared by the host and the GPU tests ----------------------------------
def border_totals(cap):
    """the totals the issue wants to see: none, one, around the cap, and the phase A / phase B border"""
    return [0, 1, cap - 1, cap, cap + 1, ET_CAP, ET_CAP + 1]


def mixed_radii(scan, cap, start=0):
    """f32 [nq], query a of kind (a + start) % 12: kinds 0..6 a radius with exactly border_totals(cap)[kind] rows within it
    -- EXACTLY the distance of the last of them, which is thereby included -- (skipped where the set is too small or tied
    there); 7: nextafter below the 6th distance (that row and its ties excluded); 8: negative; 9: +inf; 10: 2.0; 11: the
    median distance."""
    _, ds = scan
    nq, n = ds.shape
    targets = border_totals(cap)
    out = np.zeros(nq, np.float32)
    for a in range(nq):
        kind = (a + start) % 12
        r = radius_for_total(ds[a], targets[kind]) if kind < 7 else None
        if kind == 7:
            r = np.nextafter(ds[a, min(5, n - 1)], np.float32(-np.inf))
        elif kind == 8:
            r = np.float32(-0.25)
        elif kind == 9:
            r = np.float32(np.inf)
        elif kind == 10:
            r = np.float32(2.0)
        elif r is None:
            r = ds[a, n // 2]
        out[a] = r
    return out


def rows_of(oracle, rng, n, dim, int8):
    if int8:
        return np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
    return m.unit_rows(oracle, rng, n, dim)


# (int8, dim, n, nq, caps): f32 dims 3, 100, 200 (1, 4, 8 register blocks) and 333 (the memory form), int8 dims 17, 300 and
# 1500 (the memory form); n in 1, 7, 4037, 20011; nq in 1, 3, 65, 1100; cap in 1, 17, 1024
SHAPES = [
    (False, 3, 1, 3, (1, 17)),
    (False, 3, 7, 65, (1, 17, 1024)),
    (False, 100, 4037, 1100, (17,)),
    (False, 100, 20011, 65, (1, 17, 1024)),
    (False, 200, 4037, 3, (1, 1024)),
    (False, 200, 20011, 1, (1024,)),
    (False, 333, 4037, 65, (17, 1024)),
    (True, 17, 7, 3, (1, 1024)),
    (True, 17, 4037, 65, (17, 1024)),
    (True, 300, 20011, 65, (1, 17)),
    (True, 300, 1, 1, (17,)),
    (True, 1500, 4037, 3, (1, 17)),
]
_shapes = {}


def shape_input(oracle, shape):
    """(rows, queries, full scan) of a SHAPES entry, from its own seed, built once per session; two queries are rows of
    the set where it is large (distance 0 or an ulp from it)"""
    if shape not in _shapes:
        int8, dim, n, nq, _ = shape
        rng = np.random.default_rng(9000 + dim + n + nq + int(int8))
        el, q = rows_of(oracle, rng, n, dim, int8), rows_of(oracle, rng, nq, dim, int8)
        if n > 100:
            q[:2] = el[[n - 1, n // 2]][:min(2, nq)]
        _shapes[shape] = (el, q, full_scan(oracle, el, q))
    return _shapes[shape]


def shape_id(s):
    return "%s-%d-n%d-q%d" % ("i8" if s[0] else "f32", s[1], s[2], s[3])
