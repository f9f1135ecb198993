"""The host model of exact_topk_filtered (granne_amd/csrc/exact_topk.h, sources; test infrastructure, a plain module like
tests/exact_topk_model.py, whose bins, key and two-level rule it reuses):

  * the selection over a subset: exact_topk_model.select on the allowed rows' distances, mapped back to global ids;
  * the stage rule of the list form: prefixes(n) as the host computes them, and for a list of m entries which stages are
    live and which one is final;
  * the per-query form's priming, stage by stage, with the rule by which a non-final stage may narrow a bound -- and the
    naive rule beside it, which the priming trap defeats;
  * the filters and inputs the host and the GPU tests share."""
import numpy as np

from tests import exact_topk_model as m
from tests import filter_model as fm

PRIME_MIN, PRIME_STEP = 16384, 16  # ET_PRIME_MIN, ET_PRIME_STEP
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ALL_ONES = 0xFFFFFFFF


# ---- the selection over a subset ----------------------------------------------------------------------------------
def allowed_ids(mask):
    """the ascending id list of a bool mask: what the compaction writes"""
    return np.nonzero(np.asarray(mask, bool))[0].astype(np.uint64)


def select(dists, mask, k):
    """exact_topk_model.select over the allowed rows of one query's distances (all n of them): (global ids ascending by
    (distance bits, id), level, overflow, candidates ranked). Nothing allowed: no ids, nothing ranked."""
    ids = allowed_ids(mask)
    if len(ids) == 0:
        return np.zeros(0, np.uint64), 1, False, 0
    got, level, over, ranked = m.select(np.asarray(dists, np.float32)[ids.astype(np.int64)], k)
    return ids[got.astype(np.int64)], level, over, ranked


def oracle_subset(oracle, el, mask, q, k):
    """oracle.Index(el[allowed], []).scan_topk, its ids mapped through the ascending allowed list: ids [nq, k] u64, dists
    [nq, k] f32, counts [nq] u32 -- the places past min(k, m) UINT64_MAX / +inf"""
    ids = allowed_ids(mask)
    nq, t = len(q), min(k, len(ids))
    out_i, out_d = np.full((nq, k), NONE, np.uint64), np.full((nq, k), np.inf, np.float32)
    if t:
        _, oi, od = oracle.Index(np.ascontiguousarray(el[ids.astype(np.int64)]), []).scan_topk(q, t)
        out_i[:, :t], out_d[:, :t] = ids[oi.astype(np.int64)], od
    return out_i, out_d, np.full(nq, t, np.uint32)


# ---- the stage rule --------------------------------------------------------------------------------------------------
def prefixes(n):
    """the priming prefixes p_0 < .. < p_last = n, a function of n alone (granne_hip.hip)"""
    rev, p = [n], n
    while p > 2 * PRIME_MIN and len(rev) < 16:
        p = max(p // PRIME_STEP, PRIME_MIN)
        rev.append(p)
    return rev[::-1]


def stages(n, count):
    """the list form over `count` entries: [(entries scanned, live, final)] per stage. A stage whose predecessor covered
    the whole list is idle; the first stage with p_st >= count is final."""
    out, P = [], prefixes(n)
    for st, p in enumerate(P):
        live = st == 0 or P[st - 1] < count
        out.append((min(p, count) if live else 0, live, live and p >= count))
    return out


# ---- the per-query form's priming -----------------------------------------------------------------------------------
def narrow_target(total, k, final, naive=False):
    """The target a stage narrows a query's bound to, given `total` allowed rows of its prefix at or below the bound; None:
    the bound stays. The rule: a non-final stage narrows only with total >= k; the final one uses min(k, total). The
    naive rule -- min(k, total) in every stage -- takes a bound from fewer than k rows."""
    if final or naive:
        t = min(k, total)
        return t if t else None
    return k if total >= k else None


def staged_select(dists, mask, k, naive=False):
    """The per-query form on one query: the bound through every stage (both levels, as et_select_kernel narrows it), then
    the allowed rows at or below it ranked by (distance bits, id). Returns (global ids, overflow)."""
    d = np.ascontiguousarray(dists, np.float32)
    mask = np.asarray(mask, bool)
    n = len(d)
    key = m.key(d)
    bound, over = ALL_ONES, False
    P = prefixes(n)
    for st, p in enumerate(P):
        final = st + 1 == len(P)
        inp = np.nonzero(mask[:p] & (key[:p] <= bound))[0]
        target = narrow_target(len(inp), k, final, naive)
        over = False
        if target is None:
            continue
        b1 = key[inp] >> 11
        B1, below1, pop1 = m._first_reaching(np.bincount(b1, minlength=m.BINS1), target)
        if below1 + pop1 <= m.CAP:
            bound = min(bound, (B1 << 11) | 2047)
            continue
        b2 = key[inp][b1 == B1] & 2047
        B2, below2, pop2 = m._first_reaching(np.bincount(b2, minlength=m.BINS2), target - below1)
        bound = min(bound, (B1 << 11) | B2)
        over = below1 + below2 + pop2 > m.CAP
    if over:
        return np.zeros(0, np.uint64), True
    cand = np.nonzero(mask & (key <= bound))[0]
    order = np.lexsort((cand, d.view(np.uint32)[cand].astype(np.int64)))
    return cand[order][:k].astype(np.uint64), False


# ---- filters ---------------------------------------------------------------------------------------------------------
def words(mask, garbage_past_n=False):
    """the bitmap's u32 words; garbage_past_n: the bits at positions >= n of the last word set"""
    w = fm.pack_bits(np.asarray(mask, bool)).copy()
    tail = len(mask) & 31
    if garbage_past_n and tail:
        w[-1] |= np.uint32((0xFFFFFFFF << tail) & 0xFFFFFFFF)
    return w


def only(n, ids):
    a = np.zeros(n, bool)
    a[np.asarray(ids, np.int64)] = True
    return a


def random_mask(rng, n, selectivity):
    return rng.random(n) < selectivity


def exactly(rng, n, count):
    """`count` allowed ids drawn at random"""
    return only(n, rng.choice(n, count, replace=False))


def shared_filters(rng, n, k):
    """name -> mask: the shared filters of the issue at (n, k) -- all ones, random at about 0.5 and 0.01, one id, none,
    only n - 1, only the last partial word, a block from mid-word to mid-word, and m = k - 1, k, k + 1 where they fit"""
    f = {"ones": np.ones(n, bool), "half": random_mask(rng, n, 0.5), "percent": random_mask(rng, n, 0.01),
         "one": only(n, [n // 3]), "none": np.zeros(n, bool), "last": only(n, [n - 1]),
         "last_word": only(n, np.arange((n - 1) & ~31, n))}
    if n > 70:
        f["block"] = only(n, np.arange(n // 4 | 5, (n // 4 | 5) + min(n // 2, 1000) | 3))
    for name, c in (("k-1", k - 1), ("k", k), ("k+1", k + 1)):
        if 0 < c <= n:
            f[name] = exactly(rng, n, c)
    return f


def trap_input(oracle, rng, n=40009, dim=32, k=17, early=5, nearest=8):
    """(rows, query, mask): the priming trap at k. The query's allowed ids are `early` < k rows inside the first 16384,
    at a middling distance, and 200 rows past them: its `nearest` allowed rows (early + nearest < k) and 200 - nearest
    farther ones. The true answer is the nearest rows, the early rows, then k - early - nearest of the farther ones. A
    bound taken from the prefix's min(k, early) = early rows lies at the last early row, BELOW the farther rows the answer
    needs: the final stage would count early + nearest < k rows at or below it and return those alone."""
    assert early + nearest < k
    rows = m.unit_rows(oracle, rng, n, dim)
    q = m.unit_rows(oracle, rng, 1, dim)[0]
    noise = m.unit_rows(oracle, rng, early + 200, dim)
    mask = np.zeros(n, bool)
    early_ids = rng.choice(PRIME_MIN, early, replace=False)
    late_ids = PRIME_MIN + rng.choice(n - PRIME_MIN, 200, replace=False)
    tilt = np.concatenate([np.full(early, 0.3), np.full(nearest, 0.05), np.full(200 - nearest, 0.6)]).astype(np.float32)
    ids = np.concatenate([early_ids, late_ids])
    rows[ids] = oracle.normalize_f32((q[None, :] + tilt[:, None] * noise).astype(np.float32))
    mask[ids] = True
    return rows, q, mask


# ---- the shapes the host and the GPU tests share -----------------------------------------------------------------------
# (int8, dim, n, nq, k): f32 dims 3, 100, 200 (rows in registers: 1, 4 and 8 blocks) and 333 (the memory form), int8 dims 17,
# 100, 300 (1, 1 and 4 blocks) and 1500 (the memory form); every n of 7, 4037, 20011, 40009 (two stages), every nq of 1, 3,
# 65, 1100 (past one round of queries), every k of 1, 17, 100, 1024
CASES = [
    (False, 3, 7, 3, 17),
    (False, 100, 4037, 65, 1),
    (False, 100, 20011, 1100, 17),
    (False, 200, 4037, 3, 1024),
    (False, 200, 20011, 1, 100),
    (False, 333, 4037, 65, 17),
    (False, 100, 40009, 65, 100),
    (True, 17, 7, 3, 1),
    (True, 17, 4037, 65, 1024),
    (True, 100, 4037, 1100, 17),
    (True, 300, 20011, 65, 100),
    (True, 1500, 4037, 3, 17),
    (True, 100, 40009, 3, 1024),
]


def case_id(c):
    return "%s-%d-n%d-q%d-k%d" % (("i8" if c[0] else "f32",) + tuple(c[1:]))


def case_input(oracle, c):
    """(rows, queries, {name: mask}) of a case, from its own seed; two queries are rows of the set where it is large"""
    int8, dim, n, nq, k = c
    rng = np.random.default_rng(9000 + dim + n + nq + k + int(int8))
    if int8:
        el = np.trunc(rng.uniform(-1.0, 1.0, (n, dim)) * 127.0).astype(np.int8)
        q = np.trunc(rng.uniform(-1.0, 1.0, (nq, dim)) * 127.0).astype(np.int8)
    else:
        el, q = m.unit_rows(oracle, rng, n, dim), m.unit_rows(oracle, rng, nq, dim)
    if n > 100:
        q[:2] = el[[n - 1, n // 2]][:min(2, nq)]
    return el, q, shared_filters(rng, n, k)
