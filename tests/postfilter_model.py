"""The model of post-filtered search (TEST INFRASTRUCTURE, a plain module like tests/exact_topk_filtered_model.py): the
pseudo-code of include/granne_hip.h ("post-filtered search") over the CPU oracle --

    postfiltered(q):
      for s in 0 .. S-1:
          L = Granne::search(q, max_search = E_s, num_neighbors = E_s)     # oracle.Index.search_batch(q, E_s, E_s)
          A = [x for x in L if allowed(x.id)]
          if len(A) >= min_allowed or len(L) < E_s: return A[:k], stage = s
      if fallback == EXACT: return exact_topk_filtered(q, k), stage = STAGE_EXACT   # exact_topk_filtered_model.oracle_subset
      else:                 return A[:k] of the last stage, stage = STAGE_SHORT

-- and the worlds, filters and inputs the host and the GPU tests share. Escalation is per query: a stage searches only the
queries the stages before it left pending."""
import numpy as np

from tests import exact_topk_filtered_model as efm
from tests.conftest import random_floats

NONE = efm.NONE
STAGE_EXACT, STAGE_SHORT = 0xFFFFFFFF, 0xFFFFFFFE  # GRANNE_HIP_PF_STAGE_*
EXACT, SHORT = "exact", "short"


class Answer:
    """ids [nq, k] u64, dists [nq, k] f32, counts [nq] u32, stage [nq] u32, unfinished: the queries no stage finished
    (status[3]), per_stage: how many queries each stage searched."""

    def __init__(self, nq, k):
        self.ids = np.full((nq, k), NONE, np.uint64)
        self.dists = np.full((nq, k), np.inf, np.float32)
        self.counts = np.zeros(nq, np.uint32)
        self.stage = np.zeros(nq, np.uint32)
        self.unfinished = 0
        self.per_stage = []

    def outcome_counts(self, n_stages):
        """queries per outcome: stage 0 .. n_stages - 1, then the fallback"""
        return [int((self.stage == s).sum()) for s in range(n_stages)] + [int((self.stage >= STAGE_SHORT).sum())]


def _take(ans, qi, ids_row, ds_row, allowed_row, k, stage):
    ans.ids[qi], ans.dists[qi] = NONE, np.inf
    t = min(k, len(ids_row[allowed_row]))
    ans.ids[qi, :t] = ids_row[allowed_row][:t]
    ans.dists[qi, :t] = ds_row[allowed_row][:t]
    ans.counts[qi] = t
    ans.stage[qi] = stage


def postfiltered(oracle, oix, q, masks, k, min_allowed, stages, fallback):
    """The model over oracle.Index `oix`. masks: bool [n] (one filter for all queries) or bool [nq, n]."""
    masks = np.asarray(masks, bool)
    nq = len(q)
    ans = Answer(nq, k)
    pending = np.arange(nq)
    for s, E in enumerate(stages):
        ans.per_stage.append(len(pending))
        if len(pending) == 0:
            break
        ids, ds, cnt, _ = oix.search_batch(np.ascontiguousarray(q[pending]), E, E)
        left = []
        for r, qi in enumerate(pending):
            L = int(cnt[r])
            row_ids, row_ds = ids[r, :L], ds[r, :L]  # slots past the count are never bit-tested
            mask = masks if masks.ndim == 1 else masks[qi]
            ok = mask[row_ids.astype(np.int64)]
            if ok.sum() >= min_allowed or L < E:
                _take(ans, qi, row_ids, row_ds, ok, k, s)
            else:
                left.append(qi)
                if s + 1 == len(stages) and fallback == SHORT:
                    _take(ans, qi, row_ids, row_ds, ok, k, STAGE_SHORT)
        pending = np.array(left, np.int64)
    ans.unfinished = len(pending)
    if fallback == EXACT and len(pending):
        el = oix.elements
        if masks.ndim == 1:
            oi, od, oc = efm.oracle_subset(oracle, el, masks, np.ascontiguousarray(q[pending]), k)
            ans.ids[pending], ans.dists[pending], ans.counts[pending] = oi, od, oc
        else:
            for qi in pending:
                oi, od, oc = efm.oracle_subset(oracle, el, masks[qi], q[qi:qi + 1], k)
                ans.ids[qi], ans.dists[qi], ans.counts[qi] = oi[0], od[0], oc[0]
        ans.stage[pending] = STAGE_EXACT
    return ans


# ---- worlds -------------------------------------------------------------------------------------------------------------
# name -> (n, dim, kind, seed): rows normalize_f32(random_floats(rng, n, dim)), quantised for int8; n = 3000 is not a
# multiple of 32. "f16": rows16 = those rows as halves, the oracle over R = normalize_f32(widen(rows16)).
WORLDS = {
    "f32-8": (3000, 8, "f32", 11),
    "i8-8": (3000, 8, "i8", 12),
    "i8-100": (2000, 100, "i8", 14),
    "f32-200": (1200, 200, "f32", 15),
    "f16-100": (2000, 100, "f16", 16),
    "ties-8": (1500, 8, "ties", 17),  # every row stored twice: ids i and i + 1500 are equal rows
}
NQ = 300
_worlds = {}


def world(oracle, name):
    """dict(rows: what the GPU index is made from, R: the oracle's rows, rows_f: the f32 rows before quantisation, oix,
    q: NQ prepared queries, et: the element type's name), built once per session"""
    if name not in _worlds:
        n, dim, kind, seed = WORLDS[name]
        rng = np.random.default_rng(seed)
        rows_f = oracle.normalize_f32(random_floats(rng, n, dim))
        qf = oracle.normalize_f32(random_floats(rng, NQ, dim))
        if kind == "ties":
            rows_f = np.ascontiguousarray(np.concatenate([rows_f, rows_f]))
        if kind == "i8":
            rows, q, et = oracle.quantize(rows_f), oracle.quantize(qf), "angular_int"
            R = rows
        elif kind == "f16":
            rows = rows_f.astype(np.float16)
            R, q, et = oracle.normalize_f32(rows.astype(np.float32)), qf, "angular_f16"
        else:
            rows, R, q, et = rows_f, rows_f, qf, "angular"
        built = oracle.build_index(R, num_neighbors=12, max_search=20, reinsert_elements=False, n_threads=0)
        _worlds[name] = dict(rows=rows, R=R, rows_f=rows_f, oix=oracle.Index(R, built.layers), q=q, et=et, n=len(R))
    return _worlds[name]


# ---- filters ------------------------------------------------------------------------------------------------------------
def density_mask(rng, rows_f):
    """One filter whose density varies over the data, so that one call holds every outcome: with c = rows_f[:, 0] and
    s = c.std(), a row is allowed with probability 1.0 / 0.3 / 0.06 / 0.004 for c < -0.8 s / < 0 / < 0.8 s / otherwise."""
    c = rows_f[:, 0]
    s = c.std()
    p = np.where(c < -0.8 * s, 1.0, np.where(c < 0, 0.3, np.where(c < 0.8 * s, 0.06, 0.004)))
    return rng.random(len(c)) < p


PER_QUERY_SELECTIVITY = (1.0, 0.5, 0.1, 0.02, 0.0)


def per_query_masks(rng, n, nq):
    """query i: a random filter of selectivity PER_QUERY_SELECTIVITY[i % 5]"""
    return np.stack([rng.random(n) < PER_QUERY_SELECTIVITY[i % 5] for i in range(nq)])


def words(mask):
    """a bitmap's u32 words, the bits at positions >= n of the last word set to garbage"""
    return efm.words(mask, garbage_past_n=True)
