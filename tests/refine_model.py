"""Refined search, as include/granne_hip.h defines it, in Python over the CPU oracle (test infrastructure):

    refine(R, q, cand, k)  = the candidates that R holds, each with d = R.dist_to_element(id, q) (oracle.dist), sorted
                             ascending by (distance bits, id), the first min(k, kept) of them;
    search_refined(W, R, ...) = refine(R, qR, W.search(qW, max_search, m), k)   (oracle.Index.search_batch).

A caller's list may name an id twice: both entries stay, in list order."""
import numpy as np

U64_MAX = np.iinfo(np.uint64).max


def refine(orc, rows, queries, cand, counts, k):
    """rows: R's elements [n, dim]; queries [nq, dim] prepared in R's dtype; cand [nq, m] u64; counts [nq] or None (all m).
    Returns ids [nq, k] u64 (UINT64_MAX padded), dists [nq, k] f32 (+inf padded), counts [nq] u32, dropped (int)."""
    cand = np.asarray(cand, np.uint64)
    nq, m = cand.shape
    n = len(rows)
    ids = np.full((nq, k), U64_MAX, np.uint64)
    ds = np.full((nq, k), np.inf, np.float32)
    out_c = np.zeros(nq, np.uint32)
    dropped = 0
    for q in range(nq):
        c = m if counts is None else min(int(counts[q]), m)
        keys = []
        for pos in range(c):
            i = int(cand[q, pos])
            if i >= n:
                dropped += 1
                continue
            d = np.float32(orc.dist(rows[i], queries[q]))
            keys.append((int(d.view(np.uint32)), i, pos, d))
        keys.sort(key=lambda t: t[:3])
        keys = keys[:k]
        out_c[q] = len(keys)
        for r, (_, i, _, d) in enumerate(keys):
            ids[q, r], ds[q, r] = i, d
    return ids, ds, out_c, dropped


def search_refined(orc, walk_index, rows, walk_queries, refine_queries, max_search, m, k):
    """walk_index: oracle.Index (W); rows: R's elements. Returns refine(...)'s tuple and the walk's counters [nq, 3]."""
    cand, _, cnt, ctr = walk_index.search_batch(walk_queries, max_search, m)
    return refine(orc, rows, refine_queries, cand, cnt, k) + (ctr,)
