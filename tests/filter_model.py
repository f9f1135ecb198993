"""The model of filtered search (TEST INFRASTRUCTURE): the reference's search_for_neighbors (src/index/mod.rs:999-1037)
with the two changes include/granne_hip.h states -- only allowed ids enter `res`, and max_expand caps the bottom layer's
pops -- in plain Python over oracle/pyref.py (imported, not edited): its get_neighbors, its dist, and its own
search_for_neighbors for find_entrypoint (the upper layers are unfiltered).

    while let Some((d, idx)) = pq.pop():
        if res.is_full() && d > res.peek().0: break
        if n_expanded == max_expand && max_expand != 0: break      # NEW
        if allowed(idx): res.push((d, idx))                        # NEW
        n_expanded += 1
        for n in get_neighbors(idx): ...                           # unchanged: disallowed nodes are traversed

`dist_row`: optionally the distances of the query to EVERY element, as float32 (a test that has them from elsewhere --
the GPU tests take them from the library's Dist operator, checked against pyref on a sample -- saves the per-pair fmaf
loops); the walk's logic is this file's either way."""
import heapq

import numpy as np

from oracle import pyref


class Result:
    """ids (list of int), dists (list of np.float32), count, counters {n_dist, n_expand, n_adj}, cut (max_expand ended the walk)."""

    def __init__(self, pairs, counters, cut):
        self.ids = [int(i) for i, _ in pairs]
        self.dists = [np.float32(d) for _, d in pairs]
        self.count = len(pairs)
        self.counters = dict(counters)
        self.cut = bool(cut)

    def dist_bits(self):
        return [int(np.float32(d).view(np.uint32)) for d in self.dists]

    def padded(self, k):
        """The row a search entry writes: ids [k] u64 (unused = UINT64_MAX), dists [k] f32 (unused = +inf)."""
        ids = np.full(k, np.iinfo(np.uint64).max, np.uint64)
        ds = np.full(k, np.inf, np.float32)
        ids[:self.count] = self.ids
        ds[:self.count] = self.dists
        return ids, ds


class Neighbors:
    """pyref.get_neighbors(layer, idx), remembered per node: 256 queries walk the same rows."""

    def __init__(self, layer):
        self.layer, self.rows = layer, {}

    def __call__(self, idx):
        r = self.rows.get(idx)
        if r is None:
            r = self.rows[idx] = pyref.get_neighbors(self.layer, idx)
        return r


def _layer_walk(neighbors, entrypoint, dist_of, max_search, allowed, max_expand, counters):
    """One layer. allowed: None (unfiltered) or a bool sequence over ids. Returns ([(id, dist)] ascending, cut)."""
    res = []  # max-heap via negated keys
    pq = []
    visited = bytearray(len(neighbors.layer))  # HashSet<usize> over the layer's ids
    visited[entrypoint] = 1
    push, pop, replace = heapq.heappush, heapq.heappop, heapq.heapreplace

    d0 = dist_of(entrypoint)
    n_dist = 1
    push(pq, (d0, entrypoint))
    n_expanded, n_adj, cut = 0, 0, False
    while pq:
        d, idx = pq[0]
        full = len(res) >= max_search
        if full and d > -res[0][0]:
            break
        if max_expand != 0 and n_expanded == max_expand:
            cut = True
            break
        pop(pq)
        if allowed is None or allowed[idx]:
            if not full:
                push(res, (-d, -idx))
            elif (d, idx) < (-res[0][0], -res[0][1]):
                replace(res, (-d, -idx))
        n_expanded += 1
        nbrs = neighbors(idx)
        n_adj += len(nbrs)
        full = len(res) >= max_search  # `res` is frozen during an expansion
        worst = -res[0][0] if full else 0.0
        for n in nbrs:
            if not visited[n]:
                visited[n] = 1
                dn = dist_of(n)
                n_dist += 1
                if (not full) or dn < worst:
                    push(pq, (dn, n))
    counters["n_dist"] += n_dist
    counters["n_expand"] += n_expanded
    counters["n_adj"] += n_adj
    out = sorted((-a, -b) for a, b in res)
    return [(i, d) for d, i in out], cut


def _neighbors_of(layers, cache):
    if cache is None:
        return [Neighbors(l) for l in layers]
    if not cache:
        cache.extend(Neighbors(l) for l in layers)
    return cache


def search_filtered(layers, elements, query, allowed, max_search, num_neighbors, max_expand=0, dist_row=None, cache=None):
    """Granne::search (src/index/mod.rs:140-150, 963-997) under the filter. allowed: bool array over the ids (entries
    beyond it never matter: a walk meets node ids only). cache: an empty list a caller keeps per index (the neighbor
    lists, remembered). Returns a Result."""
    if max_search == 0:
        raise RuntimeError("panic: res.peek().unwrap() on empty heap (src/index/mod.rs:1019)")
    counters = {"n_dist": 0, "n_expand": 0, "n_adj": 0}
    if not len(layers):
        return Result([], counters, False)
    allowed = np.asarray(allowed, bool).tolist()
    if dist_row is None:
        def dist_of(i):
            return float(pyref.dist(elements[i], query))
    else:
        dist_of = np.asarray(dist_row, np.float32).tolist().__getitem__  # (a float32 as a Python float: exact)
    nb = _neighbors_of(layers, cache)
    entrypoint = 0
    for l, layer in enumerate(layers[:-1]):  # find_entrypoint: unchanged, unfiltered
        if dist_row is None:
            entrypoint = pyref.search_for_neighbors(layer, entrypoint, elements, query, 1, counters)[0][0]
        else:
            entrypoint = _layer_walk(nb[l], entrypoint, dist_of, 1, None, 0, counters)[0][0][0]
    pairs, cut = _layer_walk(nb[len(layers) - 1], entrypoint, dist_of, max_search, allowed, max_expand, counters)
    return Result(pairs[:num_neighbors], counters, cut)


def bottom_entrypoint(layers, elements, query, dist_row=None, cache=None):
    """The node the bottom layer's walk starts from (what find_entrypoint returns)."""
    counters = {"n_dist": 0, "n_expand": 0, "n_adj": 0}
    dist_of = (lambda i: float(pyref.dist(elements[i], query))) if dist_row is None else np.asarray(dist_row, np.float32).tolist().__getitem__
    nb = _neighbors_of(layers, cache)
    ep = 0
    for l in range(len(layers) - 1):
        ep = _layer_walk(nb[l], ep, dist_of, 1, None, 0, counters)[0][0][0]
    return ep


def pack_bits(allowed):
    """The bitmap's u32 words: bit (id & 31) of word (id >> 5)."""
    a = np.asarray(allowed, bool)
    words = np.zeros((a.size + 31) // 32, np.uint32)
    ids = np.nonzero(a)[0]
    np.bitwise_or.at(words, ids >> 5, (np.uint32(1) << (ids & 31).astype(np.uint32)))
    return words
