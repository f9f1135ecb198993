"""Refined search: walk one index, re-rank the walk's candidates by another index's rows.

`RefinedGranne(walk, refine)` pairs two `Granne` handles over the SAME elements under the same ids -- typically int8 rows
with their graph (a quarter of the bytes per walk) and the f32 rows -- or their "angular_f16" copy, half the bytes to keep
and to read -- which need no graph (`layers=[]`). A search walks
`walk` with num_neighbors = refine_from, gives every candidate its distance under `refine`'s own arithmetic and returns
the k best by (distance, id): f32 distances and f32 order for about a tenth more traffic than the int8 walk
(granne_hip_search_refined_batch*, include/granne_hip.h).

`refine` may also be a `SumEmbeddings` CONTAINER: every candidate's f32 vector is then made from its terms inside the
re-rank kernel (granne_hip_search_refined_sum_embeddings_batch*), the distances are the container's own, bit for bit those
of its materialised index, and no dense f32 rows are held: the int8 rows to walk come from `SumEmbeddings.to_rows`."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .embeddings import SumEmbeddings
from .index import DEFAULT_MAX_SEARCH, DEFAULT_NUM_ELEMENTS, EMBEDDINGS, _is_term_lists, _p, normalize, quantize

MAX_REFINE_FROM = 1024


class RefinedGranne:
    def __init__(self, walk, refine):
        """walk: the Granne whose graph is walked (any kind); refine: a dense Granne on the same device whose rows
        re-rank (it may have been made with layers=[]) -- or a SumEmbeddings container, whose term sums re-rank. Both
        handles are borrowed: keep them open."""
        if walk.device != refine.device:
            raise ValueError("the two indexes must live on one device")
        self.walk, self.refine, self.device = walk, refine, walk.device
        self._container = isinstance(refine, SumEmbeddings)
        L = lib()
        self._batch = L.granne_hip_search_refined_sum_embeddings_batch if self._container else L.granne_hip_search_refined_batch
        self._batch_device = (L.granne_hip_search_refined_sum_embeddings_batch_device if self._container
                              else L.granne_hip_search_refined_batch_device)

    def _prepare(self, elements, prepared):
        """Queries for both indexes. prepared=True: a pair (walk queries, refine queries), each in its index's dtype and
        width. prepared=False: raw float rows -- one array when both indexes have its width, else a pair -- which are
        normalised, and for an int8 index the normalised rows are then quantised, on the device. With a container as
        the refine side they may also be term lists (one sequence of term ids per query), which are embedded and
        normalised through the container first."""
        if not prepared and self._container and _is_term_lists(elements):
            rows = self.refine.create_embeddings(elements, normalized=True)
            return (rows if self.walk.query_dtype == np.float32 else quantize(rows, self.device)), rows
        if prepared:
            qw, qr = elements
            return (np.ascontiguousarray(qw, dtype=self.walk.query_dtype), np.ascontiguousarray(qr, dtype=self.refine.query_dtype))
        raw = elements if isinstance(elements, (tuple, list)) and len(elements) == 2 and np.ndim(elements[0]) == 2 else (elements, elements)
        out = []
        for ix, rows in zip((self.walk, self.refine), raw):
            if getattr(ix, "element_type", None) == EMBEDDINGS:
                out.append(ix._prepare(rows, False))
                continue
            rows = normalize(np.atleast_2d(np.asarray(rows, np.float32)), self.device)
            out.append(rows if ix.query_dtype == np.float32 else quantize(rows, self.device))
        return tuple(out)

    def search_batch(self, elements, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS, refine_from=None,
                     prepared=True, stats=False, dropped=False):
        """nq refined searches. refine_from=None means max_search (at most 1024). Returns ids [nq, k] uint64, dists
        [nq, k] float32 (the refine index's), counts [nq] uint32; with stats=True the walk's [nq, 3] counters, with
        dropped=True the number of candidates the refine index does not hold."""
        qw, qr = self._prepare(elements, prepared)
        if qw.ndim != 2 or qw.shape[1] != self.walk.dim or qr.ndim != 2 or qr.shape[1] != self.refine.dim or qw.shape[0] != qr.shape[0]:
            raise ValueError("queries must be [nq, %d] for the walk and [nq, %d] for the re-rank" % (self.walk.dim, self.refine.dim))
        nq, k = qw.shape[0], int(num_elements)
        m = int(max_search) if refine_from is None else int(refine_from)
        ids = np.empty((nq, max(k, 0)), np.uint64)
        dists = np.empty((nq, max(k, 0)), np.float32)
        counts = np.zeros(nq, np.uint32)
        st = np.zeros((nq, 3), np.uint64)
        rs = C.c_uint32(0)
        check(self._batch(self.walk._h, self.refine._h, _p(qw), _p(qr), nq, int(max_search), m, k, _p(ids), _p(dists), _p(counts),
                          _p(st), C.byref(rs)))
        res = (ids, dists, counts)
        if stats:
            res += (st,)
        if dropped:
            res += (int(rs.value),)
        return res

    def search(self, element, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS, refine_from=None, prepared=True):
        """One query: [(id, distance)] ascending by (distance, id) under the refine index. `element` as in search_batch,
        one row (or one pair of rows)."""
        pair = isinstance(element, (tuple, list)) and len(element) == 2 and np.ndim(element[0]) >= 1
        one = tuple(np.asarray(e).reshape(1, -1) for e in element) if pair else np.asarray(element).reshape(1, -1)
        ids, dists, counts = self.search_batch(one, max_search, num_elements, refine_from, prepared)
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    def search_batch_device(self, d_walk_queries, d_refine_queries, nq, max_search, refine_from, num_elements, d_ids, d_dists,
                            d_counts, d_stats=0, d_status=0, d_refine_status=0, stream=0):
        """Device-resident, asynchronous variant: every argument is a raw device pointer (int)."""
        check(self._batch_device(
            self.walk._h, self.refine._h, C.c_void_p(d_walk_queries), C.c_void_p(d_refine_queries), int(nq), int(max_search),
            int(refine_from), int(num_elements), C.c_void_p(d_ids), C.c_void_p(d_dists), C.c_void_p(d_counts),
            C.c_void_p(d_stats), C.c_void_p(d_status), C.c_void_p(d_refine_status), C.c_void_p(stream)))
