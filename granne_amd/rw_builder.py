"""RwGranneBuilder on the GPU: the builder that takes inserts while it answers searches
(src/index/rw/mod.rs:15-224) on top of granne_hip_rw_builder_* (include/granne_hip.h)."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import check, lib
from .index import DEFAULT_MAX_SEARCH, DEFAULT_NUM_ELEMENTS, Granne, _p, normalize, quantize


class RwGranneBuilder:
    def __init__(self, builder, max_elements, dim=None, prepared=True):
        """RwGranneBuilder::new(builder, max_elements, _) (rw/mod.rs:32-61). `builder` is a granne_amd.GranneBuilder over
        dense rows ("angular" / "angular_int"); it is built over all its elements and CLOSED by this call -- the new
        object owns what it held. A builder that has no element yet has no dimension either: give `dim`, or the first
        inserted row decides. prepared=False applies Vector::from to inserted rows and queries, as on GranneBuilder."""
        self.element_type = builder.element_type
        self.dtype_code, self.np_dtype = builder.dtype_code, builder.np_dtype
        self.device = builder.device
        self.config = builder.config
        self.max_elements = int(max_elements)
        self._prepared = prepared
        self._h = None
        self._builder = builder
        self.dim = builder.dim if builder.dim is not None else dim
        if self.dim is not None:
            self._create()

    def _create(self):
        b = self._builder
        if b.dim is None:
            b.dim = self.dim
        b._ensure()
        h = C.c_void_p()
        check(lib().granne_hip_rw_builder_create(C.byref(h), b._h, self.max_elements))
        b._h = None  # consumed: the handle is ours now
        self._builder = None
        self._h = h

    def _handle(self):
        if self._h is None:
            if self._builder is None:
                raise ValueError("the RwGranneBuilder is closed")
            raise ValueError("the dimension is not known yet: pass dim=, or insert an element first")
        return self._h

    def _prep(self, rows):
        if self._prepared:
            return np.ascontiguousarray(rows, dtype=self.np_dtype)
        return normalize(rows, self.device) if self.element_type == "angular" else quantize(rows, self.device)

    # ---- insert (rw/mod.rs:99-182) ----------------------------------------------------------------
    def insert_batch(self, rows):
        """The ids the rows got, in order (fewer than rows once max_elements is reached): np.ndarray of uint64."""
        rows = np.asarray(rows)
        if rows.ndim != 2:
            raise ValueError("rows must be [n, dim]")
        if self._h is None and self._builder is not None and self.dim is None:
            self.dim = rows.shape[1]
            self._create()
        if rows.shape[1] != self.dim:
            raise ValueError("rows must be [n, %d]" % self.dim)
        rows = self._prep(rows)
        ids = np.empty(rows.shape[0], np.uint64)
        count = C.c_uint64(0)
        check(lib().granne_hip_rw_builder_insert_batch(self._handle(), _p(rows), rows.shape[0], _p(ids), C.byref(count)))
        return ids[: count.value].copy()

    def insert(self, element):
        """The element's id, or None when the builder is full."""
        ids = self.insert_batch(np.asarray(element).reshape(1, -1))
        return int(ids[0]) if len(ids) else None

    # ---- search (rw/mod.rs:184-207) ---------------------------------------------------------------
    def search_batch(self, elements, max_search=DEFAULT_MAX_SEARCH, num_neighbors=DEFAULT_NUM_ELEMENTS, stats=False):
        """ids [nq,k] uint64, dists [nq,k] float32, counts [nq] uint32 (and stats [nq,3] uint64 = n_dist, n_expand, n_adj
        when stats=True). Without a previous layer every result is empty (the reference's behaviour, rw/mod.rs:198-206).
        Removed elements are never returned (`remove`)."""
        q = np.asarray(elements)
        if q.ndim != 2 or (self.dim is not None and q.shape[1] != self.dim):
            raise ValueError("queries must be [nq, %s]" % self.dim)
        nq, k = q.shape[0], int(num_neighbors)
        ids = np.full((nq, max(k, 0)), np.iinfo(np.uint64).max, np.uint64)
        dists = np.full((nq, max(k, 0)), np.inf, np.float32)
        counts = np.zeros(nq, np.uint32)
        st = np.zeros((nq, 3), np.uint64)
        if self._h is None and self._builder is not None:  # nothing inserted, no dimension yet: empty
            return (ids, dists, counts, st) if stats else (ids, dists, counts)
        q = self._prep(q)
        check(lib().granne_hip_rw_builder_search_batch(self._handle(), _p(q), nq, int(max_search), k, _p(ids), _p(dists),
                                                       _p(counts), _p(st) if stats else None))
        return (ids, dists, counts, st) if stats else (ids, dists, counts)

    def search(self, query, max_search=DEFAULT_MAX_SEARCH, num_neighbors=DEFAULT_NUM_ELEMENTS):
        ids, dists, counts = self.search_batch(np.asarray(query).reshape(1, -1), max_search, num_neighbors)
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    # ---- tombstones (include/granne_hip.h, "removing elements") -------------------
    def _mark(self, fn, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        counts = np.zeros(3, np.uint64)
        check(fn(self._handle(), _p(ids) if ids.size else None, ids.size, _p(counts)))
        return int(counts[0]), int(counts[1]), int(counts[2])

    def remove(self, ids):
        """Marks the elements removed: searches never return them again, the graph keeps them (they are traversed, and
        inserts may link to them), their slots are not reused. Returns (newly removed, removed already -- repeats within
        `ids` included --, ids >= len(self), which are ignored)."""
        return self._mark(lib().granne_hip_rw_builder_remove, ids)

    def restore(self, ids):
        """The inverse of `remove`: (newly restored, alive already, ids >= len(self))."""
        return self._mark(lib().granne_hip_rw_builder_restore, ids)

    def removed_count(self):
        return int(lib().granne_hip_rw_builder_removed_count(self._handle()))

    def alive_filter(self):
        """A granne_amd.Filter over the len(self) ids with the bits of the elements that are not removed: a copy, for
        `search_filtered` / `exact_topk_filtered` on a `get_index()` snapshot taken with no insert in between. `save`
        and `get_index` know nothing of removals: keep `alive_filter().words()` beside the files, or `compact` first."""
        from .filters import Filter
        h, n = self._handle(), len(self)
        f = Filter(max(self.max_elements, n), self.device)  # (room for whatever a concurrent insert adds)
        f.n = n
        check(lib().granne_hip_rw_builder_alive(h, C.c_void_p(f.ptr), None))
        check(lib().granne_hip_stream_synchronize(None, self.device))
        return f

    def compact(self, max_elements=None):
        """(a new RwGranneBuilder over the elements that are not removed, in ascending old-id order and built afresh
        under this one's config; old_ids [len(new)] uint64 with old_ids[new_id] = the element's id here). This handle
        is left as it is. max_elements: the new handle's (default: this one's)."""
        h = self._handle()
        max_elements = self.max_elements if max_elements is None else int(max_elements)
        old = np.empty(max(self.max_elements, len(self)), np.uint64)
        count, out = C.c_uint64(0), C.c_void_p()
        check(lib().granne_hip_rw_builder_compact(h, max_elements, C.byref(out), _p(old), C.byref(count)))
        new = RwGranneBuilder.__new__(RwGranneBuilder)
        new.element_type, new.dtype_code, new.np_dtype = self.element_type, self.dtype_code, self.np_dtype
        new.device, new.config, new.dim = self.device, self.config, self.dim
        new.max_elements, new._prepared = max_elements, self._prepared
        new._h, new._builder = out, None
        return new, old[: count.value].copy()

    # ---- accessors --------------------------------------------------------------------------------
    def __len__(self):
        return int(lib().granne_hip_rw_builder_len(self._h)) if self._h is not None else 0

    def num_layers(self):
        return int(lib().granne_hip_rw_builder_num_layers(self._handle()))

    def layer_len(self, layer):
        return int(lib().granne_hip_rw_builder_layer_len(self._handle(), layer))

    def get_layer(self, layer):
        """[layer_len, num_neighbors] uint32, UNUSED padded; the current (last) layer has len(self) rows."""
        out = np.empty((self.layer_len(layer), self.config.num_neighbors), np.uint32)
        check(lib().granne_hip_rw_builder_get_layer(self._handle(), layer, _p(out)))
        return out

    def layers(self):
        """Previous layers followed by the current one."""
        return [self.get_layer(l) for l in range(self.num_layers())]

    def get_element(self, idx):
        out = np.empty(self.dim, self.np_dtype)
        check(lib().granne_hip_rw_builder_get_element(self._handle(), int(idx), _p(out)))
        return out

    def get_index(self):
        """A static granne_amd.Granne snapshot of the graph as it is now."""
        h = C.c_void_p()
        check(lib().granne_hip_rw_builder_get_index(self._handle(), C.byref(h)))
        ix = Granne.__new__(Granne)
        ix._se, ix.compact = None, False
        ix.element_type = self.element_type
        ix.dtype_code, ix.np_dtype = self.dtype_code, self.np_dtype
        ix.device = self.device
        ix._h = h
        ix.dim = self.dim
        return ix

    def save(self, index_path, elements_path):
        """save_index_and_elements_to_disk (rw/mod.rs:63-68)."""
        check(lib().granne_hip_rw_builder_save(self._handle(), os.fsencode(index_path), os.fsencode(elements_path)))

    def set_option(self, option, value):
        check(lib().granne_hip_rw_builder_set_option(self._handle(), int(option), int(value)))

    def get_option(self, option):
        v = C.c_uint64(0)
        check(lib().granne_hip_rw_builder_get_option(self._handle(), int(option), C.byref(v)))
        return int(v.value)

    def close(self):
        if getattr(self, "_h", None):
            lib().granne_hip_rw_builder_destroy(self._h)
        self._h = None
        self._builder = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SMALL_OPS = _lib.RW_OPT_SMALL_OPS
SMALL_LAUNCHES = _lib.RW_OPT_SMALL_LAUNCHES
SORTED_LAUNCHES = _lib.RW_OPT_SORTED_LAUNCHES
REMOVED = _lib.RW_OPT_REMOVED
FILTERED_SEARCHES = _lib.RW_OPT_FILTERED_SEARCHES
