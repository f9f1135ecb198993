"""Host-side mirror of the reference's search interface over libgranne_hip.so.

`Granne` follows the reference's Python class (py/src/lib.rs:149-344) -- search, get_element,
get_neighbors, __len__, num_layers, layer_len -- and the Rust `Granne` it wraps
(src/index/mod.rs:106-185), with `search_batch` added (the reference has no batch API; its
callers loop or par_iter over `search`). Elements are prepared like the reference does it:
`normalize` = angular::Vector::from (src/elements/angular.rs:55-61), `quantize` =
angular_int::Vector::from (src/elements/angular_int.rs:19-45), both executed on the device.
"""
import ctypes as C
import os

import numpy as np

from ._lib import ERR_INVALID, ERR_OVERFLOW, EXACT_TOPK_CAP, F16, F32, I8, RANGE_CAP_MAX, GranneHipError, check, lib

DEFAULT_MAX_SEARCH = 200   # py/src/lib.rs:14
DEFAULT_NUM_ELEMENTS = 10  # py/src/lib.rs:15
# search_range_batch's list lengths: of the ascending subsets of the register walkers' list sizes 60 / 124 / 252 / 508 / 1020
# the cheapest whose recall was not below search_batch(1020, 1020)'s at any radius (tools/range_bench.py)
RANGE_DEFAULT_STAGES = (252, 1020)

# "angular_f16": rows of IEEE halves; the element a row stands for is Vector::from(widen(row)) -- normalised where it is
# read -- and queries are prepared float32 rows, as for "angular"
_ELEMENT_TYPES = {"angular": (F32, np.float32), "angular_int": (I8, np.int8), "angular_f16": (F16, np.float16)}
EMBEDDINGS = "embeddings"  # embeddings::SumEmbeddings: `elements` is a granne_amd.SumEmbeddings, vectors are f32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def normalize(rows, device=0):
    """angular::Vector::from for every row of `rows` (float32). Returns a new array."""
    a = np.array(rows, dtype=np.float32, order="C", copy=True)
    flat = a.reshape(1, -1) if a.ndim == 1 else a
    if flat.size:
        check(lib().granne_hip_normalize_f32(_p(flat), flat.shape[0], flat.shape[1], device))
    return a


def quantize(rows, device=0):
    """angular_int::Vector::from for every row of `rows` (float32 in, int8 out)."""
    a = np.ascontiguousarray(rows, dtype=np.float32)
    flat = a.reshape(1, -1) if a.ndim == 1 else a
    out = np.empty(flat.shape, np.int8)
    if flat.size:
        check(lib().granne_hip_quantize_f32(_p(flat), _p(out), flat.shape[0], flat.shape[1], device))
    return out.reshape(a.shape)


def to_f16(rows, prepared=True, device=0):
    """float32 rows -> the halves of an "angular_f16" container, rounded to nearest even on the device (the bits of
    astype(float16)). prepared=False normalises in float32 first (Vector::from), then rounds."""
    a = np.ascontiguousarray(rows, dtype=np.float32) if prepared else normalize(rows, device)
    flat = a.reshape(1, -1) if a.ndim == 1 else a
    out = np.empty(flat.shape, np.float16)
    if flat.size:
        check(lib().granne_hip_f32_to_f16(_p(flat), _p(out), flat.shape[0], flat.shape[1], device))
    return out.reshape(a.shape)


def from_f16(rows16, normalized=True, device=0):
    """The float32 rows the halves stand for: widened exactly and (normalized=True) passed through Vector::from -- what
    an "angular_f16" index computes its distances with."""
    a = np.ascontiguousarray(rows16, dtype=np.float16)
    flat = a.reshape(1, -1) if a.ndim == 1 else a
    out = np.empty(flat.shape, np.float32)
    if flat.size:
        check(lib().granne_hip_f16_to_f32(_p(flat), _p(out), flat.shape[0], flat.shape[1], int(bool(normalized)), device))
    return out.reshape(a.shape)


def _prepare_elements(et, elements, device):
    """Vector::from for raw float rows of a dense element type."""
    if et == "angular":
        return normalize(elements, device)
    if et == "angular_f16":
        return to_f16(elements, prepared=False, device=device)
    return quantize(elements, device)


def _is_term_lists(x):
    """A batch of queries for an "embeddings" index: sequences of term ids (True) or float rows (False)."""
    if isinstance(x, np.ndarray):
        return x.dtype.kind in "iu"
    for t in x:
        a = np.asarray(t)
        if a.size:
            return a.dtype.kind in "iu"
    return True  # nothing but empty lists


class Granne:
    """An HNSW index resident in the HBM of one MI355X."""

    def __init__(self, element_type, elements, layers, device=0, prepared=True, compact=False, coalesce=False):
        """element_type: "angular" (f32), "angular_int" (int8), "angular_f16" (halves, searched with f32 queries) or "embeddings" (`elements` is a SumEmbeddings; with
        compact=True the index keeps the container instead of dense rows and makes vectors as it walks).
        coalesce=True: concurrent `search` calls of host threads share launches (the `coalesce` property).
        elements: [n, dim] array. With prepared=True (default) rows are taken as stored in a
        Vectors file (already normalised / quantised); with prepared=False raw float rows go
        through Vector::from first.
        layers: list of [layer_len, width] uint32 arrays (UNUSED padded), top layer first --
        what GranneBuilder::get_index hands to Granne (src/index/mod.rs:483-488)."""
        et = element_type.lower()
        if et == EMBEDDINGS:
            self._init_embeddings(elements, layers, compact)
            if coalesce:
                self.coalesce = True
            return
        if et not in _ELEMENT_TYPES:
            raise ValueError("Invalid element type")  # the reference panics (py/src/lib.rs:210)
        self.element_type = et
        self.dtype_code, self.np_dtype = _ELEMENT_TYPES[et]
        self.device = device
        if not prepared:
            elements = _prepare_elements(et, elements, device)
        el = np.ascontiguousarray(elements, dtype=self.np_dtype)
        if el.ndim != 2:
            raise ValueError("elements must be [n, dim]")
        layers = [np.ascontiguousarray(l, dtype=np.uint32) for l in layers]
        n = len(layers)
        lens = (C.c_uint64 * max(n, 1))(*[l.shape[0] for l in layers])
        widths = (C.c_uint32 * max(n, 1))(*[l.shape[1] for l in layers])
        rows = (C.c_void_p * max(n, 1))(*[l.ctypes.data for l in layers])
        h = C.c_void_p()
        check(lib().granne_hip_index_create(C.byref(h), _p(el), el.shape[0], el.shape[1], self.dtype_code, n, lens,
                                            rows, widths, device))
        self._h = h
        self.dim = el.shape[1]
        if coalesce:
            self.coalesce = True

    def _init_embeddings(self, se, layers, compact):
        self.element_type = EMBEDDINGS
        self.dtype_code, self.np_dtype = F32, np.float32
        self.device, self.compact, self._se = se.device, bool(compact), se
        layers = [np.ascontiguousarray(l, dtype=np.uint32) for l in layers]
        n = len(layers)
        lens = (C.c_uint64 * max(n, 1))(*[l.shape[0] for l in layers])
        widths = (C.c_uint32 * max(n, 1))(*[l.shape[1] for l in layers])
        rows = (C.c_void_p * max(n, 1))(*[l.ctypes.data for l in layers])
        h = C.c_void_p()
        check(lib().granne_hip_index_create_sum_embeddings(C.byref(h), se._h, n, lens, rows, widths, int(bool(compact))))
        self._h = h
        self.dim = se.dim

    @classmethod
    def from_csr(cls, element_type, elements, offsets, ids, device=0):
        """From decoded on-disk layers: per layer (offsets[len+1] u64, ids u32)."""
        self = cls.__new__(cls)
        et = element_type.lower()
        if et not in _ELEMENT_TYPES:
            raise ValueError("Invalid element type")
        self.element_type = et
        self.dtype_code, self.np_dtype = _ELEMENT_TYPES[et]
        self.device = device
        el = np.ascontiguousarray(elements, dtype=self.np_dtype)
        offs = [np.ascontiguousarray(o, dtype=np.uint64) for o in offsets]
        idl = [np.ascontiguousarray(i, dtype=np.uint32) for i in ids]
        n = len(offs)
        lens = (C.c_uint64 * max(n, 1))(*[o.size - 1 for o in offs])
        po = (C.c_void_p * max(n, 1))(*[o.ctypes.data for o in offs])
        pi = (C.c_void_p * max(n, 1))(*[i.ctypes.data if i.size else None for i in idl])
        h = C.c_void_p()
        check(lib().granne_hip_index_create_csr(C.byref(h), _p(el), el.shape[0], el.shape[1], self.dtype_code, n,
                                                lens, po, pi, device))
        self._h = h
        self.dim = el.shape[1]
        return self

    @classmethod
    def from_files(cls, index_path, element_type, elements_path, device=0, embeddings_path=None, compact=False,
                   on_device=False, staging_bytes=None):
        """Granne(index_path, element_type, elements_path) of the reference's binding
        (py/src/lib.rs:177-214): an index file written by write_index + a Vectors file -- or, for "embeddings", an
        elements file of term lists + embeddings_path (the table), materialised or compact.
        on_device=True (dense element types): the files are read in pieces into a pinned ring of `staging_bytes` (None: the
        library's default) and decoded on the GPU; the index is the same, `last_codec_info` holds the call's info words."""
        self = cls.__new__(cls)
        et = element_type.lower()
        if et == EMBEDDINGS:
            from .embeddings import SumEmbeddings
            if embeddings_path is None:
                raise ValueError("embeddings_path is required")  # the reference panics (py/src/lib.rs:199-202)
            if on_device:
                raise ValueError("on_device reads dense element files; an \"embeddings\" index loads through the host codec")
            self.element_type = EMBEDDINGS
            self.dtype_code, self.np_dtype = F32, np.float32
            self.device, self.compact = device, bool(compact)
            self._se = SumEmbeddings.from_files(embeddings_path, elements_path, device)  # term-id queries embed through it
            h = C.c_void_p()
            check(lib().granne_hip_index_load_files_sum_embeddings(C.byref(h), os.fsencode(index_path), os.fsencode(embeddings_path),
                                                                   os.fsencode(elements_path), int(bool(compact)), device))
            self._h = h
            self.dim = int(lib().granne_hip_index_dim(h))
            return self
        if et not in _ELEMENT_TYPES:
            raise ValueError("Invalid element type")
        self.element_type = et
        self.dtype_code, self.np_dtype = _ELEMENT_TYPES[et]
        self.device = device
        h = C.c_void_p()
        if on_device:
            info = (C.c_uint64 * 4)()
            check(lib().granne_hip_index_load_files_on_device(C.byref(h), os.fsencode(index_path), os.fsencode(elements_path),
                                                              self.dtype_code, device, int(staging_bytes or 0), info))
            self.last_codec_info = tuple(int(v) for v in info)
        else:
            check(lib().granne_hip_index_load_files(C.byref(h), os.fsencode(index_path), os.fsencode(elements_path),
                                                    self.dtype_code, device))
        self._h = h
        self.dim = int(lib().granne_hip_index_dim(h))
        return self

    @classmethod
    def from_bytes(cls, index_bytes, element_type, elements_bytes, device=0, on_device=False, staging_bytes=None):
        """Granne::from_bytes (src/index/mod.rs:106-113) over Vectors::from_bytes. on_device=True: decoded by the device
        codec (see from_files)."""
        self = cls.__new__(cls)
        et = element_type.lower()
        if et not in _ELEMENT_TYPES:
            raise ValueError("Invalid element type")
        self.element_type = et
        self.dtype_code, self.np_dtype = _ELEMENT_TYPES[et]
        self.device = device
        ib = np.frombuffer(index_bytes, np.uint8)
        eb = np.frombuffer(elements_bytes, np.uint8)
        h = C.c_void_p()
        if on_device:
            info = (C.c_uint64 * 4)()
            check(lib().granne_hip_index_load_on_device(C.byref(h), _p(ib), ib.size, _p(eb), eb.size, self.dtype_code, device,
                                                        int(staging_bytes or 0), info))
            self.last_codec_info = tuple(int(v) for v in info)
        else:
            check(lib().granne_hip_index_load(C.byref(h), _p(ib), ib.size, _p(eb), eb.size, self.dtype_code, device))
        self._h = h
        self.dim = int(lib().granne_hip_index_dim(h))
        return self

    # the four info words of the last on-device codec call of this object (include/granne_hip.h: layers through the device
    # codec, layers through the host codec, peak device scratch bytes, peak host staging bytes), or None
    last_codec_info = None

    def _save(self, index_path, elements_path, on_device, staging_bytes):
        ip = os.fsencode(index_path) if index_path is not None else None
        ep = os.fsencode(elements_path) if elements_path is not None else None
        if not on_device:
            check(lib().granne_hip_index_save(self._h, ip, ep))
            return
        info = (C.c_uint64 * 4)()
        try:
            check(lib().granne_hip_index_save_on_device(self._h, ip, ep, int(staging_bytes or 0), info))
        finally:
            self.last_codec_info = tuple(int(v) for v in info)

    def save_index(self, path, on_device=False, staging_bytes=None):
        """py/src/lib.rs:318-330. on_device=True: encoded by the device codec and streamed through a pinned ring of
        `staging_bytes` (None: the library's default); the file's bytes are the same."""
        self._save(path, None, on_device, staging_bytes)

    def index_bytes(self, on_device=False, staging_bytes=None):
        """Index::write_index into a buffer (src/index/mod.rs:67-70): the bytes of the index file."""
        out, n = C.c_void_p(), C.c_uint64(0)
        if on_device:
            info = (C.c_uint64 * 4)()
            check(lib().granne_hip_index_encode_on_device(self._h, int(staging_bytes or 0), C.byref(out), C.byref(n), info))
            self.last_codec_info = tuple(int(v) for v in info)
        else:
            check(lib().granne_hip_index_encode(self._h, C.byref(out), C.byref(n)))
        try:
            return C.string_at(out, n.value)
        finally:
            lib().granne_hip_bytes_free(out)

    def save_elements(self, path, on_device=False, staging_bytes=None):
        """py/src/lib.rs:332-343."""
        self._save(None, path, on_device, staging_bytes)

    def save(self, index_path, elements_path, on_device=False, staging_bytes=None):
        """save_index and save_elements in one call."""
        self._save(index_path, elements_path, on_device, staging_bytes)

    @classmethod
    def from_device(cls, element_type, d_elements_ptr, n_elements, dim, layer_lens, d_layer_ptrs, layer_widths,
                    device=0, stream=0):
        """Elements and fixed-width layers already in device memory (raw pointers)."""
        self = cls.__new__(cls)
        et = element_type.lower()
        self.element_type = et
        self.dtype_code, self.np_dtype = _ELEMENT_TYPES[et]
        self.device = device
        n = len(layer_lens)
        lens = (C.c_uint64 * max(n, 1))(*layer_lens)
        widths = (C.c_uint32 * max(n, 1))(*layer_widths)
        rows = (C.c_void_p * max(n, 1))(*d_layer_ptrs)
        h = C.c_void_p()
        check(lib().granne_hip_index_create_device(C.byref(h), C.c_void_p(d_elements_ptr), n_elements, dim,
                                                   self.dtype_code, n, lens, rows, widths, device,
                                                   C.c_void_p(stream)))
        self._h = h
        self.dim = dim
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().granne_hip_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def query_dtype(self):
        """numpy dtype of a prepared query: the elements', except that rows of halves take float32 queries."""
        return np.float32 if self.dtype_code == F16 else self.np_dtype

    # ---- Index trait (src/index/mod.rs:54-71) --------------------------------------------------
    def __len__(self):
        return int(lib().granne_hip_index_len(self._h))

    def num_layers(self):
        return int(lib().granne_hip_index_num_layers(self._h))

    def layer_len(self, layer):
        return int(lib().granne_hip_index_layer_len(self._h, layer))

    def get_neighbors(self, idx, layer=None):
        if layer is None:
            layer = self.num_layers() - 1
        buf = np.empty(512, np.uint32)
        n = C.c_uint32()
        check(lib().granne_hip_index_get_neighbors(self._h, idx, layer, _p(buf), buf.size, C.byref(n)))
        return buf[: n.value].astype(np.int64).tolist()

    def get_element(self, idx):
        out = np.empty(self.dim, self.np_dtype)
        check(lib().granne_hip_index_get_element(self._h, idx, _p(out)))
        return out

    def hbm_bytes(self):
        return int(lib().granne_hip_index_hbm_bytes(self._h))

    def get_sketch(self, first=0, count=None):
        """The row sketches of OPT_SKETCH (uint8 [count][128]), or None when the index holds none."""
        count = len(self) - first if count is None else count
        out = np.empty((count, 128), np.uint8)
        if lib().granne_hip_index_get_sketch(self._h, first, count, _p(out)) != 0:
            return None
        return out

    # ---- reorder (src/index/reorder.rs) --------------------------------------------------------------
    def reorder(self):
        """Granne::reorder: places similar elements closer together, in place. Returns the permutation
        (uint64): permutation[i] == j means the element with idx j has been moved to idx i."""
        order = np.empty(len(self), np.uint64)
        check(lib().granne_hip_index_reorder(self._h, _p(order)))
        return order

    def reorder_by_keys(self, keys):
        """Granne::reorder_by_keys: layer-preserving sort by (key, idx); keys are u64."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        if k.shape != (len(self),):
            raise ValueError("need one key per element")  # assert_eq!(self.len(), keys.len()), reorder.rs:91
        order = np.empty(len(self), np.uint64)
        check(lib().granne_hip_index_reorder_by_keys(self._h, _p(k), _p(order)))
        return order

    # ---- options --------------------------------------------------------------------------------
    def set_option(self, option, value):
        check(lib().granne_hip_index_set_option(self._h, option, value))

    def get_option(self, option):
        import ctypes as C
        v = C.c_uint64(0)
        check(lib().granne_hip_index_get_option(self._h, option, C.byref(v)))
        return int(v.value)

    def last_slow_count(self):
        """Queries of the last host search_batch that the exact walker served; after reorder(), done or failed, the trail
        walks handed over, summed over its trail launches."""
        return int(lib().granne_hip_index_last_slow_count(self._h))

    @property
    def coalesce(self):
        """OPT_COALESCE: `search` / `search_batch` calls of up to 64 queries that host threads make at the same moment
        share search launches (the reference's par_iter over Granne::search). Off by default; results do not depend on
        it. It gains nothing for one thread or for a caller that already batches."""
        from ._lib import OPT_COALESCE
        return bool(self.get_option(OPT_COALESCE))

    @coalesce.setter
    def coalesce(self, on):
        from ._lib import OPT_COALESCE
        self.set_option(OPT_COALESCE, 1 if on else 0)

    # ---- search -----------------------------------------------------------------------------------
    def _prepare(self, element, prepared):
        if self.element_type == EMBEDDINGS:
            # term-id lists are embedded and normalised on the device (py/src/lib.rs:260-268: create_embedding +
            # Vector::from); float rows are taken like "angular" queries
            if _is_term_lists(element):
                if getattr(self, "_se", None) is None:
                    raise ValueError("term-id queries need the index's SumEmbeddings container")
                return self._se.create_embeddings(element, normalized=True)
            return np.ascontiguousarray(element, np.float32) if prepared else normalize(element, self.device)
        if prepared:
            return np.ascontiguousarray(element, dtype=self.query_dtype)
        return quantize(element, self.device) if self.element_type == "angular_int" else normalize(element, self.device)

    def search(self, element, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS, prepared=True):
        """Granne.search (py/src/lib.rs:227-233): [(id, distance)] ascending by (distance, id).
        prepared=False applies Vector::from to `element` first, as the reference's binding does."""
        terms = self.element_type == EMBEDDINGS and (len(element) == 0 or np.asarray(element).dtype.kind in "iu")
        one = [list(element)] if terms else np.asarray(element).reshape(1, -1)
        ids, dists, counts = self.search_batch(one, max_search, num_elements, prepared)
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    def search_batch(self, elements, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS, prepared=True,
                     stats=False):
        """nq independent searches on the GPU. Returns ids [nq,k] uint64, dists [nq,k] float32,
        counts [nq] uint32 (and stats [nq,3] uint64 = n_dist, n_expand, n_adj when stats=True)."""
        q = self._prepare(elements, prepared)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        nq, k = q.shape[0], int(num_elements)
        ids = np.empty((nq, max(k, 0)), np.uint64)
        dists = np.empty((nq, max(k, 0)), np.float32)
        counts = np.zeros(nq, np.uint32)
        st = np.zeros((nq, 3), np.uint64)
        check(lib().granne_hip_search_batch(self._h, _p(q), nq, int(max_search), k, _p(ids), _p(dists), _p(counts),
                                            _p(st)))
        return (ids, dists, counts, st) if stats else (ids, dists, counts)

    def search_batch_device(self, d_queries, nq, max_search, num_elements, d_ids, d_dists, d_counts, d_stats=0,
                            d_status=0, stream=0):
        """Device-resident, asynchronous variant: every argument is a raw device pointer (int)."""
        check(lib().granne_hip_search_batch_device(self._h, C.c_void_p(d_queries), nq, int(max_search),
                                                   int(num_elements), C.c_void_p(d_ids), C.c_void_p(d_dists),
                                                   C.c_void_p(d_counts), C.c_void_p(d_stats), C.c_void_p(d_status),
                                                   C.c_void_p(stream)))

    # ---- filtered search: the walk under an id bitmap (granne_amd/filters.py) ------------------------
    def _filter_arg(self, allowed, nq, n=None):
        """`allowed` as (owner, device pointer, stride in words): a Filter, a bool array of length n (len() unless given),
        an integer id array, or a sequence of Filters, one per query (packed with a stride)."""
        from .filters import Filter, _DeviceBlock, filter_words
        n = len(self) if n is None else n
        if isinstance(allowed, Filter):
            f = allowed
        elif isinstance(allowed, (list, tuple)) and len(allowed) and all(isinstance(f, Filter) for f in allowed):
            if len(allowed) != nq:
                raise ValueError("need one Filter per query")
            if any(f.n != n or f.device != self.device for f in allowed):
                raise ValueError("every Filter must cover the index's %d ids on its device" % n)
            block = _DeviceBlock(nq * filter_words(n) * 4, self.device).upload(np.stack([f.words() for f in allowed]))
            return block, block.ptr, filter_words(n)
        else:
            a = np.asarray(allowed)
            if a.dtype.kind == "b":
                if a.shape != (n,):
                    raise ValueError("a bool filter needs one entry per element")
                f = Filter.from_mask(a, self.device)
            elif a.dtype.kind in "iu":
                f = Filter.from_ids(a, n, self.device)
            else:
                raise TypeError("allowed: a Filter, a bool array, an id array or one Filter per query")
        if f.n != n or f.device != self.device:
            raise ValueError("the Filter must cover the index's %d ids on its device" % n)
        return f, f.ptr, 0

    def search_filtered(self, element, allowed, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS, max_expand=0,
                        prepared=True):
        """`search` among the ids `allowed` lets through: [(id, distance)] ascending by (distance, id), fewer than
        num_elements when the walk met fewer allowed ids. max_expand > 0 caps the bottom layer's expansions."""
        terms = self.element_type == EMBEDDINGS and (len(element) == 0 or np.asarray(element).dtype.kind in "iu")
        one = [list(element)] if terms else np.asarray(element).reshape(1, -1)
        ids, dists, counts = self.search_filtered_batch(one, allowed, max_search, num_elements, max_expand, prepared)
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    def search_filtered_batch(self, elements, allowed, max_search=DEFAULT_MAX_SEARCH, num_elements=DEFAULT_NUM_ELEMENTS,
                              max_expand=0, prepared=True, stats=False, status=False):
        """nq filtered searches (granne_hip_search_filtered_batch_device). Returns ids [nq,k] uint64, dists [nq,k] float32,
        counts [nq] uint32, then stats [nq,3] uint64 (stats=True) and the four status words -- [1] walks the exact walker
        served, [3] walks max_expand cut -- (status=True). `allowed`: see `_filter_arg`."""
        from ._lib import OK
        from .filters import _DeviceBlock
        q = self._prepare(elements, prepared)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        nq, k = q.shape[0], int(num_elements)
        owner, fptr, stride = self._filter_arg(allowed, nq)
        up = lambda v: (v + 255) & ~255  # noqa: E731
        o_ids = up(q.nbytes)
        o_d = o_ids + up(nq * k * 8)
        o_c = o_d + up(nq * k * 4)
        o_s = o_c + up(nq * 4)
        o_st = o_s + up(nq * 24)
        block = _DeviceBlock(o_st + 16, self.device)
        host = np.zeros(o_st + 16, np.uint8)
        host[:q.nbytes] = q.view(np.uint8).reshape(-1)
        block.upload(host)
        rc = OK
        if nq:
            rc = lib().granne_hip_search_filtered_batch_device(
                self._h, C.c_void_p(block.ptr), nq, int(max_search), k, C.c_void_p(fptr), stride, int(max_expand),
                C.c_void_p(block.ptr + o_ids), C.c_void_p(block.ptr + o_d), C.c_void_p(block.ptr + o_c),
                C.c_void_p(block.ptr + o_s), C.c_void_p(block.ptr + o_st), None)
        check(lib().granne_hip_stream_synchronize(None, self.device))
        check(rc)
        host = block.download(np.uint8, o_st + 16)
        del owner
        st4 = host[o_st:o_st + 16].view(np.uint32).copy()
        if st4[0]:
            raise GranneHipError(ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)")
        out = [host[o_ids:o_ids + nq * k * 8].view(np.uint64).reshape(nq, k).copy(),
               host[o_d:o_d + nq * k * 4].view(np.float32).reshape(nq, k).copy(),
               host[o_c:o_c + nq * 4].view(np.uint32).copy()]
        if stats:
            out.append(host[o_s:o_s + nq * 24].view(np.uint64).reshape(nq, 3).copy())
        if status:
            out.append(st4)
        return tuple(out)

    def search_filtered_batch_device(self, d_queries, nq, max_search, num_elements, d_filter, filter_stride_words, max_expand,
                                     d_ids, d_dists, d_counts, d_stats=0, d_status=0, stream=0):
        """Device-resident, asynchronous variant: raw device pointers (int); d_filter e.g. a Filter's `ptr`."""
        check(lib().granne_hip_search_filtered_batch_device(
            self._h, C.c_void_p(d_queries), int(nq), int(max_search), int(num_elements), C.c_void_p(d_filter),
            int(filter_stride_words), int(max_expand), C.c_void_p(d_ids), C.c_void_p(d_dists), C.c_void_p(d_counts),
            C.c_void_p(d_stats), C.c_void_p(d_status), C.c_void_p(stream)))

    # ---- post-filtered search: staged over-fetch on the ordinary search (include/granne_hip.h) ------
    def search_postfiltered(self, element, num_elements, allowed, min_allowed=50, stages=None, fallback="exact", prepared=True):
        """`search_postfiltered_batch` for one query: [(id, distance)] ascending by (distance, id)."""
        terms = self.element_type == EMBEDDINGS and (len(element) == 0 or np.asarray(element).dtype.kind in "iu")
        one = [list(element)] if terms else np.asarray(element).reshape(1, -1)
        ids, dists, counts = self.search_postfiltered_batch(one, num_elements, allowed, min_allowed, stages, fallback, prepared=prepared)
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    def search_postfiltered_batch(self, queries, num_elements, allowed, min_allowed=50, stages=None, fallback="exact", scratch_bytes=0,
                                  return_stage=False, status=False, prepared=True):
        """The k = num_elements nearest ALLOWED ids by the ordinary search with a long list and a filter of its result
        (granne_hip_search_postfiltered_batch_device): a query's list of stages[s] entries answers it once it holds
        min_allowed allowed ids (or the walk ran out of graph), else the query goes on to the next stage; what no stage
        finishes gets the exact scan under the filter (fallback="exact") or its short answer (fallback="short").
        `allowed`: see `_filter_arg`. stages=None: `filters.postfilter_stages`, from the filter's count where one filter
        serves all queries. Returns ids [nq,k] uint64, dists [nq,k] float32, counts [nq] uint32, then the stage that answered
        each query (return_stage=True; _lib.PF_STAGE_EXACT / PF_STAGE_SHORT for the fallback) and the four status words --
        [3] the queries no stage finished -- (status=True)."""
        from ._lib import OK, PF_FALLBACK_EXACT, PF_FALLBACK_SHORT
        from .filters import Filter, _DeviceBlock, postfilter_stages
        q = self._prepare(queries, prepared)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        fb = {"exact": PF_FALLBACK_EXACT, "short": PF_FALLBACK_SHORT}.get(fallback, fallback)
        nq, k = q.shape[0], int(num_elements)
        owner, fptr, stride = self._filter_arg(allowed, nq, self.num_elements())
        if stages is None:
            sel = owner.count() / max(owner.n, 1) if isinstance(owner, Filter) else None
            stages = postfilter_stages(int(min_allowed), sel)
        st_arr = (C.c_uint32 * max(len(stages), 1))(*[int(e) for e in stages])
        up = lambda v: (v + 255) & ~255  # noqa: E731
        o_ids = up(q.nbytes)
        o_d = o_ids + up(nq * max(k, 0) * 8)
        o_c = o_d + up(nq * max(k, 0) * 4)
        o_sg = o_c + up(nq * 4)
        o_st = o_sg + up(nq * 4)
        block = _DeviceBlock(o_st + 16, self.device)
        host = np.zeros(o_st + 16, np.uint8)
        host[:q.nbytes] = q.view(np.uint8).reshape(-1)
        block.upload(host)
        rc = lib().granne_hip_search_postfiltered_batch_device(
            self._h, C.c_void_p(block.ptr), nq, k, int(min_allowed), st_arr, len(stages), int(fb), C.c_void_p(fptr), stride,
            int(scratch_bytes), C.c_void_p(block.ptr + o_ids), C.c_void_p(block.ptr + o_d), C.c_void_p(block.ptr + o_c),
            C.c_void_p(block.ptr + o_sg), C.c_void_p(block.ptr + o_st), None)
        check(lib().granne_hip_stream_synchronize(None, self.device))
        check(rc)
        host = block.download(np.uint8, o_st + 16)
        del owner
        st4 = host[o_st:o_st + 16].view(np.uint32).copy()
        if st4[0]:
            raise GranneHipError(ERR_OVERFLOW, "search_postfiltered: a walk ran out of exact-search scratch (raise "
                                 "GRANNE_HIP_OPT_SLOW_SLOTS) or the fallback's selection overflowed")
        out = [host[o_ids:o_ids + nq * k * 8].view(np.uint64).reshape(nq, k).copy(),
               host[o_d:o_d + nq * k * 4].view(np.float32).reshape(nq, k).copy(),
               host[o_c:o_c + nq * 4].view(np.uint32).copy()]
        if return_stage:
            out.append(host[o_sg:o_sg + nq * 4].view(np.uint32).copy())
        if status:
            out.append(st4)
        return tuple(out)

    def search_postfiltered_batch_device(self, d_queries, nq, num_elements, min_allowed, stages, fallback, d_filter,
                                         filter_stride_words, d_ids, d_dists, d_counts, d_stage=0, d_status=0, scratch_bytes=0,
                                         stream=0):
        """Device-resident variant: raw device pointers (int); `stages` a sequence on the host, `fallback`
        _lib.PF_FALLBACK_*. Stream-ordered, but the call waits on `stream` once per stage it goes beyond."""
        st_arr = (C.c_uint32 * max(len(stages), 1))(*[int(e) for e in stages])
        check(lib().granne_hip_search_postfiltered_batch_device(
            self._h, C.c_void_p(d_queries), int(nq), int(num_elements), int(min_allowed), st_arr, len(stages), int(fallback),
            C.c_void_p(d_filter), int(filter_stride_words), int(scratch_bytes), C.c_void_p(d_ids), C.c_void_p(d_dists),
            C.c_void_p(d_counts), C.c_void_p(d_stage), C.c_void_p(d_status), C.c_void_p(stream)))

    def search_batches_device(self, d_queries, nq, max_search, num_elements, d_ids, d_dists, d_counts, d_stats=None,
                              d_status=0, stream=0):
        """Several batches of nq queries through ONE launch (granne_hip_search_batches_device). d_queries, d_ids,
        d_dists, d_counts (and d_stats, optional): sequences of raw device pointers (int), one per batch -- or ctypes
        pointer arrays prepared once with `pointer_array`. Asynchronous on `stream`."""
        n = len(d_queries)
        arr = lambda v: v if isinstance(v, C.Array) else pointer_array(v)  # noqa: E731
        check(lib().granne_hip_search_batches_device(self._h, n, arr(d_queries), int(nq), int(max_search), int(num_elements),
                                                     arr(d_ids), arr(d_dists), arr(d_counts),
                                                     arr(d_stats) if d_stats is not None else None, C.c_void_p(d_status),
                                                     C.c_void_p(stream)))

    def search_begin_device(self, d_queries, nq, max_search, num_elements, d_ids, d_dists, d_counts, d_stats=0, d_status=0,
                            stream=0):
        """granne_hip_search_begin_device: the batch runs beside `stream` on a stream of the index; returns the ticket."""
        t = C.c_uint64(0)
        check(lib().granne_hip_search_begin_device(self._h, C.c_void_p(d_queries), int(nq), int(max_search), int(num_elements),
                                                   C.c_void_p(d_ids), C.c_void_p(d_dists), C.c_void_p(d_counts),
                                                   C.c_void_p(d_stats), C.c_void_p(d_status), C.c_void_p(stream), C.byref(t)))
        return int(t.value)

    def search_end_device(self, ticket, stream=0):
        """granne_hip_search_end_device: `stream` continues after the batch of `ticket`."""
        check(lib().granne_hip_search_end_device(self._h, C.c_uint64(ticket), C.c_void_p(stream)))

    def search_batch_device_timed(self, d_queries, nq, max_search, num_elements, d_ids, d_dists, d_counts, d_stats,
                                  d_status, stream, ev_before, ev_after):
        """search_batch_device plus two raw hipEvent_t recorded around the search kernel's dispatch."""
        check(lib().granne_hip_search_batch_device_timed(self._h, C.c_void_p(d_queries), nq, int(max_search),
                                                         int(num_elements), C.c_void_p(d_ids), C.c_void_p(d_dists),
                                                         C.c_void_p(d_counts), C.c_void_p(d_stats), C.c_void_p(d_status),
                                                         C.c_void_p(stream), C.c_void_p(ev_before), C.c_void_p(ev_after)))

    def brute_force_device(self, d_queries, nq, k, d_ids, d_dists, d_counts, stream=0):
        """Exact k nearest elements of every query by a scan of all elements on the matrix cores
        (granne_hip_brute_force_device). Raw device pointers (int), asynchronous on `stream`."""
        check(lib().granne_hip_brute_force_device(self._h, C.c_void_p(d_queries), int(nq), int(k), C.c_void_p(d_ids),
                                                  C.c_void_p(d_dists), C.c_void_p(d_counts), C.c_void_p(stream)))

    def brute_force(self, queries, k, prepared=True):
        """Host convenience over brute_force_device (torch moves the buffers): ids [nq, k] u64, dists [nq, k] f32,
        counts [nq] u32, ascending by (distance, id) -- the exact answer Granne::search approximates.
        prepared=False applies Vector::from to the queries first, as `search` does."""
        import torch
        q = self._prepare(queries, prepared)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(q.shape[0], -1)).to(dev)
        ids = torch.empty((q.shape[0], k), dtype=torch.int64, device=dev)
        ds = torch.empty((q.shape[0], k), dtype=torch.float32, device=dev)
        cnt = torch.empty(q.shape[0], dtype=torch.int32, device=dev)
        self.brute_force_device(tq.data_ptr(), q.shape[0], k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        return ids.cpu().numpy().astype(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)

    def exact_topk_device(self, d_queries, nq, k, d_ids, d_dists, d_counts, d_status=0, stream=0):
        """Exact k (up to EXACT_TOPK_KMAX) nearest elements of every query in the reference's own arithmetic, selected by
        (distance bits, id) (granne_hip_exact_topk_device). Raw device pointers (int; d_status: u32[4] zeroed by the
        caller, or 0), asynchronous on `stream`."""
        check(lib().granne_hip_exact_topk_device(self._h, C.c_void_p(d_queries), int(nq), int(k), C.c_void_p(d_ids),
                                                 C.c_void_p(d_dists), C.c_void_p(d_counts), C.c_void_p(d_status),
                                                 C.c_void_p(stream)))

    def exact_topk(self, queries, k, prepared=True, stats=False):
        """Host convenience over exact_topk_device (torch moves the buffers): ids [nq, k] u64, dists [nq, k] f32, counts
        [nq] u32, ascending by (distance, id) -- what a scalar scan sorted by that key gives, ties included, k up to
        EXACT_TOPK_KMAX. A query that overflows the selection (status[0]: more than EXACT_TOPK_CAP rows inside one
        second-level bin at its k-th distance) gets count 0 and a filled row: with stats=False that raises
        GranneHipError(ERR_OVERFLOW); with stats=True the four status words are returned as a fourth value instead.
        prepared=False applies Vector::from to the queries first, as `search` does."""
        import torch
        q = self._prepare(queries, prepared)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        k = int(k)
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(q.shape[0], -1)).to(dev)
        ids = torch.empty((q.shape[0], max(k, 0)), dtype=torch.int64, device=dev)
        ds = torch.empty((q.shape[0], max(k, 0)), dtype=torch.float32, device=dev)
        cnt = torch.empty(q.shape[0], dtype=torch.int32, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        self.exact_topk_device(tq.data_ptr(), q.shape[0], k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), st.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        status = st.cpu().numpy().astype(np.uint32)
        out = ids.cpu().numpy().astype(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
        if stats:
            return out + (status,)
        if status[0]:
            raise GranneHipError(ERR_OVERFLOW, "exact_topk: %d queries have more than %d rows inside one second-level bin "
                                 "at their k-th distance" % (int(status[0]), EXACT_TOPK_CAP))
        return out

    def num_elements(self):
        """Rows of the element set (at least len()): what exact_topk and exact_topk_filtered scan."""
        return int(lib().granne_hip_index_num_elements(self._h))

    def exact_topk_filtered_device(self, d_queries, nq, k, d_filter, filter_stride_words, d_ids, d_dists, d_counts, d_status=0,
                                   stream=0):
        """exact_topk among the ids a bitmap allows (granne_hip_exact_topk_filtered_device): raw device pointers (int);
        d_filter e.g. a Filter's `ptr` over num_elements() ids with filter_stride_words 0 -- the scan then walks the
        bitmap's id list and d_status[3] is its length -- or one bitmap per query, filter_stride_words apart.
        Asynchronous on `stream`."""
        check(lib().granne_hip_exact_topk_filtered_device(self._h, C.c_void_p(d_queries), int(nq), int(k), C.c_void_p(d_filter),
                                                          int(filter_stride_words), C.c_void_p(d_ids), C.c_void_p(d_dists),
                                                          C.c_void_p(d_counts), C.c_void_p(d_status), C.c_void_p(stream)))

    def exact_topk_filtered(self, queries, k, allowed, prepared=True, stats=False):
        """The k (up to EXACT_TOPK_KMAX) nearest elements among those `allowed` lets through, exact by construction: ids
        [nq, k] u64, dists [nq, k] f32, counts [nq] u32 = min(k, allowed ids), ascending by (distance, id), the places past
        the count UINT64_MAX / +inf. `allowed`: what search_filtered takes (`_filter_arg`), over num_elements() ids. One
        filter for all queries is scanned as a list of its ids (status[3]: how many); one Filter per query scans all rows
        under a bit test. Overflow and stats as `exact_topk`."""
        import torch
        q = self._prepare(queries, prepared)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        k, nq = int(k), q.shape[0]
        owner, fptr, stride = self._filter_arg(allowed, nq, self.num_elements())
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(nq, q.shape[1] * q.itemsize)).to(dev)
        ids = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
        ds = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # (the filter was made on the null stream)
        self.exact_topk_filtered_device(tq.data_ptr(), nq, k, fptr, stride, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                        st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        del owner
        status = st.cpu().numpy().astype(np.uint32)
        out = ids.cpu().numpy().astype(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)
        if stats:
            return out + (status,)
        if status[0]:
            raise GranneHipError(ERR_OVERFLOW, "exact_topk_filtered: %d queries have more than %d rows inside one second-level "
                                 "bin at their k-th distance" % (int(status[0]), EXACT_TOPK_CAP))
        return out

    # ---- range search: all elements within a radius, by scan and by walk (include/granne_hip.h) -----
    def _radii(self, radius, nq):
        """`radius` -- a scalar or one value per query -- as float32 [nq]; a NaN is refused here as by the host entries"""
        r = np.array(np.broadcast_to(np.asarray(radius, np.float32), (nq,)) if np.ndim(radius) == 0 else radius, np.float32, order="C")
        if r.shape != (nq,):
            raise ValueError("radius: a scalar or one value per query")
        if np.isnan(r).any():
            raise GranneHipError(ERR_INVALID, "range search: the radius of query %d is NaN" % int(np.argmax(np.isnan(r))))
        return r

    def exact_range_device(self, d_queries, nq, d_radii, max_results, d_filter, filter_stride_words, d_ids, d_dists, d_counts,
                           d_totals, d_status=0, stream=0):
        """Every element within d_radii[q] of query q (granne_hip_exact_range_device): raw device pointers (int); d_filter 0
        for all rows, else as exact_topk_filtered_device. Stream-ordered, but the call waits on `stream` once."""
        check(lib().granne_hip_exact_range_device(self._h, C.c_void_p(d_queries), int(nq), C.c_void_p(d_radii), int(max_results),
                                                  C.c_void_p(d_filter), int(filter_stride_words), C.c_void_p(d_ids),
                                                  C.c_void_p(d_dists), C.c_void_p(d_counts), C.c_void_p(d_totals),
                                                  C.c_void_p(d_status), C.c_void_p(stream)))

    def exact_range(self, queries, radius, max_results=RANGE_CAP_MAX, allowed=None, prepared=True, stats=False):
        """The elements within `radius` (a scalar or one value per query) of every query, exact by construction: ids
        [nq, max_results] u64 and dists f32 -- the nearest min(total, max_results), ascending by (distance, id), the places
        past the count UINT64_MAX / +inf --, counts [nq] u32 and totals [nq] u32, the exact number within the radius also
        beyond max_results (up to RANGE_CAP_MAX). `allowed`: None for all rows, else what exact_topk_filtered takes. A query
        voided by the selection's overflow (status[0]; only with total > EXACT_TOPK_CAP) has count 0 and its exact total:
        with stats=False that raises GranneHipError(ERR_OVERFLOW); with stats=True the four status words are returned last."""
        import torch
        q = self._prepare(queries, prepared)
        if q.ndim == 1:
            q = q[None]
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        cap, nq = int(max_results), q.shape[0]
        r = self._radii(radius, nq)
        owner, fptr, stride = (None, 0, 0) if allowed is None else self._filter_arg(allowed, nq, self.num_elements())
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(nq, q.shape[1] * q.itemsize)).to(dev)
        tr = torch.from_numpy(r).to(dev)
        ids = torch.empty((nq, max(cap, 0)), dtype=torch.int64, device=dev)
        ds = torch.empty((nq, max(cap, 0)), dtype=torch.float32, device=dev)
        cnt = torch.empty(nq, dtype=torch.int32, device=dev)
        tot = torch.empty(nq, dtype=torch.int32, device=dev)
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # (the filter was made on the null stream)
        self.exact_range_device(tq.data_ptr(), nq, tr.data_ptr(), cap, fptr, stride, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                tot.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        del owner
        status = st.cpu().numpy().view(np.uint32)
        out = (ids.cpu().numpy().view(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), tot.cpu().numpy().view(np.uint32))
        if stats:
            return out + (status,)
        if status[0]:
            raise GranneHipError(ERR_OVERFLOW, "exact_range: %d queries have more than %d rows inside one second-level bin at "
                                 "their cap-th distance" % (int(status[0]), EXACT_TOPK_CAP))
        return out

    def search_range(self, element, radius, max_results=DEFAULT_NUM_ELEMENTS, stages=None, fallback="exact", prepared=True):
        """`search_range_batch` for one query: [(id, distance)] ascending by (distance, id), every distance <= radius."""
        terms = self.element_type == EMBEDDINGS and (len(element) == 0 or np.asarray(element).dtype.kind in "iu")
        one = [list(element)] if terms else np.asarray(element).reshape(1, -1)
        ids, dists, counts = self.search_range_batch(one, radius, max_results, stages, fallback, prepared=prepared)[:3]
        return [(int(ids[0, i]), float(dists[0, i])) for i in range(int(counts[0]))]

    def search_range_batch(self, queries, radius, max_results, stages=None, fallback="exact", scratch_bytes=0, prepared=True,
                           stats=False):
        """The elements within `radius` of every query by the ordinary search with a long list, cut at the radius
        (granne_hip_search_range_batch_device): a query's list of stages[s] entries answers it once it holds an entry beyond
        the radius (or the walk ran out of graph), else the query goes on to the next stage; what no stage finishes gets
        the exact scan (fallback="exact") or its short answer (fallback="short"). stages=None: RANGE_DEFAULT_STAGES. Returns
        ids [nq, max_results] uint64, dists float32, counts [nq] uint32, found [nq] uint32 (the entries within the radius
        of the answering list, or the exact total), stage [nq] uint32 (_lib.RG_STAGE_EXACT / RG_STAGE_SHORT for the
        fallback), then the four status words -- [3] the queries no stage finished -- (stats=True)."""
        import torch
        from ._lib import RG_FALLBACK_EXACT, RG_FALLBACK_SHORT
        q = self._prepare(queries, prepared)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise ValueError("queries must be [nq, %d]" % self.dim)
        fb = {"exact": RG_FALLBACK_EXACT, "short": RG_FALLBACK_SHORT}.get(fallback, fallback)
        nq, cap = q.shape[0], int(max_results)
        r = self._radii(radius, nq)
        stages = RANGE_DEFAULT_STAGES if stages is None else stages
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(nq, q.shape[1] * q.itemsize)).to(dev)
        tr = torch.from_numpy(r).to(dev)
        ids = torch.empty((nq, max(cap, 0)), dtype=torch.int64, device=dev)
        ds = torch.empty((nq, max(cap, 0)), dtype=torch.float32, device=dev)
        cnt, found, stage = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(3))
        st = torch.zeros(4, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        self.search_range_batch_device(tq.data_ptr(), nq, tr.data_ptr(), cap, stages, fb, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                       found.data_ptr(), stage.data_ptr(), st.data_ptr(), scratch_bytes, stream)
        torch.cuda.synchronize(dev)
        status = st.cpu().numpy().view(np.uint32)
        if status[0]:
            raise GranneHipError(ERR_OVERFLOW, "search_range: a walk ran out of exact-search scratch (raise GRANNE_HIP_OPT_SLOW_SLOTS) "
                                 "or the fallback's selection overflowed")
        out = (ids.cpu().numpy().view(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().view(np.uint32),
               found.cpu().numpy().view(np.uint32), stage.cpu().numpy().view(np.uint32))
        return out + (status,) if stats else out

    def search_range_batch_device(self, d_queries, nq, d_radii, max_results, stages, fallback, d_ids, d_dists, d_counts, d_found=0,
                                  d_stage=0, d_status=0, scratch_bytes=0, stream=0):
        """Device-resident variant: raw device pointers (int); `stages` a sequence on the host, `fallback`
        _lib.RG_FALLBACK_*. Stream-ordered, but the call waits on `stream` once per stage it goes beyond."""
        st_arr = (C.c_uint32 * max(len(stages), 1))(*[int(e) for e in stages])
        check(lib().granne_hip_search_range_batch_device(
            self._h, C.c_void_p(d_queries), int(nq), C.c_void_p(d_radii), int(max_results), st_arr, len(stages), int(fallback),
            int(scratch_bytes), C.c_void_p(d_ids), C.c_void_p(d_dists), C.c_void_p(d_counts), C.c_void_p(d_found),
            C.c_void_p(d_stage), C.c_void_p(d_status), C.c_void_p(stream)))

    def dists_device(self, d_queries, nq, d_ids, m, d_out, d_status=0, stream=0):
        """ElementContainer::dists (src/elements/mod.rs:35-39) batched on device: out[q, j] =
        dist(element ids[q, j], query q). Raw device pointers (int), asynchronous on `stream`."""
        check(lib().granne_hip_dists_device(self._h, C.c_void_p(d_queries), int(nq), C.c_void_p(d_ids), int(m),
                                            C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(stream)))

    def refine_device(self, d_queries, nq, d_cand_ids, d_cand_counts, m, k, d_ids, d_dists, d_counts, d_refine_status=0,
                      stream=0):
        """granne_hip_refine_device: re-rank u64 candidate lists [nq, m] by this index's rows. Raw device pointers (int;
        d_cand_counts and d_refine_status may be 0), asynchronous on `stream`."""
        check(lib().granne_hip_refine_device(self._h, C.c_void_p(d_queries), int(nq), C.c_void_p(d_cand_ids),
                                             C.c_void_p(d_cand_counts), int(m), int(k), C.c_void_p(d_ids), C.c_void_p(d_dists),
                                             C.c_void_p(d_counts), C.c_void_p(d_refine_status), C.c_void_p(stream)))

    def refine(self, queries, ids, counts=None, k=DEFAULT_NUM_ELEMENTS, prepared=True, dropped=False):
        """Host convenience over refine_device (torch moves the buffers): the candidates ids [nq, m] (query q's list: its
        first counts[q] entries; None = all m) by THIS index's distances to queries [nq, dim], the k best ascending by
        (distance, id): ids [nq, k] u64, dists [nq, k] f32, counts [nq] u32 -- and, with dropped=True, how many candidates
        were out of range. prepared=False applies Vector::from to the queries first, as `search` does."""
        import torch
        q = self._prepare(queries, prepared)
        if q.ndim == 1:
            q = q[None]
        ii = np.ascontiguousarray(ids, dtype=np.uint64)
        if q.ndim != 2 or q.shape[1] != self.dim or ii.ndim != 2 or ii.shape[0] != q.shape[0]:
            raise ValueError("queries must be [nq, %d] and ids [nq, m]" % self.dim)
        nq, m, k = q.shape[0], ii.shape[1], int(k)
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(nq, -1)).to(dev)
        ti = torch.from_numpy(ii.view(np.int64)).to(dev)
        tc = None
        if counts is not None:
            cc = np.ascontiguousarray(counts, dtype=np.uint32)
            if cc.shape != (nq,):
                raise ValueError("counts must be [nq]")
            tc = torch.from_numpy(cc.view(np.int32)).to(dev)
        out_ids = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=dev)
        out_d = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=dev)
        out_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            self.refine_device(tq.data_ptr(), nq, ti.data_ptr(), tc.data_ptr() if tc is not None else 0, m, k,
                               out_ids.data_ptr(), out_d.data_ptr(), out_c.data_ptr(), st.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        res = (out_ids.cpu().numpy().view(np.uint64), out_d.cpu().numpy(), out_c.cpu().numpy().view(np.uint32))
        return res + (int(st.cpu().numpy().view(np.uint32)[0]),) if dropped else res

    def dists_many(self, queries, ids):
        """ElementContainer::dists for a batch: queries [nq, dim] (prepared), ids [nq, m] -> [nq, m] f32
        (+inf where an id is out of range)."""
        import torch
        q = np.ascontiguousarray(queries, dtype=self.query_dtype)
        ii = np.ascontiguousarray(ids, dtype=np.uint32)
        if q.ndim != 2 or q.shape[1] != self.dim or ii.ndim != 2 or ii.shape[0] != q.shape[0]:
            raise ValueError("queries must be [nq, %d] and ids [nq, m]" % self.dim)
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q.view(np.uint8).reshape(q.shape[0], -1)).to(dev)
        ti = torch.from_numpy(ii.view(np.int32)).to(dev)
        out = torch.empty(ii.shape, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            s = torch.cuda.current_stream().cuda_stream
            self.dists_device(tq.data_ptr(), q.shape[0], ti.data_ptr(), ii.shape[1], out.data_ptr(), 0, s)
            torch.cuda.synchronize()
        return out.cpu().numpy()

    def dists(self, queries, qidx, ids):
        """ElementContainer::dist_to_element for explicit (query, element) pairs."""
        q = np.ascontiguousarray(queries, dtype=self.query_dtype)
        qi = np.ascontiguousarray(qidx, dtype=np.uint32)
        ii = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.empty(qi.size, np.float32)
        check(lib().granne_hip_dist_pairs(self._h, _p(q), q.shape[0], _p(qi), _p(ii), qi.size, _p(out)))
        return out


def pointer_array(ptrs):
    """A ctypes array of device pointers (ints) for the multi-batch calls; build it once when the buffers are fixed."""
    return (C.c_void_p * len(ptrs))(*[int(x) for x in ptrs])


def compute_distance(element_type, a, b, device=0):
    """compute_distance (py/src/lib.rs:58-86): both vectors go through Vector::from."""
    et = element_type.lower()
    if et not in _ELEMENT_TYPES:
        raise ValueError("Unsupported element type")
    prep = quantize if et == "angular_int" else normalize
    pa = _prepare_elements(et, np.asarray(a, np.float32), device).reshape(1, -1)
    pb = prep(np.asarray(b, np.float32), device).reshape(1, -1)
    ix = Granne(et, pa, [], device=device)
    try:
        return float(ix.dists(pb, [0], [0])[0])
    finally:
        ix.close()
