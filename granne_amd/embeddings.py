"""embeddings::SumEmbeddings (src/elements/embeddings/mod.rs:41-216) over granne_hip_sum_embeddings_*: an element is a
list of term ids, its vector the sum of those terms' rows of an embedding table (normalised when searched)."""
import ctypes as C
import os

import numpy as np

from ._lib import ERR_INVALID, GranneHipError, check, lib

SE_MATERIALIZED, SE_COMPACT = 0, 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32_table(embeddings):
    """The table as float32 rows. A table of halves is refused: the container's sums are f32 chains over f32 rows
    (create_embedding), and "angular_f16" is a dense element type, not a table format."""
    if getattr(embeddings, "dtype", None) == np.float16:
        raise GranneHipError(ERR_INVALID, "a SumEmbeddings table has no form for GRANNE_HIP_F16 (angular_f16) rows: pass float32 embeddings")
    return np.ascontiguousarray(embeddings, dtype=np.float32)


def _dense_type(element_type):
    """(GRANNE_HIP_* code, numpy dtype) of a dense element type: its name ("angular", "angular_int", "angular_f16") or its
    code (F32, I8, F16). Anything else is ERR_INVALID here, before a buffer is sized by it."""
    from .index import _ELEMENT_TYPES
    if isinstance(element_type, str):
        if element_type.lower() in _ELEMENT_TYPES:
            return _ELEMENT_TYPES[element_type.lower()]
    else:
        for code, np_dtype in _ELEMENT_TYPES.values():
            if element_type == code and not isinstance(element_type, bool):
                return code, np_dtype
    raise GranneHipError(ERR_INVALID, "to_rows: unknown %s %r" % ("element type" if isinstance(element_type, str) else "dtype", element_type))


def csr_of(term_lists):
    """(offsets u64 [n + 1], terms u32) of a sequence of term-id sequences."""
    lists = [np.asarray(t, dtype=np.int64).reshape(-1) for t in term_lists]
    off = np.zeros(len(lists) + 1, np.uint64)
    if lists:
        off[1:] = np.cumsum([t.size for t in lists], dtype=np.uint64)
    cat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    if cat.size and (cat.min() < 0 or cat.max() > 0xFFFFFFFF):
        raise ValueError("term ids must be in [0, 2^32)")
    return off, np.ascontiguousarray(cat, dtype=np.uint32)


class SumEmbeddings:
    """The container: `embeddings` [V, dim] float32 (not normalised) and the elements' term lists."""

    def __init__(self, embeddings, elements=(), device=0, offsets=None, terms=None):
        """elements: a sequence of term-id sequences -- or pass the CSR form (offsets [n + 1], terms) directly."""
        tab = _f32_table(embeddings)
        if tab.ndim != 2 or tab.shape[1] == 0:
            raise ValueError("embeddings must be [V, dim]")
        if offsets is None:
            offsets, terms = csr_of(elements)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        ids = np.ascontiguousarray(terms if terms is not None else [], dtype=np.uint32)
        h = C.c_void_p()
        check(lib().granne_hip_sum_embeddings_create(C.byref(h), _p(tab), tab.shape[0], tab.shape[1], _p(off), _p(ids),
                                                     off.size - 1, device))
        self._h, self.dim, self.device = h, tab.shape[1], device

    @classmethod
    def from_files(cls, embeddings_path, elements_path, device=0):
        """An f32 Vectors file and an elements file (5-byte offsets, 3-byte ids)."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().granne_hip_sum_embeddings_load_files(C.byref(h), os.fsencode(embeddings_path), os.fsencode(elements_path),
                                                         device))
        self._h, self.dim, self.device = h, int(lib().granne_hip_sum_embeddings_dim(h)), device
        return self

    @classmethod
    def from_bytes(cls, embeddings, elements_bytes, device=0):
        """SumEmbeddings::from_bytes: a table and the bytes of an elements file."""
        self = cls.__new__(cls)
        tab = _f32_table(embeddings)
        buf = np.frombuffer(elements_bytes, np.uint8)
        h = C.c_void_p()
        check(lib().granne_hip_sum_embeddings_load(C.byref(h), _p(tab), tab.shape[0], tab.shape[1], _p(buf), buf.size, device))
        self._h, self.dim, self.device = h, tab.shape[1], device
        return self

    @classmethod
    def from_device(cls, d_table, n_embeddings, dim, d_offsets, d_terms, n_elements, device=0, stream=0):
        """granne_hip_sum_embeddings_create_device: the table (float32 [n_embeddings, dim], dense) and the CSR (u64 offsets
        [n_elements + 1], u32 term ids) at raw device pointers (int) on `device`. They are copied (the term lists are
        checked on the host): the caller's buffers are free again when the call returns."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().granne_hip_sum_embeddings_create_device(C.byref(h), C.c_void_p(d_table), int(n_embeddings), int(dim),
                                                            C.c_void_p(d_offsets), C.c_void_p(d_terms), int(n_elements), device,
                                                            C.c_void_p(stream)))
        self._h, self.dim, self.device = h, int(dim), device
        return self

    def close(self):
        if getattr(self, "_h", None):
            lib().granne_hip_sum_embeddings_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(lib().granne_hip_sum_embeddings_len(self._h))

    def num_embeddings(self):
        return int(lib().granne_hip_sum_embeddings_num_embeddings(self._h))

    def hbm_bytes(self):
        return int(lib().granne_hip_sum_embeddings_hbm_bytes(self._h))

    def push(self, element):
        """SumEmbeddings::push: one element (a sequence of term ids)."""
        self.extend([element])

    def extend(self, elements):
        off, ids = csr_of(elements)
        check(lib().granne_hip_sum_embeddings_append(self._h, _p(off), _p(ids), off.size - 1))

    def get_terms(self, idx):
        n = C.c_uint32(0)
        check(lib().granne_hip_sum_embeddings_get_terms(self._h, idx, None, 0, C.byref(n)))
        out = np.empty(max(n.value, 1), np.uint32)
        check(lib().granne_hip_sum_embeddings_get_terms(self._h, idx, _p(out), n.value, C.byref(n)))
        return out[: n.value].astype(np.int64).tolist()

    def get_embeddings(self, first=0, count=None, normalized=False):
        """Rows first .. first + count - 1: the raw sums (get_embedding) or the normalised vectors (ElementContainer::get)."""
        count = len(self) - first if count is None else count
        out = np.empty((count, self.dim), np.float32)
        check(lib().granne_hip_sum_embeddings_materialize(self._h, first, count, int(bool(normalized)), _p(out)))
        return out

    def get_embedding(self, idx):
        """SumEmbeddings::get_embedding: the raw sum of element idx."""
        return self.get_embeddings(idx, 1)[0]

    def get(self, idx):
        """ElementContainer::get: the normalised vector of element idx."""
        return self.get_embeddings(idx, 1, normalized=True)[0]

    def create_embeddings(self, term_lists, normalized=False):
        """create_embedding for a batch of term lists, on the device: [len(term_lists), dim] float32."""
        off, ids = csr_of(term_lists)
        out = np.empty((off.size - 1, self.dim), np.float32)
        check(lib().granne_hip_sum_embeddings_embed(self._h, _p(off), _p(ids), off.size - 1, int(bool(normalized)), _p(out)))
        return out

    def create_embedding(self, terms, normalized=False):
        """SumEmbeddings::create_embedding: the raw sum of the terms' rows."""
        return self.create_embeddings([terms], normalized)[0]

    # ---- the container as the re-ranking side of refined search, and as the rows of the index that is walked ----
    query_dtype = np.float32  # queries are prepared float32 rows, as for "angular"

    def _queries(self, queries, prepared):
        """Prepared float32 queries [nq, dim] from prepared rows, raw rows (prepared=False) or term lists."""
        from .index import _is_term_lists, normalize
        if not prepared and _is_term_lists(queries):
            return self.create_embeddings(queries, normalized=True)
        q = np.ascontiguousarray(queries, np.float32) if prepared else normalize(queries, self.device)
        return q[None] if q.ndim == 1 else q

    def refine_device(self, d_queries, nq, d_cand_ids, d_cand_counts, m, k, d_ids, d_dists, d_counts, d_refine_status=0,
                      stream=0):
        """granne_hip_refine_sum_embeddings_device: re-rank u64 candidate lists [nq, m] by the vectors this container
        stands for. Raw device pointers (int; d_cand_counts and d_refine_status may be 0), asynchronous on `stream`."""
        check(lib().granne_hip_refine_sum_embeddings_device(self._h, C.c_void_p(d_queries), int(nq), C.c_void_p(d_cand_ids),
                                                            C.c_void_p(d_cand_counts), int(m), int(k), C.c_void_p(d_ids),
                                                            C.c_void_p(d_dists), C.c_void_p(d_counts),
                                                            C.c_void_p(d_refine_status), C.c_void_p(stream)))

    def refine(self, queries, ids, counts=None, k=10, prepared=True, dropped=False):
        """Granne.refine with the container as the rows side: the candidates ids [nq, m] (query q's list: its first
        counts[q] entries; None = all m) by get(id).dist(query), the k best ascending by (distance, id): ids [nq, k] u64,
        dists [nq, k] f32, counts [nq] u32 -- and, with dropped=True, how many candidates were out of range. Queries are
        prepared float32 rows; prepared=False takes raw rows or term lists. Bad shapes, m outside [1, 1024] and k < 1 are
        GranneHipError(ERR_INVALID) before anything touches the device."""
        q = self._queries(queries, prepared)
        ii = np.ascontiguousarray(ids, dtype=np.uint64)
        if q.ndim != 2 or q.shape[1] != self.dim or ii.ndim != 2 or ii.shape[0] != q.shape[0]:
            raise GranneHipError(ERR_INVALID, "refine: queries must be [nq, %d] and ids [nq, m]" % self.dim)
        nq, m, k = q.shape[0], ii.shape[1], int(k)
        cc = None
        if counts is not None:
            cc = np.ascontiguousarray(counts, dtype=np.uint32)
            if cc.shape != (nq,):
                raise GranneHipError(ERR_INVALID, "refine: counts must be [nq]")
        if not 1 <= m <= 1024:  # (the library checks the same; here nothing has been moved to the device yet)
            raise GranneHipError(ERR_INVALID, "refine: candidates per query must be in [1, 1024]")
        if k < 1:
            raise GranneHipError(ERR_INVALID, "refine: k must be > 0")
        if nq == 0:  # nothing to do
            res = (np.empty((0, k), np.uint64), np.empty((0, k), np.float32), np.zeros(0, np.uint32))
            return res + (0,) if dropped else res
        import torch
        dev = torch.device("cuda", self.device)
        tq = torch.from_numpy(q).to(dev)
        ti = torch.from_numpy(ii.view(np.int64)).to(dev)
        tc = torch.from_numpy(cc.view(np.int32)).to(dev) if cc is not None else None
        out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        out_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_c = torch.zeros(nq, dtype=torch.int32, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            self.refine_device(tq.data_ptr(), nq, ti.data_ptr(), tc.data_ptr() if tc is not None else 0, m, k,
                               out_ids.data_ptr(), out_d.data_ptr(), out_c.data_ptr(), st.data_ptr(),
                               torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        res = (out_ids.cpu().numpy().view(np.uint64), out_d.cpu().numpy(), out_c.cpu().numpy().view(np.uint32))
        return res + (int(st.cpu().numpy().view(np.uint32)[0]),) if dropped else res

    def to_rows_device(self, element_type, d_out, first=0, count=None, stride_bytes=None, stream=0):
        """granne_hip_sum_embeddings_rows_device: elements first .. first + count - 1 as prepared rows of a dense
        element type ("angular", "angular_int", "angular_f16") at the raw device pointer d_out (int), stride_bytes from
        one row to the next (None: dense). Asynchronous on `stream`; at most 64 MB of scratch whatever count is."""
        code, np_dtype = _dense_type(element_type)
        count = len(self) - first if count is None else count
        stride = self.dim * np.dtype(np_dtype).itemsize if stride_bytes is None else stride_bytes
        check(lib().granne_hip_sum_embeddings_rows_device(self._h, int(first), int(count), code, C.c_void_p(d_out), int(stride),
                                                          C.c_void_p(stream)))

    def to_rows(self, element_type, first=0, count=None):
        """The same as a numpy array [count, dim] of the element type's scalar: what Granne(element_type, rows, layers)
        and GranneBuilder(element_type, rows) take as prepared elements."""
        code, np_dtype = _dense_type(element_type)
        count = len(self) - first if count is None else count
        out = np.empty((max(int(count), 0), self.dim), np_dtype)
        check(lib().granne_hip_sum_embeddings_rows(self._h, int(first), int(count), code, _p(out)))
        return out

    def save_elements(self, path):
        check(lib().granne_hip_sum_embeddings_save_elements(self._h, os.fsencode(path)))

    def save_embeddings(self, path):
        check(lib().granne_hip_sum_embeddings_save_embeddings(self._h, os.fsencode(path)))
