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

    def save_elements(self, path):
        check(lib().granne_hip_sum_embeddings_save_elements(self._h, os.fsencode(path)))

    def save_embeddings(self, path):
        check(lib().granne_hip_sum_embeddings_save_embeddings(self._h, os.fsencode(path)))
