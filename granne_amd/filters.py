"""Id bitmaps for filtered search (include/granne_hip.h, "filtered search").

A `Filter` is one bit per element id in device memory -- bit (id & 31) of u32 word (id >> 5) -- made and counted by the
library's kernels (granne_amd/csrc/filter.h) and owned through its malloc / free."""
import ctypes as C

import numpy as np

from ._lib import check, lib


def filter_words(n):
    """u32 words of a bitmap over n ids: ceil(n / 32)."""
    w = C.c_uint64(0)
    check(lib().granne_hip_filter_words(int(n), C.byref(w)))
    return int(w.value)


PF_MAX_STAGES = 8  # GRANNE_HIP_PF_MAX_STAGES
# postfilter_stages' default over-fetch: the smallest margin of tools/postfilter_bench.py's sweep whose recall is not
# below the filtered walk's at selectivity 0.1 and 0.01 (profiles/postfiltered_search.json): every margin
# of the sweep, 1.0 included, reached it on f32 and on int8 rows
PF_DEFAULT_MARGIN = 1.0


def postfilter_stages(min_allowed, selectivity=None, e_max=8192, n_stages=4, margin=PF_DEFAULT_MARGIN):
    """The stages E_0 < E_1 < .. of a post-filtered search (Granne.search_postfiltered_batch): list lengths of the ordinary
    search, tried in turn by the queries whose list held fewer than min_allowed allowed ids. Pure Python.

    With a selectivity (the allowed share of the ids, 0..1): a list of E holds about E * selectivity allowed ids, so
    E_0 = margin * min_allowed / selectivity, rounded up to a multiple of 64 and kept within [min_allowed, e_max], then
    doubled up to e_max. Without one: min_allowed * (1, 4, 16, 64), capped at e_max. Always strictly ascending, at most
    min(n_stages, 8) entries, E_0 >= min_allowed."""
    min_allowed, e_max, n_stages = int(min_allowed), int(e_max), int(n_stages)
    if min_allowed < 1 or n_stages < 1 or margin <= 0:
        raise ValueError("min_allowed >= 1, n_stages >= 1 and margin > 0")
    if selectivity is not None and not 0.0 <= selectivity <= 1.0:
        raise ValueError("selectivity is a share: 0..1")
    e_max = max(e_max, min_allowed)
    n_stages = min(n_stages, PF_MAX_STAGES)
    if selectivity is None:
        want = [min_allowed * 4 ** i for i in range(n_stages)]
    else:
        e0 = e_max if selectivity * e_max <= margin * min_allowed else -(-margin * min_allowed / selectivity // 64) * 64
        e0 = min(max(int(e0), min_allowed), e_max)
        want = [e0 << i for i in range(n_stages)]
    out = []
    for e in want:
        e = min(e, e_max)
        if out and e <= out[-1]:
            break
        out.append(e)
    return out


class _DeviceBlock:
    """Device memory from granne_hip_device_malloc, freed with the object."""

    def __init__(self, nbytes, device):
        self.device, self.nbytes = device, int(nbytes)
        p = C.c_void_p()
        check(lib().granne_hip_device_malloc(C.byref(p), max(self.nbytes, 16), device))
        self.ptr = p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        check(lib().granne_hip_copy_to_device(C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p), a.nbytes, self.device, None))
        check(lib().granne_hip_stream_synchronize(None, self.device))
        return self

    def download(self, dtype, count):
        out = np.empty(count, dtype)
        check(lib().granne_hip_copy_to_host(out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr), out.nbytes, self.device, None))
        check(lib().granne_hip_stream_synchronize(None, self.device))
        return out

    def close(self):
        if getattr(self, "ptr", None):
            lib().granne_hip_device_free(C.c_void_p(self.ptr), self.device)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Filter:
    """A bitmap over the ids 0..n-1 on one device. `ptr` is its raw device pointer (filter_words(n) u32 words)."""

    def __init__(self, n, device=0):
        self.n, self.device = int(n), device
        self._block = _DeviceBlock(filter_words(self.n) * 4, device)
        self.bad = 0  # from_ids: ids >= n it was given (not written)

    @property
    def ptr(self):
        return self._block.ptr

    @classmethod
    def from_ids(cls, ids, n, device=0):
        """The bitmap with the bits of `ids` set; duplicates are harmless, ids >= n are left out and counted in `.bad`."""
        ids = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        f = cls(n, device)
        d_ids = _DeviceBlock(ids.nbytes + 4, device)
        d_ids.upload(ids)
        d_bad = _DeviceBlock(4, device).upload(np.zeros(1, np.uint32))
        check(lib().granne_hip_filter_from_ids_device(C.c_void_p(d_ids.ptr), ids.size, f.n, C.c_void_p(f.ptr), C.c_void_p(d_bad.ptr),
                                                      device, None))
        f.bad = int(d_bad.download(np.uint32, 1)[0])
        return f

    @classmethod
    def from_mask(cls, mask, device=0):
        """The bitmap of a bool (or 0 / non-zero) array, one entry per id."""
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        f = cls(m.size, device)
        d_mask = _DeviceBlock(m.nbytes, device).upload(m)
        check(lib().granne_hip_filter_from_mask_device(C.c_void_p(d_mask.ptr), f.n, C.c_void_p(f.ptr), device, None))
        check(lib().granne_hip_stream_synchronize(None, device))
        return f

    @classmethod
    def from_words(cls, words, n, device=0):
        """The bitmap whose u32 words the caller packed (at least filter_words(n) of them)."""
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        if w.size < filter_words(n):
            raise ValueError("need %d words" % filter_words(n))
        f = cls(n, device)
        f._block.upload(w[:filter_words(n)])
        return f

    def count(self):
        """Number of set bits among the first n."""
        d_out = _DeviceBlock(8, self.device)
        check(lib().granne_hip_filter_count_device(C.c_void_p(self.ptr), self.n, C.c_void_p(d_out.ptr), self.device, None))
        return int(d_out.download(np.uint64, 1)[0])

    def ids(self):
        """The allowed ids, ascending, as a uint64 array: what `from_ids` would take back
        (granne_hip_filter_to_ids_device)."""
        d_ids = _DeviceBlock(self.n * 8, self.device)
        d_count = _DeviceBlock(8, self.device)
        check(lib().granne_hip_filter_to_ids_device(C.c_void_p(self.ptr), self.n, C.c_void_p(d_ids.ptr), C.c_void_p(d_count.ptr),
                                                    self.device, None))
        m = int(d_count.download(np.uint64, 1)[0])
        return d_ids.download(np.uint64, m)

    def words(self):
        """The bitmap's u32 words, copied to the host."""
        return self._block.download(np.uint32, filter_words(self.n))

    def close(self):
        self._block.close()
