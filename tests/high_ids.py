"""Checks of the row-reading operators at ids whose rows lie past byte offset 2^32 of an index's device rows (test
infrastructure, shared by test_gpu_fullsize.py and test_gpu_past_4gib.py).

Every operator finds a row at `elements + id * row_stride`. With the product taken in 32 bits, id reads the bytes at
(id * row_stride) mod 2^32 -- for a stride that divides 2^32 (128, 512) the row of id - 2^32 / row_stride, for the 896
bytes of 200-d f32 rows a window that straddles two lower rows. The checks here compare against rows fetched from the
caller's own device tensor by torch indexing (independent of the library) and `aliases_differ` asserts that the row such
a truncation would read instead holds other bytes, so a truncated product cannot pass.

Host reference: the CPU oracle's distance (oracle.dist) and tests/refine_model.py; the exact scan's reference is made
in two stages (scan_reference)."""
import ctypes as C

import numpy as np
import pytest

from granne_amd._lib import GranneHipError

MARK = 1 << 32


def device_row_stride(kind, dim):
    """Bytes from one device row to the next (granne_hip.hip device_row_stride): f32 rows are padded to 16 bytes and, from
    256 bytes on, to a 128-byte line; rows of halves likewise from 128 bytes on; int8 rows (up to 1024 components) to a
    power of two of at least 16. The tests that can see it through hbm_bytes assert it."""
    if kind == "f32":
        rb = (dim * 4 + 15) & ~15
        return (rb + 127) & ~127 if rb >= 256 else rb
    if kind == "f16":
        rb = (dim * 2 + 15) & ~15
        return (rb + 127) & ~127 if rb >= 128 else rb
    assert kind == "i8" and dim <= 1024
    rb = 16
    while rb < dim:
        rb *= 2
    return rb


def first_high(row_stride):
    """the smallest id whose row starts at or past byte offset 2^32"""
    return -(-MARK // row_stride)


class Range:
    """The ids a test draws from: [top0, n) is "high". past: top0 is the first id past the 4 GiB mark; otherwise the
    index is smaller than that and top0 is just the start of the top of its id range."""

    def __init__(self, n, row_stride, what):
        self.n, self.row_stride = n, row_stride
        fh = first_high(row_stride)
        self.past = fh < n
        self.top0 = fh if self.past else n - max(1, min(n // 2, 1 << 20))
        if self.past:
            print("%s: ids %d .. %d lie past the 4 GiB mark (row stride %d)" % (what, fh, n - 1, row_stride))
        else:
            print("%s: %d rows of %d bytes end below the 4 GiB mark; checked on ids %d .. %d, the top of the range"
                  % (what, n, row_stride, self.top0, n - 1))

    def mix(self, rng, count):
        """count ids: half from [top0, n), half below, with n - 1, top0 and top0 - 1 among them"""
        hi = rng.integers(self.top0, self.n, count // 2)
        lo = rng.integers(0, max(self.top0, 1), count - count // 2)
        ids = np.concatenate([hi, lo])[rng.permutation(count)].astype(np.int64)
        ids[:3] = self.n - 1, self.top0, max(self.top0 - 1, 0)  # (the first three places: a caller that overwrites an entry takes a later one)
        return ids

    def assert_covers(self, ids):
        """the "ids past the mark were used" assertions: conditional on the index reaching the mark"""
        ids = np.asarray(ids).reshape(-1).astype(np.int64)
        ids = ids[ids < self.n]
        if not self.past:
            print("  (index below the mark: the past-the-mark assertions did not run)")
            return
        have = set(ids.tolist())
        assert self.n - 1 in have and self.top0 in have and self.top0 - 1 in have
        assert len({i for i in have if i >= self.top0}) >= 1003
        print("  past-the-mark assertions ran: %d distinct ids >= %d" % (len({i for i in have if i >= self.top0}), self.top0))


def _stream(dev):
    """the current stream of the tensors' device, synchronised: what was queued before is done when a pointer is handed
    over, and a call made with it is waited for by the caller's next copy to the host on that stream"""
    import torch
    if dev.type != "cuda":
        return 0
    torch.cuda.synchronize(dev)
    return torch.cuda.current_stream(dev).cuda_stream


def fetch(el, ids):
    """rows of the device tensor `el` by torch indexing: the library has no part in it"""
    import torch
    idx = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(el.device)
    return el[idx].cpu().numpy()


def aliases_differ(el, rng_ids, R):
    """The row a 32-bit product would read instead of id's: bytes (id * stride) mod 2^32 of the device rows. For a stride
    that divides 2^32 that is row id - 2^32 / stride, whole; otherwise it starts inside a lower row. Asserts that those
    bytes are not the row's own (they are other pseudo-random rows), for the high ids of `rng_ids`."""
    if not R.past:
        return
    ids = np.unique(np.asarray(rng_ids).reshape(-1).astype(np.int64))
    ids = ids[(ids >= R.top0) & (ids < R.n)][:256]
    own = fetch(el, ids)
    low = (ids * R.row_stride) % MARK // R.row_stride  # the row the truncated offset falls into
    assert (low < R.top0).all() and (low != ids).all()
    other = fetch(el, low)
    assert not (own.reshape(len(ids), -1) == other.reshape(len(ids), -1)).all(axis=1).any()


class FetchedRows:
    """refine_model.refine's `rows`: len() = n, [id] = the prepared host row of id, fetched once for all candidates"""

    def __init__(self, n, ids, rows):
        self.n = n
        self.rows = {int(i): rows[j] for j, i in enumerate(ids)}

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.rows[int(i)]


def check_get_element(ix, el, R, rng, count=1200):
    """get_element at `count` ids (a synchronous copy each) against the caller's rows"""
    ids = R.mix(rng, count)
    if R.past:  # 1,003 distinct high ids at least
        ids[3: count - 100] = rng.choice(np.arange(R.top0, R.n), count - 103, replace=False)
    R.assert_covers(ids)
    aliases_differ(el, ids, R)
    want = fetch(el, ids)
    for j, i in enumerate(ids.tolist()):
        assert ix.get_element(i).tobytes() == want[j].tobytes(), i
    return ids


def check_dists(oracle, ix, el, prep, q, R, rng):
    """dists_many (64 queries x 128 ids, with its status word) and the pair form (8,192 pairs): bit-equal to oracle.dist
    over rows fetched from `el` (`prep`: fetched rows -> the rows the index stands for); one id >= n gives +inf and a
    status count of 1 in the batched form (include/granne_hip.h, granne_hip_dists_device); the pair form's host entry has
    no status word and refuses a call that names such an id."""
    import torch
    n = R.n
    q = np.ascontiguousarray(q[:64])
    ids = R.mix(rng, 64 * 128).reshape(64, 128)
    oob = (5, 77)
    valid = np.ones(ids.shape, bool)
    valid[oob] = False
    R.assert_covers(ids[valid])
    aliases_differ(el, ids[valid], R)
    rows = prep(fetch(el, ids[valid]))
    want = np.full(ids.shape, np.inf, np.float32)
    want[valid] = [oracle.dist(rows[j], q[qi]) for j, qi in enumerate(np.nonzero(valid)[0])]
    send = ids.astype(np.uint32)
    send[oob] = n  # the first id that is no element
    # dists_many computes the same without the status word; the device entry is called here for it
    got_many = ix.dists_many(q, send)
    dev = el.device
    tq = torch.from_numpy(q.view(np.uint8).reshape(64, -1)).to(dev)
    ti = torch.from_numpy(send.view(np.int32)).to(dev)
    out = torch.empty((64, 128), dtype=torch.float32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    ix.dists_device(tq.data_ptr(), 64, ti.data_ptr(), 128, out.data_ptr(), st.data_ptr(), _stream(dev))
    got = out.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert got_many.tobytes() == want.tobytes()
    assert np.isinf(got[oob]) and int(st.item()) == 1
    # the pair form: (query qidx[t], element ids[t])
    pid = R.mix(rng, 8192)
    qidx = rng.integers(0, 64, 8192).astype(np.uint32)
    R.assert_covers(pid)
    prow = prep(fetch(el, pid))
    pw = np.array([oracle.dist(prow[t], q[qidx[t]]) for t in range(8192)], np.float32)
    send = pid.astype(np.uint32)
    assert ix.dists(q, qidx, send).tobytes() == pw.tobytes()
    # (dist_to_element of an id that is no element: the host entry of the pair form refuses the call, it has no status word)
    send[4000] = n
    with pytest.raises(GranneHipError, match="element id out of range"):
        ix.dists(q, qidx, send)


def check_refine(oracle, ix, el, prep, q, R, rng):
    """refine(k = 10) of 64 ragged lists of up to 257 candidates against tests/refine_model.py: ids, distance bytes,
    counts and the dropped word; one candidate >= n is dropped and counted."""
    from tests import refine_model
    n, m = R.n, 257
    q = np.ascontiguousarray(q[:64])
    cand = R.mix(rng, 64 * m).reshape(64, m).astype(np.uint64)
    counts = rng.integers(0, m + 1, 64).astype(np.uint32)
    counts[0], counts[1], counts[2], counts[3] = m, 0, 1, 33
    cand[0, 100] = n + 12345  # inside list 0 (which also holds mix()'s n - 1, top0 and top0 - 1): dropped
    inside = np.arange(m)[None, :] < counts[:, None]
    inside[0, 100] = False
    used = cand[inside].astype(np.int64)
    R.assert_covers(used)
    aliases_differ(el, used, R)
    uniq = np.unique(used)
    rows = FetchedRows(n, uniq, prep(fetch(el, uniq)))
    w_ids, w_ds, w_cnt, w_drop = refine_model.refine(oracle, rows, q, cand, counts, 10)
    ids, ds, cnt, drop = ix.refine(q, cand, counts, k=10, dropped=True)
    assert w_drop == 1 and drop == 1
    assert (cnt == w_cnt).all() and (ids == w_ids).all() and ds.tobytes() == w_ds.tobytes()


def scan_reference(oracle, el, prep, q, kind, keep=256):
    """The exact scan's reference in two stages. Stage 1 (device, torch, float64, chunks of 1M rows): the float64 distance
    of every row to every query -- for int8 rows from exact integer dots and norms -- keeping the `keep` best per query.
    Stage 2: oracle.dist on the fetched shortlist, ranked by (dist, id). Returns (ids [nq, keep], oracle dists [nq, keep],
    both in the oracle's order; the float64 distances of the shortlist ascending [nq, keep])."""
    import torch
    n, nq = el.shape[0], len(q)
    dev = el.device
    tq = torch.from_numpy(np.ascontiguousarray(q)).to(dev).double()
    if kind == "i8":
        qn = tq.square().sum(1).sqrt()
    best_d = torch.full((nq, 0), 0.0, dtype=torch.float64, device=dev)
    best_i = torch.zeros((nq, 0), dtype=torch.int64, device=dev)
    for r0 in range(0, n, 1 << 20):
        x = el[r0:r0 + (1 << 20)].double()
        dot = tq @ x.T
        if kind == "i8":
            d = 1.0 - dot / (qn[:, None] * x.square().sum(1).sqrt()[None, :])
        else:
            d = 1.0 - dot
        ids = torch.arange(r0, r0 + x.shape[0], device=dev)[None, :].expand(nq, -1)
        d, ids = torch.cat([best_d, d], 1), torch.cat([best_i, ids], 1)
        best_d, pos = torch.topk(d, min(keep, d.shape[1]), dim=1, largest=False)
        best_i = torch.gather(ids, 1, pos)
        del x, dot, d, ids
    d64 = best_d.cpu().numpy()
    short = best_i.cpu().numpy()
    order = np.argsort(d64, axis=1, kind="stable")
    d64, short = np.take_along_axis(d64, order, 1), np.take_along_axis(short, order, 1)
    rows = prep(fetch(el, short.reshape(-1))).reshape(nq, short.shape[1], -1)
    od = np.array([[oracle.dist(rows[a, b], q[a]) for b in range(short.shape[1])] for a in range(nq)], np.float32)
    rank = np.array([np.lexsort((short[a], od[a])) for a in range(nq)])
    return np.take_along_axis(short, rank, 1), np.take_along_axis(od, rank, 1), d64


def check_exact_scan(oracle, ix, el, prep, q, kind, members, ks=(10, 16)):
    """brute_force against the two-stage reference, with the assertions and tolerances of tests/test_gpu_bruteforce.py.
    members: {query index: id of the member row that query is}; rank 0 of such a query is the member at the oracle's
    self-distance, or a row with the same bytes and a smaller id. Guard, on the reference alone: the shortlist's last float64 distance exceeds the oracle's
    16th by 1e-3 at least (the oracle's f32 dot of unit rows is within dim * 2^-24 <= 1.2e-5 of the exact one, so nothing
    outside the shortlist can be among the oracle's 16 best); 64 kept rows are tried first, 256 if they do not reach it."""
    from tests.test_gpu_bruteforce import TOL, TOL_F32
    tol = TOL if kind == "i8" else TOL_F32
    ref_i, ref_d, d64 = scan_reference(oracle, el, prep, q, kind, keep=256)
    gap64, gap256 = d64[:, 63] - ref_d[:, 15], d64[:, 255] - ref_d[:, 15]
    print("  shortlist guard: 64th float64 distance - oracle's 16th: min %.4g; 256th: min %.4g" % (gap64.min(), gap256.min()))
    # (the reference ranks all 256 whichever passes: the guard says that they hold the oracle's 16 best)
    assert (gap64 >= 1e-3).all() or (gap256 >= 1e-3).all()
    nq = len(q)
    for k in ks:
        ids, ds, cnt = ix.brute_force(q, k)
        ids2, ds2, cnt2 = ix.brute_force(q, k)
        assert (ids == ids2).all() and ds.tobytes() == ds2.tobytes() and (cnt == cnt2).all()
        assert (cnt == k).all()
        want_i, want_d = ref_i[:, :k].astype(np.uint64), ref_d[:, :k]
        rows = prep(fetch(el, ids.reshape(-1).astype(np.int64))).reshape(nq, k, -1)
        for qi in range(nq):
            got = np.array([oracle.dist(rows[qi, j], q[qi]) for j in range(k)], np.float32)
            assert got.tobytes() == ds[qi].tobytes(), qi
            keys = list(zip(ds[qi].tolist(), ids[qi].tolist()))
            assert keys == sorted(keys) and len(set(ids[qi].tolist())) == k
        assert np.abs(ds - want_d).max() <= tol
        same = ids == want_i
        assert same.mean() > 0.98, same.mean()
        for qi, j in zip(*np.nonzero(~same)):
            assert abs(float(ds[qi, j]) - float(want_d[qi, j])) <= tol
        for qi, mem in members.items():
            # the member itself, unless the reference names an exact twin with a smaller id
            assert int(ids[qi, 0]) == int(want_i[qi, 0]), (qi, ids[qi, 0], want_i[qi, 0])
            if int(want_i[qi, 0]) != mem:
                tw = int(want_i[qi, 0])
                assert tw < mem and fetch(el, [tw]).tobytes() == fetch(el, [mem]).tobytes(), (qi, mem, tw)
            self_d = np.float32(oracle.dist(prep(fetch(el, [mem]))[0], q[qi]))
            assert ds[qi, 0].tobytes() == self_d.tobytes()
    return ref_i, ref_d


def synth(lib_mod, seed, row0, rows, dim, kind):
    """rows row0 .. row0 + rows - 1 of the synthetic set `seed`, prepared on the device: normalised f32, quantised int8,
    or raw (kind None)"""
    import torch
    lib = lib_mod.lib()
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    raw = torch.empty((rows, dim), dtype=torch.float32, device="cuda")
    lib_mod.check(lib.granne_hip_synth_rows_device(C.c_void_p(raw.data_ptr()), seed, row0, rows, dim, 0, sp))
    if kind == "f32":
        lib_mod.check(lib.granne_hip_normalize_f32_device(C.c_void_p(raw.data_ptr()), rows, dim, 0, sp))
    elif kind == "i8":
        out = torch.empty((rows, dim), dtype=torch.int8, device="cuda")
        lib_mod.check(lib.granne_hip_quantize_f32_device(C.c_void_p(raw.data_ptr()), C.c_void_p(out.data_ptr()), rows, dim, 0, sp))
        torch.cuda.synchronize()
        return out
    torch.cuda.synchronize()
    return raw
