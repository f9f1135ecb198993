"""The host layer gives back every byte of device memory it takes: builders, indexes, reorder, host-pointer searches, the
exact scan, from_csr and a from_csr that fails half way own their device memory through granne_amd/csrc/dev_mem.h, so a
cycle of all of them leaves the device's free memory where it was."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.conftest import random_floats  # noqa: E402

N, NN, MAX_SEARCH, CYCLES = 2000, 8, 30, 20
# Bytes of free device memory that CYCLES cycles may cost: what this same test showed on the commit before the owners
# (every free written by hand), on an MI355X: 0 bytes over 20 cycles. With the owners: 0 bytes. (The indexes of ONE cycle
# hold 6,939,512 bytes: a cycle that kept any of its blocks would show.)
ALLOWED_DRIFT = 0


def _csr(layers):
    """A builder's fixed-width rows (UNUSED padded) as per-layer (offsets, ids)."""
    offs, ids = [], []
    for rows in layers:
        keep = rows != 0xFFFFFFFF
        offs.append(np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint64))
        ids.append(rows[keep].astype(np.uint32))
    return offs, ids


def _cycle(ga, et, el, extra, q):
    """Everything of the host layer that allocates, once; returns the bytes the cycle's indexes held on the device."""
    from granne_amd import _lib
    held = 0
    b = ga.GranneBuilder(et, el, num_neighbors=NN, max_search=MAX_SEARCH)
    b.build()
    for row in extra:
        b.append(row)
    b.build()
    assert len(b) == len(el) + len(extra)
    layers = b.layers()
    ix = b.get_index()
    ix.reorder()
    ids, _, cnt = ix.search_batch(q, MAX_SEARCH, 10)
    one = ix.search(q[0], MAX_SEARCH, 10)
    assert (cnt == 10).all() and len(one) == 10
    bf = ix.brute_force(q, 10)
    assert bf[0].shape == (len(q), 10)
    held += ix.hbm_bytes()
    offs, idl = _csr(layers)
    rows = np.concatenate([el, extra])
    cx = ga.Granne.from_csr(et, rows, offs, idl)
    held += cx.hbm_bytes()
    idl[-1] = idl[-1].copy()
    idl[-1][-1] = len(rows)  # a neighbor id outside its layer: refused after the elements are on the device
    with pytest.raises(_lib.GranneHipError) as err:
        ga.Granne.from_csr(et, rows, offs, idl)
    assert err.value.code == _lib.ERR_INVALID
    cx.close()
    ix.close()
    b.close()
    return held


def test_device_memory_is_balanced_over_build_search_reorder_cycles(oracle):
    """Free device memory (torch.cuda.mem_get_info) after one warm-up cycle (code objects load on first use) and after
    CYCLES more, over 2,000 x 100-d f32 rows and 2,000 x 128 int8 rows. Refined search is left out: its stream-ordered pool
    keeps memory by design. The allowance is what the commit before the owners showed under this same test: a drift of
    0 bytes there, 0 bytes with the owners, 6,939,512 bytes held by the indexes of one cycle."""
    import torch
    import granne_amd as ga
    rng = np.random.default_rng(20)
    shapes = []
    for et, dim, int8 in (("angular", 100, False), ("angular_int", 128, True)):
        raw = random_floats(rng, N + 3 + 16, dim)
        rows = oracle.quantize(raw) if int8 else oracle.normalize_f32(raw)
        shapes.append((et, rows[:N], rows[N:N + 3], rows[N + 3:]))

    def cycle():
        return sum(_cycle(ga, et, el, extra, q) for et, el, extra, q in shapes)

    cycle_bytes = cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info(0)
    for _ in range(CYCLES):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info(0)
    drift = free0 - free1
    print("free before %d, after %d cycles %d: drift %d bytes (one cycle's indexes hold %d)" % (free0, CYCLES, free1, drift, cycle_bytes))
    assert drift <= ALLOWED_DRIFT
