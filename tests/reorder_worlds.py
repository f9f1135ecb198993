"""Seeded inputs of the reorder tests (test infrastructure, a plain module like tests/value_edges.py): indexes that send
Granne::reorder's trail walks (granne_amd/csrc/reorder_host.h) to every kernel plan_walk can hand them to, rows with exact
ties, hand-made adjacency rows for remap_rows_kernel, a ring on which a trail walk visits hundreds of nodes, and keys for
reorder_by_keys. tests/test_reorder_worlds_host.py holds these inputs, on the oracle alone, to the conditions that make
them worth running; tests/test_gpu_reorder_forms.py reorders exactly these on the GPU.

Every maker is seeded and returns the same arrays on every call; nothing is cached here (the tests keep what they share)."""
import ctypes as C

import numpy as np

from oracle import oracle as orc
from tests.scan_forms import structured_rows, uniform_rows

UNUSED = orc.UNUSED
MULT = 5.0

# name -> (int8, dim, rows, num_neighbors, the walker a trail launch takes). Uniform rows, layer_multiplier 5.
#   register: fast_kernel<DT, DIM, 1, true>; general: search_kernel<DT, 0, 1, true> -- layers of 64 device ids and wider
#   (num_neighbors 33 and more), int8 rows beyond 512 bytes
BUILT = {
    "i8_200": (True, 200, 1500, 20, "register"),     # fast_kernel<DT_I8, 256, 1, true>: 256-byte rows
    "i8_300": (True, 300, 1200, 20, "register"),     # fast_kernel<DT_I8, 512, 1, true>: 512-byte rows
    "i8_600": (True, 600, 900, 16, "general"),       # search_kernel<DT_I8, 0, 1, true>: rows beyond 512 bytes
    "f32_28_nn40": (False, 28, 1500, 40, "general"),   # search_kernel<DT_F32, 0, 1, true>: 64 device ids
    "f32_100_nn63": (False, 100, 2000, 63, "general"),
    "i8_100_nn40": (True, 100, 1500, 40, "general"),
}

# name -> (kind of rows, rows, dim, int8): exact ties. All on the register trail walkers (num_neighbors 20).
TIED = {
    "duplicates_f32": ("duplicates", 1600, 100, False), "duplicates_i8": ("duplicates", 1600, 100, True),
    "grid_f32": ("grid", 2000, 100, False), "grid_i8": ("grid", 2000, 100, True),
    "clones_f32": ("clones", 3000, 100, False), "clones_i8": ("clones", 3000, 100, True),
    "zero7_f32": ("zero7", 800, 16, False),
}

# name -> (int8, dim, links to either side, walker). 1,000 nodes on a circle, 1,200 more at seeded angles.
RING = {
    "f32_2": (False, 2, 8, "register"), "f32_100": (False, 100, 8, "register"), "i8_100": (True, 100, 8, "register"),
    "f32_100_wide": (False, 100, 20, "general"),  # 40 ids a row: 64 device ids
}
RING_NODES, RING_ALL = 1000, 2200


def prep(raw, int8):
    return orc.quantize(raw) if int8 else orc.normalize_f32(raw)


def _seed(name):
    return 7000 + sum(ord(c) * (i + 1) for i, c in enumerate(name))


def clones(rng, n, dim=100, groups=60, copies=40):
    """tests/test_gpu_large_launch_entries.py's `_clones`: groups x copies rows that are exact copies of each other, the
    rest uniform, in random order."""
    base = uniform_rows(rng, groups, dim)
    rows = np.concatenate([np.repeat(base, copies, axis=0), uniform_rows(rng, n - groups * copies, dim)])
    return rows[rng.permutation(n)]


def built(name):
    """(oracle index, queries) of a BUILT case."""
    int8, dim, n, nn, _ = BUILT[name]
    rng = np.random.default_rng(_seed(name))
    el = prep(uniform_rows(rng, n, dim), int8)
    oix = orc.build_index(el, num_neighbors=nn, max_search=max(20, nn), layer_multiplier=MULT, n_threads=4)
    return oix, queries(rng, el, dim, int8)


def queries(rng, el, dim, int8, drawn=32):
    """five members (reorder.rs:311-320) and `drawn` uniform queries"""
    n = len(el)
    members = el[[0, 10 % n, 123 % n, 99 % n, n - 1]]
    return np.concatenate([members, prep(uniform_rows(rng, drawn, dim), int8)])


def wide_rows():
    """A hand-made two-layer index whose rows hold up to 100 ids, as test_wide_rows_and_large_degree makes its own:
    12 + 600 rows of 12-d f32, declared width 100 (128 device ids: the general trail walker)."""
    rng = np.random.default_rng(_seed("wide_rows"))
    el = prep(uniform_rows(rng, 600, 12), False)
    layer = np.full((600, 100), UNUSED, np.uint32)
    for i in range(600):
        d = int(rng.integers(0, 101))
        layer[i, :d] = rng.choice(600, d, replace=False)
    layer[0, :100] = rng.choice(600, 100, replace=False)
    top = np.full((12, 100), UNUSED, np.uint32)
    for i in range(12):
        top[i, :4] = rng.choice(12, 4, replace=False)
    return orc.Index(el, [top, layer]), queries(rng, el, 12, False)


def tied_rows(name):
    kind, n, dim, int8 = TIED[name]
    rng = np.random.default_rng(_seed(kind))  # (the int8 case quantises the f32 case's rows)
    if kind == "clones":
        raw = clones(rng, n, dim)
    elif kind == "zero7":
        raw = uniform_rows(rng, n, dim)
        raw[::7] = 0
    else:
        raw = structured_rows(kind, rng, n, dim)
    return prep(raw, int8), rng


def tied(name, n_threads=4):
    """(oracle index, queries) of a TIED case: num_neighbors 20, built at max_search 20."""
    kind, n, dim, int8 = TIED[name]
    el, rng = tied_rows(name)
    oix = orc.build_index(el, num_neighbors=20, max_search=20, layer_multiplier=MULT, n_threads=n_threads)
    return oix, queries(rng, el, dim, int8)


def copies_above(oix):
    """(rows that only the bottom layer holds, how many of them have a byte-identical copy in the layer above)"""
    lo = oix.layers[-2].shape[0]
    above = {oix.elements[i].tobytes() for i in range(lo)}
    return len(oix) - lo, sum(oix.elements[i].tobytes() in above for i in range(lo, len(oix)))


# widths the edge-row index declares, one layer each, and the layers' lengths
EDGE_WIDTHS = (32, 33, 64, 100)
EDGE_LENS = (110, 240, 500, 900)
EDGE_EMPTY, EDGE_FULL, EDGE_TWICE, EDGE_THRICE, EDGE_AFTER_UNUSED = 1, 2, 3, 4, 5  # the rows of every layer that hold them


def edge_rows():
    """One hand-made index of four layers with declared widths 32, 33, 64 and 100 (32, 64, 64 and 128 device ids), 12-d
    f32 rows. In every layer: row 1 is empty, row 2 is full (no UNUSED), row 3 names an id twice, row 4 names an id three
    times (and is full), row 5 holds in-range ids after its first UNUSED, which get_neighbors drops
    (src/index/mod.rs:540-552); every other row holds 0 .. width distinct ids, row 0 at least eight."""
    rng = np.random.default_rng(_seed("edge_rows"))
    n = EDGE_LENS[-1]
    el = prep(uniform_rows(rng, n, 12), False)
    layers = []
    for W, L in zip(EDGE_WIDTHS, EDGE_LENS):
        rows = np.full((L, W), UNUSED, np.uint32)
        for i in range(L):
            d = int(rng.integers(8 if i == 0 else 0, W + 1))
            rows[i, :d] = rng.choice(L, d, replace=False)
        rows[EDGE_EMPTY] = UNUSED
        rows[EDGE_FULL] = rng.choice(L, W, replace=False)
        rows[EDGE_TWICE] = UNUSED
        rows[EDGE_TWICE, :W - 3] = rng.choice(L, W - 3, replace=False)
        rows[EDGE_TWICE, W - 4] = rows[EDGE_TWICE, 1]
        rows[EDGE_THRICE] = rng.choice(L, W, replace=False)
        rows[EDGE_THRICE, W // 2] = rows[EDGE_THRICE, 0]
        rows[EDGE_THRICE, W - 1] = rows[EDGE_THRICE, 0]
        rows[EDGE_AFTER_UNUSED] = rng.choice(L, W, replace=False)
        rows[EDGE_AFTER_UNUSED, 5] = UNUSED
        layers.append(rows)
    return orc.Index(el, layers), queries(rng, el, 12, False)


def ring(name):
    """A hand-made two-layer index on which a trail walk is long. Layer 0: RING_NODES nodes at angle 2 pi i / RING_NODES
    on a circle, each linked to i +- 1 .. +- links. Layer 1: RING_ALL nodes, the others at seeded random angles (their
    rows hold eight random ids; no trail walks layer 1). A trail from node 0 walks round the circle to the row's
    nearest node. 100-d: the circle under a seeded rotation (two orthonormal directions)."""
    int8, dim, links, _ = RING[name]
    rng = np.random.default_rng(_seed("ring"))  # (the same angles in every case)
    angle = np.concatenate([2.0 * np.pi * np.arange(RING_NODES) / RING_NODES, rng.uniform(0.0, 2.0 * np.pi, RING_ALL - RING_NODES)])
    plane = np.stack([np.cos(angle), np.sin(angle)], axis=1)
    if dim == 2:
        raw = plane.astype(np.float32)
    else:
        basis, _r = np.linalg.qr(np.random.default_rng(_seed("rotation")).standard_normal((dim, 2)))
        raw = (plane @ basis.T).astype(np.float32)
    el = prep(raw, int8)
    W = 2 * links
    step = np.concatenate([np.arange(1, links + 1), -np.arange(1, links + 1)])
    top = ((np.arange(RING_NODES)[:, None] + step[None, :]) % RING_NODES).astype(np.uint32)
    bottom = np.full((RING_ALL, W), UNUSED, np.uint32)
    bottom[:RING_NODES] = top
    for i in range(RING_NODES, RING_ALL):
        bottom[i, :8] = rng.choice(RING_ALL, 8, replace=False)
    return orc.Index(el, [top, bottom]), queries(rng, el, dim, int8, drawn=11)


class _Counters(C.Structure):
    _fields_ = [("n_dist", C.c_uint64), ("n_expand", C.c_uint64), ("n_adj", C.c_uint64)]


def walk_counts(oix, layer, entrypoint, goals):
    """gro_search_for_neighbors' counters (n_dist, n_expand, n_adj) of a max_search 1 walk of `layer` from `entrypoint`
    towards every row of `goals`: int64 [len(goals), 3]. n_dist counts the distinct nodes the walk evaluates."""
    goals = np.ascontiguousarray(goals, oix.elements.dtype)
    out = np.zeros((len(goals), 3), np.int64)
    ids, ds = np.empty(1, np.uint64), np.empty(1, np.float32)
    for i, g in enumerate(goals):
        ctr = _Counters(0, 0, 0)
        n = orc.lib().gro_search_for_neighbors(C.byref(oix._c), layer, entrypoint, g.ctypes.data_as(C.c_void_p), 1,
                                               ids.ctypes.data_as(C.c_void_p), ds.ctypes.data_as(C.c_void_p), C.byref(ctr))
        assert n == 1
        out[i] = (ctr.n_dist, ctr.n_expand, ctr.n_adj)
    return out


def ring_bounds(oix):
    """(walks, lo, hi) of a ring's one trail launch. A walk that evaluates more than 256 distinct nodes cannot keep them
    in a visited table of 256 slots: at least `lo` walks are handed over. The table takes ids up to 7/8 of its slots
    (granne_hip.hip, front_eighths), so a walk of 128 nodes or fewer is never handed over: at most `hi` are."""
    lo0 = oix.layers[0].shape[0]
    n_dist = walk_counts(oix, 0, 0, oix.elements[lo0:])[:, 0]
    return len(n_dist), int((n_dist > 256).sum()), int((n_dist > 128).sum()), n_dist


def size_70k():
    """70,000 x 8-d f32, num_neighbors 8, built at max_search 10, layer_multiplier 8: layers of 3 .. 8,750, 70,000 rows.
    The bottom layer is more than remap_rows_kernel's 65,536 blocks: its grid-stride loop runs a second trip."""
    rng = np.random.default_rng(_seed("size_70k"))
    el = prep(uniform_rows(rng, 70000, 8), False)
    return orc.build_index(el, num_neighbors=8, max_search=10, layer_multiplier=8.0, n_threads=8)


def keys_world(single_top=False):
    """The index reorder_by_keys runs on: 4,000 x 16-d f32 at layer_multiplier 7 -- or, single_top, 2,187 = 3^7 rows at
    multiplier 3, whose top layer has one row."""
    rng = np.random.default_rng(_seed("keys"))
    n, mult = (2187, 3.0) if single_top else (4000, 7.0)
    el = prep(uniform_rows(rng, n, 16), False)
    return orc.build_index(el, num_neighbors=12, max_search=20, layer_multiplier=mult, n_threads=4)


def key_sets(n):
    """name -> u64 keys [n]"""
    rng = np.random.default_rng(_seed("key_sets"))
    one = np.uint64(1)
    small = rng.integers(0, 50, n).astype(np.uint64)
    return {
        "all_equal": np.full(n, 77, np.uint64),
        "descending": (np.uint64(n) - np.arange(n, dtype=np.uint64)),
        "above_bit_32": (small << np.uint64(32)) | np.uint64(0xABCD1234),
        "below_bit_32": small | (np.uint64(5) << np.uint64(40)),
        "extremes": np.where(rng.integers(0, 2, n) == 1, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)).astype(np.uint64),
        "mixed": (rng.integers(0, 3, n).astype(np.uint64) << np.uint64(33)) | rng.integers(0, 3, n).astype(np.uint64) | (one << np.uint64(63)),
    }


def lexsort_order(oix, keys):
    """reorder.rs:96-104 by numpy: (key, idx) ascending within each layer's own rows"""
    out, lo = [], 0
    for l in oix.layers:
        hi = l.shape[0]
        idx = np.arange(lo, hi)
        out.append(idx[np.lexsort((idx, keys[lo:hi]))])
        lo = hi
    return np.concatenate(out).astype(np.uint64)
