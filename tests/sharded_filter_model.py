"""The host model of filters and the exact selection on a partitioned index (TEST INFRASTRUCTURE, a plain module like
tests/filter_model.py and tests/exact_topk_filtered_model.py, both of which it builds on):

  * slice_words: the bitmap slice in numpy, bit by bit -- what granne_hip_filter_slice_device must write;
  * expected_filtered: every shard's modelled filtered walk under mask[off : off + len], merged by oracle.merge;
  * expected_exact: the oracle's scan over the allowed rows of the CONCATENATED set -- it knows nothing of shards;
  * the fixture the CPU and GPU tests share: 4037 rows cut into shards of 31, 33, 937, 1000 and 2036 rows, so that two
    shards share a bitmap word (offsets 0 and 31), one offset is aligned and non-zero (64), two are not (1001, 2001) and
    the last shard ends mid-word."""
import numpy as np

from oracle.merge import merge_topk_numpy
from tests import exact_topk_filtered_model as etm
from tests import filter_model as fm

LENGTHS = [31, 33, 937, 1000, 2036]
N, DIM, NQ = sum(LENGTHS), 32, 50
U64_MAX = np.iinfo(np.uint64).max


def offsets(lengths=LENGTHS, gap=0):
    """the first global id of every shard; `gap` unused ids between two shards"""
    out, at = [], 0
    for n in lengths:
        out.append(at)
        at += n + gap
    return out


def id_span(lengths, offs):
    return max(o + n for o, n in zip(offs, lengths))


def fixture_rows(oracle, int8, seed=4037):
    """(elements [4037, 32], queries [50, 32]) prepared as the element type wants them; queries 0 and 1 are rows of the set
    (row 17 of the first shard, row 5 of the last), so distance 0 is among the answers"""
    rng = np.random.default_rng(seed)
    prep = oracle.quantize if int8 else oracle.normalize_f32
    el = prep((rng.random((N, DIM), dtype=np.float32) - np.float32(0.5)).astype(np.float32))
    q = prep((rng.random((NQ, DIM), dtype=np.float32) - np.float32(0.5)).astype(np.float32))
    q[0], q[1] = el[17], el[offsets()[-1] + 5]
    return el, q


def to_global(mask_local_parts, lengths, offs):
    """per-shard bool masks laid out over the global ids (gaps False)"""
    out = np.zeros(id_span(lengths, offs), bool)
    for part, n, o in zip(mask_local_parts, lengths, offs):
        out[o:o + n] = part
    return out


def slice_words(words, n_bits, first_bit, n_out_bits):
    """Bits [first_bit, first_bit + n_out_bits) of a bitmap over n_bits ids as ceil(n_out_bits / 32) u32 words: source bits
    at positions >= n_bits are 0 whatever `words` holds there, the bits past n_out_bits of the last word are 0."""
    words = np.ascontiguousarray(words, np.uint32)
    n_words = (n_bits + 31) // 32
    bits = np.unpackbits(words[:n_words].view(np.uint8), bitorder="little")[:n_bits].astype(bool)
    src = np.zeros(first_bit + n_out_bits, bool)
    m = min(len(src), n_bits)
    src[:m] = bits[:m]
    return fm.pack_bits(src[first_bit:first_bit + n_out_bits])


def merge(parts, offs, k):
    """[(ids, dists, counts)] per shard -> the merged (ids, dists, counts): oracle.merge"""
    return merge_topk_numpy(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]), offs, k)


def shard_walks(layers, el, q, allowed, max_search, k, max_expand=0, D=None, cache=None):
    """One shard's modelled batch: ids [nq, k] u64 (local), dists, counts, and how many walks max_expand cut. allowed:
    [n] (shared) or [nq, n] bool over the shard's ids; D: optionally [nq, n] distances (filter_model's dist_row)."""
    nq = len(q)
    ids, ds = np.full((nq, k), U64_MAX, np.uint64), np.full((nq, k), np.inf, np.float32)
    cnt, cut = np.zeros(nq, np.uint32), 0
    allowed = np.asarray(allowed, bool)
    for i in range(nq):
        r = fm.search_filtered(layers, el, q[i], allowed[i] if allowed.ndim == 2 else allowed, max_search, k, max_expand,
                               None if D is None else D[i], cache)
        ids[i], ds[i] = r.padded(k)
        cnt[i] = r.count
        cut += int(r.cut)
    return ids, ds, cnt, cut


def expected_filtered(shards, q, mask, offs, max_search, k, max_expand=0):
    """shards: [(layers, elements, D or None, cache list)] in shard order; mask: [span] or [nq, span] bool over global ids.
    Returns (ids, dists, counts, walks cut over all shards)."""
    mask = np.asarray(mask, bool)
    parts, cut = [], 0
    for (layers, el, D, cache), o in zip(shards, offs):
        local = mask[..., o:o + len(el)]
        i, d, c, t = shard_walks(layers, el, q, local, max_search, k, max_expand, D, cache)
        parts.append((i, d, c))
        cut += t
    return merge(parts, offs, k) + (cut,)


def expected_exact(oracle, el_global, mask, q, k):
    """The exact answer over the concatenated set (el_global: [span, dim], rows of gaps anything; mask: [span] or
    [nq, span] bool, False in gaps): exact_topk_filtered_model.oracle_subset -- independent of the shards."""
    mask = np.asarray(mask, bool)
    if mask.ndim == 1:
        return etm.oracle_subset(oracle, el_global, mask, q, k)
    rows = [etm.oracle_subset(oracle, el_global, mask[i], q[i:i + 1], k) for i in range(len(q))]
    return tuple(np.concatenate([r[j] for r in rows]) for j in range(3))
