// filter.h -- filtered search: the walk under an id bitmap.
//
// The filter is `allowed`, one bit per element id: bit (id & 31) of u32 word (id >> 5). It applies to the BOTTOM layer's
// search_for_neighbors (the reference's src/index/mod.rs:999-1037); find_entrypoint (the upper layers, max_search 1) is
// unchanged and unfiltered -- those nodes only navigate. The reference's function with the two changes (hnswlib's
// semantic for a filter functor, written as a change to the reference's own loop):
//
//     while let Some((d, idx)) = pq.pop():
//         if res.is_full() && d > res.peek().0: break           # unchanged; res now holds allowed ids only
//         if n_expanded == max_expand && max_expand != 0: break  # NEW: work cap, counted in bottom-layer pops
//         if allowed(idx): res.push((d, idx))                    # NEW: only allowed ids enter res
//         n_expanded += 1
//         for n in get_neighbors(idx):                           # unchanged: disallowed nodes are traversed
//             if visited.insert(n):
//                 dist = ...
//                 if !res.is_full() || dist < res.peek().0: pq.push(...)
//
// The result is `res` ascending by (dist, id), count = min(num_neighbors, |res|). With every bit set and max_expand = 0
// the walk IS the unfiltered one, counters included. Bits at positions >= len() are never read: a walk tests the bits of
// node ids only.
//
// This file holds the filter's own pieces: the view a walker tests bits through, the second (disallowed) queue of the
// general walker (search_kernel.h, Walker<.., FILT = true>) with the rule by which it may drop a key, and the kernels that
// make, count and list bitmaps. The exact walker's part is in slow_kernel.h. The register walkers (walk_fast.h) have no
// filtered form: they keep no visited set and find a seen candidate by its rank in one list of max_search keys, which
// does not survive keys that are expanded but may not be returned.
#pragma once

#include "filter_slice.h"
#include "wave_prims.h"

namespace granne_hip {

// words of a bitmap over n ids
__host__ __device__ inline uint64_t filter_words(uint64_t n) { return (n + 31u) >> 5; }

// one query's bitmap
struct FilterView {
    const uint32_t* words;
    __device__ __forceinline__ uint32_t word_of(uint32_t id) const { return words[id >> 5]; }
    __device__ __forceinline__ static bool bit_of(uint32_t word, uint32_t id) { return (word >> (id & 31u)) & 1u; }
    __device__ __forceinline__ bool allowed(uint32_t id) const { return bit_of(word_of(id), id); }
};

// What a filtered general walker carries beside the unfiltered one's state: its query's bitmap, the queue of DISALLOWED
// keys (64 * FILTER_QD_S entries; the allowed keys stay in Walker::pq, whose size and drop rule are the unfiltered
// walker's, so a filter of all ones hands over exactly the walks it did before), whether the layer in hand is filtered
// (the bottom one) and whether max_expand cut the walk. Filtered instantiations only: Walker<.., FILT = false> holds the
// empty form and compiles to what it did.
constexpr int FILTER_QD_S = 4;
template <bool FILT>
struct FilterState {};
template <>
struct FilterState<true> {
    FilterView view;
    SortedList<FILTER_QD_S> qd;
    bool on;
    bool cut;
};

// ---- bitmap makers (each stream-ordered; granne_hip.hip zeroes what they accumulate into) --------------------------
// u64 ids -> bits. Ids >= n are counted into *bad (optional), never written. Duplicates set their bit again.
__global__ __launch_bounds__(256) void filter_from_ids_kernel(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t n,
                                                              uint32_t* __restrict__ filter, uint32_t* bad) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ids; i += step) {
        const uint64_t id = ids[i];
        if (id < n) atomicOr(filter + (id >> 5), 1u << (uint32_t)(id & 31u));
        else mine += 1u;
    }
    if (bad) {
        for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
        if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(bad, mine);
    }
}

// one byte per id (non-zero = allowed) -> bits: a wave ballots 64 ids into two words. Writes every word of the bitmap
// (filter_words(n) of them), bits at positions >= n as zeros.
__global__ __launch_bounds__(256) void filter_from_mask_kernel(const uint8_t* __restrict__ mask, uint64_t n,
                                                               uint32_t* __restrict__ filter) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t chunks = (n + 63u) >> 6; // of 64 ids; wave-uniform loop bounds: every lane ballots
    const uint64_t words = filter_words(n);
    for (uint64_t c = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; c < chunks; c += waves) {
        const uint64_t i = c * 64u + lane;
        const bool on = i < n && mask[i] != 0;
        const uint64_t b = wave_ballot(on);
        const uint64_t w = c * 2u + (lane >> 5);
        if ((lane & 31u) == 0 && w < words) filter[w] = (uint32_t)(lane ? b >> 32 : b);
    }
}

// population count of the first n bits, added to *out (u64)
__global__ __launch_bounds__(256) void filter_count_kernel(const uint32_t* __restrict__ filter, uint64_t n,
                                                           unsigned long long* out) {
    const uint64_t words = filter_words(n);
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    uint32_t mine = 0;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += step) {
        uint32_t v = filter[w];
        const uint32_t tail = (uint32_t)(n & 31u);
        if (w + 1 == words && tail) v &= (1u << tail) - 1u;
        mine += (uint32_t)__popc(v);
    }
    for (int o = 32; o > 0; o >>= 1) mine += (uint32_t)__shfl_xor((int)mine, o, 64);
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(out, (unsigned long long)mine);
}

// ---- bitmap slice (granne_hip_filter_slice_device; the word rule is filter_slice.h's) ---------------------------------
// out[f][w] = word w of the slice [first_bit, first_bit + n_out_bits) of filter f, for every w < ceil(n_out_bits / 32).
// grid = (blocks over the output words, filters); both are strided over, so any grid covers any size. One output word per
// lane; the loop bound is the wave's first word, so a wave stays whole for the hand-over.
//   !HANDOVER every lane calls filter_slice_word: two loads per lane when unaligned, one when aligned (a guarded copy).
//             THE FORM THAT RUNS: the second load hits the line the neighbour's first one brings, and measured it is as
//             fast as the hand-over or faster.
//   HANDOVER  lane l's second source word is lane l + 1's first: each lane loads one word and takes the other from its
//             neighbour; only the wave's last lane -- and the lane of the slice's last word, whose neighbour loads
//             nothing -- load a second one. Kept behind GRANNE_HIP_FILTER_SLICE_HANDOVER for the measurement.
template <bool HANDOVER>
__global__ __launch_bounds__(256) void filter_slice_kernel(const uint32_t* __restrict__ src, uint64_t n_bits, uint64_t src_stride,
                                                           uint32_t n_filters, uint64_t first_bit, uint64_t n_out_bits,
                                                           uint32_t* __restrict__ out, uint64_t out_stride) {
    const uint64_t src_words = filter_words(n_bits), out_words = filter_words(n_out_bits);
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const bool aligned = (first_bit & 31u) == 0;
    for (uint32_t f = blockIdx.y; f < n_filters; f += gridDim.y) {
        const uint32_t* s = src + (uint64_t)f * src_stride;
        uint32_t* o = out + (uint64_t)f * out_stride;
        for (uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); w0 < out_words; w0 += step) {
            const uint64_t w = w0 + lane;
            const bool live = w < out_words;
            if constexpr (HANDOVER) {
                const uint64_t i = (first_bit >> 5) + w;
                const uint32_t lo = live ? filter_slice_load(s, src_words, n_bits, i) : 0u;
                uint32_t hi = 0u;
                if (!aligned) { // (wave-uniform)
                    hi = (uint32_t)__shfl_down((int)lo, 1, 64);
                    if (live && (lane == 63u || w + 1 == out_words)) hi = filter_slice_load(s, src_words, n_bits, i + 1);
                }
                if (live) o[w] = filter_slice_combine(lo, hi, first_bit, n_out_bits, w);
            } else {
                if (live) o[w] = filter_slice_word(s, src_words, first_bit, n_bits, n_out_bits, w);
            }
        }
    }
}

// After the merge of a partitioned exact selection. Every shard's block holds, after its packed top-k, four status words
// (status_off) and one u32 per query (flags_off): non-zero where the shard's selection overflowed for that query. A query
// flagged by ANY shard is voided in the merged result -- count 0, the row UINT64_MAX / +inf -- so that no list ever
// misses one shard's rows. (The places past a count are the merge's own fill, which is exact_topk's.) Block 0's first wave
// folds the status words: [0] += queries voided, [1] += over shards, [2] = max over shards, [3] += over shards.
// grid = ceil(nq / 256) blocks of 256.
__global__ __launch_bounds__(256) void sharded_exact_finish_kernel(const uint8_t* gathered, uint64_t stride, uint64_t status_off,
                                                                   uint64_t flags_off, uint32_t n_shards, uint32_t nq, uint32_t k,
                                                                   uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* status) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    bool voided = false;
    if (q < nq) {
        for (uint32_t s = 0; s < n_shards; ++s)
            voided = voided || reinterpret_cast<const uint32_t*>(gathered + (size_t)s * stride + flags_off)[q] != 0u;
        if (voided) {
            out_counts[q] = 0;
            for (uint32_t j = 0; j < k; ++j) {
                out_ids[(size_t)q * k + j] = ~0ull;
                out_dists[(size_t)q * k + j] = __builtin_inff();
            }
        }
    }
    if (!status) return;
    const uint32_t mine = (uint32_t)__popcll(wave_ballot(voided));
    if ((threadIdx.x & 63u) == 0 && mine) atomicAdd(status + 0, mine);
    if (blockIdx.x == 0 && threadIdx.x < 64u) {
        const uint32_t lane = threadIdx.x;
        uint32_t b = 0, c = 0, d = 0;
        if (lane < n_shards) {
            const uint32_t* st = reinterpret_cast<const uint32_t*>(gathered + (size_t)lane * stride + status_off);
            b = st[1], c = st[2], d = st[3];
        }
        for (int o = 32; o > 0; o >>= 1) {
            b += __shfl_xor(b, o, 64);
            const uint32_t t = __shfl_xor(c, o, 64);
            c = t > c ? t : c;
            d += __shfl_xor(d, o, 64);
        }
        if (lane == 0) {
            if (b) atomicAdd(status + 1, b);
            if (c) atomicMax(status + 2, c);
            if (d) atomicAdd(status + 3, d);
        }
    }
}

// ---- bitmap -> ascending id list (granne_hip_filter_to_ids_device; the exact scan's list source, exact_topk.h) -------
// per-block popcounts (fl_count_kernel), one block scanning them (fl_scan_kernel), a scatter (fl_scatter_kernel)
constexpr uint32_t FL_THREADS = 256, FL_PER = 8;             // words per thread, contiguous: ids come out in order
constexpr uint32_t FL_BLOCK_WORDS = FL_THREADS * FL_PER;     // 2048 words, 65536 ids per block
constexpr uint32_t FL_SCAN_THREADS = 1024;
constexpr uint64_t FL_MAX_BLOCKS = 65536;                    // n up to 2^32 - 1: 2^27 words, one block's scan

__host__ __device__ inline uint64_t fl_blocks(uint64_t n) { return (filter_words(n) + FL_BLOCK_WORDS - 1) / FL_BLOCK_WORDS; }

// word w of the bitmap over n ids, bits at positions >= n (and words past the last) as zeros
__device__ __forceinline__ uint32_t fl_word(const uint32_t* __restrict__ filter, uint64_t w, uint64_t n) {
    const uint64_t words = filter_words(n);
    if (w >= words) return 0u;
    uint32_t v = filter[w];
    const uint32_t tail = (uint32_t)(n & 31u);
    if (w + 1 == words && tail) v &= (1u << tail) - 1u;
    return v;
}

// exclusive prefix of `mine` over a block of WAVES waves (every thread calls it); *total: the block's sum
template <int WAVES, typename T>
__device__ __forceinline__ T fl_block_exclusive(T mine, T* s_wave, T* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T up = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    T before = incl - mine, sum = 0;
    for (uint32_t w = 0; w < (uint32_t)WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        sum += s_wave[w];
    }
    *total = sum;
    return before;
}

// counts[b]: the set bits among block b's FL_BLOCK_WORDS words. grid = fl_blocks(n)
__global__ __launch_bounds__(FL_THREADS) void fl_count_kernel(const uint32_t* __restrict__ filter, uint64_t n, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_wave[FL_THREADS / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * FL_BLOCK_WORDS + threadIdx.x * FL_PER;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < FL_PER; ++i) mine += (uint32_t)__popc(fl_word(filter, w0 + i, n));
    uint32_t total;
    (void)fl_block_exclusive<FL_THREADS / 64>(mine, s_wave, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one block: counts[0 .. blocks) become their exclusive prefix sums in place (each below 2^32: at most 2^32 - 1 ids); the
// total goes to *out_count and, where asked for, to *out_count32 (the scan's status[3])
__global__ __launch_bounds__(FL_SCAN_THREADS) void fl_scan_kernel(uint32_t* __restrict__ counts, uint32_t blocks, uint64_t* __restrict__ out_count,
                                                                  uint32_t* out_count32) {
    __shared__ uint64_t s_wave[FL_SCAN_THREADS / 64];
    const uint32_t per = (blocks + FL_SCAN_THREADS - 1) / FL_SCAN_THREADS;
    const uint32_t b0 = threadIdx.x * per < blocks ? threadIdx.x * per : blocks;
    const uint32_t b1 = b0 + per < blocks ? b0 + per : blocks;
    uint64_t mine = 0;
    for (uint32_t b = b0; b < b1; ++b) mine += counts[b];
    uint64_t total;
    uint64_t at = fl_block_exclusive<FL_SCAN_THREADS / 64>(mine, s_wave, &total);
    for (uint32_t b = b0; b < b1; ++b) { // (a thread rewrites only what it alone read)
        const uint32_t c = counts[b];
        counts[b] = (uint32_t)at;
        at += c;
    }
    if (threadIdx.x == 0) {
        *out_count = total;
        if (out_count32) *out_count32 = (uint32_t)total;
    }
}

// block b writes its ids, ascending, from out[offsets[b]] on. grid = fl_blocks(n)
template <typename ID>
__global__ __launch_bounds__(FL_THREADS) void fl_scatter_kernel(const uint32_t* __restrict__ filter, uint64_t n, const uint32_t* __restrict__ offsets,
                                                                ID* __restrict__ out) {
    __shared__ uint32_t s_wave[FL_THREADS / 64];
    const uint64_t w0 = (uint64_t)blockIdx.x * FL_BLOCK_WORDS + threadIdx.x * FL_PER;
    uint32_t v[FL_PER], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < FL_PER; ++i) {
        v[i] = fl_word(filter, w0 + i, n);
        mine += (uint32_t)__popc(v[i]);
    }
    uint32_t total;
    uint64_t pos = (uint64_t)offsets[blockIdx.x] + fl_block_exclusive<FL_THREADS / 64>(mine, s_wave, &total);
#pragma unroll
    for (uint32_t i = 0; i < FL_PER; ++i) {
        uint32_t w = v[i];
        while (w) { // (set bits only below n: pos stays below the count, the count at most n)
            const uint32_t b = (uint32_t)__ffs((int)w) - 1u;
            out[pos++] = (ID)(((w0 + i) << 5) + b);
            w &= w - 1u;
        }
    }
}

} // namespace granne_hip
