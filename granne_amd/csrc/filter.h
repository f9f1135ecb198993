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
// make and count bitmaps. The exact walker's part is in slow_kernel.h. The register walkers (walk_fast.h) have no filtered
// form: they keep no visited set and find a seen candidate by its rank in one list of max_search keys, which does not
// survive keys that are expanded but may not be returned.
#pragma once

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

} // namespace granne_hip
