// filter_slice.h -- the word rule of a bitmap slice: plain C++, no device header, so that the slice
// kernel (filter.h) and a host program (tests/cpp/filter_slice_host.cpp) compile the same text.
//
// A slice of a bitmap over n_bits ids is the bitmap of the ids [first_bit, first_bit + n_out_bits): output bit i is
// source bit first_bit + i, source bits at positions >= n_bits read as 0, output bits at positions >= n_out_bits of the
// last word are 0. The source has src_words = ceil(n_bits / 32) words and no word at or past that is ever read -- the
// second word of the funnel shift at the bitmap's end included.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GRANNE_HIP_HD __host__ __device__
#else
#define GRANNE_HIP_HD
#endif

namespace granne_hip {

// source word i with the bits at positions >= n_bits as zeros; 0 for a word the source does not have
GRANNE_HIP_HD inline uint32_t filter_slice_load(const uint32_t* src, uint64_t src_words, uint64_t n_bits, uint64_t i) {
    if (i >= src_words) return 0u;
    uint32_t v = src[i];
    const uint32_t tail = (uint32_t)(n_bits & 31u);
    if (i + 1 == src_words && tail) v &= (1u << tail) - 1u;
    return v;
}

// output word w from the two source words it straddles: lo = word (first_bit + 32 w) / 32, hi = the one after (unused
// when the slice is word-aligned)
GRANNE_HIP_HD inline uint32_t filter_slice_combine(uint32_t lo, uint32_t hi, uint64_t first_bit, uint64_t n_out_bits, uint64_t w) {
    const uint32_t sh = (uint32_t)(first_bit & 31u);
    uint32_t v = sh ? (lo >> sh) | (hi << (32u - sh)) : lo;
    const uint64_t left = n_out_bits - w * 32u; // bits of the slice from this word on (w < ceil(n_out_bits / 32): > 0)
    if (left < 32u) v &= (1u << (uint32_t)left) - 1u;
    return v;
}

// output word w (w < ceil(n_out_bits / 32)) of the slice
GRANNE_HIP_HD inline uint32_t filter_slice_word(const uint32_t* src, uint64_t src_words, uint64_t first_bit, uint64_t n_bits,
                                                uint64_t n_out_bits, uint64_t w) {
    const uint64_t i = (first_bit >> 5) + w;
    const uint32_t lo = filter_slice_load(src, src_words, n_bits, i);
    const uint32_t hi = (first_bit & 31u) ? filter_slice_load(src, src_words, n_bits, i + 1) : 0u;
    return filter_slice_combine(lo, hi, first_bit, n_out_bits, w);
}

} // namespace granne_hip
