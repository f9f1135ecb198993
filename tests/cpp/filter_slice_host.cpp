// The bitmap slice's word rule (granne_amd/csrc/filter_slice.h) on the host, under AddressSanitizer and UBSan: the same
// text the slice kernel compiles. Every source bitmap is a heap block of exactly ceil(n_bits / 32) words -- no slack --
// so a read of the word after the last, the funnel shift's second word at the bitmap's end included, is a heap overflow
// the sanitizer reports. The result is compared with a bit-by-bit loop.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I granne_amd/csrc filter_slice_host.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "filter_slice.h"

using granne_hip::filter_slice_word;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

static int check(uint64_t n_bits, uint64_t first, uint64_t n_out) {
    const uint64_t src_words = (n_bits + 31) / 32, out_words = (n_out + 31) / 32;
    uint32_t* src = (uint32_t*)malloc(src_words ? src_words * 4 : 1); // exact size: ASan guards the next byte
    for (uint64_t i = 0; i < src_words; ++i) src[i] = rnd();          // garbage past n_bits in the last word included
    std::vector<uint32_t> want(out_words, 0u);
    for (uint64_t i = 0; i < n_out; ++i) {
        const uint64_t b = first + i;
        if (b < n_bits && (src[b >> 5] >> (b & 31)) & 1u) want[i >> 5] |= 1u << (i & 31);
    }
    int bad = 0;
    for (uint64_t w = 0; w < out_words; ++w) {
        const uint32_t got = filter_slice_word(src, src_words, first, n_bits, n_out, w);
        if (got != want[w]) {
            if (!bad)
                fprintf(stderr, "n_bits %llu first %llu n_out %llu word %llu: got %08x want %08x\n", (unsigned long long)n_bits,
                        (unsigned long long)first, (unsigned long long)n_out, (unsigned long long)w, got, want[w]);
            bad = 1;
        }
    }
    free(src);
    return bad;
}

int main() {
    const uint64_t first_mod[] = {0, 1, 9, 31}, n_outs[] = {0, 1, 31, 32, 33, 937}, bases[] = {0, 64, 992};
    int bad = 0, cases = 0;
    for (uint64_t fm : first_mod)
        for (uint64_t base : bases)
            for (uint64_t n_out : n_outs) {
                const uint64_t first = base + fm;
                // the slice ends exactly at n_bits, runs past it, or stops short of it
                const uint64_t ends[] = {first + n_out, first + n_out / 2, first, first + n_out + 5, first + n_out + 77};
                for (uint64_t n_bits : ends) {
                    bad |= check(n_bits, first, n_out);
                    ++cases;
                }
            }
    // the shards of the GPU fixture inside their 4037-bit bitmap
    const uint64_t lens[] = {31, 33, 937, 1000, 2036};
    uint64_t off = 0;
    for (uint64_t n : lens) {
        bad |= check(4037, off, n);
        off += n;
        ++cases;
    }
    printf("%d cases %s\n", cases, bad ? "FAILED" : "ok");
    return bad;
}
