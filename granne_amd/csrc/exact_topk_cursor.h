// exact_topk_cursor.h -- the cursor of granne_hip_exact_topk_after* and granne_hip_exact_topk_screened_after* (DESIGN.md
// 3.7h), shared by exact_topk.h's scan and exact_topk_screened.hip's key kernel: one definition of "beyond the cursor".
// The exact entries order their answer by one total key, distance bits << 32 | id; a query's cursor is such a key, and
// its answer is made of the rows whose key is STRICTLY greater. Every kernel that decides it calls et_past on the bits
// of the distance the reference's arithmetic gave the row.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace granne_hip {

struct EtCursor {
    const float* dists;  // [nq] the distance of the last entry the caller has (this round's)
    const uint64_t* ids; // [nq] its id; UINT64_MAX: the query has no cursor
};

// The lowest eligible key of a cursor, the key after (bits(d), id); 0 without a cursor: every key is eligible. No row
// has an id above 2^32 - 2 (the entries take n < 2^32 elements), so a cursor id that does not fit 32 bits stands for
// 2^32 - 1, and the one key that has no successor, all-ones, is no row's: it stays, and nothing is eligible.
__device__ __forceinline__ uint64_t et_from(float d, uint64_t id) {
    if (id == ~0ull) return 0ull;
    const uint64_t cur = (uint64_t)__float_as_uint(d) << 32 | (id < 0xFFFFFFFFull ? id : 0xFFFFFFFFull);
    return cur == ~0ull ? cur : cur + 1ull;
}
__device__ __forceinline__ bool et_past(float d, uint32_t id, uint64_t from) {
    return ((uint64_t)__float_as_uint(d) << 32 | (uint64_t)id) >= from;
}

} // namespace granne_hip
