// rw_tombstone.h -- RwGranneBuilder's tombstones (included by granne_hip.hip): the kernels that change
// the handle's `alive` bitmap and the one that gathers the surviving rows for a compaction. The bitmap is a filter in
// filter.h's layout -- bit (id & 31) of u32 word (id >> 5), one = alive -- and the live searches walk under it exactly as
// search_filtered walks under a caller's (search_kernel.h / slow_kernel.h, FILT): nothing here is on the search path.
// The survivors' ascending id list comes from filter.h's fl_count / fl_scan / fl_scatter over the first len() bits.
#pragma once

#include "filter.h"

namespace granne_hip {

// remove (REMOVE: clear the bit) or restore (set it) the ids [n_ids]; one thread per id, grid-stride beyond the grid.
// counters (u64 [3], zeroed by the caller) receive: [0] ids whose bit this call changed, [1] ids whose bit already had the
// value -- a second occurrence of an id within the call included: the atomic's returned word says which occurrence came
// first, so the three sums do not depend on the order the threads ran in -- [2] ids >= n, never written.
template <bool REMOVE>
__global__ __launch_bounds__(256) void tomb_mark_kernel(const uint64_t* __restrict__ ids, uint64_t n_ids, uint64_t n,
                                                        uint32_t* __restrict__ alive, unsigned long long* counters) {
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    uint32_t changed = 0, same = 0, bad = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_ids; i += step) {
        const uint64_t id = ids[i];
        if (id >= n) {
            bad += 1u;
            continue;
        }
        const uint32_t bit = 1u << (uint32_t)(id & 31u);
        const uint32_t old = REMOVE ? atomicAnd(alive + (id >> 5), ~bit) : atomicOr(alive + (id >> 5), bit);
        if (((old & bit) != 0u) == REMOVE) changed += 1u;
        else same += 1u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        changed += (uint32_t)__shfl_xor((int)changed, o, 64);
        same += (uint32_t)__shfl_xor((int)same, o, 64);
        bad += (uint32_t)__shfl_xor((int)bad, o, 64);
    }
    if ((threadIdx.x & 63u) == 0) {
        if (changed) atomicAdd(counters + 0, (unsigned long long)changed);
        if (same) atomicAdd(counters + 1, (unsigned long long)same);
        if (bad) atomicAdd(counters + 2, (unsigned long long)bad);
    }
}

// device rows (row_stride bytes apart, each starting on a 16-byte boundary) of the ids [m] -> dense [m][dense_bytes].
// A thread moves one unit U: uint4 where dense_bytes is a multiple of 16, else uint32_t where it is a multiple of 4, else
// bytes -- the host picks, so every unit of both sides is aligned. ids[i] < the number of rows (fl_scatter_kernel's ids).
template <typename U>
__global__ __launch_bounds__(256) void gather_dense_rows_kernel(const uint8_t* __restrict__ rows, uint32_t row_stride,
                                                                const uint32_t* __restrict__ ids, uint64_t m, uint32_t dense_bytes,
                                                                uint8_t* __restrict__ out) {
    const uint32_t units = dense_bytes / (uint32_t)sizeof(U);
    const uint64_t total = m * units;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = t / units;
        const uint64_t at = (t - row * units) * sizeof(U);
        *reinterpret_cast<U*>(out + row * dense_bytes + at) = *reinterpret_cast<const U*>(rows + (uint64_t)ids[row] * row_stride + at);
    }
}

} // namespace granne_hip
