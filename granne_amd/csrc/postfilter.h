// postfilter.h -- post-filtered search: the kernels beside the walkers.
//
// granne_hip_search_postfiltered_batch* run the ORDINARY search with a long list -- max_search = num_neighbors = E, on
// whichever walker the plan picks, the register walkers included -- and keep the allowed ids of that list. The semantic is
// the model in include/granne_hip.h ("post-filtered search"): stage after stage with a longer list for the queries whose
// list held fewer than min_allowed allowed ids, then the exact scan under the filter or the short answer. No walker knows
// about the filter; what is new is here:
//
//   pf_take_kernel         one stage's lists -> the first k allowed entries of every list, in the list's own order, written
//                          to the ORIGINAL query's output row; the queries the stage does not finish get their bit set in a
//                          pending bitmap, which filter.h's compaction (fl_*) turns into the next stage's ascending list
//   pf_gather_rows_kernel  dense rows by index: the pending queries' rows, and for the exact fallback their bitmaps
//   pf_scatter_kernel      the fallback's dense [np][k] answer back to the original rows
#pragma once

#include "filter.h"

namespace granne_hip {

constexpr uint32_t PF_STAGE_EXACT = 0xFFFFFFFFu, PF_STAGE_SHORT = 0xFFFFFFFEu; // GRANNE_HIP_PF_STAGE_*
constexpr uint32_t PF_TAKE_WAVES = 4;

struct PfTake {
    // the stage's lists: the search's output for `np` queries with max_search = num_neighbors = E
    const uint64_t* ids;    // [np][E]
    const float* dists;     // [np][E]
    const uint32_t* counts; // [np]
    uint32_t np, E;
    // list row r belongs to query orig[r], or to query row0 + r where orig is null (stage 0)
    const uint32_t* orig;
    uint32_t row0;
    uint32_t k, min_allowed;
    uint32_t stage;      // what a finished query's out_stage receives
    uint32_t last_short; // the last stage of a call with GRANNE_HIP_PF_FALLBACK_SHORT: every query ends here
    uint32_t last;       // the last stage: a query it does not finish is counted in status[3]
    const uint32_t* filter;
    uint64_t filter_stride; // words from one query's bitmap to the next; 0: one bitmap
    uint64_t n_elements;
    uint64_t* out_ids;   // [nq][k]
    float* out_dists;    // [nq][k]
    uint32_t* out_counts; // [nq]
    uint32_t* out_stage; // [nq], optional
    uint32_t* pending;   // one bit per query of the call, zeroed before the stage
    uint32_t* status;    // u32[4], optional
};

// One wavefront per list, PF_TAKE_WAVES per block, no LDS. The list is read 64 entries at a time (8-byte ids, coalesced);
// each lane tests its id's bit (a 4-byte gather: a shared bitmap stays in L2), and the rank of an allowed entry is the
// running count plus the allowed lanes below it. Entries past the list's count are never bit-tested. The loop stops once
// min_allowed (>= k) allowed entries are seen: the answer is complete and the stage finishes the query.
__global__ __launch_bounds__(64 * PF_TAKE_WAVES) void pf_take_kernel(PfTake P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * PF_TAKE_WAVES + (threadIdx.x >> 6);
    if (row >= P.np) return; // (wave-uniform)
    const uint32_t q = P.orig ? P.orig[row] : P.row0 + row;
    const uint32_t len = P.counts[row] < P.E ? P.counts[row] : P.E;
    const uint64_t* ids = P.ids + (size_t)row * P.E;
    const float* dists = P.dists + (size_t)row * P.E;
    const uint32_t* words = P.filter + (size_t)q * P.filter_stride;
    uint64_t* out_ids = P.out_ids + (size_t)q * P.k;
    float* out_dists = P.out_dists + (size_t)q * P.k;
    uint32_t total = 0;
    for (uint32_t j0 = 0; j0 < len && total < P.min_allowed; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const bool live = j < len;
        const uint64_t id = live ? ids[j] : ~0ull;
        const float d = live ? dists[j] : 0.0f;
        bool ok = live && id < P.n_elements; // (a list holds node ids only: the bound keeps a stray id off the bitmap)
        if (ok) ok = FilterView::bit_of(words[id >> 5], (uint32_t)id);
        const uint64_t b = wave_ballot(ok);
        const uint32_t rank = total + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (ok && rank < P.k) {
            out_ids[rank] = id;
            out_dists[rank] = d;
        }
        total += (uint32_t)__popcll(b);
    }
    const bool done = total >= P.min_allowed || len < P.E; // enough allowed ids, or the walk ran out of graph
    if (done || P.last_short) {
        const uint32_t count = total < P.k ? total : P.k;
        for (uint32_t j = count + lane; j < P.k; j += 64u) {
            out_ids[j] = ~0ull;
            out_dists[j] = __builtin_inff();
        }
        if (lane == 0) {
            P.out_counts[q] = count;
            if (P.out_stage) P.out_stage[q] = done ? P.stage : PF_STAGE_SHORT;
        }
    } else if (lane == 0) {
        atomicOr(P.pending + (q >> 5), 1u << (q & 31u));
    }
    if (!done && P.last && P.status && lane == 0) atomicAdd(P.status + 3, 1u);
}

// out row r = src row idx[r], rows of `units` elements of U, src rows src_units apart (>= units); one thread per element
template <typename U>
__global__ __launch_bounds__(256) void pf_gather_rows_kernel(const U* __restrict__ src, uint64_t src_units, const uint32_t* __restrict__ idx,
                                                             uint32_t rows, uint64_t units, U* __restrict__ out) {
    const uint64_t total = (uint64_t)rows * units;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += step) {
        const uint64_t r = t / units, c = t - r * units;
        out[t] = src[(uint64_t)idx[r] * src_units + c];
    }
}

// The exact fallback's answer for the pending queries -- ids / dists [np][k], counts [np] -- to the rows of the queries
// orig[0 .. np), with the EXACT code; the first thread folds the scan's overflow count (fb_status[0]) into status[0].
__global__ __launch_bounds__(256) void pf_scatter_kernel(const uint64_t* __restrict__ ids, const float* __restrict__ dists,
                                                         const uint32_t* __restrict__ counts, const uint32_t* __restrict__ orig, uint32_t np,
                                                         uint32_t k, uint64_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                         uint32_t* __restrict__ out_counts, uint32_t* out_stage, const uint32_t* fb_status,
                                                         uint32_t* status) {
    const uint64_t total = (uint64_t)np * k;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t t = t0; t < total; t += step) {
        const uint64_t r = t / k, j = t - r * k;
        const uint32_t q = orig[r];
        out_ids[(size_t)q * k + j] = ids[t];
        out_dists[(size_t)q * k + j] = dists[t];
        if (j == 0) {
            out_counts[q] = counts[r];
            if (out_stage) out_stage[q] = PF_STAGE_EXACT;
        }
    }
    if (t0 == 0 && status && fb_status[0]) atomicAdd(status + 0, fb_status[0]);
}

} // namespace granne_hip
