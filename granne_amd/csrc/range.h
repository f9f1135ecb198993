// range.h -- range search by the walk: the kernel beside the walkers.
//
// granne_hip_search_range_batch* run the ORDINARY search with a long list -- max_search = num_neighbors = E, on whichever
// walker the plan picks -- and cut that list at the query's radius. The semantic is the model in include/granne_hip.h
// ("range search"): a list answers its query once it reaches PAST the radius (an entry beyond r: every nearer node the
// walk knows is in front of it) or the walk ran out of graph; otherwise the query goes on to a longer list, then to the
// exact scan under the radius (exact_range.h) or its short answer. No walker sees the radius; what is new is here:
//
//   rg_take_kernel  one stage's lists -> the entries within the radius (a prefix: a list ascends by (distance, id)), the
//                   first `cap` of them written to the ORIGINAL query's row with counts, found and stage; the queries the
//                   stage does not finish get their bit set in a pending bitmap (filter.h's fl_* compact it)
// The pending queries' rows and radii are gathered by postfilter.h's pf_gather_rows_kernel, the fallback's answer is
// scattered by exact_range.h's er_scatter_kernel.
#pragma once

#include "filter.h"

namespace granne_hip {

constexpr uint32_t RG_STAGE_EXACT = 0xFFFFFFFFu, RG_STAGE_SHORT = 0xFFFFFFFEu; // GRANNE_HIP_RG_STAGE_*
constexpr uint32_t RG_TAKE_WAVES = 4;

struct RgTake {
    // the stage's lists: the search's output for `np` queries with max_search = num_neighbors = E
    const uint64_t* ids;    // [np][E]
    const float* dists;     // [np][E]
    const uint32_t* counts; // [np]
    uint32_t np, E;
    // list row r belongs to query orig[r], or to query row0 + r where orig is null (stage 0)
    const uint32_t* orig;
    uint32_t row0;
    uint32_t cap;
    uint32_t stage;      // what a finished query's out_stage receives
    uint32_t last_short; // the last stage of a call with GRANNE_HIP_RG_FALLBACK_SHORT: every query ends here
    uint32_t last;       // the last stage: a query it does not finish is counted in status[3]
    const float* radii;  // [nq], by the ORIGINAL query
    uint64_t* out_ids;   // [nq][cap]
    float* out_dists;    // [nq][cap]
    uint32_t* out_counts; // [nq]
    uint32_t* out_found; // [nq], optional
    uint32_t* out_stage; // [nq], optional
    uint32_t* pending;   // one bit per query of the call, zeroed before the stage
    uint32_t* status;    // u32[4], optional
};

// One wavefront per list, RG_TAKE_WAVES per block, no LDS. The list is read 64 entries at a time; `within` is the running
// popcount of the ballot of (live and d <= r), and the loop stops at the first chunk that holds an entry beyond r: the
// list ascends, nothing after it is within.
__global__ __launch_bounds__(64 * RG_TAKE_WAVES) void rg_take_kernel(RgTake P) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t row = blockIdx.x * RG_TAKE_WAVES + (threadIdx.x >> 6);
    if (row >= P.np) return; // (wave-uniform)
    const uint32_t q = P.orig ? P.orig[row] : P.row0 + row;
    const uint32_t len = P.counts[row] < P.E ? P.counts[row] : P.E;
    const float r = P.radii[q];
    const uint64_t* ids = P.ids + (size_t)row * P.E;
    const float* dists = P.dists + (size_t)row * P.E;
    uint64_t* out_ids = P.out_ids + (size_t)q * P.cap;
    float* out_dists = P.out_dists + (size_t)q * P.cap;
    uint32_t within = 0;
    for (uint32_t j0 = 0; j0 < len; j0 += 64u) {
        const uint32_t j = j0 + lane;
        const bool live = j < len;
        const float d = live ? dists[j] : 0.0f;
        const bool in = live && d <= r;
        const uint64_t b = wave_ballot(in);
        const uint32_t rank = within + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        if (in && rank < P.cap) {
            out_ids[rank] = ids[j];
            out_dists[rank] = d;
        }
        within += (uint32_t)__popcll(b);
        if (b != wave_ballot(live)) break; // an entry beyond the radius (wave-uniform)
    }
    const bool done = within < len || len < P.E; // the list reaches past the radius, or the walk ran out of graph
    if (done || P.last_short) {
        const uint32_t count = within < P.cap ? within : P.cap;
        for (uint32_t j = count + lane; j < P.cap; j += 64u) {
            out_ids[j] = ~0ull;
            out_dists[j] = __builtin_inff();
        }
        if (lane == 0) {
            P.out_counts[q] = count;
            if (P.out_found) P.out_found[q] = within;
            if (P.out_stage) P.out_stage[q] = done ? P.stage : RG_STAGE_SHORT;
        }
    } else if (lane == 0) {
        atomicOr(P.pending + (q >> 5), 1u << (q & 31u));
    }
    if (!done && P.last && P.status && lane == 0) atomicAdd(P.status + 3, 1u);
}

} // namespace granne_hip
