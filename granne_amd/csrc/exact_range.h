// exact_range.h -- every element within a radius of every query, exact by construction (granne_hip_exact_range_device):
// the scan of exact_topk.h with a RADIUS for its admission rule instead of a rank. Distances are et_dist's -- a row's
// distance here is its distance in exact_topk, bit for bit --, compares are f32 compares, the order is (distance bits, id).
//
//   W(q)     = { i < n_elements : allowed(q, i) and dist(i, q) <= r[q] }
//   total[q] = |W(q)|, ALWAYS exact; answer = the first min(total, cap) members of W by (distance bits, id)
//
//   phase A  ONE pass over the rows, no priming stages: er_scan_kernel has et_scan_kernel's grid, block geometry (ET_QT
//            queries staged in LDS, eight lanes per row, the row in registers up to 1024 bytes) and sources (EtSrc: all
//            rows, the compacted list, per-query bits). A pair is a hit iff d <= r[q] (and the pair is allowed). Per query
//            it produces
//              total  counted without an atomic in the loop: the hits of a wave's eight rows come from one ballot, and
//                     lane qi of the wave keeps the running count of the tile's query qi in a register. After the row
//                     range the waves add their lanes into LDS and the block issues ONE global atomicAdd per query it
//                     saw a hit of. (A radius of 2.0 makes every pair a hit: one global atomic per hit, all on nq
//                     addresses, is the design this avoids.)
//              cand   up to ET_CAP keys, distance bits << 32 | id (the list source: the GLOBAL id). A wave asks for the
//                     slots of its hits with one atomicAdd on a second per-query counter; once a block has seen that
//                     counter reach ET_CAP it sets the query's flag in LDS and asks no more: a dense query costs about
//                     ET_CAP / (hits per wave step) slot atomics per block that still asks, not `total`.
//            er_rank_kernel, one block per query: total <= ET_CAP -- the candidates are all of W: sorted in LDS
//            (et_sort_keys), min(total, cap) written; otherwise the query's bit is set in the `dense` bitmap.
//   phase B  only for the dense queries (exact_range_host.h): more than ET_CAP >= cap rows lie within the radius, so the
//            cap nearest allowed rows overall all lie within it: the answer is exact_topk[_filtered](k = cap), by
//            exact_topk_run unchanged, scattered back by er_scatter_kernel. `total` stays phase A's.
// Compiled with -ffp-contract=off, as exact_topk.h.
#pragma once

#include "exact_topk.h"

namespace granne_hip {

constexpr uint32_t ER_CAP_MAX = ET_KMAX; // GRANNE_HIP_RANGE_CAP_MAX

struct ErParams {
    const uint8_t* elements; // as EtParams
    uint64_t rows;           // n; ET_LIST: clipped to *m in the kernel
    uint32_t row_bytes, row_stride, dim;
    const uint8_t* queries;  // dense [nq][dim] (this round's)
    uint32_t nq, q_lds;
    uint64_t per_range;      // rows per blockIdx.y (a multiple of ET_GROUPS). ET_LIST: not read
    const float* radii;      // [nq]
    uint32_t* totals;        // [nq] zeroed: the hits
    uint32_t* cnt;           // [nq] zeroed: the slots asked for (>= ET_CAP: the query is dense or exactly full)
    uint64_t* cand;          // [nq][ET_CAP]
    const uint32_t* list;    // ET_LIST: the allowed ids, ascending
    const uint64_t* m;       // ET_LIST: how many, on the device
    const uint32_t* filter;  // ET_BITS: the queries' bitmaps (this round's first)
    uint64_t filter_stride;  // ET_BITS: words from one query's bitmap to the next
};

// grid = (query tiles of ET_QT, row ranges), as et_scan_kernel's collecting pass
template <bool I8, int NBLK, EtSrc SRC>
__global__ __launch_bounds__(ET_THREADS) void er_scan_kernel(const ErParams P) {
    static_assert(ET_GROUPS == 32u && ET_QT <= 32u, "a step's rows share one filter word; lane qi of a wave counts query qi");
    extern __shared__ __align__(16) uint8_t smem_er[];
    __shared__ float s_r[ET_QT];
    __shared__ int s_dy[ET_QT];
    __shared__ uint32_t s_tot[ET_QT], s_full[ET_QT];
    uint64_t rows = P.rows;
    if constexpr (SRC == ET_LIST) {
        const uint64_t m = *P.m;
        if (m < rows) rows = m;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, sub = lane & 7u, grp = tid >> 3;
    const uint32_t q0 = blockIdx.x * ET_QT;
    const uint32_t qn = P.nq - q0 < ET_QT ? P.nq - q0 : ET_QT;
    uint64_t per_range = P.per_range;
    if constexpr (SRC == ET_LIST) per_range = ((rows + gridDim.y - 1) / gridDim.y + ET_GROUPS - 1) / ET_GROUPS * ET_GROUPS;
    const uint64_t r0_64 = (uint64_t)blockIdx.y * per_range;
    const uint64_t r1_64 = r0_64 + per_range < rows ? r0_64 + per_range : rows;
    if (r0_64 >= r1_64) return; // (the whole block alike)
    // rows <= 2^32 - 1 (the host refuses more): the range in 32 bits, walked by a step count so that nothing wraps
    const uint32_t r0 = (uint32_t)r0_64, r1 = (uint32_t)r1_64, steps = (r1 - r0 + ET_GROUPS - 1) / ET_GROUPS;
    if (tid < ET_QT) {
        s_r[tid] = tid < qn ? P.radii[q0 + tid] : -1.0f;
        s_dy[tid] = 0, s_tot[tid] = 0, s_full[tid] = 0;
    }
    if constexpr (NBLK > 0) {
        if constexpr (!I8) {
            float* sq = reinterpret_cast<float*>(smem_er);
            const float* gq = reinterpret_cast<const float*>(P.queries) + (size_t)q0 * P.dim;
            const uint32_t qsf = P.q_lds / 4u;
            for (uint32_t i = tid; i < qn * P.dim; i += ET_THREADS) {
                const uint32_t qi = i / P.dim, c = i - qi * P.dim;
                sq[qi * qsf + c] = gq[i];
            }
        } else {
            const uint8_t* gq = P.queries + (size_t)q0 * P.dim;
            for (uint32_t i = tid; i < qn * P.q_lds; i += ET_THREADS) {
                const uint32_t qi = i / P.q_lds, c = i - qi * P.q_lds;
                smem_er[i] = c < P.dim ? gq[(size_t)qi * P.dim + c] : (uint8_t)0;
            }
        }
    }
    __syncthreads();
    if constexpr (NBLK > 0 && I8) {
        if (tid < qn) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(smem_er + (size_t)tid * P.q_lds);
            int dy = 0;
            for (uint32_t i = 0; i < P.q_lds / 4u; ++i) dy = dot4_i8(w[i], w[i], dy);
            s_dy[tid] = dy;
        }
        __syncthreads();
    }
    volatile uint32_t* const full = s_full; // written by other waves while this one loops
    // ET_BITS: lane l & 31 reads the words of the tile's query l & 31 (a per-lane pointer: the scalar registers are short
    // in the eight-block f32 form)
    const uint32_t* fwords = nullptr;
    if constexpr (SRC == ET_BITS) fwords = P.filter + (uint64_t)(q0 + ((lane & 31u) < qn ? (lane & 31u) : 0u)) * P.filter_stride;
    uint32_t mine = 0;                      // lane qi: the hits of the tile's query qi this wave has seen
    for (uint32_t it = 0; it < steps; ++it) {
        const uint32_t e0 = r0 + it * ET_GROUPS; // a multiple of ET_GROUPS = 32 (per_range is one)
        const bool live = r1 - e0 > grp;
        const uint32_t e = live ? e0 + grp : r1 - 1;
        uint64_t row = e;
        if constexpr (SRC == ET_LIST) row = P.list[row];
        uint32_t fw = 0;
        if constexpr (SRC == ET_BITS) {
            if ((lane & 31u) < qn) fw = fwords[e0 >> 5];
        }
        EtRow<I8, NBLK> R;
        et_load_row<I8, NBLK>(R, P.elements + row * (uint64_t)P.row_stride, P.row_bytes, lane);
        for (uint32_t qi = 0; qi < qn; ++qi) {
            bool allowed = true;
            if constexpr (SRC == ET_BITS) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)fw, (int)qi);
                if (((w >> ((tid >> 6) * 8u)) & 0xFFu) == 0u) continue; // none of this wave's eight rows: the whole wave skips
                allowed = (w >> grp) & 1u;
            }
            const uint8_t* qp = NBLK > 0 ? smem_er + (size_t)qi * P.q_lds
                                         : P.queries + (size_t)(q0 + qi) * P.dim * (I8 ? 1u : 4u);
            const float d = et_dist<I8, NBLK>(R, qp, s_dy[qi], P.dim, P.row_bytes, lane);
            const bool hit = live && allowed && sub == 0u && d <= s_r[qi];
            const uint64_t b = wave_ballot(hit);
            if (b == 0ull) continue; // (wave-uniform)
            const uint32_t nh = (uint32_t)__popcll(b);
            if (lane == qi) mine += nh;
            if (full[qi]) continue; // (one LDS word: the same for every lane)
            const size_t q = q0 + qi;
            if (hit) { // the lowest hit lane asks for the wave's slots; it is the first active lane in here
                const uint32_t rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
                uint32_t pos0 = 0;
                if (rank == 0u) pos0 = atomicAdd(P.cnt + q, nh);
                pos0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)pos0);
                if (pos0 + rank < ET_CAP) P.cand[q * ET_CAP + pos0 + rank] = (uint64_t)__float_as_uint(d) << 32 | (uint64_t)(SRC == ET_LIST ? (uint32_t)row : e);
                if (rank == 0u && pos0 + nh >= ET_CAP) full[qi] = 1u;
            }
        }
    }
    if (lane < qn && mine) atomicAdd(&s_tot[lane], mine);
    __syncthreads();
    if (tid < qn && s_tot[tid]) atomicAdd(P.totals + q0 + tid, s_tot[tid]);
}

// One block per query of the round (query q0 + blockIdx.x of the call): out_totals; total <= ET_CAP: the candidates are W,
// sorted, the first min(total, cap) written, the rest filled, out_counts; otherwise the query's bit in `dense` (over the
// call's queries, zeroed) and status[1] += 1 -- phase B writes its answer.
__global__ __launch_bounds__(ET_RANK_THREADS) void er_rank_kernel(const uint64_t* cand, const uint32_t* totals, uint32_t q0, uint32_t cap,
                                                                  uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                                  uint32_t* out_totals, uint32_t* dense, uint32_t* status) {
    __shared__ uint64_t keys[ET_CAP];
    const uint32_t tid = threadIdx.x, q = q0 + blockIdx.x;
    const uint32_t total = totals[blockIdx.x];
    if (tid == 0) out_totals[q] = total;
    if (total > ET_CAP) { // (the whole block alike)
        if (tid == 0) {
            atomicOr(dense + (q >> 5), 1u << (q & 31u));
            if (status) atomicAdd(status + 1, 1u);
        }
        return;
    }
    et_sort_keys(keys, cand + (size_t)blockIdx.x * ET_CAP, total, tid);
    const uint32_t count = total < cap ? total : cap;
    for (uint32_t i = tid; i < cap; i += ET_RANK_THREADS) {
        const uint64_t key = i < count ? keys[i] : 0;
        out_ids[(size_t)q * cap + i] = i < count ? (key & 0xFFFFFFFFull) : ~0ull;
        out_dists[(size_t)q * cap + i] = i < count ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
    }
    if (tid == 0) {
        out_counts[q] = count;
        if (status) atomicMax(status + 2, total);
    }
}

// A dense [np][k] answer -- ids, dists, counts [np], and (optional) found [np] -- to the rows of the queries orig[0 .. np).
// out_found / out_stage (optional) receive found[r] / `stage`. The first thread folds the producer's status words into
// the call's: [0] is added, [2] raised to (fold_ranked only).
__global__ __launch_bounds__(256) void er_scatter_kernel(const uint64_t* __restrict__ ids, const float* __restrict__ dists,
                                                         const uint32_t* __restrict__ counts, const uint32_t* __restrict__ found,
                                                         const uint32_t* __restrict__ orig, uint32_t np, uint32_t k,
                                                         uint64_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                         uint32_t* __restrict__ out_counts, uint32_t* out_found, uint32_t* out_stage,
                                                         uint32_t stage, const uint32_t* from_status, uint32_t fold_ranked, uint32_t* status) {
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
            if (out_found && found) out_found[q] = found[r];
            if (out_stage) out_stage[q] = stage;
        }
    }
    if (t0 == 0 && status) {
        if (from_status[0]) atomicAdd(status + 0, from_status[0]);
        if (fold_ranked) atomicMax(status + 2, from_status[2]);
    }
}

typedef void (*ErScanFn)(const ErParams);
template <bool I8, EtSrc SRC>
inline ErScanFn er_scan_blocks(uint32_t nblk) {
    return nblk <= 1 ? er_scan_kernel<I8, 1, SRC> : nblk <= 2 ? er_scan_kernel<I8, 2, SRC> : nblk <= 4 ? er_scan_kernel<I8, 4, SRC>
         : nblk <= 8 ? er_scan_kernel<I8, 8, SRC> : er_scan_kernel<I8, 0, SRC>;
}
template <bool I8>
inline ErScanFn er_scan_src(uint32_t nblk, EtSrc src) {
    return src == ET_ALL ? er_scan_blocks<I8, ET_ALL>(nblk) : src == ET_LIST ? er_scan_blocks<I8, ET_LIST>(nblk) : er_scan_blocks<I8, ET_BITS>(nblk);
}
// the kernel for device rows of row_bytes: the fewest register blocks that hold the row, or the memory form
inline ErScanFn er_scan_fn(bool i8, uint32_t row_bytes, EtSrc src) {
    const uint32_t nblk = (row_bytes + 127u) / 128u;
    return i8 ? er_scan_src<true>(nblk, src) : er_scan_src<false>(nblk, src);
}

} // namespace granne_hip
