// exact_topk_filtered.h -- exact_topk among the ids a bitmap allows (granne_hip_exact_topk_filtered_device; DESIGN.md
// 3.10a): the distances, the key, the two-level selection and the ranking are exact_topk.h's own (EtRow, et_load_row,
// et_dist, et_key, EtSel, et_rank_kernel, unchanged); what differs is which (query, row) pairs a pass looks at.
//
//   list form  one bitmap for every query (filter_stride_words == 0). The bitmap is compacted to its ids, ascending
//              (fl_count_kernel, fl_scan_kernel, fl_scatter_kernel: per-block popcounts, one block scanning them, a
//              scatter), and the passes walk that list: entry e names row list[e]. Work ~ m x nq for m allowed ids. The
//              candidate key holds list[e], the GLOBAL id: et_rank_kernel orders ties by it.
//              m lives on the device only; nothing is read back. The grids and the priming prefixes p_0 < .. < p_last = n
//              stay functions of n; a stage's entries are [0, min(p_st, m)), split over gridDim.y in the kernel. A stage
//              whose predecessor covered the whole list (st > 0 and p_{st-1} >= m) is IDLE: its scan blocks return at
//              once, its select leaves bound and sel alone. The stage with p_st >= m whose predecessor did not is the
//              FINAL one: its verdicts go to the status words. Stage 0 is never idle, so sel is always written -- also
//              for m == 0 (target 0: an all-zero EtSel, the bound untouched, nothing collected, count 0).
//              A non-final prefix holds p_st >= ET_PRIME_MIN > ET_KMAX entries, all allowed: its bound holds k rows.
//   bit form   one bitmap per query (filter_stride_words != 0): the scan over all n rows, a pair counted and collected
//              only if the row's bit is set in that query's bitmap. Work ~ n x nq. A block's 32 rows of one step share
//              one filter word per query (the step starts at a multiple of 32): lane (l & 31) of every wave loads query
//              l's word beside the row, the query loop reads it back by readlane. A query none of the wave's eight rows
//              is allowed for is skipped by that wave -- a wave-uniform skip: et_dist shuffles across the wave.
//              Priming: see etf_select_kernel.
// Compiled with -ffp-contract=off, like everything that calls et_dist.
#pragma once

#include "exact_topk.h"
#include "filter.h"

namespace granne_hip {

// ---- bitmap -> ascending id list ---------------------------------------------------------------------------------
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

// ---- the passes ---------------------------------------------------------------------------------------------------
struct EtfParams {
    EtParams P;             // exact_topk's own; P.rows: the stage's prefix p_st (pass 3: n). List form: of list ENTRIES,
                            // clipped to *m in the kernel, and P.per_range is not read (the kernel splits what is left)
    const uint32_t* list;   // list form: the allowed ids, ascending
    const uint64_t* m;      // list form: how many, on the device
    uint64_t prev_rows;     // list form: p_{st-1}; 0: no predecessor (stage 0 and pass 3 are never idle)
    const uint32_t* filter; // bit form: the queries' bitmaps (this round's first)
    uint64_t filter_stride; // bit form: words from one query's bitmap to the next
};

// et_scan_kernel's three passes over the list (LIST) or over all rows under per-query bits (!LIST). Same grid, same LDS.
template <bool I8, int NBLK, int PASS, bool LIST>
__global__ __launch_bounds__(ET_THREADS) void etf_scan_kernel(const EtfParams F) {
    static_assert(ET_GROUPS == 32u && ET_QT <= 32u, "a step's rows share one filter word; a wave's lanes 0..31 hold a tile's words");
    const EtParams& P = F.P;
    extern __shared__ __align__(16) uint8_t smem_etf[];
    __shared__ uint32_t s_bound[ET_QT], s_b1[ET_QT], s_on[ET_QT];
    __shared__ int s_dy[ET_QT];
    uint64_t rows = P.rows;
    if constexpr (LIST) {
        const uint64_t m = *F.m;
        if (F.prev_rows != 0 && F.prev_rows >= m) return; // an idle stage (the whole grid alike)
        if (m < rows) rows = m;
    }
    const uint32_t tid = threadIdx.x, lane = tid & 63u, sub = lane & 7u, grp = tid >> 3;
    const uint32_t q0 = blockIdx.x * ET_QT;
    const uint32_t qn = P.nq - q0 < ET_QT ? P.nq - q0 : ET_QT;
    uint32_t on = 0;
    if (tid < ET_QT) {
        uint32_t b1 = 0, bound = 0;
        if (tid < qn) {
            bound = P.bound[q0 + tid];
            on = 1;
            if constexpr (PASS == 2) {
                const EtSel s = P.sel[q0 + tid];
                on = s.need2;
                b1 = s.b1;
            }
            if constexpr (PASS == 3) on = P.sel[q0 + tid].over ? 0u : 1u;
        }
        s_bound[tid] = bound, s_b1[tid] = b1, s_on[tid] = on, s_dy[tid] = 0;
    }
    if (!__syncthreads_or((int)on)) return; // no query of the tile takes part in this pass
    uint64_t per_range = P.per_range;
    if constexpr (LIST) per_range = ((rows + gridDim.y - 1) / gridDim.y + ET_GROUPS - 1) / ET_GROUPS * ET_GROUPS;
    const uint64_t r0 = (uint64_t)blockIdx.y * per_range;
    const uint64_t r1 = r0 + per_range < rows ? r0 + per_range : rows;
    if (r0 >= r1) return; // (list form: the ranges past the m entries)
    if constexpr (NBLK > 0) {
        if constexpr (!I8) {
            float* sq = reinterpret_cast<float*>(smem_etf);
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
                smem_etf[i] = c < P.dim ? gq[(size_t)qi * P.dim + c] : (uint8_t)0;
            }
        }
        __syncthreads();
        if constexpr (I8) {
            if (tid < qn) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(smem_etf + (size_t)tid * P.q_lds);
                int dy = 0;
                for (uint32_t i = 0; i < P.q_lds / 4u; ++i) dy = dot4_i8(w[i], w[i], dy);
                s_dy[tid] = dy;
            }
            __syncthreads();
        }
    }
    for (uint64_t e0 = r0; e0 < r1; e0 += ET_GROUPS) { // e0: a multiple of ET_GROUPS = 32 (per_range is one)
        const uint64_t e = e0 + grp;
        const bool live = e < r1;
        uint64_t row = live ? e : r1 - 1;
        if constexpr (LIST) row = F.list[row];
        uint32_t fw = 0; // bit form: lane l & 31 holds the word of the tile's query l & 31 with this step's 32 rows
        if constexpr (!LIST) {
            if ((lane & 31u) < qn) fw = F.filter[(uint64_t)(q0 + (lane & 31u)) * F.filter_stride + (e0 >> 5)];
        }
        EtRow<I8, NBLK> R;
        et_load_row<I8, NBLK>(R, P.elements + row * (uint64_t)P.row_stride, P.row_bytes, lane);
        for (uint32_t qi = 0; qi < qn; ++qi) {
            if (!s_on[qi]) continue;
            bool allowed = true;
            if constexpr (!LIST) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)fw, (int)qi);
                if (((w >> ((tid >> 6) * 8u)) & 0xFFu) == 0u) continue; // none of this wave's eight rows: the whole wave skips
                allowed = (w >> grp) & 1u;
            }
            const uint8_t* qp = NBLK > 0 ? smem_etf + (size_t)qi * P.q_lds
                                         : P.queries + (size_t)(q0 + qi) * P.dim * (I8 ? 1u : 4u);
            const float d = et_dist<I8, NBLK>(R, qp, s_dy[qi], P.dim, P.row_bytes, lane);
            if (live && allowed && sub == 0u) {
                const uint32_t key = et_key(d);
                if (key <= s_bound[qi]) {
                    const size_t q = q0 + qi;
                    if constexpr (PASS == 1) {
                        atomicAdd(P.hist + q * ET_BINS1 + (key >> 11), 1u);
                    } else if constexpr (PASS == 2) {
                        if ((key >> 11) == s_b1[qi]) atomicAdd(P.hist + q * ET_BINS2 + (key & 2047u), 1u);
                    } else {
                        const uint32_t pos = atomicAdd(P.cnt + q, 1u);
                        if (pos < ET_CAP) P.cand[q * ET_CAP + pos] = (uint64_t)__float_as_uint(d) << 32 | (uint64_t)(uint32_t)row;
                    }
                }
            }
        }
    }
}

// et_select_kernel for the filtered passes. `rows`: the stage's prefix p_st; `total`: what the pass counted at or below
// the query's bound.
//   LIST   prev_rows and *m decide whether the stage is idle (nothing is touched) and whether it is final (the header).
//          The target is min(k, min(p_st, m)): every entry of the prefix is an allowed row.
//   !LIST  `final` is the host's (the last stage scans all n rows). A prefix may hold fewer than k allowed rows of a
//          query. A bound taken from those -- a key that min(k, allowed rows OF THE PREFIX) rows are at or below -- would
//          be too tight for a longer prefix, which may hold allowed rows between it and the true k-th key. So a NON-FINAL
//          stage narrows only on evidence that lasts: total >= k rows of the prefix at or below the new bound are k rows
//          of every longer prefix too. With total < k it keeps the bound it has. Only the final stage, which has seen
//          every row, uses target = min(k, total): a bound below all-ones already holds k allowed rows (total >= k), so
//          total < k means the bound is all-ones and total is every allowed row of the query.
// A target of 0 (no allowed id) stores an all-zero EtSel and leaves the bound: pass 3 collects nothing, the count is 0.
// The second level is reached only past ET_CAP > ET_KMAX rows at or below B1: its target is k - below1 in both forms.
template <int LEVEL, bool LIST>
__global__ __launch_bounds__(256) void etf_select_kernel(const uint32_t* hist, uint32_t k, uint64_t rows, uint64_t prev_rows, const uint64_t* m_ptr,
                                                         uint32_t* bound, EtSel* sel, uint32_t final, uint32_t* status) {
    constexpr uint32_t NB = LEVEL == 1 ? ET_BINS1 : ET_BINS2, PER = NB / 256u;
    __shared__ uint32_t s_wave[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if constexpr (LIST) {
        const uint64_t m = *m_ptr;
        if (prev_rows != 0 && prev_rows >= m) return; // idle: bound and sel stay the final stage's
        final = rows >= m ? 1u : 0u;
        if (m < rows) rows = m;
    }
    EtSel s = sel[q];
    if constexpr (LEVEL == 2) {
        if (!s.need2) return;
    } else {
        s.b1 = 0, s.below1 = 0, s.need2 = 0, s.over = 0;
    }
    uint32_t c[PER], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        c[i] = hist[(size_t)q * NB + tid * PER + i];
        mine += c[i];
    }
    uint32_t total;
    const uint32_t before = fl_block_exclusive<4>(mine, s_wave, &total);
    uint32_t target;
    if constexpr (LEVEL == 2) target = k - s.below1;
    else if constexpr (LIST) target = rows < k ? (uint32_t)rows : k;
    else target = final && total < k ? total : k;
    if (target == 0 || total < target) { // nothing allowed, or (!LIST, not final) too few allowed rows yet: nothing is narrowed
        if (tid == 0) {
            s.need2 = 0;
            sel[q] = s;
        }
        return;
    }
    if (before < target && before + mine >= target) { // one thread's bins hold the target
        uint32_t b = 0, below = before;
#pragma unroll
        for (uint32_t i = 0; i < PER; ++i) {
            if (below < target && below + c[i] >= target) {
                b = tid * PER + i;
                break;
            }
            below += c[i];
        }
        const uint32_t pop = hist[(size_t)q * NB + b];
        const uint32_t old = bound[q];
        if constexpr (LEVEL == 1) {
            s.b1 = b, s.below1 = below;
            if (below + pop <= ET_CAP) {
                const uint32_t nb = (b << 11) | 2047u;
                bound[q] = nb < old ? nb : old;
            } else {
                s.need2 = 1;
                if (final && status) atomicAdd(status + 1, 1u);
            }
        } else {
            const uint32_t nb = (s.b1 << 11) | b;
            bound[q] = nb < old ? nb : old; // holds k rows whether or not they fit
            if (s.below1 + below + pop > ET_CAP) {
                s.over = 1;
                if (final && status) atomicAdd(status + 0, 1u);
            }
        }
        sel[q] = s;
    }
}

typedef void (*EtfScanFn)(const EtfParams);
template <bool I8, int NBLK, bool LIST>
inline EtfScanFn etf_scan_pass(int pass) {
    return pass == 1 ? etf_scan_kernel<I8, NBLK, 1, LIST> : pass == 2 ? etf_scan_kernel<I8, NBLK, 2, LIST> : etf_scan_kernel<I8, NBLK, 3, LIST>;
}
template <bool I8, bool LIST>
inline EtfScanFn etf_scan_blocks(uint32_t nblk, int pass) {
    return nblk <= 1 ? etf_scan_pass<I8, 1, LIST>(pass) : nblk <= 2 ? etf_scan_pass<I8, 2, LIST>(pass) : nblk <= 4 ? etf_scan_pass<I8, 4, LIST>(pass)
         : nblk <= 8 ? etf_scan_pass<I8, 8, LIST>(pass) : etf_scan_pass<I8, 0, LIST>(pass);
}
// the pass's kernel as et_scan_fn picks it: the fewest register blocks that hold the row, or the memory form
inline EtfScanFn etf_scan_fn(bool i8, uint32_t row_bytes, int pass, bool list) {
    const uint32_t nblk = (row_bytes + 127u) / 128u;
    if (i8) return list ? etf_scan_blocks<true, true>(nblk, pass) : etf_scan_blocks<true, false>(nblk, pass);
    return list ? etf_scan_blocks<false, true>(nblk, pass) : etf_scan_blocks<false, false>(nblk, pass);
}

} // namespace granne_hip
