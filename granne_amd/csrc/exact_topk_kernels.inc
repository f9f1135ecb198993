// exact_topk_kernels.inc -- the scan and the select of the exact selection (exact_topk.h, which includes this text TWICE,
// inside namespace granne_hip): once as et_scan_kernel / et_select_kernel with ET_CURSOR false -- the kernels there have
// always been, under their names, compiled to the instructions they were -- and once as et_scan_after_kernel /
// et_select_after_kernel with ET_CURSOR true, the forms with a cursor per query (granne_hip_exact_topk_after*; DESIGN.md
// 3.7h). One text, two kernel families: a body shared through an inlined device function is scheduled a little differently
// from the kernel it was (60 of the 90 scans), and a flag among the template parameters renames all of them.
// Expects: ET_SCAN_KERNEL, ET_SELECT_KERNEL (the names), ET_CURSOR (false / true). No include guard, on purpose.

// One pass over the rows (ET_LIST: the list's entries) [0, P.rows): grid = (query tiles of ET_QT, row ranges). PASS 1
// counts first-level bins, PASS 2 the second-level bins inside sel.b1 of the queries that need them, PASS 3 collects the
// keys at or below the bound. SRC: where a row index comes from, whether a pair is admitted, what the range is clipped to.
//
// AFTER (granne_hip_exact_topk_after*; DESIGN.md 3.7h): every query has a CURSOR, a full key (distance bits << 32 | id),
// and a pair is counted or collected only if its full key lies beyond it -- et_past, the one expression of all three
// passes, on the bits of the distance et_key bins: a row's key in the counting passes is its key in the collecting pass,
// and a row is eligible in all of them or in none. The tile's cursors lie in LDS beside its queries as `from`, the lowest
// eligible key (et_from; 0: no cursor). Bins, bound, EtSel and the overflow rule are what they are without a cursor; the
// bins just hold the eligible rows only. A prefix may hold fewer than k of those: see et_select_kernel.
template <bool I8, int NBLK, int PASS, EtSrc SRC>
__global__ __launch_bounds__(ET_THREADS) void ET_SCAN_KERNEL(const EtParams P) {
    constexpr bool AFTER = ET_CURSOR;
    static_assert(ET_GROUPS == 32u && ET_QT <= 32u, "a step's rows share one filter word; a wave's lanes 0..31 hold a tile's words");
    extern __shared__ __align__(16) uint8_t smem_et[];
    __shared__ uint32_t s_bound[ET_QT], s_b1[ET_QT], s_on[ET_QT];
    __shared__ int s_dy[ET_QT];
    __shared__ uint64_t s_from[AFTER ? ET_QT : 1u];
    uint64_t rows = P.rows;
    if constexpr (SRC == ET_LIST) {
        const uint64_t m = *P.m;
        if (P.prev_rows != 0 && P.prev_rows >= m) return; // an idle stage (the whole grid alike)
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
        if constexpr (AFTER) s_from[tid] = tid < qn ? et_from(P.after.dists[q0 + tid], P.after.ids[q0 + tid]) : 0ull;
    }
    if (!__syncthreads_or((int)on)) return; // no query of the tile takes part in this pass
    // The range of blockIdx.y, a multiple of ET_GROUPS rows: `rows` split over the G = gridDim.y ranges launched,
    // ceil(ceil(rows / G) / 32) * 32. ET_ALL, ET_BITS: the host's P.per_range -- this expression over P.rows, raised to 32
    // for rows == 0, where r1 = 0 and nothing runs whatever the value. ET_LIST: rows was clipped to *m, known here alone.
    // (The other two could divide here too and drop the field; measured on the 10M-row f32 scan that costs ~0.15 %.)
    uint64_t per_range = P.per_range;
    if constexpr (SRC == ET_LIST) per_range = ((rows + gridDim.y - 1) / gridDim.y + ET_GROUPS - 1) / ET_GROUPS * ET_GROUPS;
    const uint64_t r0 = (uint64_t)blockIdx.y * per_range;
    const uint64_t r1 = r0 + per_range < rows ? r0 + per_range : rows;
    if (r0 >= r1) return; // (the ranges past the last row; ET_LIST: past the m entries)
    if constexpr (NBLK > 0) {
        if constexpr (!I8) {
            float* sq = reinterpret_cast<float*>(smem_et);
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
                smem_et[i] = c < P.dim ? gq[(size_t)qi * P.dim + c] : (uint8_t)0;
            }
        }
        __syncthreads();
        if constexpr (I8) {
            if (tid < qn) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(smem_et + (size_t)tid * P.q_lds);
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
        if constexpr (SRC == ET_LIST) row = P.list[row];
        uint32_t fw = 0; // ET_BITS: lane l & 31 holds the word of the tile's query l & 31 with this step's 32 rows
        if constexpr (SRC == ET_BITS) {
            if ((lane & 31u) < qn) fw = P.filter[(uint64_t)(q0 + (lane & 31u)) * P.filter_stride + (e0 >> 5)];
        }
        EtRow<I8, NBLK> R;
        et_load_row<I8, NBLK>(R, P.elements + row * (uint64_t)P.row_stride, P.row_bytes, lane);
        for (uint32_t qi = 0; qi < qn; ++qi) {
            if (!s_on[qi]) continue;
            bool allowed = true;
            if constexpr (SRC == ET_BITS) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)fw, (int)qi);
                if (((w >> ((tid >> 6) * 8u)) & 0xFFu) == 0u) continue; // none of this wave's eight rows: the whole wave skips
                allowed = (w >> grp) & 1u;
            }
            const uint8_t* qp = NBLK > 0 ? smem_et + (size_t)qi * P.q_lds
                                         : P.queries + (size_t)(q0 + qi) * P.dim * (I8 ? 1u : 4u);
            const float d = et_dist<I8, NBLK>(R, qp, s_dy[qi], P.dim, P.row_bytes, lane);
            if (live && allowed && sub == 0u) {
                const uint32_t key = et_key(d);
                bool take = key <= s_bound[qi];
                if constexpr (AFTER) take = take && et_past(d, (uint32_t)(SRC == ET_LIST ? row : e), s_from[qi]);
                if (take) {
                    const size_t q = q0 + qi;
                    if constexpr (PASS == 1) {
                        atomicAdd(P.hist + q * ET_BINS1 + (key >> 11), 1u);
                    } else if constexpr (PASS == 2) {
                        if ((key >> 11) == s_b1[qi]) atomicAdd(P.hist + q * ET_BINS2 + (key & 2047u), 1u);
                    } else {
                        const uint32_t pos = atomicAdd(P.cnt + q, 1u);
                        if (pos < ET_CAP) P.cand[q * ET_CAP + pos] = (uint64_t)__float_as_uint(d) << 32 | (uint64_t)(uint32_t)(SRC == ET_LIST ? row : e);
                    }
                }
            }
        }
    }
}

// One block per query over the histogram of a counting pass: the first bin whose prefix reaches the target, and what
// follows from it (the header's rule). `rows`: the stage's prefix p_st; `total`: what the pass counted at or below the
// query's bound; `final`: the pass saw every row there is -- its verdicts go to the status words.
//   ET_LIST  m (the list's length: *m_ptr; for ET_ALL, served by this instantiation with no m_ptr, m_all = n) and prev_rows
//            decide whether the stage is idle (nothing is touched) and whether it is final (the header). The target is
//            min(k, min(p_st, m)): every entry of the prefix is a row that counts.
//   ET_BITS  `final` is the host's (the last stage scans all n rows). A prefix may hold fewer than k allowed rows of a
//            query. A bound taken from those -- a key that min(k, allowed rows OF THE PREFIX) rows are at or below -- would
//            be too tight for a longer prefix, which may hold allowed rows between it and the true k-th key. So a NON-FINAL
//            stage narrows only on evidence that lasts: total >= k rows of the prefix at or below the new bound are k rows
//            of every longer prefix too. With total < k it keeps the bound it has. Only the final stage, which has seen
//            every row, uses target = min(k, total): a bound below all-ones already holds k allowed rows (total >= k), so
//            total < k means the bound is all-ones and total is every allowed row of the query.
// A target of 0 (no row that counts) stores an all-zero EtSel and leaves the bound: pass 3 collects nothing, the count is 0.
// The second level is reached only past ET_CAP > ET_KMAX rows at or below B1: its target is k - below1 for every source.
//   AFTER    (the scans with a cursor.) Only the rows beyond the cursor count, so ANY source's prefix may hold fewer than k
//            rows that count, as ET_BITS' may, and the same rule decides: a non-final stage narrows only on total >= k, the
//            final one uses target = min(k, total) -- the argument above, with "eligible" for "allowed". ET_LIST (and ET_ALL
//            through it) still finds idle and final on the device; only its target is ET_BITS'.
template <int LEVEL, EtSrc SRC>
__global__ __launch_bounds__(256) void ET_SELECT_KERNEL(const uint32_t* hist, uint32_t k, uint64_t rows, uint64_t prev_rows, const uint64_t* m_ptr,
                                                        uint64_t m_all, uint32_t* bound, EtSel* sel, uint32_t final, uint32_t* status) {
    constexpr bool AFTER = ET_CURSOR;
    static_assert(SRC != ET_ALL, "all rows: the list rule with m = n by value");
    constexpr uint32_t NB = LEVEL == 1 ? ET_BINS1 : ET_BINS2, PER = NB / 256u;
    __shared__ uint32_t s_wave[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if constexpr (SRC == ET_LIST) {
        const uint64_t m = m_ptr ? *m_ptr : m_all;
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
    else if constexpr (SRC == ET_LIST && !AFTER) target = rows < k ? (uint32_t)rows : k;
    else target = final && total < k ? total : k;
    // nothing that counts, or (ET_BITS, not final) too few allowed rows yet: nothing is narrowed. (ET_LIST: total < target
    // cannot happen for target > 0 -- the bound holds min(k, rows) entries.)
    if (target == 0 || total < target) {
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
