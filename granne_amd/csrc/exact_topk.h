// exact_topk.h -- the k nearest elements of every query, exact by construction (granne_hip_exact_topk_device): every
// (query, row) distance is computed in the reference's own arithmetic -- dists_kernel's, bit for bit (util_kernels.h) --
// and the k smallest are selected by the total key (distance bits, id). No score, no spare margin: the yardstick next to
// brute_force.h's matrix-core scan, for k up to 1024. Slower than that scan (all VALU, several passes over the rows).
//
//   distance  et_dist: eight lanes per row, lane `sub` owns accumulators 4 sub .. 4 sub + 3 of the reference's 32
//             (src/math.rs:5-52), ordered_sum8 down the eight lanes, the tail by sequential fmas, angular_from_dot; int8
//             rows by dot4_i8 sums and angular_int_from_sums. EVERY pass calls this one function: a row's key in the
//             counting passes is its key in the collecting pass.
//   movement  a block stages a tile of ET_QT queries in LDS; each eight-lane group keeps ITS ROW IN REGISTERS across the
//             query loop (device rows of up to 1024 bytes: f32 to 256 components, int8 to 1024). Longer rows (NBLK = 0)
//             are read again per query, with the query, from memory -- dists_kernel's own loop.
//   key       et_key(d): a monotone 32-bit function of the distance over [0, +inf]. d < 2: floor(d * 2^21) (exact: a
//             power-of-two product); d >= 2: (bits(d) >> 9) + 2^21. Its upper bits are the first-level bin (3072 of them:
//             floor(d * 1024) below 2, 2048 + (bits >> 20) - 1024 from 2 on), its low 11 bits the second-level bin inside
//             it ((d * 1024 - B1) * 2048 below 2, (bits >> 9) & 2047 from 2 on).
//   selection per query, a `bound`: a key that at least min(k, rows) rows are at or below. PASS 1 counts the rows at or
//             below the bound per first-level bin; et_select_kernel<1> finds B1, the first bin whose prefix reaches
//             min(k, rows). If the rows up to B1 number at most ET_CAP the bound becomes B1's last key; otherwise PASS 2
//             counts B1's rows per second-level bin for that query alone (blocks without such a query exit at once) and
//             et_select_kernel<2> finds B2 by the same rule with k - below1. More than ET_CAP rows at or below (B1, B2):
//             the query OVERFLOWS (thousands of rows inside one 2^-21 wide bin at the k-th distance) -- status[0], count 0,
//             a filled row; never a partial list. PASS 3 collects the (distance bits, id) keys at or below the bound --
//             exactly the rows counted -- and et_rank_kernel sorts them in LDS (bitonic, 4096 x 8 bytes) and writes k.
//   priming   counting EVERY pair would be rows x queries atomics on a few hot bins per query. The selection (passes 1
//             and 2, no collection) first runs over prefixes of the rows, each 16 times the one before, the first
//             unbounded: a prefix's bound holds for every longer prefix, so a stage counts about 16 k rows per query
//             whatever its length. The stages are a function of (n) alone: no host decision between kernels.
//   sources   which (query, row) pairs a pass looks at (EtSrc) -- the one thing in which
//             granne_hip_exact_topk_filtered_device differs. Distances, keys, selection and ranking are the same code.
//             ET_ALL   every row of the prefix, for every query.
//             ET_LIST  one bitmap for every query, compacted to its ids, ascending (filter.h, fl_*): the passes walk that
//                      list, entry e names row list[e]. Work ~ m x nq for m allowed ids. The candidate key holds list[e],
//                      the GLOBAL id: et_rank_kernel orders ties by it. m lives on the device only; nothing is read back.
//                      The grids and the prefixes p_0 < .. < p_last = n stay functions of n; a stage's entries are
//                      [0, min(p_st, m)). A stage whose predecessor covered the whole list (st > 0 and p_{st-1} >= m) is
//                      IDLE: its scan blocks return at once, its select leaves bound and sel alone. The stage with
//                      p_st >= m whose predecessor did not is the FINAL one: its verdicts go to the status words. Stage 0
//                      is never idle, so sel is always written -- also for m == 0 (target 0: an all-zero EtSel, the bound
//                      untouched, nothing collected, count 0). A non-final prefix holds p_st >= ET_PRIME_MIN > ET_KMAX
//                      entries, all allowed: its bound holds k rows. ET_ALL is this rule with the identity list and
//                      m = n (never idle, the last stage final); its scan reads no list and no m.
//             ET_BITS  one bitmap per query: the scan over all n rows, a pair counted and collected only if the row's bit
//                      is set in that query's bitmap. Work ~ n x nq. A block's 32 rows of one step share one filter word
//                      per query (the step starts at a multiple of 32): lane (l & 31) of every wave loads query l's word
//                      beside the row, the query loop reads it back by readlane. A query none of the wave's eight rows is
//                      allowed for is skipped by that wave -- a wave-uniform skip: et_dist shuffles across the wave.
//                      Priming: see et_select_kernel.
// Compiled with -ffp-contract=off: every fused operation is an explicit fmaf.
#pragma once

#include "dist.h"
#include "filter.h"
#include "ordered_sum.h"

namespace granne_hip {

constexpr uint32_t ET_KMAX = 1024;   // GRANNE_HIP_EXACT_TOPK_KMAX
constexpr uint32_t ET_CAP = 4096;    // GRANNE_HIP_EXACT_TOPK_CAP: keys ranked per query
constexpr uint32_t ET_BINS1 = 3072, ET_BINS2 = 2048;
constexpr uint32_t ET_CHUNK = 1024;  // queries per round of the passes (the scratch is sized by it)
constexpr uint32_t ET_QT = 32;       // queries staged per block
constexpr uint32_t ET_THREADS = 256; // 32 groups of eight lanes
constexpr uint32_t ET_GROUPS = ET_THREADS / 8u;
constexpr uint32_t ET_RANK_THREADS = 512;
constexpr uint32_t ET_PRIME_MIN = 16384; // shortest prefix a priming stage scans (> ET_KMAX: a prefix holds k rows)
constexpr uint32_t ET_PRIME_STEP = 16;   // a stage's prefix over the one before

__device__ __forceinline__ uint32_t et_key(float d) {
    return d < 2.0f ? (uint32_t)(d * 2097152.0f) : (__float_as_uint(d) >> 9) + (1024u << 11);
}

struct EtSel {
    uint32_t b1, below1; // the first-level bin of the k-th key, the rows in the bins before it
    uint32_t need2;      // the rows up to b1 exceed ET_CAP: the second level decides
    uint32_t over;       // the rows up to (b1, b2) still do
};

enum EtSrc { ET_ALL, ET_LIST, ET_BITS }; // the pairs a pass looks at (the header, sources)

struct EtParams {
    const uint8_t* elements; // device rows: row_bytes of (zero padded) data every row_stride bytes
    uint64_t rows;           // the prefix this pass scans: the stage's p_st (pass 3: n). ET_LIST: of list ENTRIES, clipped
                             // to *m in the kernel
    uint32_t row_bytes, row_stride, dim;
    const uint8_t* queries;  // dense [nq][dim] (this round's)
    uint32_t nq, q_lds;      // q_lds: bytes of a staged query (a multiple of 16; int8: zero padded to row_bytes)
    uint64_t per_range;      // rows per blockIdx.y (a multiple of ET_GROUPS). ET_LIST: not read, the kernel splits what is left
    const uint32_t* bound;   // [nq] keys above it are not counted or collected
    const EtSel* sel;        // [nq] (passes 2 and 3)
    uint32_t* hist;          // pass 1: [nq][ET_BINS1], pass 2: [nq][ET_BINS2]
    uint32_t* cnt;           // pass 3: [nq] keys collected
    uint64_t* cand;          // pass 3: [nq][ET_CAP] distance bits << 32 | id
    // the sources' own fields. (Last on purpose: between q_lds and bound they change how the kernel's arguments are
    // loaded, and the f32 memory form's collecting pass then takes 66 VGPRs for 46 -- seven waves per SIMD for eight.)
    const uint32_t* list;    // ET_LIST: the allowed ids, ascending
    const uint64_t* m;       // ET_LIST: how many, on the device
    uint64_t prev_rows;      // ET_LIST: p_{st-1}; 0: no predecessor (stage 0 and pass 3 are never idle)
    const uint32_t* filter;  // ET_BITS: the queries' bitmaps (this round's first)
    uint64_t filter_stride;  // ET_BITS: words from one query's bitmap to the next
};

// A group's row. NBLK > 0: its 128-byte blocks in registers, lane `sub` holding the 16-byte piece `sub` of each (pieces
// past row_bytes are zero); int8: the row's own sum of squares. NBLK = 0: the row stays in memory.
template <bool I8, int NBLK>
struct EtRow {
    uint4 v[NBLK > 0 ? NBLK : 1];
    const uint8_t* p;
    int dx;
};

template <bool I8, int NBLK>
__device__ __forceinline__ void et_load_row(EtRow<I8, NBLK>& R, const uint8_t* row, uint32_t row_bytes, uint32_t lane) {
    const uint32_t sub = lane & 7u;
    R.p = row;
    R.dx = 0;
    if constexpr (NBLK > 0) {
#pragma unroll
        for (int c = 0; c < NBLK; ++c) {
            R.v[c] = make_uint4(0, 0, 0, 0);
            if ((uint32_t)c * 128u + sub * 16u + 16u <= row_bytes)
                R.v[c] = *reinterpret_cast<const uint4*>(row + (size_t)c * 128u + sub * 16u);
        }
        if constexpr (I8) {
            int dx = 0;
#pragma unroll
            for (int c = 0; c < NBLK; ++c) {
                dx = dot4_i8(R.v[c].x, R.v[c].x, dx); dx = dot4_i8(R.v[c].y, R.v[c].y, dx);
                dx = dot4_i8(R.v[c].z, R.v[c].z, dx); dx = dot4_i8(R.v[c].w, R.v[c].w, dx);
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) dx += __shfl_xor(dx, o, 64);
            R.dx = dx;
        }
    }
}

// The distance of the group's row to one query, in every lane of the group. q: the staged query (NBLK > 0: LDS, 16-byte
// aligned, int8 zero padded to row_bytes) or the caller's own (NBLK = 0). dy: the staged int8 query's sum of squares.
// Every lane of the wave calls it.
template <bool I8, int NBLK>
__device__ __forceinline__ float et_dist(const EtRow<I8, NBLK>& R, const uint8_t* q, int dy, uint32_t dim, uint32_t row_bytes,
                                         uint32_t lane) {
    const uint32_t sub = lane & 7u;
    if constexpr (!I8) {
        const float* qf = reinterpret_cast<const float*>(q);
        const uint32_t nfull = dim >> 5, tail = dim & 31u;
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        uint4 vt = make_uint4(0, 0, 0, 0); // the (zero padded) tail block
        if constexpr (NBLK > 0) {
#pragma unroll
            for (int c = 0; c < NBLK; ++c) {
                if ((uint32_t)c < nfull) {
                    const float4 qc = *reinterpret_cast<const float4*>(qf + c * 32 + sub * 4u);
                    a0 = __builtin_fmaf(__uint_as_float(R.v[c].x), qc.x, a0);
                    a1 = __builtin_fmaf(__uint_as_float(R.v[c].y), qc.y, a1);
                    a2 = __builtin_fmaf(__uint_as_float(R.v[c].z), qc.z, a2);
                    a3 = __builtin_fmaf(__uint_as_float(R.v[c].w), qc.w, a3);
                } else if ((uint32_t)c == nfull) {
                    vt = R.v[c];
                }
            }
        } else {
#pragma unroll 4
            for (uint32_t c = 0; c < nfull; ++c) {
                const uint4 v = *reinterpret_cast<const uint4*>(R.p + (size_t)c * 128u + sub * 16u);
                const float* qc = qf + c * 32u + sub * 4u;
                a0 = __builtin_fmaf(__uint_as_float(v.x), qc[0], a0);
                a1 = __builtin_fmaf(__uint_as_float(v.y), qc[1], a1);
                a2 = __builtin_fmaf(__uint_as_float(v.z), qc[2], a2);
                a3 = __builtin_fmaf(__uint_as_float(v.w), qc[3], a3);
            }
            if (nfull * 128u + sub * 16u + 16u <= row_bytes)
                vt = *reinterpret_cast<const uint4*>(R.p + (size_t)nfull * 128u + sub * 16u);
        }
        float r = ordered_sum8(a0, a1, a2, a3, lane); // acc[0] .. acc[31] in order
        for (uint32_t k = 0; k < tail; ++k) {         // src/math.rs:47-49
            const uint32_t w = (k & 3u) == 0 ? vt.x : (k & 3u) == 1 ? vt.y : (k & 3u) == 2 ? vt.z : vt.w;
            const float xv = __uint_as_float((uint32_t)__shfl((int)w, (int)((lane & ~7u) + (k >> 2)), 64));
            r = __builtin_fmaf(xv, qf[nfull * 32u + k], r);
        }
        return angular_from_dot(r);
    } else {
        int r = 0, dx = R.dx;
        if constexpr (NBLK > 0) {
#pragma unroll
            for (int c = 0; c < NBLK; ++c) {
                if ((uint32_t)c * 128u + sub * 16u + 16u <= row_bytes) {
                    const uint4 qw = *reinterpret_cast<const uint4*>(q + c * 128 + sub * 16u);
                    r = dot4_i8(R.v[c].x, qw.x, r); r = dot4_i8(R.v[c].y, qw.y, r);
                    r = dot4_i8(R.v[c].z, qw.z, r); r = dot4_i8(R.v[c].w, qw.w, r);
                }
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) r += __shfl_xor(r, o, 64);
        } else {
            const int8_t* qb = reinterpret_cast<const int8_t*>(q);
            dy = 0;
            for (uint32_t b = sub * 16u; b < row_bytes; b += 128u) {
                const uint4 v = *reinterpret_cast<const uint4*>(R.p + b);
                uint32_t qw[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t o = b + 4u * j;
                    uint32_t w = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (o + e < dim) w |= (uint32_t)(uint8_t)qb[o + e] << (8 * e);
                    qw[j] = w;
                }
                r = dot4_i8(v.x, qw[0], r); r = dot4_i8(v.y, qw[1], r);
                r = dot4_i8(v.z, qw[2], r); r = dot4_i8(v.w, qw[3], r);
                dx = dot4_i8(v.x, v.x, dx); dx = dot4_i8(v.y, v.y, dx);
                dx = dot4_i8(v.z, v.z, dx); dx = dot4_i8(v.w, v.w, dx);
                dy = dot4_i8(qw[0], qw[0], dy); dy = dot4_i8(qw[1], qw[1], dy);
                dy = dot4_i8(qw[2], qw[2], dy); dy = dot4_i8(qw[3], qw[3], dy);
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                r += __shfl_xor(r, o, 64);
                dx += __shfl_xor(dx, o, 64);
                dy += __shfl_xor(dy, o, 64);
            }
        }
        return angular_int_from_sums(r, dx, dy);
    }
}

// One pass over the rows (ET_LIST: the list's entries) [0, P.rows): grid = (query tiles of ET_QT, row ranges). PASS 1
// counts first-level bins, PASS 2 the second-level bins inside sel.b1 of the queries that need them, PASS 3 collects the
// keys at or below the bound. SRC: where a row index comes from, whether a pair is admitted, what the range is clipped to.
template <bool I8, int NBLK, int PASS, EtSrc SRC>
__global__ __launch_bounds__(ET_THREADS) void et_scan_kernel(const EtParams P) {
    static_assert(ET_GROUPS == 32u && ET_QT <= 32u, "a step's rows share one filter word; a wave's lanes 0..31 hold a tile's words");
    extern __shared__ __align__(16) uint8_t smem_et[];
    __shared__ uint32_t s_bound[ET_QT], s_b1[ET_QT], s_on[ET_QT];
    __shared__ int s_dy[ET_QT];
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
                if (key <= s_bound[qi]) {
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
template <int LEVEL, EtSrc SRC>
__global__ __launch_bounds__(256) void et_select_kernel(const uint32_t* hist, uint32_t k, uint64_t rows, uint64_t prev_rows, const uint64_t* m_ptr,
                                                        uint64_t m_all, uint32_t* bound, EtSel* sel, uint32_t final, uint32_t* status) {
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
    else if constexpr (SRC == ET_LIST) target = rows < k ? (uint32_t)rows : k;
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

// The first m (<= ET_CAP) keys of `cand` into `keys` (LDS, ET_CAP entries), sorted ascending (bitonic, padded with all-ones
// to a power of two); every thread of a block of ET_RANK_THREADS calls it, and the keys are in place when it returns.
__device__ __forceinline__ void et_sort_keys(uint64_t* keys, const uint64_t* cand, uint32_t m, uint32_t tid) {
    uint32_t n2 = 2;
    while (n2 < m) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += ET_RANK_THREADS) keys[i] = i < m ? cand[i] : ~0ull;
    for (uint32_t size = 2; size <= n2; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (uint32_t i = tid; i < n2 / 2u; i += ET_RANK_THREADS) {
                const uint32_t lo = 2u * i - (i & (stride - 1u)), hi = lo + stride;
                const bool asc = (lo & size) == 0u;
                const uint64_t a = keys[lo], b = keys[hi];
                if ((a > b) == asc) keys[lo] = b, keys[hi] = a;
            }
        }
    }
    __syncthreads();
}

// One block per query: the collected keys sorted in LDS, the first k written; places past the count hold UINT64_MAX / +inf.
// `over` (optional, u32 per query): 1 where EtSel.over voids the query, else 0 (the partitioned selection carries it on).
__global__ __launch_bounds__(ET_RANK_THREADS) void et_rank_kernel(const uint64_t* cand, const uint32_t* cnt, const EtSel* sel, uint32_t k,
                                                                  uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                                  uint32_t* status, uint32_t* over) {
    __shared__ uint64_t keys[ET_CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t m = cnt[q] < ET_CAP ? cnt[q] : ET_CAP;
    if (sel[q].over) m = 0;
    et_sort_keys(keys, cand + (size_t)q * ET_CAP, m, tid);
    const uint32_t count = m < k ? m : k;
    for (uint32_t i = tid; i < k; i += ET_RANK_THREADS) {
        const uint64_t key = i < count ? keys[i] : 0;
        out_ids[(size_t)q * k + i] = i < count ? (key & 0xFFFFFFFFull) : ~0ull;
        out_dists[(size_t)q * k + i] = i < count ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
    }
    if (tid == 0) {
        out_counts[q] = count;
        if (over) over[q] = sel[q].over ? 1u : 0u;
        if (status) atomicMax(status + 2, m);
    }
}

typedef void (*EtScanFn)(const EtParams);
template <bool I8, int NBLK, EtSrc SRC>
inline EtScanFn et_scan_pass(int pass) {
    return pass == 1 ? et_scan_kernel<I8, NBLK, 1, SRC> : pass == 2 ? et_scan_kernel<I8, NBLK, 2, SRC> : et_scan_kernel<I8, NBLK, 3, SRC>;
}
template <bool I8, EtSrc SRC>
inline EtScanFn et_scan_blocks(uint32_t nblk, int pass) {
    return nblk <= 1 ? et_scan_pass<I8, 1, SRC>(pass) : nblk <= 2 ? et_scan_pass<I8, 2, SRC>(pass) : nblk <= 4 ? et_scan_pass<I8, 4, SRC>(pass)
         : nblk <= 8 ? et_scan_pass<I8, 8, SRC>(pass) : et_scan_pass<I8, 0, SRC>(pass);
}
template <bool I8>
inline EtScanFn et_scan_src(uint32_t nblk, int pass, EtSrc src) {
    return src == ET_ALL ? et_scan_blocks<I8, ET_ALL>(nblk, pass) : src == ET_LIST ? et_scan_blocks<I8, ET_LIST>(nblk, pass)
                                                                                    : et_scan_blocks<I8, ET_BITS>(nblk, pass);
}
// the pass's kernel for device rows of row_bytes: the fewest register blocks that hold the row, or the memory form
inline EtScanFn et_scan_fn(bool i8, uint32_t row_bytes, int pass, EtSrc src) {
    const uint32_t nblk = (row_bytes + 127u) / 128u;
    return i8 ? et_scan_src<true>(nblk, pass, src) : et_scan_src<false>(nblk, pass, src);
}
// the level's select for the source: ET_ALL is served by the list rule (et_select_kernel)
typedef void (*EtSelectFn)(const uint32_t*, uint32_t, uint64_t, uint64_t, const uint64_t*, uint64_t, uint32_t*, EtSel*, uint32_t, uint32_t*);
inline EtSelectFn et_select_fn(int level, EtSrc src) {
    if (src == ET_BITS) return level == 1 ? et_select_kernel<1, ET_BITS> : et_select_kernel<2, ET_BITS>;
    return level == 1 ? et_select_kernel<1, ET_LIST> : et_select_kernel<2, ET_LIST>;
}

} // namespace granne_hip
