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
// Compiled with -ffp-contract=off: every fused operation is an explicit fmaf.
#pragma once

#include "dist.h"
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

struct EtParams {
    const uint8_t* elements; // device rows: row_bytes of (zero padded) data every row_stride bytes
    uint64_t rows;           // the prefix this pass scans
    uint32_t row_bytes, row_stride, dim;
    const uint8_t* queries;  // dense [nq][dim] (this round's)
    uint32_t nq, q_lds;      // q_lds: bytes of a staged query (a multiple of 16; int8: zero padded to row_bytes)
    uint64_t per_range;      // rows per blockIdx.y (a multiple of ET_GROUPS)
    const uint32_t* bound;   // [nq] keys above it are not counted or collected
    const EtSel* sel;        // [nq] (passes 2 and 3)
    uint32_t* hist;          // pass 1: [nq][ET_BINS1], pass 2: [nq][ET_BINS2]
    uint32_t* cnt;           // pass 3: [nq] keys collected
    uint64_t* cand;          // pass 3: [nq][ET_CAP] distance bits << 32 | id
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

// One pass over rows [0, P.rows): grid = (query tiles of ET_QT, row ranges). PASS 1 counts first-level bins, PASS 2 the
// second-level bins inside sel.b1 of the queries that need them, PASS 3 collects the keys at or below the bound.
template <bool I8, int NBLK, int PASS>
__global__ __launch_bounds__(ET_THREADS) void et_scan_kernel(const EtParams P) {
    extern __shared__ __align__(16) uint8_t smem_et[];
    __shared__ uint32_t s_bound[ET_QT], s_b1[ET_QT], s_on[ET_QT];
    __shared__ int s_dy[ET_QT];
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
    const uint64_t r0 = (uint64_t)blockIdx.y * P.per_range;
    const uint64_t r1 = r0 + P.per_range < P.rows ? r0 + P.per_range : P.rows;
    for (uint64_t e0 = r0; e0 < r1; e0 += ET_GROUPS) {
        const uint64_t e = e0 + grp;
        const bool live = e < r1;
        EtRow<I8, NBLK> R;
        et_load_row<I8, NBLK>(R, P.elements + (live ? e : r1 - 1) * (uint64_t)P.row_stride, P.row_bytes, lane);
        for (uint32_t qi = 0; qi < qn; ++qi) {
            if (!s_on[qi]) continue;
            const uint8_t* qp = NBLK > 0 ? smem_et + (size_t)qi * P.q_lds
                                         : P.queries + (size_t)(q0 + qi) * P.dim * (I8 ? 1u : 4u);
            const float d = et_dist<I8, NBLK>(R, qp, s_dy[qi], P.dim, P.row_bytes, lane);
            if (live && sub == 0u) {
                const uint32_t key = et_key(d);
                if (key <= s_bound[qi]) {
                    const size_t q = q0 + qi;
                    if constexpr (PASS == 1) {
                        atomicAdd(P.hist + q * ET_BINS1 + (key >> 11), 1u);
                    } else if constexpr (PASS == 2) {
                        if ((key >> 11) == s_b1[qi]) atomicAdd(P.hist + q * ET_BINS2 + (key & 2047u), 1u);
                    } else {
                        const uint32_t pos = atomicAdd(P.cnt + q, 1u);
                        if (pos < ET_CAP) P.cand[q * ET_CAP + pos] = (uint64_t)__float_as_uint(d) << 32 | (uint64_t)(uint32_t)e;
                    }
                }
            }
        }
    }
}

// One block per query over the histogram of a counting pass: the first bin whose prefix reaches the target, and what
// follows from it (the header's rule). `final`: the pass ran over all rows -- its verdicts go to the status words.
template <int LEVEL>
__global__ __launch_bounds__(256) void et_select_kernel(const uint32_t* hist, uint32_t k, uint64_t rows, uint32_t* bound, EtSel* sel,
                                                        uint32_t final, uint32_t* status) {
    constexpr uint32_t NB = LEVEL == 1 ? ET_BINS1 : ET_BINS2, PER = NB / 256u;
    __shared__ uint32_t s_wave[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    EtSel s = sel[q];
    if constexpr (LEVEL == 2) {
        if (!s.need2) return;
    } else {
        s.b1 = 0, s.below1 = 0, s.need2 = 0, s.over = 0;
    }
    uint32_t target = rows < k ? (uint32_t)rows : k;
    if constexpr (LEVEL == 2) target -= s.below1;
    uint32_t c[PER], mine = 0;
#pragma unroll
    for (uint32_t i = 0; i < PER; ++i) {
        c[i] = hist[(size_t)q * NB + tid * PER + i];
        mine += c[i];
    }
    uint32_t incl = mine; // inclusive scan over the wave, then over the four waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
        if (lane >= (uint32_t)o) incl += up;
    }
    if (lane == 63u) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = incl - mine, total = 0;
    for (uint32_t w = 0; w < 4; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    if (total < target) { // (cannot happen: the bound holds min(k, rows) rows; then nothing is narrowed)
        if (tid == 0) {
            s.over = total > ET_CAP ? 1u : 0u;
            s.need2 = 0;
            sel[q] = s;
            if (s.over && final && status) atomicAdd(status + 0, 1u);
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

// One block per query: the collected keys sorted in LDS, the first k written; places past the count hold UINT64_MAX / +inf.
__global__ __launch_bounds__(ET_RANK_THREADS) void et_rank_kernel(const uint64_t* cand, const uint32_t* cnt, const EtSel* sel, uint32_t k,
                                                                  uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                                  uint32_t* status) {
    __shared__ uint64_t keys[ET_CAP];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t m = cnt[q] < ET_CAP ? cnt[q] : ET_CAP;
    if (sel[q].over) m = 0;
    uint32_t n2 = 2;
    while (n2 < m) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += ET_RANK_THREADS) keys[i] = i < m ? cand[(size_t)q * ET_CAP + i] : ~0ull;
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
    const uint32_t count = m < k ? m : k;
    for (uint32_t i = tid; i < k; i += ET_RANK_THREADS) {
        const uint64_t key = i < count ? keys[i] : 0;
        out_ids[(size_t)q * k + i] = i < count ? (key & 0xFFFFFFFFull) : ~0ull;
        out_dists[(size_t)q * k + i] = i < count ? __uint_as_float((uint32_t)(key >> 32)) : __builtin_inff();
    }
    if (tid == 0) {
        out_counts[q] = count;
        if (status) atomicMax(status + 2, m);
    }
}

typedef void (*EtScanFn)(const EtParams);
template <bool I8, int NBLK>
inline EtScanFn et_scan_pass(int pass) {
    return pass == 1 ? et_scan_kernel<I8, NBLK, 1> : pass == 2 ? et_scan_kernel<I8, NBLK, 2> : et_scan_kernel<I8, NBLK, 3>;
}
// the pass's kernel for device rows of row_bytes: the fewest register blocks that hold the row, or the memory form
inline EtScanFn et_scan_fn(bool i8, uint32_t row_bytes, int pass) {
    const uint32_t nblk = (row_bytes + 127u) / 128u;
    if (i8) return nblk <= 1 ? et_scan_pass<true, 1>(pass) : nblk <= 2 ? et_scan_pass<true, 2>(pass) : nblk <= 4 ? et_scan_pass<true, 4>(pass)
                 : nblk <= 8 ? et_scan_pass<true, 8>(pass) : et_scan_pass<true, 0>(pass);
    return nblk <= 1 ? et_scan_pass<false, 1>(pass) : nblk <= 2 ? et_scan_pass<false, 2>(pass) : nblk <= 4 ? et_scan_pass<false, 4>(pass)
         : nblk <= 8 ? et_scan_pass<false, 8>(pass) : et_scan_pass<false, 0>(pass);
}

} // namespace granne_hip
