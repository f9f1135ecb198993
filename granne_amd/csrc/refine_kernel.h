// refine_kernel.h -- re-rank a query's candidate ids by the rows of one index: refine(R, q, cand, k) of
// include/granne_hip.h. The walk that made the candidates may have run on another index (int8 rows, fewer
// dimensions); here every candidate gets R's own distance, d = R.dist_to_element(id, q) -- bit for bit the
// distance of dists_kernel (util_kernels.h) and of the walkers -- and the k best by (d, id) are written in the
// walk's result order (src/index/mod.rs:1036). Citations (src/...) are paths in the reference's source tree.
//
// One workgroup of four waves per query:
//   1. the query is staged once in LDS (int8: zero padded to the device row length, so that a lane reads it in the
//      same 16-byte pieces it reads of a row);
//   2. eight lanes share a candidate's row, lane `sub` reading the 16-byte piece `sub` of every 128-byte block --
//      dists_kernel's layout: whole lines, lane `sub` owns accumulators 4 sub .. 4 sub + 3 of the reference's 32
//      (src/math.rs:5-52), the ordered sum runs down the eight lanes, the tail is folded by sequential fmas. A
//      group takes two candidates per round (64 per workgroup) and issues every load of up to four blocks of both
//      rows before it consumes one;
//   3. the (distance bits, id) keys are ranked in LDS by counting: a candidate's place is the number of keys
//      before it, ids (u64) breaking equal distances, list positions breaking equal (distance, id) pairs -- a
//      caller's list may name an id twice, and keeps both. m <= 1024, so a thread ranks at most four keys in one
//      pass over the list. Nothing depends on m being a multiple of anything.
// Rows of halves (DT_F16, f16.h) keep the eight-lanes-per-row shape: a lane's share of a 32-component block is 8 bytes of
// a 64-byte block; the row is widened, normalised (its norm by the same ordered sum, the divides spread over the eight
// lanes) and then met with the staged f32 query: f16_dist_group.
// Compiled with -ffp-contract=off: every fused operation is an explicit fmaf.
#pragma once

#include "dist.h"
#include "util_kernels.h"

namespace granne_hip {

constexpr uint32_t REFINE_MAX_M = 1024;  // candidates per query
constexpr uint32_t REFINE_THREADS = 256; // four waves: 32 groups of eight lanes
constexpr uint32_t REFINE_GROUPS = REFINE_THREADS / 8u;
constexpr uint32_t REFINE_KEYS_PER_THREAD = REFINE_MAX_M / REFINE_THREADS;

struct RefineParams {
    const uint8_t* elements;
    uint64_t n_elements;
    uint32_t row_bytes, row_stride, dim;
    const uint8_t* queries; // [nq][dim] scalars of the index's dtype, prepared
    const uint64_t* cand;   // [nq][m]
    const uint32_t* counts; // [nq]: valid entries of a list (clamped to m), or null = all m
    uint32_t m, k;
    uint32_t q_lds_bytes;   // the staged query: f32 (also for rows of halves) dim x 4 padded to 16, int8 row_bytes
    uint64_t* out_ids;      // [nq][k]
    float* out_dists;       // [nq][k]
    uint32_t* out_counts;   // [nq]
    uint32_t* status;       // optional u32: += candidates dropped (id >= n_elements, UINT64_MAX included)
};

// bytes of dynamic LDS: [m] u64 ids, [m] u32 distance bits, the query
__host__ __device__ inline uint32_t refine_lds_q_off(uint32_t m) { return (m * 12u + 15u) & ~15u; }

// NB blocks (c0 .. c0 + NB - 1) of R rows against the staged query: all loads first, then the fmas in block order
template <int NB, int R>
__device__ __forceinline__ void refine_blocks_f32(const uint8_t* (&row)[R], const float* q, uint32_t c0, uint32_t sub,
                                                  float (&a)[R][4]) {
    uint4 v[R][NB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < NB; ++i) v[r][i] = *reinterpret_cast<const uint4*>(row[r] + (size_t)(c0 + i) * 128u + sub * 16u);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const float4 qc = *reinterpret_cast<const float4*>(q + (c0 + i) * 32u + sub * 4u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r][0] = __builtin_fmaf(__uint_as_float(v[r][i].x), qc.x, a[r][0]);
            a[r][1] = __builtin_fmaf(__uint_as_float(v[r][i].y), qc.y, a[r][1]);
            a[r][2] = __builtin_fmaf(__uint_as_float(v[r][i].z), qc.z, a[r][2]);
            a[r][3] = __builtin_fmaf(__uint_as_float(v[r][i].w), qc.w, a[r][3]);
        }
    }
}

// angular distance of R rows (src/elements/angular.rs:63-74 over src/math.rs:5-52); the result is valid in every lane
// of a row's group
template <int R>
__device__ __forceinline__ void refine_dist_f32(const uint8_t* (&row)[R], const float* q, uint32_t dim, uint32_t row_bytes,
                                                uint32_t lane, float (&d)[R]) {
    const uint32_t sub = lane & 7u, nfull = dim >> 5, tail = dim & 31u;
    uint4 vt[R]; // the (zero padded) tail block
#pragma unroll
    for (int r = 0; r < R; ++r) {
        vt[r] = make_uint4(0, 0, 0, 0);
        if (nfull * 128u + sub * 16u + 16u <= row_bytes) vt[r] = *reinterpret_cast<const uint4*>(row[r] + (size_t)nfull * 128u + sub * 16u);
    }
    float a[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r][0] = a[r][1] = a[r][2] = a[r][3] = 0.0f;
    uint32_t c = 0;
    for (; c + 4u <= nfull; c += 4u) refine_blocks_f32<4, R>(row, q, c, sub, a);
    switch (nfull - c) { // (wave-uniform)
    case 3: refine_blocks_f32<3, R>(row, q, c, sub, a); break;
    case 2: refine_blocks_f32<2, R>(row, q, c, sub, a); break;
    case 1: refine_blocks_f32<1, R>(row, q, c, sub, a); break;
    default: break;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = ordered_sum8(a[r][0], a[r][1], a[r][2], a[r][3], lane); // acc[0] .. acc[31] in order
        for (uint32_t t = 0; t < tail; ++t) { // src/math.rs:47-49
            const uint32_t w = (t & 3u) == 0 ? vt[r].x : (t & 3u) == 1 ? vt[r].y : (t & 3u) == 2 ? vt[r].z : vt[r].w;
            const float xv = __uint_as_float((uint32_t)__shfl((int)w, (int)((lane & ~7u) + (t >> 2)), 64));
            s = __builtin_fmaf(xv, q[nfull * 32u + t], s);
        }
        d[r] = angular_from_dot(s);
    }
}

// NB 16-byte pieces (128 bytes apart, from byte b0) of R int8 rows: the dot with the staged query and the row's own
template <int NB, int R>
__device__ __forceinline__ void refine_pieces_i8(const uint8_t* (&row)[R], const uint8_t* q, uint32_t b0, int (&dot)[R],
                                                 int (&dx)[R]) {
    uint4 v[R][NB];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < NB; ++i) v[r][i] = *reinterpret_cast<const uint4*>(row[r] + b0 + (size_t)i * 128u);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const uint4 qw = *reinterpret_cast<const uint4*>(q + b0 + i * 128u);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint4 x = v[r][i];
            dot[r] = dot4_i8(x.x, qw.x, dot[r]); dot[r] = dot4_i8(x.y, qw.y, dot[r]);
            dot[r] = dot4_i8(x.z, qw.z, dot[r]); dot[r] = dot4_i8(x.w, qw.w, dot[r]);
            dx[r] = dot4_i8(x.x, x.x, dx[r]); dx[r] = dot4_i8(x.y, x.y, dx[r]);
            dx[r] = dot4_i8(x.z, x.z, dx[r]); dx[r] = dot4_i8(x.w, x.w, dx[r]);
        }
    }
}

// angular_int distance of R rows (src/elements/angular_int.rs:47-60 over src/math.rs:59-89): the three sums are exact in
// i32 in any order. dy = the query's own sum of squares (the same for every row: made once by the caller).
template <int R>
__device__ __forceinline__ void refine_dist_i8(const uint8_t* (&row)[R], const uint8_t* q, uint32_t row_bytes, uint32_t lane,
                                               int dy, float (&d)[R]) {
    const uint32_t sub = lane & 7u;
    int dot[R], dx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) dot[r] = dx[r] = 0;
    if (row_bytes >= 128u) { // a multiple of 128: every lane has row_bytes / 128 pieces
        const uint32_t np = row_bytes >> 7;
        uint32_t p = 0;
        for (; p + 4u <= np; p += 4u) refine_pieces_i8<4, R>(row, q, p * 128u + sub * 16u, dot, dx);
        switch (np - p) { // (wave-uniform)
        case 3: refine_pieces_i8<3, R>(row, q, p * 128u + sub * 16u, dot, dx); break;
        case 2: refine_pieces_i8<2, R>(row, q, p * 128u + sub * 16u, dot, dx); break;
        case 1: refine_pieces_i8<1, R>(row, q, p * 128u + sub * 16u, dot, dx); break;
        default: break;
        }
    } else if (sub * 16u < row_bytes) { // rows of 16, 32 or 64 bytes: the first lanes of a group hold one piece each
        refine_pieces_i8<1, R>(row, q, sub * 16u, dot, dx);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            dot[r] += __shfl_xor(dot[r], o, 64);
            dx[r] += __shfl_xor(dx[r], o, 64);
        }
        d[r] = angular_int_from_sums(dot[r], dx[r], dy);
    }
}

// key a before key b: distance bits, then id, then place in the list
__device__ __forceinline__ bool refine_before(uint32_t da, uint64_t ia, uint32_t pa, uint32_t db, uint64_t ib, uint32_t pb) {
    return da < db || (da == db && (ia < ib || (ia == ib && pa < pb)));
}

// Phase 1 of the re-rank kernels (refine_kernel below, refine_se_kernel.h): the query's qbytes bytes staged in LDS, zero
// padded to lds_bytes
__device__ __forceinline__ void refine_stage_query(const uint8_t* gq, uint32_t qbytes, uint8_t* lq, uint32_t lds_bytes, uint32_t tid) {
    if ((qbytes & 3u) == 0 && (reinterpret_cast<uintptr_t>(gq) & 3u) == 0) {
        for (uint32_t w = tid; w < (lds_bytes >> 2); w += REFINE_THREADS)
            reinterpret_cast<uint32_t*>(lq)[w] = (w * 4u < qbytes) ? reinterpret_cast<const uint32_t*>(gq)[w] : 0u;
    } else {
        for (uint32_t b = tid; b < lds_bytes; b += REFINE_THREADS) lq[b] = b < qbytes ? gq[b] : (uint8_t)0;
    }
}

// Phase 3 of the re-rank kernels: the cnt keys (kd, ki) of LDS ranked by counting, the k best of query qi written, the
// rest of its k slots padded, its count and the dropped-candidates word. A dropped candidate's key (0xFFFFFFFF,
// UINT64_MAX) lies behind every kept one: distances are >= 0 and never NaN (angular.rs:70-72, angular_int.rs:55), so
// their bits order as unsigned numbers and stay below it.
__device__ __forceinline__ void refine_rank_write(const uint64_t* ki, const uint32_t* kd, uint32_t cnt, uint32_t n_dropped,
                                                  uint32_t k, uint32_t qi, uint32_t tid, uint64_t* out_ids, float* out_dists,
                                                  uint32_t* out_counts, uint32_t* status) {
    const uint32_t kept = cnt - n_dropped;
    uint32_t md[REFINE_KEYS_PER_THREAD], rank[REFINE_KEYS_PER_THREAD];
    uint64_t mi[REFINE_KEYS_PER_THREAD];
#pragma unroll
    for (uint32_t t = 0; t < REFINE_KEYS_PER_THREAD; ++t) {
        const uint32_t p = tid + t * REFINE_THREADS;
        md[t] = p < cnt ? kd[p] : 0xFFFFFFFFu;
        mi[t] = p < cnt ? ki[p] : ~0ull;
        rank[t] = 0;
    }
    if (cnt <= REFINE_THREADS) { // one key per thread: the common shape (m = max_search of a walk)
        for (uint32_t p = 0; p < cnt; ++p) rank[0] += refine_before(kd[p], ki[p], p, md[0], mi[0], tid) ? 1u : 0u;
    } else {
        for (uint32_t p = 0; p < cnt; ++p) {
            const uint32_t dp = kd[p];
            const uint64_t ip = ki[p];
#pragma unroll
            for (uint32_t t = 0; t < REFINE_KEYS_PER_THREAD; ++t)
                rank[t] += refine_before(dp, ip, p, md[t], mi[t], tid + t * REFINE_THREADS) ? 1u : 0u;
        }
    }
    const uint32_t out_n = kept < k ? kept : k;
#pragma unroll
    for (uint32_t t = 0; t < REFINE_KEYS_PER_THREAD; ++t) {
        if (tid + t * REFINE_THREADS < cnt && rank[t] < out_n) { // (ranks below `kept` belong to kept candidates)
            out_ids[(size_t)qi * k + rank[t]] = mi[t];
            out_dists[(size_t)qi * k + rank[t]] = __uint_as_float(md[t]);
        }
    }
    for (uint32_t e = out_n + tid; e < k; e += REFINE_THREADS) {
        out_ids[(size_t)qi * k + e] = ~0ull;
        out_dists[(size_t)qi * k + e] = __builtin_inff();
    }
    if (tid == 0) {
        out_counts[qi] = out_n;
        if (n_dropped && status) atomicAdd(status, n_dropped);
    }
}

template <int DT>
__global__ __launch_bounds__(REFINE_THREADS) void refine_kernel(const RefineParams P) {
    extern __shared__ __align__(16) uint8_t smem_r[];
    uint64_t* ki = reinterpret_cast<uint64_t*>(smem_r);          // [m] candidate ids; UINT64_MAX = dropped
    uint32_t* kd = reinterpret_cast<uint32_t*>(smem_r + (size_t)P.m * 8u); // [m] distance bits
    uint8_t* lq = smem_r + refine_lds_q_off(P.m);
    __shared__ uint32_t n_dropped;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, sub = tid & 7u, group = tid >> 3;
    const uint32_t qi = blockIdx.x;
    const uint32_t m = P.m, k = P.k;
    // the list's first 64 entries are requested before anything waits for memory: slots below m exist whatever the
    // count says, so these loads, the count's and the query's are in flight together
    uint64_t first[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t jj = group + (uint32_t)r * REFINE_GROUPS;
        first[r] = jj < m ? P.cand[(size_t)qi * m + jj] : ~0ull;
    }
    uint32_t cnt = m; // entries of this query's list
    if (P.counts) {
        cnt = P.counts[qi];
        cnt = cnt < m ? cnt : m;
    }

    // 1. the query, once
    refine_stage_query(P.queries + (size_t)qi * (P.dim * (DT == 1 ? 1u : 4u)), P.dim * (DT == 1 ? 1u : 4u), lq, P.q_lds_bytes, tid); // (rows of halves take f32 queries)
    if (tid == 0) n_dropped = 0;
    __syncthreads();

    // 2. the candidates' distances
    int dy = 0;
    if constexpr (DT == 1) {
        for (uint32_t b = sub * 16u; b < P.row_bytes; b += 128u) {
            const uint4 qw = *reinterpret_cast<const uint4*>(lq + b);
            dy = dot4_i8(qw.x, qw.x, dy); dy = dot4_i8(qw.y, qw.y, dy);
            dy = dot4_i8(qw.z, qw.z, dy); dy = dot4_i8(qw.w, qw.w, dy);
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) dy += __shfl_xor(dy, o, 64);
    }
    uint32_t dropped = 0;
    if (P.n_elements == 0) { // no row to read: every entry is dropped
        for (uint32_t p = tid; p < cnt; p += REFINE_THREADS) {
            ki[p] = ~0ull;
            kd[p] = 0xFFFFFFFFu;
            dropped += 1u;
        }
    }
    for (uint32_t base = 0; base < (P.n_elements ? cnt : 0u); base += 2u * REFINE_GROUPS) { // (workgroup-uniform trip count)
        uint32_t j[2] = {base + group, base + REFINE_GROUPS + group};
        uint64_t id[2];
        bool valid[2];
        const uint8_t* row[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint64_t entry = base == 0 ? first[r] : (j[r] < m ? P.cand[(size_t)qi * m + j[r]] : ~0ull);
            id[r] = j[r] < cnt ? entry : ~0ull;
            valid[r] = id[r] < P.n_elements;
            row[r] = P.elements + (valid[r] ? id[r] : 0ull) * P.row_stride; // (a dropped candidate reads row 0, and its result is not used)
        }
        float d[2];
        if (base + REFINE_GROUPS < cnt) { // (uniform) the round has candidates for the groups' second rows
            if constexpr (DT == 0) refine_dist_f32<2>(row, reinterpret_cast<const float*>(lq), P.dim, P.row_bytes, lane, d);
            else if constexpr (DT == DT_F16) f16_dist_group<2>(row, reinterpret_cast<const float*>(lq), P.dim, P.row_bytes, lane, d);
            else refine_dist_i8<2>(row, lq, P.row_bytes, lane, dy, d);
        } else {
            const uint8_t* one[1] = {row[0]};
            float d1[1];
            if constexpr (DT == 0) refine_dist_f32<1>(one, reinterpret_cast<const float*>(lq), P.dim, P.row_bytes, lane, d1);
            else if constexpr (DT == DT_F16) f16_dist_group<1>(one, reinterpret_cast<const float*>(lq), P.dim, P.row_bytes, lane, d1);
            else refine_dist_i8<1>(one, lq, P.row_bytes, lane, dy, d1);
            d[0] = d1[0];
            d[1] = 0.0f;
        }
        if (sub == 0) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (j[r] < cnt) {
                    ki[j[r]] = valid[r] ? id[r] : ~0ull;
                    kd[j[r]] = valid[r] ? __float_as_uint(d[r]) : 0xFFFFFFFFu;
                    dropped += valid[r] ? 0u : 1u;
                }
            }
        }
    }
    if (dropped) atomicAdd(&n_dropped, dropped);
    __syncthreads();

    // 3. rank
    refine_rank_write(ki, kd, cnt, n_dropped, k, qi, tid, P.out_ids, P.out_dists, P.out_counts, P.status);
}

} // namespace granne_hip
