// refine_se_kernel.h -- re-rank a query's candidate ids by a SumEmbeddings CONTAINER: refine_kernel (refine_kernel.h) with the
// candidate's f32 vector made where it is needed, from the container's table and term lists, instead of read from a dense
// row. d = get(id).dist(q) of embeddings::SumEmbeddings (sum_embeddings.h): the sum of the terms' table rows in list order,
// normalised as angular::Vector::from does, met with the prepared f32 query -- bit for bit se_finish_dist's distance and
// the distance refine_kernel<0> gives over the materialised row.
//
// One workgroup of four waves per query; phases 1 (the query staged in LDS) and 3 (the keys ranked in LDS by counting)
// are refine_kernel's own helpers. Phase 2, eight lanes to a candidate, one candidate per group and round (32 per
// workgroup):
//   a. offsets[id], offsets[id + 1] (u64) and the term ids; every lane of the group reads the same words;
//   b. the sum. Lane `sub` owns the 16-byte piece `sub` of every 128-byte block of a table row -- dists_kernel's layout,
//      accumulators 4 sub .. 4 sub + 3 of the reference's 32 -- so the components are spread over lanes and blocks while
//      every component stays ONE chain of f32 adds in term order (mod.rs:124-143): no terms gives zeros, the first term's
//      piece is copied (-0.0 stays -0.0), every further term's is added; a term id >= n_embeddings counts as a row of
//      zeros, as in se_sum_row. The pieces of TT terms are requested before the first of them is added. The groups of a
//      wave hold lists of different lengths: the term loop's trip count is a group's own, and nothing in it crosses lanes;
//   c. norm = sqrt(dot_product_f32(x, x)): x * x folded block by block into the lane's four accumulators, the ordered sum
//      down the eight lanes (ordered_sum.h), the tail's sequential fmas; x /= norm only when norm > 0 (math.rs:132-138);
//   d. the dot with the staged query in the same order, then angular_from_dot -- f16_dist_group (f16.h) with the sums in
//      place of the widened halves.
// RESIDENT DIMS. refine_se_kernel<NBF> keeps the whole sum in registers when the row has up to NBF full 32-float blocks
// (plus its tail piece): NBF = 1 (dim < 64), 3 (dim < 128: 100-d), 4 (dim < 160), 8 (dim < 288: 200-d, 256-d). The terms in
// flight shrink as the row grows (TT = 4, 4, 3, 1) so that every form stays within 128 VGPRs without scratch. Longer rows
// (NBF = 0) are summed TWICE, four blocks a round: once into the norm, once -- divided -- into the dot; the second pass
// finds the table lines of the first in the cache. Their tail piece is summed once and kept.
// BYTES. A candidate costs 16 bytes of offsets, 4 per term id and terms x (dim x 4 padded to 16) of table rows where
// refine_kernel reads one row of dim x 4: six times the bytes for a six-term element -- of a table that is small beside the
// element set (200k x 100-d: 80 MB, within the Infinity Cache), so most of them are presumably served by the caches, not
// HBM (inferred from the sizes; not measured).
// Compiled with -ffp-contract=off and correctly rounded divide and sqrt: every fused operation is an explicit fmaf.
#pragma once

#include "refine_kernel.h"
#include "sum_embeddings.h"

namespace granne_hip {

struct RefineSeParams {
    SeView se;
    uint64_t n_elements;
    uint32_t dim;
    const float* queries;   // [nq][dim] f32, prepared
    const uint64_t* cand;   // [nq][m]
    const uint32_t* counts; // [nq]: valid entries of a list (clamped to m), or null = all m
    uint32_t m, k;
    uint32_t q_lds_bytes;   // the staged query: dim x 4 padded to 16
    uint64_t* out_ids;      // [nq][k]
    float* out_dists;       // [nq][k]
    uint32_t* out_counts;   // [nq]
    uint32_t* status;       // optional u32: += candidates dropped (id >= n_elements, UINT64_MAX included)
};

// full blocks held in registers for a row of `dim` floats: the NBF of the kernel to launch (0 = the two-pass form)
__host__ __device__ inline int refine_se_resident_blocks(uint32_t dim) {
    const uint32_t nfull = dim >> 5;
    return nfull <= 1u ? 1 : nfull <= 3u ? 3 : nfull <= 4u ? 4 : nfull <= 8u ? 8 : 0;
}

// Slot i of the lane = the 16 bytes at byte boff[i] of a table row (ok[i]: the slot exists in this row for this lane; a
// slot that does not stays zero). x[i] = the sum of those pieces over terms[0 .. cnt) in list order. TT terms per step:
// their ids, then all their pieces, then the adds.
template <int NP, int TT>
__device__ __forceinline__ void se_sum_slots(const SeView& se, const uint32_t* __restrict__ terms, uint32_t cnt,
                                             const uint32_t (&boff)[NP], const bool (&ok)[NP], float (&x)[NP][4]) {
#pragma unroll
    for (int i = 0; i < NP; ++i) x[i][0] = x[i][1] = x[i][2] = x[i][3] = 0.0f;
    const uint8_t* table = reinterpret_cast<const uint8_t*>(se.table);
    const uint64_t pitch = (uint64_t)se.tstride * 4u;
    for (uint32_t t0 = 0; t0 < cnt; t0 += (uint32_t)TT) { // (a group's own trip count)
        uint32_t id[TT];
#pragma unroll
        for (int u = 0; u < TT; ++u) id[u] = t0 + (uint32_t)u < cnt ? terms[t0 + (uint32_t)u] : 0xFFFFFFFFu;
        float4 v[TT][NP];
#pragma unroll
        for (int u = 0; u < TT; ++u) {
            const bool in = id[u] < se.n_embeddings; // (n_embeddings <= 2^32 - 1: false past the list's end, where nothing is read)
            const uint8_t* rp = table + (uint64_t)(in ? id[u] : 0u) * pitch;
#pragma unroll
            for (int i = 0; i < NP; ++i) {
                v[u][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (in && ok[i]) v[u][i] = *reinterpret_cast<const float4*>(rp + boff[i]);
            }
        }
#pragma unroll
        for (int u = 0; u < TT; ++u) {
            if (t0 + (uint32_t)u < cnt) {
                const bool first = t0 + (uint32_t)u == 0u; // copied, not added to zero
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    x[i][0] = first ? v[u][i].x : x[i][0] + v[u][i].x;
                    x[i][1] = first ? v[u][i].y : x[i][1] + v[u][i].y;
                    x[i][2] = first ? v[u][i].z : x[i][2] + v[u][i].z;
                    x[i][3] = first ? v[u][i].w : x[i][3] + v[u][i].w;
                }
            }
        }
    }
}

// the tail's part of a dot, after the ordered sum (math.rs:47-49): component t of the tail block lives in lane t / 4 of
// the group, slot t % 4. y: the other operand's tail (null = the vector itself, for the norm)
__device__ __forceinline__ float refine_se_tail(float s, const float (&xt)[4], const float* y, uint32_t tail, uint32_t lane) {
    for (uint32_t t = 0; t < tail; ++t) { // (uniform)
        const float mine = (t & 3u) == 0 ? xt[0] : (t & 3u) == 1 ? xt[1] : (t & 3u) == 2 ? xt[2] : xt[3];
        const float xv = __shfl(mine, (int)((lane & ~7u) + (t >> 2)), 64);
        s = __builtin_fmaf(xv, y ? y[t] : xv, s);
    }
    return s;
}

// get(id).dist(q) of one candidate per group of eight lanes; terms[0 .. cnt) is the group's list (cnt = 0: the zero
// vector, distance 1). Every lane of the wave calls it; the result is valid in every lane of a group.
template <int NBF>
__device__ __forceinline__ float refine_se_dist(const SeView& se, const uint32_t* __restrict__ terms, uint32_t cnt, const float* q,
                                                uint32_t dim, uint32_t lane) {
    constexpr int TT = NBF <= 3 ? 4 : NBF <= 4 ? 3 : 1;
    const uint32_t sub = lane & 7u, nfull = dim >> 5, tail = dim & 31u;
    const uint32_t tail_off = nfull * 128u + sub * 16u;
    const bool tail_ok = tail_off + 16u <= se.tstride * 4u; // (rows are padded to 16 bytes with zeros)
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float xt[4];
    if constexpr (NBF > 0) {
        // the whole sum in registers: slots 0 .. NBF - 1 are the full blocks, slot NBF the tail piece
        uint32_t boff[NBF + 1];
        bool ok[NBF + 1];
#pragma unroll
        for (int i = 0; i < NBF; ++i) {
            boff[i] = (uint32_t)i * 128u + sub * 16u;
            ok[i] = (uint32_t)i < nfull;
        }
        boff[NBF] = tail_off;
        ok[NBF] = tail_ok;
        float x[NBF + 1][4];
        se_sum_slots<NBF + 1, TT>(se, terms, cnt, boff, ok, x);
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = x[NBF][j];
#pragma unroll
        for (int i = 0; i < NBF; ++i)
            if ((uint32_t)i < nfull) {
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] = __builtin_fmaf(x[i][j], x[i][j], a[j]);
            }
        const float norm = __builtin_sqrtf(refine_se_tail(ordered_sum8(a[0], a[1], a[2], a[3], lane), xt, nullptr, tail, lane));
        if (norm > 0.0f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[j] = xt[j] / norm;
        }
        a[0] = a[1] = a[2] = a[3] = 0.0f;
#pragma unroll
        for (int i = 0; i < NBF; ++i)
            if ((uint32_t)i < nfull) {
                const float4 qc = *reinterpret_cast<const float4*>(q + (uint32_t)i * 32u + sub * 4u);
                const float qv[4] = {qc.x, qc.y, qc.z, qc.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float xn = norm > 0.0f ? x[i][j] / norm : x[i][j];
                    a[j] = __builtin_fmaf(xn, qv[j], a[j]);
                }
            }
    } else {
        // two passes of four blocks a round; the tail piece once
        {
            const uint32_t boff[1] = {tail_off};
            const bool ok[1] = {tail_ok};
            float x1[1][4];
            se_sum_slots<1, 4>(se, terms, cnt, boff, ok, x1);
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[j] = x1[0][j];
        }
        for (uint32_t c = 0; c < nfull; c += 4u) { // (uniform)
            uint32_t boff[4];
            bool ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                boff[i] = (c + (uint32_t)i) * 128u + sub * 16u;
                ok[i] = c + (uint32_t)i < nfull;
            }
            float x[4][4];
            se_sum_slots<4, 3>(se, terms, cnt, boff, ok, x);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + (uint32_t)i < nfull) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[j] = __builtin_fmaf(x[i][j], x[i][j], a[j]);
                }
        }
        const float norm = __builtin_sqrtf(refine_se_tail(ordered_sum8(a[0], a[1], a[2], a[3], lane), xt, nullptr, tail, lane));
        if (norm > 0.0f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[j] = xt[j] / norm;
        }
        a[0] = a[1] = a[2] = a[3] = 0.0f;
        for (uint32_t c = 0; c < nfull; c += 4u) {
            uint32_t boff[4];
            bool ok[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                boff[i] = (c + (uint32_t)i) * 128u + sub * 16u;
                ok[i] = c + (uint32_t)i < nfull;
            }
            float x[4][4];
            se_sum_slots<4, 3>(se, terms, cnt, boff, ok, x);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (c + (uint32_t)i < nfull) {
                    const float4 qc = *reinterpret_cast<const float4*>(q + (c + (uint32_t)i) * 32u + sub * 4u);
                    const float qv[4] = {qc.x, qc.y, qc.z, qc.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xn = norm > 0.0f ? x[i][j] / norm : x[i][j];
                        a[j] = __builtin_fmaf(xn, qv[j], a[j]);
                    }
                }
        }
    }
    return angular_from_dot(refine_se_tail(ordered_sum8(a[0], a[1], a[2], a[3], lane), xt, q + nfull * 32u, tail, lane));
}

template <int NBF>
__global__ __launch_bounds__(REFINE_THREADS) void refine_se_kernel(const RefineSeParams P) {
    extern __shared__ __align__(16) uint8_t smem_rs[];
    uint64_t* ki = reinterpret_cast<uint64_t*>(smem_rs);                     // [m] candidate ids; UINT64_MAX = dropped
    uint32_t* kd = reinterpret_cast<uint32_t*>(smem_rs + (size_t)P.m * 8u); // [m] distance bits
    uint8_t* lq = smem_rs + refine_lds_q_off(P.m);
    __shared__ uint32_t n_dropped;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, sub = tid & 7u, group = tid >> 3;
    const uint32_t qi = blockIdx.x;
    const uint32_t m = P.m, k = P.k;
    // the group's first entry is requested before anything waits for memory (slots below m exist whatever the count says)
    const uint64_t first = group < m ? P.cand[(size_t)qi * m + group] : ~0ull;
    uint32_t cnt = m; // entries of this query's list
    if (P.counts) {
        cnt = P.counts[qi];
        cnt = cnt < m ? cnt : m;
    }

    // 1. the query, once
    refine_stage_query(reinterpret_cast<const uint8_t*>(P.queries) + (size_t)qi * P.dim * 4u, P.dim * 4u, lq, P.q_lds_bytes, tid);
    if (tid == 0) n_dropped = 0;
    __syncthreads();

    // 2. the candidates' distances: one per group and round
    uint32_t dropped = 0;
    for (uint32_t base = 0; base < cnt; base += REFINE_GROUPS) { // (workgroup-uniform trip count)
        const uint32_t j = base + group;
        const uint64_t entry = base == 0 ? first : (j < m ? P.cand[(size_t)qi * m + j] : ~0ull);
        const uint64_t id = j < cnt ? entry : ~0ull;
        const bool valid = id < P.n_elements;
        uint64_t o0 = 0, o1 = 0;
        if (valid) { // (a dropped candidate reads nothing: an empty list, and its result is not used)
            o0 = P.se.offsets[id];
            o1 = P.se.offsets[id + 1];
        }
        const uint32_t nt = o1 > o0 ? (uint32_t)min(o1 - o0, (uint64_t)0xFFFFFFFFu) : 0u;
        const float d = refine_se_dist<NBF>(P.se, P.se.terms + o0, nt, reinterpret_cast<const float*>(lq), P.dim, lane);
        if (sub == 0 && j < cnt) {
            ki[j] = valid ? id : ~0ull;
            kd[j] = valid ? __float_as_uint(d) : 0xFFFFFFFFu;
            dropped += valid ? 0u : 1u;
        }
    }
    if (dropped) atomicAdd(&n_dropped, dropped);
    __syncthreads();

    // 3. rank
    refine_rank_write(ki, kd, cnt, n_dropped, k, qi, tid, P.out_ids, P.out_dists, P.out_counts, P.status);
}

} // namespace granne_hip
