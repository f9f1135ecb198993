// f16.h -- angular_f16 elements: a row is dim IEEE binary16 values, and the element it stands for is
// angular::Vector::from(widen(row)) -- the halves widened exactly to f32, then normalised the way src/math.rs:123-150
// does it (norm = sqrt(dot_product_f32(x, x)), x[c] /= norm when norm > 0), as embeddings::SumEmbeddings::get does with
// its sums (sum_embeddings.h). dist_to_element(i, q) = get(i).dist(q) with q an ordinary prepared f32 query.
//
//   f16_dist_lane     one lane, the widened row in memory of its own: the walkers' provider (search_kernel.h
//                     Walker::distances, slow_kernel.h slow_dist) -- se_finish_dist of sum_embeddings.h
//   f16_dist_group    eight lanes to a row, rows read straight from HBM: dists_kernel (util_kernels.h) and refine_kernel
//                     (refine_kernel.h). Lane `sub` owns accumulators 4 sub .. 4 sub + 3 of the reference's 32, which are
//                     8 bytes of every 64-byte block of halves; the norm's sum and the dot's run down the eight lanes in
//                     the reference's order and the tails are folded by sequential fmas, so the result has the bits of
//                     f16_dist_lane: a walk handed from one walker to the other, dists and refine agree bit for bit.
// The conversion kernels at the end are granne_hip_f32_to_f16_device / granne_hip_f16_to_f32_device.
// Compiled with -ffp-contract=off and correctly rounded divide and sqrt.
#pragma once

#include "dist.h"
#include "ordered_sum.h"
#include "sum_embeddings.h"

namespace granne_hip {

constexpr int DT_F16 = 2;

// binary16 <-> binary32: widening is exact (subnormals included), narrowing rounds to nearest, ties to even
__device__ __forceinline__ float f16_widen(uint32_t bits) {
    union { uint16_t u; _Float16 h; } c;
    c.u = (uint16_t)bits;
    return (float)c.h;
}
__device__ __forceinline__ uint16_t f16_narrow(float v) {
    union { uint16_t u; _Float16 h; } c;
    c.h = (_Float16)v;
    return c.u;
}
// the four halves of 8 bytes
__device__ __forceinline__ void f16_widen4(uint2 v, float (&x)[4]) {
    x[0] = f16_widen(v.x & 0xFFFFu);
    x[1] = f16_widen(v.x >> 16);
    x[2] = f16_widen(v.y & 0xFFFFu);
    x[3] = f16_widen(v.y >> 16);
}

// bytes of a device row of halves (zero padded to 16)
__host__ __device__ inline uint32_t f16_row_bytes(uint32_t dim) { return (dim * 2u + 15u) & ~15u; }

// One lane: row[0..dim) halves -> x[0..dim) floats, then get(idx).dist(q). x is left holding the normalised vector.
__device__ __forceinline__ float f16_dist_lane(const uint16_t* __restrict__ row, float* x, const float* q, uint32_t dim) {
    for (uint32_t c = 0; c < dim; ++c) x[c] = f16_widen(row[c]);
    return se_finish_dist(x, q, dim);
}

// the ordered sum acc[0] .. acc[31] of a group of eight lanes (ordered_sum.h); every lane of the group returns it
__device__ __forceinline__ float f16_group_sum(const float (&a)[4], uint32_t lane) {
    return ordered_sum8(a[0], a[1], a[2], a[3], lane);
}

// NB blocks (c0 .. c0 + NB - 1) of R rows of halves: all loads first
template <int NB, int R>
__device__ __forceinline__ void f16_load_blocks(const uint8_t* (&row)[R], uint32_t c0, uint32_t sub, uint2 (&v)[R][NB]) {
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < NB; ++i) v[r][i] = *reinterpret_cast<const uint2*>(row[r] + (size_t)(c0 + i) * 64u + sub * 8u);
}
// ... into the norm's accumulators: a += x * x
template <int NB, int R>
__device__ __forceinline__ void f16_norm_blocks(const uint8_t* (&row)[R], uint32_t c0, uint32_t sub, float (&a)[R][4]) {
    uint2 v[R][NB];
    f16_load_blocks<NB, R>(row, c0, sub, v);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float x[4];
            f16_widen4(v[r][i], x);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[r][j] = __builtin_fmaf(x[j], x[j], a[r][j]);
        }
}
// ... into the dot's accumulators: a += (x / norm) * q, the divide skipped for a zero row (math.rs:133)
template <int NB, int R>
__device__ __forceinline__ void f16_dot_blocks(const uint8_t* (&row)[R], const float* q, uint32_t c0, uint32_t sub,
                                               const float (&norm)[R], float (&a)[R][4]) {
    uint2 v[R][NB];
    f16_load_blocks<NB, R>(row, c0, sub, v);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const float* qc = q + (c0 + i) * 32u + sub * 4u;
        const float qv[4] = {qc[0], qc[1], qc[2], qc[3]};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float x[4];
            f16_widen4(v[r][i], x);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float xn = norm[r] > 0.0f ? x[j] / norm[r] : x[j];
                a[r][j] = __builtin_fmaf(xn, qv[j], a[r][j]);
            }
        }
    }
}

// get(idx).dist(q) of R rows, eight lanes to a row (lane & 7 = the lane's place in its group; the groups of a wave may
// hold different rows). row_bytes = f16_row_bytes(dim): the loads stay inside it. q: dim floats, 4-byte aligned (LDS or
// global). The result is valid in every lane of a row's group.
template <int R>
__device__ __forceinline__ void f16_dist_group(const uint8_t* (&row)[R], const float* q, uint32_t dim, uint32_t row_bytes,
                                               uint32_t lane, float (&d)[R]) {
    const uint32_t sub = lane & 7u, nfull = dim >> 5, tail = dim & 31u;
    float xt[R][4]; // the lane's four components of the (zero padded) tail block
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint2 vt = make_uint2(0, 0);
        if (nfull * 64u + sub * 8u + 8u <= row_bytes) vt = *reinterpret_cast<const uint2*>(row[r] + (size_t)nfull * 64u + sub * 8u);
        f16_widen4(vt, xt[r]);
    }
    float a[R][4], norm[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r][0] = a[r][1] = a[r][2] = a[r][3] = 0.0f;
    // Rows of up to four full blocks (dims below 160: a 100-d row is three and a tail) are read ONCE: every load of the
    // round is issued before the arithmetic and the widened row stays in registers for the norm and for the dot. Longer
    // rows are read twice, four blocks a round; the second read finds the lines of the first in the cache.
    const bool held = nfull <= 4u; // (uniform: one dim)
    float x[R][4][4];
    if (held) {
        uint2 v[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[r][i] = make_uint2(0, 0);
                if ((uint32_t)i < nfull) v[r][i] = *reinterpret_cast<const uint2*>(row[r] + (size_t)i * 64u + sub * 8u);
            }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) f16_widen4(v[r][i], x[r][i]);
    }
    // 1. norm = sqrt(dot_product_f32(x, x)), math.rs:132
    if (held) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((uint32_t)i < nfull) {
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) a[r][j] = __builtin_fmaf(x[r][i][j], x[r][i][j], a[r][j]);
            }
    } else {
        uint32_t c = 0;
        for (; c + 4u <= nfull; c += 4u) f16_norm_blocks<4, R>(row, c, sub, a);
        switch (nfull - c) {
        case 3: f16_norm_blocks<3, R>(row, c, sub, a); break;
        case 2: f16_norm_blocks<2, R>(row, c, sub, a); break;
        case 1: f16_norm_blocks<1, R>(row, c, sub, a); break;
        default: break;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = f16_group_sum(a[r], lane);
        for (uint32_t t = 0; t < tail; ++t) { // math.rs:47-49
            const float mine = (t & 3u) == 0 ? xt[r][0] : (t & 3u) == 1 ? xt[r][1] : (t & 3u) == 2 ? xt[r][2] : xt[r][3];
            const float xv = __shfl(mine, (int)((lane & ~7u) + (t >> 2)), 64);
            s = __builtin_fmaf(xv, xv, s);
        }
        norm[r] = __builtin_sqrtf(s);
        // 2. x[c] /= norm, math.rs:134-138: the tail's here, the blocks' where they meet the query
        if (norm[r] > 0.0f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) xt[r][j] = xt[r][j] / norm[r];
        }
        a[r][0] = a[r][1] = a[r][2] = a[r][3] = 0.0f;
    }
    // 3. the dot with the query
    if (held) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if ((uint32_t)i < nfull) {
                const float* qc = q + (uint32_t)i * 32u + sub * 4u;
                const float qv[4] = {qc[0], qc[1], qc[2], qc[3]};
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xn = norm[r] > 0.0f ? x[r][i][j] / norm[r] : x[r][i][j];
                        a[r][j] = __builtin_fmaf(xn, qv[j], a[r][j]);
                    }
            }
    } else {
        uint32_t c = 0;
        for (; c + 4u <= nfull; c += 4u) f16_dot_blocks<4, R>(row, q, c, sub, norm, a);
        switch (nfull - c) {
        case 3: f16_dot_blocks<3, R>(row, q, c, sub, norm, a); break;
        case 2: f16_dot_blocks<2, R>(row, q, c, sub, norm, a); break;
        case 1: f16_dot_blocks<1, R>(row, q, c, sub, norm, a); break;
        default: break;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float s = f16_group_sum(a[r], lane);
        for (uint32_t t = 0; t < tail; ++t) {
            const float mine = (t & 3u) == 0 ? xt[r][0] : (t & 3u) == 1 ? xt[r][1] : (t & 3u) == 2 ? xt[r][2] : xt[r][3];
            const float xv = __shfl(mine, (int)((lane & ~7u) + (t >> 2)), 64);
            s = __builtin_fmaf(xv, q[nfull * 32u + t], s);
        }
        d[r] = angular_from_dot(s);
    }
}

// f32 rows -> halves, round to nearest even: one component per thread
__global__ void f32_to_f16_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, uint64_t total) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x)
        out[t] = f16_narrow(in[t]);
}

// Rows of halves (in_stride BYTES from one to the next) -> dense f32 rows [n][dim], widened and, when asked, normalised as
// angular::Vector::from does. The shape of normalize_rows_kernel (util_kernels.h): a block stages rows_per_block rows in
// LDS, one lane per row normalises, the rows go out coalesced.
__global__ void f16_to_f32_kernel(const uint8_t* __restrict__ in, uint64_t in_stride, float* __restrict__ out, uint64_t n,
                                  uint32_t dim, int normalised, uint32_t rows_per_block, uint32_t lstride) {
    extern __shared__ __align__(16) uint8_t smem_h[];
    float* lds = reinterpret_cast<float*>(smem_h);
    for (uint64_t r0 = (uint64_t)blockIdx.x * rows_per_block; r0 < n; r0 += (uint64_t)gridDim.x * rows_per_block) {
        const uint32_t nr = (uint32_t)min((uint64_t)rows_per_block, n - r0);
        const uint32_t total = nr * dim;
        for (uint32_t t = threadIdx.x; t < total; t += blockDim.x) {
            const uint32_t r = t / dim, c = t - r * dim;
            lds[r * lstride + c] = f16_widen(reinterpret_cast<const uint16_t*>(in + (r0 + r) * in_stride)[c]);
        }
        __syncthreads();
        if (normalised && threadIdx.x < nr) se_normalize(lds + threadIdx.x * lstride, dim);
        __syncthreads();
        for (uint32_t t = threadIdx.x; t < total; t += blockDim.x) {
            const uint32_t r = t / dim, c = t - r * dim;
            out[r0 * dim + t] = lds[r * lstride + c];
        }
        __syncthreads();
    }
}

} // namespace granne_hip
