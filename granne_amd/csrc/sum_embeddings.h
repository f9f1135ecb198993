// sum_embeddings.h -- embeddings::SumEmbeddings (/root/reference/src/elements/embeddings/mod.rs:41-216) as gfx950
// device code: an element is a list of term ids, its vector the sum of those terms' rows of an embedding table.
//
//   raw embedding   mod.rs:124-143: no terms -> dim zeros; else a copy of the first term's row, then `x[i] += y[i]`
//                   (math.rs:100-106) per further term in list order: every component is a chain of f32 adds in
//                   term order, so the components may be spread over lanes but the terms may not be reassociated
//   get             mod.rs:164-166 -> angular::Vector::from: norm = sqrt(dot_product_f32(x, x)), x[i] /= norm when
//                   norm > 0 (angular.rs:55-61, math.rs:132-140): the ordered dot of dist.h, IEEE sqrt and divide
//   dist_to_element mod.rs:172-174: get(idx).dist(q)
//
// Two users: sum_embeddings_rows_kernel writes such vectors as dense rows (materialised indexes, builders, query
// batches); se_sum_row / se_finish_dist are the walkers' provider for a compact index, which keeps no dense rows
// (search_kernel.h Walker::distances, slow_kernel.h slow_dist).
#pragma once

#include "dist.h"
#include "wave_prims.h"

namespace granne_hip {

// the container on the device: table [V][tstride] f32 (rows 16-byte aligned, not normalised), CSR of term ids
struct SeView {
    const float* table;
    const uint64_t* offsets; // [n + 1], counted in ids
    const uint32_t* terms;   // [offsets[n]]
    uint32_t tstride;        // floats from one table row to the next
    uint32_t n_embeddings;   // V: a term id beyond it contributes nothing (the host checks what it uploads)
};

// The wave sums terms[0..cnt) into slot[0..dim): lanes over components, terms in list order. Four rows are in
// flight per step: the loads of a step are issued before its adds.
__device__ __forceinline__ void se_sum_row(const float* __restrict__ table, uint32_t tstride, uint32_t n_embeddings,
                                           const uint32_t* __restrict__ terms, uint32_t cnt, uint32_t dim,
                                           float* __restrict__ slot, uint32_t lane) {
    for (uint32_t c = lane; c < dim; c += 64u) {
        float acc = 0.0f;
        uint32_t t = 0;
        if (cnt) { // the first term is copied, not added to zero (-0.0 stays -0.0)
            const uint32_t t0 = terms[0];
            acc = t0 < n_embeddings ? table[(size_t)t0 * tstride + c] : 0.0f;
            t = 1;
        }
        for (; t + 4u <= cnt; t += 4u) {
            const uint32_t i0 = terms[t], i1 = terms[t + 1], i2 = terms[t + 2], i3 = terms[t + 3];
            const float v0 = i0 < n_embeddings ? table[(size_t)i0 * tstride + c] : 0.0f;
            const float v1 = i1 < n_embeddings ? table[(size_t)i1 * tstride + c] : 0.0f;
            const float v2 = i2 < n_embeddings ? table[(size_t)i2 * tstride + c] : 0.0f;
            const float v3 = i3 < n_embeddings ? table[(size_t)i3 * tstride + c] : 0.0f;
            acc = acc + v0;
            acc = acc + v1;
            acc = acc + v2;
            acc = acc + v3;
        }
        for (; t < cnt; ++t) {
            const uint32_t i0 = terms[t];
            acc = acc + (i0 < n_embeddings ? table[(size_t)i0 * tstride + c] : 0.0f);
        }
        slot[c] = acc;
    }
}

// One lane: normalise x[0..dim) in place the way angular::Vector::from does.
__device__ __forceinline__ void se_normalize(float* x, uint32_t dim) {
    const float norm = __builtin_sqrtf(dot_f32_exact_rt(x, x, dim)); // math.rs:132
    if (norm > 0.0f)
        for (uint32_t c = 0; c < dim; ++c) x[c] = x[c] / norm; // math.rs:134-138
}

// One lane: the raw sum in x -> get(idx).dist(q). x is overwritten with the normalised vector.
__device__ __forceinline__ float se_finish_dist(float* x, const float* q, uint32_t dim) {
    se_normalize(x, dim);
    return angular_from_dot(dot_f32_exact_rt(x, q, dim));
}

// One lane, everything in global memory (the exact walker): x = dim floats of scratch of this lane's own.
__device__ inline float se_dist_scalar(const SeView& se, uint32_t id, const float* q, uint32_t dim, float* x) {
    const uint64_t o0 = se.offsets[id], o1 = se.offsets[(size_t)id + 1];
    const uint32_t* terms = se.terms + o0;
    const uint32_t cnt = (uint32_t)(o1 - o0);
    for (uint32_t c = 0; c < dim; ++c) {
        float acc = 0.0f;
        for (uint32_t t = 0; t < cnt; ++t) {
            const uint32_t i = terms[t];
            const float v = i < se.n_embeddings ? se.table[(size_t)i * se.tstride + c] : 0.0f;
            acc = t == 0 ? v : acc + v;
        }
        x[c] = acc;
    }
    return se_finish_dist(x, q, dim);
}

// Elements first .. first + count - 1 of a CSR of term lists -> dense f32 rows of out_stride floats, raw or
// normalised. One wave per block; a pass stages `rows_per_pass` (<= 64) rows in LDS (row stride lstride floats, odd):
// the lanes read the pass's offsets together, the wave sums one row after the other (lanes over components), one
// lane per row normalises, the rows go out coalesced.
__global__ __launch_bounds__(64) void sum_embeddings_rows_kernel(const SeView se, uint64_t first, uint64_t count,
                                                                 uint32_t dim, int normalised, float* __restrict__ out,
                                                                 uint64_t out_stride, uint32_t rows_per_pass,
                                                                 uint32_t lstride) {
    extern __shared__ __align__(16) uint8_t se_smem[];
    float* lds = reinterpret_cast<float*>(se_smem);
    const uint32_t lane = threadIdx.x;
    for (uint64_t r0 = (uint64_t)blockIdx.x * rows_per_pass; r0 < count; r0 += (uint64_t)gridDim.x * rows_per_pass) {
        const uint32_t nr = (uint32_t)min((uint64_t)rows_per_pass, count - r0);
        uint64_t o0 = 0, o1 = 0;
        if (lane < nr) {
            o0 = se.offsets[first + r0 + lane];
            o1 = se.offsets[first + r0 + lane + 1];
        }
        for (uint32_t r = 0; r < nr; ++r) {
            const uint64_t b = readlane64(o0, r), e = readlane64(o1, r);
            const uint32_t cnt = e > b ? (uint32_t)min(e - b, (uint64_t)0xFFFFFFFFu) : 0u;
            se_sum_row(se.table, se.tstride, se.n_embeddings, se.terms + b, cnt, dim, lds + (size_t)r * lstride, lane);
        }
        __syncthreads();
        if (normalised && lane < nr) se_normalize(lds + (size_t)lane * lstride, dim);
        __syncthreads();
        const uint32_t total = nr * dim;
        for (uint32_t t = lane; t < total; t += 64u) {
            const uint32_t r = t / dim, c = t - r * dim;
            out[(r0 + r) * out_stride + c] = lds[(size_t)r * lstride + c];
        }
        __syncthreads();
    }
}

} // namespace granne_hip
