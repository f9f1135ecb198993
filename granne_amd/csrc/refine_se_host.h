// refine_se_host.h -- host side of refined search over a SumEmbeddings CONTAINER (included by granne_hip.hip after
// sum_embeddings_host.h and refine_host.h): granne_hip_refine_sum_embeddings_device re-ranks candidate lists by the
// vectors the container stands for (refine_se_kernel.h), granne_hip_search_refined_sum_embeddings_batch* put a walk of
// any index in front of it, and granne_hip_sum_embeddings_rows* write the container's elements as prepared rows of a
// dense element type, chunk by chunk, so that the index to walk can be made without a dense f32 copy of the whole set.
#pragma once

#include "refine_se_kernel.h"

// what every entry checks before any device call, the plain numbers first (refine_check with the container as the rows side)
static int refine_se_check(const granne_hip_sum_embeddings* se, uint32_t m, uint32_t k, const char* what, bool fused = false,
                           const granne_hip_index* wx = nullptr, uint32_t max_search = 0) {
    if (m == 0 || m > REFINE_MAX_M) return fail(GRANNE_HIP_ERR_INVALID, "%s: candidates per query must be in [1, %u]", what, REFINE_MAX_M);
    if (k == 0) return fail(GRANNE_HIP_ERR_INVALID, "%s: k must be > 0", what);
    if (fused && m > max_search)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: refine_from (%u) must not exceed max_search (%u)", what, m, max_search);
    if (fused && !wx) return fail(GRANNE_HIP_ERR_INVALID, "%s: the walk index is null", what);
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "%s: the SumEmbeddings container is null", what);
    if (fused && wx->device != se->device)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: the walk index and the container live on devices %d and %d", what, wx->device, se->device);
    const uint64_t lds = (uint64_t)refine_lds_q_off(m) + (((uint64_t)se->dim * 4u + 15u) & ~15ull);
    if (lds > 160u * 1024u - 64u) return fail(GRANNE_HIP_ERR_INVALID, "refine: dimension too large for the LDS stage");
    return GRANNE_HIP_OK;
}

// the kernel over checked arguments (nq > 0, buffers not null) and a device copy the caller holds for the call
static int refine_se_launch(const SeDev& d, const float* d_queries, uint32_t nq, const uint64_t* d_cand_ids,
                            const uint32_t* d_cand_counts, uint32_t m, uint32_t k, uint64_t* d_out_ids, float* d_out_dists,
                            uint32_t* d_out_counts, uint32_t* d_refine_status, hipStream_t s) {
    RefineSeParams P;
    P.se = SeView{d.d_table.as<float>(), d.d_offsets.as<uint64_t>(), d.d_terms.as<uint32_t>(), d.tstride, (uint32_t)d.n_embeddings};
    P.n_elements = d.n;
    P.dim = d.dim;
    P.queries = d_queries;
    P.cand = d_cand_ids;
    P.counts = d_cand_counts;
    P.m = m;
    P.k = k;
    P.q_lds_bytes = (d.dim * 4u + 15u) & ~15u;
    P.out_ids = d_out_ids;
    P.out_dists = d_out_dists;
    P.out_counts = d_out_counts;
    P.status = d_refine_status;
    const uint32_t lds = refine_lds_q_off(m) + P.q_lds_bytes; // (refine_se_check bounded it)
    void (*fn)(const RefineSeParams) = nullptr;
    switch (refine_se_resident_blocks(d.dim)) {
    case 1: fn = refine_se_kernel<1>; break;
    case 3: fn = refine_se_kernel<3>; break;
    case 4: fn = refine_se_kernel<4>; break;
    case 8: fn = refine_se_kernel<8>; break;
    default: fn = refine_se_kernel<0>; break;
    }
    if (lds > 32u * 1024u) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3(nq), dim3(REFINE_THREADS), lds, s, P);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// Every entry takes the container's device copy under its mutex and holds it for the call, as
// granne_hip_sum_embeddings_materialize_device does: an append between two calls is seen by the second, and a copy that an
// append drops while a kernel still reads it is freed by hipFree, which waits for the device.
extern "C" int granne_hip_refine_sum_embeddings_device(const granne_hip_sum_embeddings* se, const float* d_queries, uint32_t nq,
                                                       const uint64_t* d_cand_ids, const uint32_t* d_cand_counts, uint32_t m,
                                                       uint32_t k, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                                       uint32_t* d_refine_status, void* stream) {
    int rc = refine_se_check(se, m, k, "refine_sum_embeddings");
    if (rc) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_queries || !d_cand_ids || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(GRANNE_HIP_ERR_INVALID, "refine_sum_embeddings: null buffer");
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    GRANNE_HIP_ON_DEVICE(d->device);
    return refine_se_launch(*d, d_queries, nq, d_cand_ids, d_cand_counts, m, k, d_out_ids, d_out_dists, d_out_counts, d_refine_status,
                            (hipStream_t)stream);
}

extern "C" int granne_hip_search_refined_sum_embeddings_batch_device(const granne_hip_index* wx, const granne_hip_sum_embeddings* se,
                                                                     const void* d_walk_queries, const void* d_refine_queries,
                                                                     uint32_t nq, uint32_t max_search, uint32_t refine_from, uint32_t k,
                                                                     uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                                                     uint64_t* d_out_stats, uint32_t* d_status,
                                                                     uint32_t* d_refine_status, void* stream) {
    int rc = refine_se_check(se, refine_from, k, "search_refined_sum_embeddings", true, wx, max_search);
    if (rc) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_walk_queries || !d_refine_queries || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(GRANNE_HIP_ERR_INVALID, "search_refined_sum_embeddings: null buffer");
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    GRANNE_HIP_ON_DEVICE(wx->device);
    hipStream_t s = (hipStream_t)stream;
    // the walk's lists: [nq][m] u64 ids, [nq][m] f32 distances (the walk's own, not used), [nq] u32 counts
    const uint32_t m = refine_from;
    const size_t o_d = (size_t)nq * m * 8, o_c = o_d + (size_t)nq * m * 4, total = o_c + (size_t)nq * 4;
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, total, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() { (void)hipFreeAsync(p, s); }
    } release{scratch, s};
    rc = search_launch(SearchTarget(wx, wx->d_layers.as<LayerDev>(), (uint32_t)wx->layers.size()),
                       index_call(d_walk_queries, nq, max_search, m, (uint64_t*)scratch, (float*)(scratch + o_d), (uint32_t*)(scratch + o_c),
                                  d_out_stats, d_status, stream));
    if (rc == 0)
        rc = refine_se_launch(*d, (const float*)d_refine_queries, nq, (const uint64_t*)scratch, (const uint32_t*)(scratch + o_c), m, k,
                              d_out_ids, d_out_dists, d_out_counts, d_refine_status, s);
    return rc;
}

// the same with host buffers in and out (synchronous)
extern "C" int granne_hip_search_refined_sum_embeddings_batch(const granne_hip_index* wx, const granne_hip_sum_embeddings* se,
                                                              const void* walk_queries, const void* refine_queries, uint32_t nq,
                                                              uint32_t max_search, uint32_t refine_from, uint32_t k, uint64_t* out_ids,
                                                              float* out_dists, uint32_t* out_counts, uint64_t* out_stats,
                                                              uint32_t* out_refine_status) {
    int rc = refine_se_check(se, refine_from, k, "search_refined_sum_embeddings", true, wx, max_search);
    if (rc) return rc;
    if (out_refine_status) *out_refine_status = 0;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!walk_queries || !refine_queries || !out_ids || !out_dists || !out_counts)
        return fail(GRANNE_HIP_ERR_INVALID, "search_refined_sum_embeddings: null buffer");
    GRANNE_HIP_ON_DEVICE(wx->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t wqb = (size_t)nq * wx->dim * query_elem_size(wx->dtype), rqb = (size_t)nq * se->dim * 4u;
    const size_t o_rq = up(wqb), o_ids = o_rq + up(rqb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4);
    const size_t o_s = o_c + up((size_t)nq * 4), o_st = o_s + (size_t)nq * 24, total = o_st + 32; // status: the walk's four words, then the refine word
    granne_hip_index* mwx = const_cast<granne_hip_index*>(wx);
    granne_hip_index::HostCall* c = host_call_acquire(mwx);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // (as granne_hip_search_refined_batch: the context goes back once its stream is idle)
        granne_hip_index* ix;
        granne_hip_index::HostCall* c;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            host_call_release(ix, c);
        }
    } release{mwx, c};
    HIP_TRY(c->d_buf.reserve(total));
    uint8_t* buf = c->d_buf.as<uint8_t>();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(buf, walk_queries, wqb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(buf + o_rq, refine_queries, rqb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(buf + o_st, 0, 32, s));
    rc = granne_hip_search_refined_sum_embeddings_batch_device(wx, se, buf, buf + o_rq, nq, max_search, refine_from, k,
                                                               (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                                               out_stats ? (uint64_t*)(buf + o_s) : nullptr, (uint32_t*)(buf + o_st),
                                                               (uint32_t*)(buf + o_st + 16), s);
    if (rc) return rc;
    uint32_t st[5] = {0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, buf + o_st, 20, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, buf + o_s, (size_t)nq * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st[0]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
    if (out_refine_status) *out_refine_status = st[4];
    return GRANNE_HIP_OK;
}

// ---- the container's elements as prepared rows of a dense element type ------------------------------------------------
constexpr uint64_t SE_ROWS_F32_SCRATCH = 40ull << 20; // bytes of normalised f32 rows per chunk; the converted chunk adds up to half

static uint32_t se_rows_elem_size(int dtype) { return dtype == GRANNE_HIP_F32 ? 4u : dtype == GRANNE_HIP_F16 ? 2u : 1u; }

// rows per chunk: what SE_ROWS_F32_SCRATCH holds, or fewer when GRANNE_HIP_SE_ROWS_CHUNK says so (tests cross a chunk's
// end with a handful of rows); read at every call
static uint64_t se_rows_chunk(uint32_t dim) {
    uint64_t rows = SE_ROWS_F32_SCRATCH / ((uint64_t)dim * 4u);
    if (rows < 1) rows = 1;
    const char* e = getenv("GRANNE_HIP_SE_ROWS_CHUNK");
    const long long want = e ? atoll(e) : 0;
    if (want > 0 && (uint64_t)want < rows) rows = (uint64_t)want;
    return rows;
}

// the container's length, read under its mutex: an append on another thread may be growing the offsets. (Elements are
// only ever added, so a range that is inside this length is inside the device copy a call takes afterwards.)
static uint64_t se_locked_len(const granne_hip_sum_embeddings* cse) {
    auto* se = const_cast<granne_hip_sum_embeddings*>(cse);
    std::lock_guard<std::mutex> lk(se->mu);
    return se->offsets.size() - 1;
}

static int se_rows_check(const granne_hip_sum_embeddings* se, uint64_t first, uint64_t count, int dtype) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: the container is null");
    if (dtype != GRANNE_HIP_F32 && dtype != GRANNE_HIP_I8 && dtype != GRANNE_HIP_F16)
        return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: unknown dtype %d", dtype);
    const uint64_t n = se_locked_len(se);
    if (first > n || count > n - first) return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: elements out of range");
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_sum_embeddings_rows_device(const granne_hip_sum_embeddings* se, uint64_t first, uint64_t count, int dtype,
                                                     void* d_out, uint64_t stride_bytes, void* stream) {
    int rc = se_rows_check(se, first, count, dtype);
    if (rc) return rc;
    const uint32_t es = se_rows_elem_size(dtype);
    const uint64_t row = (uint64_t)se->dim * es;
    if (stride_bytes < row || stride_bytes % es)
        return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: the row stride (%llu bytes) must be a multiple of %u and at least %llu",
                    (unsigned long long)stride_bytes, es, (unsigned long long)row);
    if (count == 0) return GRANNE_HIP_OK;
    if (!d_out) return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: out is null");
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    GRANNE_HIP_ON_DEVICE(d->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* off = d->d_offsets.as<uint64_t>();
    const uint32_t* terms = d->d_terms.as<uint32_t>();
    if (dtype == GRANNE_HIP_F32) { // the rows kernel writes strided rows itself: no scratch
        return se_rows_launch(*d, off, terms, first, count, 1, (float*)d_out, stride_bytes / 4u, s);
    }
    // normalised f32 rows of a chunk in stream-ordered scratch, converted by the kernels of granne_hip_quantize_f32_device /
    // granne_hip_f32_to_f16_device (dense on both sides); a stride beyond the row takes the converted chunk through scratch
    // of its own and a strided copy
    const uint64_t chunk = std::min<uint64_t>(se_rows_chunk(d->dim), count);
    const bool dense = stride_bytes == row;
    uint8_t* scratch = nullptr;
    const size_t f32_bytes = (size_t)chunk * d->dim * 4u, total = f32_bytes + (dense ? 0 : (size_t)chunk * row);
    HIP_TRY(hipMallocAsync((void**)&scratch, total, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() { (void)hipFreeAsync(p, s); }
    } release{scratch, s};
    for (uint64_t r0 = 0; rc == 0 && r0 < count; r0 += chunk) {
        const uint64_t nr = std::min(chunk, count - r0);
        uint8_t* dst = (uint8_t*)d_out + r0 * stride_bytes;
        uint8_t* conv = dense ? dst : scratch + f32_bytes;
        rc = se_rows_launch(*d, off, terms, first + r0, nr, 1, (float*)scratch, d->dim, s);
        if (rc) break;
        if (dtype == GRANNE_HIP_I8)
            hipLaunchKernelGGL(quantize_rows_kernel, dim3(grid_for(nr * 64, 256)), dim3(256), 0, s, (const float*)scratch, (int8_t*)conv, nr, d->dim);
        else
            hipLaunchKernelGGL(f32_to_f16_kernel, dim3(grid_for(nr * d->dim, 256)), dim3(256), 0, s, (const float*)scratch, (uint16_t*)conv, nr * d->dim);
        if (hipGetLastError() != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "sum_embeddings_rows: launch failed");
        if (rc == 0 && !dense && hipMemcpy2DAsync(dst, stride_bytes, conv, row, row, nr, hipMemcpyDeviceToDevice, s) != hipSuccess)
            rc = fail(GRANNE_HIP_ERR_HIP, "sum_embeddings_rows: hipMemcpy2DAsync failed");
    }
    return rc;
}

// the same into host memory: dense rows [count][dim] of dtype (synchronous)
extern "C" int granne_hip_sum_embeddings_rows(const granne_hip_sum_embeddings* se, uint64_t first, uint64_t count, int dtype, void* out) {
    int rc = se_rows_check(se, first, count, dtype);
    if (rc) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "sum_embeddings_rows: out is null");
    GRANNE_HIP_ON_DEVICE(se->device);
    // chunk by chunk through one device buffer of the chunk's rows (f32 rows too), so that the host form is bounded like
    // the device form
    const uint64_t row = (uint64_t)se->dim * se_rows_elem_size(dtype);
    const uint64_t chunk = std::min<uint64_t>(se_rows_chunk(se->dim), count);
    DevBuf d_rows;
    HIP_TRY(d_rows.alloc((size_t)chunk * row));
    for (uint64_t r0 = 0; r0 < count; r0 += chunk) {
        const uint64_t nr = std::min(chunk, count - r0);
        rc = granne_hip_sum_embeddings_rows_device(se, first + r0, nr, dtype, d_rows.get(), row, nullptr);
        if (rc) return rc;
        HIP_TRY(hipMemcpy((uint8_t*)out + r0 * row, d_rows.get(), (size_t)nr * row, hipMemcpyDeviceToHost));
    }
    return GRANNE_HIP_OK;
}
