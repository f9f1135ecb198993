// refine_host.h -- host side of refined search (included by granne_hip.hip): granne_hip_refine_device re-ranks candidate
// lists by the rows of one index (refine_kernel.h); granne_hip_search_refined_batch_device is a walk of one index followed
// by that kernel over another's rows, on one stream, the candidate lists in stream-ordered scratch.
#pragma once

#include "refine_kernel.h"

// what every entry checks before any device call, the plain numbers first; `what` names the entry in the message.
// `wx`: the walk index of a fused call (max_search is its), or null with max_search = 0 for the re-rank alone.
static int refine_check(const granne_hip_index* rx, uint32_t m, uint32_t k, const char* what, bool fused = false,
                        const granne_hip_index* wx = nullptr, uint32_t max_search = 0) {
    if (m == 0 || m > REFINE_MAX_M) return fail(GRANNE_HIP_ERR_INVALID, "%s: candidates per query must be in [1, %u]", what, REFINE_MAX_M);
    if (k == 0) return fail(GRANNE_HIP_ERR_INVALID, "%s: k must be > 0", what);
    if (fused && m > max_search)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: refine_from (%u) must not exceed max_search (%u)", what, m, max_search);
    if (fused && !wx) return fail(GRANNE_HIP_ERR_INVALID, "%s: the walk index is null", what);
    if (!rx) return fail(GRANNE_HIP_ERR_INVALID, "%s: the refine index is null", what);
    GRANNE_HIP_COMPACT_UNSUPPORTED(rx, "refine");
    if (fused && wx->device != rx->device)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: the two indexes live on devices %d and %d", what, wx->device, rx->device);
    return GRANNE_HIP_OK;
}

// the kernel over checked arguments (nq > 0, buffers not null)
static int refine_launch(const granne_hip_index* rx, const void* d_queries, uint32_t nq, const uint64_t* d_cand_ids,
                         const uint32_t* d_cand_counts, uint32_t m, uint32_t k, uint64_t* d_out_ids, float* d_out_dists,
                         uint32_t* d_out_counts, uint32_t* d_refine_status, hipStream_t s) {
    RefineParams P;
    P.elements = rx->d_elements.as<uint8_t>();
    P.n_elements = rx->n_elements;
    P.row_bytes = rx->row_bytes;
    P.row_stride = rx->row_stride;
    P.dim = rx->dim;
    P.queries = (const uint8_t*)d_queries;
    P.cand = d_cand_ids;
    P.counts = d_cand_counts;
    P.m = m;
    P.k = k;
    P.q_lds_bytes = rx->dtype != GRANNE_HIP_I8 ? ((rx->dim * 4u + 15u) & ~15u) : rx->row_bytes; // (rows of halves: f32 queries)
    P.out_ids = d_out_ids;
    P.out_dists = d_out_dists;
    P.out_counts = d_out_counts;
    P.status = d_refine_status;
    const uint64_t lds = (uint64_t)refine_lds_q_off(m) + P.q_lds_bytes;
    if (lds > 160u * 1024u - 64u) return fail(GRANNE_HIP_ERR_INVALID, "refine: dimension too large for the LDS stage");
    void (*fn)(const RefineParams) = rx->dtype == GRANNE_HIP_F32 ? refine_kernel<0> : rx->dtype == GRANNE_HIP_F16 ? refine_kernel<DT_F16> : refine_kernel<1>;
    if (lds > 32u * 1024u) HIP_TRY(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fn, dim3(nq), dim3(REFINE_THREADS), (uint32_t)lds, s, P);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_refine_device(const granne_hip_index* rx, const void* d_queries, uint32_t nq, const uint64_t* d_cand_ids,
                                        const uint32_t* d_cand_counts, uint32_t m, uint32_t k, uint64_t* d_out_ids,
                                        float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_refine_status, void* stream) {
    int rc = refine_check(rx, m, k, "refine");
    if (rc) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_queries || !d_cand_ids || !d_out_ids || !d_out_dists || !d_out_counts) return fail(GRANNE_HIP_ERR_INVALID, "refine: null buffer");
    GRANNE_HIP_ON_DEVICE(rx->device);
    return refine_launch(rx, d_queries, nq, d_cand_ids, d_cand_counts, m, k, d_out_ids, d_out_dists, d_out_counts, d_refine_status,
                         (hipStream_t)stream);
}

extern "C" int granne_hip_search_refined_batch_device(const granne_hip_index* wx, const granne_hip_index* rx, const void* d_walk_queries,
                                                      const void* d_refine_queries, uint32_t nq, uint32_t max_search,
                                                      uint32_t refine_from, uint32_t k, uint64_t* d_out_ids, float* d_out_dists,
                                                      uint32_t* d_out_counts, uint64_t* d_out_stats, uint32_t* d_status,
                                                      uint32_t* d_refine_status, void* stream) {
    int rc = refine_check(rx, refine_from, k, "search_refined", true, wx, max_search);
    if (rc) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_walk_queries || !d_refine_queries || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(GRANNE_HIP_ERR_INVALID, "search_refined: null buffer");
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
    if (rc) return rc;
    return refine_launch(rx, d_refine_queries, nq, (const uint64_t*)scratch, (const uint32_t*)(scratch + o_c), m, k, d_out_ids,
                         d_out_dists, d_out_counts, d_refine_status, s);
}

// the same with host buffers in and out (synchronous)
extern "C" int granne_hip_search_refined_batch(const granne_hip_index* wx, const granne_hip_index* rx, const void* walk_queries,
                                               const void* refine_queries, uint32_t nq, uint32_t max_search, uint32_t refine_from,
                                               uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                               uint64_t* out_stats, uint32_t* out_refine_status) {
    int rc = refine_check(rx, refine_from, k, "search_refined", true, wx, max_search);
    if (rc) return rc;
    if (out_refine_status) *out_refine_status = 0;
    if (nq == 0) return GRANNE_HIP_OK;
    if (!walk_queries || !refine_queries || !out_ids || !out_dists || !out_counts) return fail(GRANNE_HIP_ERR_INVALID, "search_refined: null buffer");
    GRANNE_HIP_ON_DEVICE(wx->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t wqb = (size_t)nq * wx->dim * query_elem_size(wx->dtype), rqb = (size_t)nq * rx->dim * query_elem_size(rx->dtype);
    const size_t o_rq = up(wqb), o_ids = o_rq + up(rqb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4);
    const size_t o_s = o_c + up((size_t)nq * 4), o_st = o_s + (size_t)nq * 24, total = o_st + 32; // status: the walk's four words, then the refine word
    granne_hip_index* mwx = const_cast<granne_hip_index*>(wx);
    granne_hip_index::HostCall* c = host_call_acquire(mwx);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // (as search_batch_direct: the context goes back once its stream is idle)
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
    rc = granne_hip_search_refined_batch_device(wx, rx, buf, buf + o_rq, nq, max_search, refine_from, k, (uint64_t*)(buf + o_ids),
                                                (float*)(buf + o_d), (uint32_t*)(buf + o_c), out_stats ? (uint64_t*)(buf + o_s) : nullptr,
                                                (uint32_t*)(buf + o_st), (uint32_t*)(buf + o_st + 16), s);
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
