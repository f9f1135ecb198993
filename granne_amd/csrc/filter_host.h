// filter_host.h -- host side of filtered search (included by granne_hip.hip): granne_hip_search_filtered_batch* plan a
// walk under an id bitmap on the general walker (search_kernel.h, FILT) or, beyond its lists, on the exact walker
// (slow_kernel.h, FILT) -- never on a register walker; granne_hip_filter_* make and count bitmaps (filter.h).
#pragma once

#include "filter.h"

// what every filtered entry checks before any device call; OK with *run = false: nothing to do
static int filtered_check(const granne_hip_index* ix, uint32_t nq, uint32_t max_search, const void* filter,
                          uint64_t filter_stride_words, bool* run) {
    *run = false;
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "search_filtered: index is null");
    if (ix->dtype == GRANNE_HIP_F16)
        return fail(GRANNE_HIP_ERR_INVALID, "search_filtered: GRANNE_HIP_F16 (angular_f16) handles have no filtered walk");
    if (ix->se)
        return fail(GRANNE_HIP_ERR_INVALID, "search_filtered: compact SumEmbeddings handles have no filtered walk: make the index with GRANNE_HIP_SE_MATERIALIZED");
    if (max_search == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!filter) return fail(GRANNE_HIP_ERR_INVALID, "search_filtered: the filter is null");
    if (filter_stride_words && filter_stride_words < filter_words(ix->n_elements))
        return fail(GRANNE_HIP_ERR_INVALID, "search_filtered: filter_stride_words (%llu) must be 0 or at least ceil(len / 32) = %llu",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(ix->n_elements));
    *run = true;
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_search_filtered_batch_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq,
                                                       uint32_t max_search, uint32_t num_neighbors, const uint32_t* d_filter,
                                                       uint64_t filter_stride_words, uint64_t max_expand, uint64_t* d_out_ids,
                                                       float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_stats,
                                                       uint32_t* d_status, void* stream) {
    bool run;
    int rc = filtered_check(ix, nq, max_search, d_filter, filter_stride_words, &run);
    if (rc || !run) return rc;
    SearchCall c = index_call(d_queries, nq, max_search, num_neighbors, d_out_ids, d_out_dists, d_out_counts, d_out_stats, d_status, stream);
    c.filter = d_filter;
    c.filter_stride = filter_stride_words;
    c.max_expand = max_expand > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)max_expand; // (a layer has fewer nodes than that: no cap)
    return search_launch(SearchTarget(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size()), c);
}

// the same with host buffers in and out (synchronous); never part of a GRANNE_HIP_OPT_COALESCE group
extern "C" int granne_hip_search_filtered_batch(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t max_search,
                                                uint32_t num_neighbors, const uint32_t* filter, uint64_t filter_stride_words,
                                                uint64_t max_expand, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                uint64_t* out_stats, uint32_t* out_status) {
    bool run;
    int rc = filtered_check(ix, nq, max_search, filter, filter_stride_words, &run);
    if (out_status && !rc) out_status[0] = out_status[1] = out_status[2] = out_status[3] = 0;
    if (rc || !run) return rc;
    if (num_neighbors == 0) { // .take(0), src/index/mod.rs:974-977
        if (!out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
        memset(out_counts, 0, (size_t)nq * 4);
        return GRANNE_HIP_OK;
    }
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t k = num_neighbors;
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t fb = (filter_stride_words ? (size_t)nq * filter_stride_words : (size_t)filter_words(ix->n_elements)) * 4;
    const size_t o_f = up(qb), o_ids = o_f + up(fb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4);
    const size_t o_s = o_c + up((size_t)nq * 4), o_st = o_s + (size_t)nq * 24, total = o_st + 16;
    granne_hip_index* mix = const_cast<granne_hip_index*>(ix);
    granne_hip_index::HostCall* c = host_call_acquire(mix);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // (as search_batch_direct: the context goes back once its stream is idle)
        granne_hip_index* ix;
        granne_hip_index::HostCall* c;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            host_call_release(ix, c);
        }
    } release{mix, c};
    HIP_TRY(c->d_buf.reserve(total));
    uint8_t* buf = c->d_buf.as<uint8_t>();
    hipStream_t s = c->stream;
    HIP_TRY(hipMemcpyAsync(buf, queries, qb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(buf + o_f, filter, fb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(buf + o_st, 0, 16, s));
    rc = granne_hip_search_filtered_batch_device(ix, buf, nq, max_search, num_neighbors, (const uint32_t*)(buf + o_f), filter_stride_words,
                                                 max_expand, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                                 out_stats ? (uint64_t*)(buf + o_s) : nullptr, (uint32_t*)(buf + o_st), s);
    if (rc) return rc;
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, buf + o_st, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, buf + o_s, (size_t)nq * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    mix->last_slow_count.store(st[1]);
    if (out_status) memcpy(out_status, st, 16);
    if (st[0]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
    return GRANNE_HIP_OK;
}

// ---- bitmaps --------------------------------------------------------------------------------------------------------
extern "C" int granne_hip_filter_words(uint64_t n_elements, uint64_t* out_words) {
    if (!out_words) return fail(GRANNE_HIP_ERR_INVALID, "filter_words: out_words is null");
    *out_words = filter_words(n_elements);
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_filter_from_ids_device(const uint64_t* d_ids, uint64_t n_ids, uint64_t n_elements, uint32_t* d_filter,
                                                 uint32_t* d_bad, int device_id, void* stream) {
    if (!d_filter && n_elements) return fail(GRANNE_HIP_ERR_INVALID, "filter_from_ids: the filter is null");
    if (!d_ids && n_ids) return fail(GRANNE_HIP_ERR_INVALID, "filter_from_ids: ids is null");
    if (n_elements == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_filter, 0, (size_t)filter_words(n_elements) * 4, s));
    if (n_ids == 0) return GRANNE_HIP_OK;
    hipLaunchKernelGGL(filter_from_ids_kernel, dim3(grid_for(n_ids, 256)), dim3(256), 0, s, d_ids, n_ids, n_elements, d_filter, d_bad);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_filter_from_mask_device(const uint8_t* d_mask, uint64_t n_elements, uint32_t* d_filter, int device_id,
                                                  void* stream) {
    if (n_elements == 0) return GRANNE_HIP_OK;
    if (!d_mask || !d_filter) return fail(GRANNE_HIP_ERR_INVALID, "filter_from_mask: null buffer");
    GRANNE_HIP_ON_DEVICE(device_id);
    hipLaunchKernelGGL(filter_from_mask_kernel, dim3(grid_for(n_elements, 256)), dim3(256), 0, (hipStream_t)stream, d_mask, n_elements, d_filter);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// GRANNE_HIP_FILTER_SLICE_HANDOVER=1: the slice kernel with the lane hand-over instead of two loads per lane (read at
// every call: the measurement in tools/sharded_filtered_bench.py switches it inside one process)
static bool filter_slice_handover() {
    const char* e = getenv("GRANNE_HIP_FILTER_SLICE_HANDOVER");
    return e && *e && *e != '0';
}

// bits [first_bit, first_bit + n_out_bits) of n_filters bitmaps over n_bits ids as bitmaps of their own (filter_slice.h)
extern "C" int granne_hip_filter_slice_device(const uint32_t* d_filter, uint64_t n_bits, uint64_t filter_stride_words, uint32_t n_filters,
                                              uint64_t first_bit, uint64_t n_out_bits, uint32_t* d_out, uint64_t out_stride_words,
                                              int device_id, void* stream) {
    if (first_bit > n_bits) return fail(GRANNE_HIP_ERR_INVALID, "filter_slice: first_bit (%llu) is past the bitmap's %llu bits",
                                        (unsigned long long)first_bit, (unsigned long long)n_bits);
    if (n_out_bits == 0) return GRANNE_HIP_OK;
    if (n_filters == 0) return fail(GRANNE_HIP_ERR_INVALID, "filter_slice: n_filters is 0");
    if (!d_filter || !d_out) return fail(GRANNE_HIP_ERR_INVALID, "filter_slice: null buffer");
    if (filter_stride_words == 0 ? n_filters != 1 : filter_stride_words < filter_words(n_bits))
        return fail(GRANNE_HIP_ERR_INVALID, "filter_slice: filter_stride_words (%llu) must be at least ceil(n_bits / 32) = %llu, or 0 for one filter",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(n_bits));
    if (out_stride_words < filter_words(n_out_bits))
        return fail(GRANNE_HIP_ERR_INVALID, "filter_slice: out_stride_words (%llu) must be at least ceil(n_out_bits / 32) = %llu",
                    (unsigned long long)out_stride_words, (unsigned long long)filter_words(n_out_bits));
    GRANNE_HIP_ON_DEVICE(device_id);
    const dim3 grid(grid_for(filter_words(n_out_bits), 256), n_filters < 1024u ? n_filters : 1024u);
    auto kernel = filter_slice_handover() ? filter_slice_kernel<true> : filter_slice_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, d_filter, n_bits, filter_stride_words, n_filters, first_bit,
                       n_out_bits, d_out, out_stride_words);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_filter_count_device(const uint32_t* d_filter, uint64_t n_elements, uint64_t* d_out, int device_id,
                                              void* stream) {
    if (!d_out) return fail(GRANNE_HIP_ERR_INVALID, "filter_count: out is null");
    if (!d_filter && n_elements) return fail(GRANNE_HIP_ERR_INVALID, "filter_count: the filter is null");
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(d_out, 0, 8, s));
    if (n_elements == 0) return GRANNE_HIP_OK;
    hipLaunchKernelGGL(filter_count_kernel, dim3(grid_for(filter_words(n_elements), 256)), dim3(256), 0, s, d_filter, n_elements,
                       (unsigned long long*)d_out);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}
