// exact_topk_screened_filtered_host.h -- granne_hip_exact_topk_screened_filtered*: exact_topk_filtered's answer with the
// matrix cores screening the rows first (included by granne_hip.hip after exact_topk_screened_host.h, whose driver runs
// the call: exact_topk_screened_run with a filter; the kernels' sources are exact_topk_screened.h's ETS_LIST and ETS_BITS;
// DESIGN.md 3.7c). Here: the argument checks, the fallback under per-query bitmaps, and the two entries.
#pragma once

#include "exact_topk_screened_host.h"

static int exact_topk_screened_filtered_args(const granne_hip_index* ix, uint32_t nq, uint32_t k, bool buffers, const void* filter,
                                             uint64_t filter_stride_words) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened_filtered: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_topk_screened_filtered");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_topk_screened_filtered");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened_filtered: null buffer");
    if (k == 0 || k > ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened_filtered: k must be in [1, %u]", ET_KMAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened_filtered takes up to 2^32 - 1 elements");
    if (!filter) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened_filtered: the filter is null");
    if (filter_stride_words && filter_stride_words < filter_words(ix->n_elements))
        return fail(GRANNE_HIP_ERR_INVALID,
                    "exact_topk_screened_filtered: filter_stride_words (%llu) must be 0 or at least ceil(n_elements / 32) = %llu",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(ix->n_elements));
    return GRANNE_HIP_OK;
}

// The nfb queries of the fallback list (dense at d_fb_queries, their places among the call's in d_fb_list) by
// exact_topk_run, each under its own bitmap: the listed queries' bitmaps are gathered a bounded number (256 MiB) at a
// time, as exact_range_run's phase B gathers them. d_fb_after_*: the listed queries' cursors, dense like their queries (null: none).
static int ets_fallback_bits(const granne_hip_index* ix, const uint8_t* d_fb_queries, const uint32_t* d_fb_list, uint32_t nfb, uint32_t k,
                             const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_ids, float* d_dists, uint32_t* d_counts,
                             uint32_t* d_xs, hipStream_t s, const float* d_fb_after_dists, const uint64_t* d_fb_after_ids) {
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    const uint64_t words = filter_words(ix->n_elements);
    uint64_t chunk = (256ull << 20) / (words * 4u);
    if (chunk < 1) chunk = 1;
    if (chunk > nfb) chunk = nfb;
    PfStreamMem maps;
    HIP_TRY(maps.alloc((size_t)chunk * words * 4, s));
    for (uint32_t c0 = 0; c0 < nfb; c0 += (uint32_t)chunk) {
        const uint32_t qc = nfb - c0 < chunk ? nfb - c0 : (uint32_t)chunk;
        if (const int rc = pf_gather_rows(d_filter, filter_stride_words * 4u, d_fb_list + c0, qc, words * 4u, maps.p, s)) return rc;
        if (const int rc = exact_topk_run(ix, d_fb_queries + (size_t)c0 * qbytes, qc, k, maps.as<uint32_t>(), words, d_ids + (size_t)c0 * k,
                                          d_dists + (size_t)c0 * k, d_counts + c0, d_xs, s, nullptr, nullptr,
                                          d_fb_after_ids ? d_fb_after_dists + c0 : nullptr, d_fb_after_ids ? d_fb_after_ids + c0 : nullptr))
            return rc;
    }
    return GRANNE_HIP_OK;
}

// exact_topk_filtered's answer, the matrix cores screening the rows first
extern "C" int granne_hip_exact_topk_screened_filtered_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                                              const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids,
                                                              float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = exact_topk_screened_filtered_args(ix, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, d_filter,
                                                         filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_screened_run(ix, d_queries, nq, k, d_out_ids, d_out_dists, d_out_counts, d_status, (hipStream_t)stream, d_filter,
                                   filter_stride_words);
}

// host buffers in and out, the filter's words on the host (ceil(n_elements / 32), or nq * filter_stride_words);
// GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where exact_topk_filtered itself would give it
extern "C" int granne_hip_exact_topk_screened_filtered(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k,
                                                       const uint32_t* filter, uint64_t filter_stride_words, uint64_t* out_ids,
                                                       float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = exact_topk_screened_filtered_args(ix, nq, k, queries && out_ids && out_dists && out_counts, filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t fb = (filter_stride_words ? (size_t)nq * filter_stride_words : (size_t)filter_words(ix->n_elements)) * 4;
    const size_t o_f = up(qb), o_ids = o_f + up(fb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4);
    const size_t o_st = o_c + up((size_t)nq * 4);
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the passes left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(buf + o_f, filter, fb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = exact_topk_screened_run(ix, buf, nq, k, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                               (uint32_t*)(buf + o_st), nullptr, (const uint32_t*)(buf + o_f), filter_stride_words))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[3] & ETS_VOIDED)
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_topk_screened_filtered: exact_topk's own selection overflowed for a query handed to it (more "
                    "than %u rows inside one second-level bin at its k-th distance)", ET_CAP);
    return GRANNE_HIP_OK;
}
