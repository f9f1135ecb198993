// exact_topk_after_host.h -- granne_hip_exact_topk_after*, granne_hip_exact_topk_screened_after*: the exact entries paged
// by a key cursor (included by granne_hip.hip after exact_topk_screened_filtered_host.h). Per query the
// caller names the last entry it has, (after_dists[q], after_ids[q]); the answer is the next k rows of exact_topk's own
// order -- the rows whose key (distance bits << 32 | id) is strictly greater -- so feeding a page's last entry back
// enumerates the whole order, k at a time, with no limit but the rows there are. The work is the siblings' drivers',
// exact_topk_run and exact_topk_screened_run with their optional cursor; here: the argument checks (the siblings', with
// the siblings' messages), the host staging, and the four entries. One pair of entries covers plain and filtered use: a
// null filter is all rows, filter_stride_words == 0 one bitmap for every query, anything else one bitmap per query.
#pragma once

#include "exact_topk_screened_filtered_host.h"

static int exact_topk_after_args(const granne_hip_index* ix, bool screened, uint32_t nq, uint32_t k, bool buffers, bool cursor_whole,
                                 const void* filter, uint64_t filter_stride_words) {
    if (const int rc = !screened ? exact_topk_args(ix, nq, k, buffers, filter != nullptr, filter, filter_stride_words)
                       : filter  ? exact_topk_screened_filtered_args(ix, nq, k, buffers, filter, filter_stride_words)
                                 : exact_topk_screened_args(ix, nq, k, buffers))
        return rc;
    if (nq && !cursor_whole) return fail(GRANNE_HIP_ERR_INVALID, "%s: after_ids without after_dists", screened ? "exact_topk_screened_after" : "exact_topk_after");
    return GRANNE_HIP_OK;
}

static int exact_topk_after_run(const granne_hip_index* ix, bool screened, const void* d_queries, uint32_t nq, uint32_t k,
                                const float* d_after_dists, const uint64_t* d_after_ids, const uint32_t* d_filter, uint64_t filter_stride_words,
                                uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, hipStream_t s) {
    if (screened)
        return exact_topk_screened_run(ix, d_queries, nq, k, d_out_ids, d_out_dists, d_out_counts, d_status, s, d_filter, filter_stride_words,
                                       nullptr, nullptr, 0, d_after_dists, d_after_ids);
    return exact_topk_run(ix, d_queries, nq, k, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts, d_status, s, nullptr, nullptr,
                          d_after_dists, d_after_ids);
}

// Host buffers in and out around exact_topk_after_run: the queries, the cursors and the filter's words go up, the answer
// and the status words come back; GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where the sibling gives it.
static int exact_topk_after_staged(const granne_hip_index* ix, bool screened, const void* queries, uint32_t nq, uint32_t k,
                                   const float* after_dists, const uint64_t* after_ids, const uint32_t* filter, uint64_t filter_stride_words,
                                   uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t fb = !filter ? 0 : (filter_stride_words ? (size_t)nq * filter_stride_words : (size_t)filter_words(ix->n_elements)) * 4;
    const size_t o_f = up(qb), o_ai = o_f + up(fb), o_ad = o_ai + (size_t)nq * 8, o_ids = o_ad + up((size_t)nq * 4);
    const size_t o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4), o_st = o_c + up((size_t)nq * 4);
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the passes left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    if (filter) HIP_TRY(hipMemcpy(buf + o_f, filter, fb, hipMemcpyHostToDevice));
    if (after_ids) {
        HIP_TRY(hipMemcpy(buf + o_ai, after_ids, (size_t)nq * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(buf + o_ad, after_dists, (size_t)nq * 4, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = exact_topk_after_run(ix, screened, buf, nq, k, after_ids ? (const float*)(buf + o_ad) : nullptr,
                                            after_ids ? (const uint64_t*)(buf + o_ai) : nullptr, filter ? (const uint32_t*)(buf + o_f) : nullptr,
                                            filter_stride_words, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                            (uint32_t*)(buf + o_st), nullptr))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (!screened && st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_topk_after: %u queries have more than %u rows inside one second-level bin at their k-th distance",
                    st[0], ET_CAP);
    if (screened && (st[3] & ETS_VOIDED))
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_topk_screened_after: exact_topk's own selection overflowed for a query handed to it (more than "
                    "%u rows inside one second-level bin at its k-th distance)", ET_CAP);
    return GRANNE_HIP_OK;
}

// the k rows that follow each query's cursor in exact_topk's order
extern "C" int granne_hip_exact_topk_after_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                                  const float* d_after_dists, const uint64_t* d_after_ids, const uint32_t* d_filter,
                                                  uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                                  uint32_t* d_status, void* stream) {
    if (const int rc = exact_topk_after_args(ix, false, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, !d_after_ids || d_after_dists,
                                             d_filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_after_run(ix, false, d_queries, nq, k, d_after_dists, d_after_ids, d_filter, filter_stride_words, d_out_ids, d_out_dists,
                                d_out_counts, d_status, (hipStream_t)stream);
}

extern "C" int granne_hip_exact_topk_after(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k, const float* after_dists,
                                           const uint64_t* after_ids, const uint32_t* filter, uint64_t filter_stride_words, uint64_t* out_ids,
                                           float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = exact_topk_after_args(ix, false, nq, k, queries && out_ids && out_dists && out_counts, !after_ids || after_dists, filter,
                                             filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_after_staged(ix, false, queries, nq, k, after_dists, after_ids, filter, filter_stride_words, out_ids, out_dists, out_counts,
                                   out_status);
}

// the same answer, the matrix cores screening the rows first
extern "C" int granne_hip_exact_topk_screened_after_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                                           const float* d_after_dists, const uint64_t* d_after_ids, const uint32_t* d_filter,
                                                           uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists,
                                                           uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = exact_topk_after_args(ix, true, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, !d_after_ids || d_after_dists,
                                             d_filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_after_run(ix, true, d_queries, nq, k, d_after_dists, d_after_ids, d_filter, filter_stride_words, d_out_ids, d_out_dists,
                                d_out_counts, d_status, (hipStream_t)stream);
}

extern "C" int granne_hip_exact_topk_screened_after(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k,
                                                    const float* after_dists, const uint64_t* after_ids, const uint32_t* filter,
                                                    uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                    uint32_t* out_status) {
    if (const int rc = exact_topk_after_args(ix, true, nq, k, queries && out_ids && out_dists && out_counts, !after_ids || after_dists, filter,
                                             filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_after_staged(ix, true, queries, nq, k, after_dists, after_ids, filter, filter_stride_words, out_ids, out_dists, out_counts,
                                   out_status);
}
