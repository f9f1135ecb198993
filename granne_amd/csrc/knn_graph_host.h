// knn_graph_host.h -- host side of granne_hip_knn_graph* (included by granne_hip.hip after exact_topk_screened_host.h):
// every element's exact k nearest OTHER elements. The driver is exact_topk_screened_run with the handle's own rows as the
// queries (own_first): the scan kernels' ETS_Q_ROWS variant reads a query where its row lies and takes the score of a row
// with itself out before anything counts it. The kernels: exact_topk_screened.hip; the method: DESIGN.md 3.7e.
#pragma once

#include "exact_topk_screened.h"

static int knn_graph_args(const granne_hip_index* ix, uint64_t first, uint64_t count, uint32_t k, bool buffers) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "knn_graph");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "knn_graph");
    if (first > ix->n_elements || count > ix->n_elements - first)
        return fail(GRANNE_HIP_ERR_INVALID, "knn_graph: first + count (%llu + %llu) is beyond the %llu elements", (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)ix->n_elements);
    if (count == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph: null buffer");
    if (k == 0 || k >= ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph: k must be in [1, %u]", ET_KMAX - 1u);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph takes up to 2^32 - 1 elements");
    return GRANNE_HIP_OK;
}

// The rows first + p (p = d_list[f], or f where d_list is null; f < m) answered by exact_topk's own scan: gathered as dense
// queries a round of ET_CHUNK at a time, asked for k + 1, and the row itself dropped on the way to place p of the outputs
// (kg_drop_self_kernel). d_xs: exact_topk's status words. d_filter with d_allowed, its id list (graph_filtered_host.h): the
// rows are the ids at the list's positions first + p, and the scan runs under the filter.
static int kg_by_scan(const granne_hip_index* ix, uint64_t first, const uint32_t* d_list, uint32_t m, uint32_t k, uint64_t* d_out_ids,
                      float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_xs, hipStream_t s, const uint32_t* d_filter,
                      const uint32_t* d_allowed) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qbytes = ix->dim * query_elem_size(ix->dtype);
    const uint32_t mc_max = m < ET_CHUNK ? m : ET_CHUNK, k1 = k + 1u;
    const size_t o_ids = up((size_t)mc_max * qbytes), o_d = o_ids + (size_t)mc_max * k1 * 8, o_c = o_d + up((size_t)mc_max * k1 * 4);
    uint8_t* buf = nullptr;
    HIP_TRY(hipMallocAsync((void**)&buf, o_c + (size_t)mc_max * 4, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() { (void)hipFreeAsync(p, s); }
    } release{buf, s};
    for (uint32_t c0 = 0; c0 < m; c0 += ET_CHUNK) {
        const uint32_t mc = m - c0 < ET_CHUNK ? m - c0 : ET_CHUNK;
        const uint32_t* const list = d_list ? d_list + c0 : nullptr;
        HIP_TRY(ets_gather_rows(ix->d_elements.as<uint8_t>(), ix->row_stride, qbytes, first, list, c0, mc, buf, s, d_allowed));
        if (const int rc = exact_topk_run(ix, buf, mc, k1, d_filter, 0, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c), d_xs, s))
            return rc;
        HIP_TRY(kg_drop_self(first, list, c0, mc, k, (const uint64_t*)(buf + o_ids), (const float*)(buf + o_d), (const uint32_t*)(buf + o_c), d_out_ids,
                             d_out_dists, d_out_counts, s, d_allowed));
    }
    return GRANNE_HIP_OK;
}

// For e in [first, first + count): the first k of all elements j != e by (distance bits of dist(element e, element j), j),
// into row e - first of the outputs. Ordered on `stream`, which the call waits on once at its end (the fallback list's length).
extern "C" int granne_hip_knn_graph_device(const granne_hip_index* ix, uint64_t first, uint64_t count, uint32_t k, uint64_t* d_out_ids,
                                           float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = knn_graph_args(ix, first, count, k, d_out_ids && d_out_dists && d_out_counts)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    return exact_topk_screened_run(ix, nullptr, (uint32_t)count, k, d_out_ids, d_out_dists, d_out_counts, d_status, (hipStream_t)stream, nullptr, 0,
                                   &first);
}

// host buffers out; GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where exact_topk itself would give it
extern "C" int granne_hip_knn_graph(const granne_hip_index* ix, uint64_t first, uint64_t count, uint32_t k, uint64_t* out_ids, float* out_dists,
                                    uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = knn_graph_args(ix, first, count, k, out_ids && out_dists && out_counts)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_d = (size_t)count * k * 8, o_c = o_d + up((size_t)count * k * 4), o_st = o_c + up((size_t)count * 4);
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the passes left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = granne_hip_knn_graph_device(ix, first, count, k, (uint64_t*)buf, (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                                   (uint32_t*)(buf + o_st), nullptr))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf, (size_t)count * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)count * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[3] & ETS_VOIDED)
        return fail(GRANNE_HIP_ERR_OVERFLOW, "knn_graph: exact_topk's own selection overflowed for an element handed to it (more than %u rows "
                    "inside one second-level bin at its k-th distance)", ET_CAP);
    return GRANNE_HIP_OK;
}
