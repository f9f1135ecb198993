// graph_filtered_host.h -- host side of granne_hip_knn_graph_filtered* and granne_hip_range_graph_filtered* (included by
// granne_hip.hip after range_graph_host.h): the two graphs of a SUBSET -- every allowed element's exact neighbours among
// the allowed elements, under one shared id bitmap. A is the bitmap's ascending id list, m its length; a window is a range
// of POSITIONS of A, and output row p belongs to element A[first + p]. The bitmap is compacted here, once, by the filter's
// own compaction, and m is read back at the start of the call (the one wait the list costs, as in
// exact_topk_screened_filtered); the drivers are knn_graph's and range_graph's with the list AND the own rows set:
// exact_topk_screened_run(own_first, d_allowed) and range_graph_run(d_allowed). Their scans are the nine instantiations of
// ETS_LIST with ETS_Q_ROWS (exact_topk_screened.hip): rows and queries are both positions of A, so the diagonal is a compare
// of positions and an element needs no search for its own place in the list. The method: DESIGN.md 3.7g.
#pragma once

#include "range_graph_host.h"

// the checks that need no device; the window is held to the handle's size here and to m once m is known
static int knn_graph_filtered_args(const granne_hip_index* ix, const void* filter, uint64_t first, uint64_t count, uint32_t k, bool buffers) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph_filtered: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "knn_graph_filtered");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "knn_graph_filtered");
    if (count == 0) return GRANNE_HIP_OK;
    if (!buffers || !filter) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph_filtered: null buffer");
    if (k == 0 || k >= ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph_filtered: k must be in [1, %u]", ET_KMAX - 1u);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "knn_graph_filtered takes up to 2^32 - 1 elements");
    if (first > ix->n_elements || count > ix->n_elements - first)
        return fail(GRANNE_HIP_ERR_INVALID, "knn_graph_filtered: first + count (%llu + %llu) is beyond the %llu elements", (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)ix->n_elements);
    return GRANNE_HIP_OK;
}
static int range_graph_filtered_args(const granne_hip_index* ix, const void* filter, uint64_t first, uint64_t count, uint32_t cap, bool buffers) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "range_graph_filtered");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "range_graph_filtered");
    if (count == 0) return GRANNE_HIP_OK;
    if (!buffers || !filter) return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered: null buffer");
    if (cap == 0 || cap > ER_CAP_MAX) return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered: cap (%u) must be in [1, %u]", cap, ER_CAP_MAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered takes up to 2^32 - 1 elements");
    if (first > ix->n_elements || count > ix->n_elements - first)
        return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered: first + count (%llu + %llu) is beyond the %llu elements", (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)ix->n_elements);
    return GRANNE_HIP_OK;
}

// A on the device: its length (u64), the compaction's block counts, the ids -- the call's own until its stream has run
struct GfAllowed {
    PfStreamMem mem;
    const uint32_t* ids = nullptr;
    uint64_t m = 0;
};
// Compacts d_filter on s, waits for m and holds the window to it; `what` names the entry in the refusal.
static int gf_compact(const granne_hip_index* ix, const char* what, const uint32_t* d_filter, uint64_t first, uint64_t count, GfAllowed* a,
                      hipStream_t s) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint64_t n = ix->n_elements;
    const size_t o_blk = 256, o_ids = o_blk + up((size_t)fl_blocks(n) * 4);
    HIP_TRY(a->mem.alloc(o_ids + (size_t)n * 4, s));
    uint8_t* const buf = a->mem.as<uint8_t>();
    if (const int rc = filter_compact<uint32_t>(d_filter, n, (uint32_t*)(buf + o_blk), (uint32_t*)(buf + o_ids), (uint64_t*)buf, nullptr, s)) return rc;
    HIP_TRY(hipMemcpyAsync(&a->m, buf, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    a->ids = (const uint32_t*)(buf + o_ids);
    if (first > a->m || count > a->m - first)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: first + count (%llu + %llu) is beyond the %llu allowed elements", what, (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)a->m);
    return GRANNE_HIP_OK;
}
// m == 1: the one allowed element has no allowed neighbour -- an empty row (and total), the form in the status words
static int gf_alone(const granne_hip_index* ix, uint32_t width, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                    uint32_t* d_out_totals, uint32_t* d_status, hipStream_t s) {
    uint32_t form = ETS_FORM_ROUTED;
    if (const int rc = ets_form(ix, s, &form, false)) return rc;
    HIP_TRY(ets_empty(1u, width, d_out_ids, d_out_dists, d_out_counts, s));
    if (d_out_totals) HIP_TRY(ets_clear(d_out_totals, 1u, s));
    if (d_status) HIP_TRY(ers_status(d_status, nullptr, 0u, form, s));
    return GRANNE_HIP_OK;
}

// For p in [0, count), e = A[first + p]: d_out_elements[p] = e, and the first k of all allowed j != e by (distance bits of
// dist(element e, element j), j) into row p. Ordered on `stream`, which the call waits on at its start (m) and its end.
extern "C" int granne_hip_knn_graph_filtered_device(const granne_hip_index* ix, const uint32_t* d_filter, uint64_t first, uint64_t count, uint32_t k,
                                                    uint64_t* d_out_elements, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                                    uint32_t* d_status, void* stream) {
    if (const int rc = knn_graph_filtered_args(ix, d_filter, first, count, k, d_out_elements && d_out_ids && d_out_dists && d_out_counts)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(ix->device);
    hipStream_t s = (hipStream_t)stream;
    GfAllowed a;
    if (const int rc = gf_compact(ix, "knn_graph_filtered", d_filter, first, count, &a, s)) return rc;
    HIP_TRY(gf_elements(a.ids, first, (uint32_t)count, d_out_elements, s));
    if (a.m == 1) return gf_alone(ix, k, d_out_ids, d_out_dists, d_out_counts, nullptr, d_status, s);
    return exact_topk_screened_run(ix, nullptr, (uint32_t)count, k, d_out_ids, d_out_dists, d_out_counts, d_status, s, d_filter, 0, &first, a.ids, a.m);
}

// the same under a radius per element of the window: granne_hip_range_graph's outputs, row p for element A[first + p]
extern "C" int granne_hip_range_graph_filtered_device(const granne_hip_index* ix, const uint32_t* d_filter, uint64_t first, uint64_t count,
                                                      const float* d_radii, uint32_t cap, uint64_t* d_out_elements, uint64_t* d_out_ids,
                                                      float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status,
                                                      void* stream) {
    if (const int rc = range_graph_filtered_args(ix, d_filter, first, count, cap,
                                                 d_radii && d_out_elements && d_out_ids && d_out_dists && d_out_counts && d_out_totals))
        return rc;
    if (count == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(ix->device);
    hipStream_t s = (hipStream_t)stream;
    GfAllowed a;
    if (const int rc = gf_compact(ix, "range_graph_filtered", d_filter, first, count, &a, s)) return rc;
    HIP_TRY(gf_elements(a.ids, first, (uint32_t)count, d_out_elements, s));
    if (a.m == 1) return gf_alone(ix, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, d_status, s);
    return range_graph_run(ix, first, (uint32_t)count, d_radii, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, d_status, s, d_filter, a.ids,
                           a.m);
}

// The host entries' staging: the filter's words and the radii (range; else null) in, `width` ids and distances per row out.
// run(filter, radii, elements, ids, dists, counts, totals, status) is the device entry on the null stream.
template <class Run>
static int gf_staged(const granne_hip_index* ix, const uint32_t* filter, uint64_t count, const float* radii, uint32_t width, uint64_t* out_elements,
                     uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_totals, uint32_t st[4], Run run) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t fb = (size_t)filter_words(ix->n_elements) * 4, w = up((size_t)count * 4);
    const size_t o_r = up(fb), o_e = o_r + w, o_ids = o_e + up((size_t)count * 8), o_d = o_ids + up((size_t)count * width * 8);
    const size_t o_c = o_d + up((size_t)count * width * 4), o_t = o_c + w, o_st = o_t + w;
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the call left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, filter, fb, hipMemcpyHostToDevice));
    if (radii) HIP_TRY(hipMemcpy(buf + o_r, radii, (size_t)count * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = run((const uint32_t*)buf, (const float*)(buf + o_r), (uint64_t*)(buf + o_e), (uint64_t*)(buf + o_ids), (float*)(buf + o_d),
                           (uint32_t*)(buf + o_c), (uint32_t*)(buf + o_t), (uint32_t*)(buf + o_st)))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_elements, buf + o_e, (size_t)count * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)count * width * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)count * width * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)count * 4, hipMemcpyDeviceToHost));
    if (out_totals) HIP_TRY(hipMemcpy(out_totals, buf + o_t, (size_t)count * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

// host buffers in and out (the filter's ceil(n_elements / 32) words on the host); GRANNE_HIP_ERR_OVERFLOW (outputs and
// status still written) where exact_topk itself would give it
extern "C" int granne_hip_knn_graph_filtered(const granne_hip_index* ix, const uint32_t* filter, uint64_t first, uint64_t count, uint32_t k,
                                             uint64_t* out_elements, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                             uint32_t* out_status) {
    if (const int rc = knn_graph_filtered_args(ix, filter, first, count, k, out_elements && out_ids && out_dists && out_counts)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    uint32_t st[4] = {0, 0, 0, 0};
    if (const int rc = gf_staged(ix, filter, count, nullptr, k, out_elements, out_ids, out_dists, out_counts, nullptr, st,
                                 [&](const uint32_t* f, const float*, uint64_t* e, uint64_t* ids, float* d, uint32_t* c, uint32_t*, uint32_t* status) {
                                     return granne_hip_knn_graph_filtered_device(ix, f, first, count, k, e, ids, d, c, status, nullptr);
                                 }))
        return rc;
    if (out_status) memcpy(out_status, st, 16);
    if (st[3] & ETS_VOIDED)
        return fail(GRANNE_HIP_ERR_OVERFLOW, "knn_graph_filtered: exact_topk's own selection overflowed for an element handed to it (more than %u "
                    "rows inside one second-level bin at its k-th distance)", ET_CAP);
    return GRANNE_HIP_OK;
}

// the same for the radius graph; a NaN radius is refused here, where it can be seen
extern "C" int granne_hip_range_graph_filtered(const granne_hip_index* ix, const uint32_t* filter, uint64_t first, uint64_t count,
                                               const float* radii, uint32_t cap, uint64_t* out_elements, uint64_t* out_ids, float* out_dists,
                                               uint32_t* out_counts, uint32_t* out_totals, uint32_t* out_status) {
    if (const int rc = range_graph_filtered_args(ix, filter, first, count, cap, radii && out_elements && out_ids && out_dists && out_counts && out_totals))
        return rc;
    if (count == 0) return GRANNE_HIP_OK;
    if (const uint32_t bad = range_first_nan(radii, (uint32_t)count); bad < count)
        return fail(GRANNE_HIP_ERR_INVALID, "range_graph_filtered: the radius of position %llu is NaN", (unsigned long long)(first + bad));
    uint32_t st[4] = {0, 0, 0, 0};
    if (const int rc = gf_staged(ix, filter, count, radii, cap, out_elements, out_ids, out_dists, out_counts, out_totals, st,
                                 [&](const uint32_t* f, const float* r, uint64_t* e, uint64_t* ids, float* d, uint32_t* c, uint32_t* t, uint32_t* status) {
                                     return granne_hip_range_graph_filtered_device(ix, f, first, count, r, cap, e, ids, d, c, t, status, nullptr);
                                 }))
        return rc;
    if (out_status) memcpy(out_status, st, 16);
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "range_graph_filtered: %u elements have more than %u rows inside one second-level bin at their cap-th "
                    "distance", st[0], ET_CAP);
    return GRANNE_HIP_OK;
}
