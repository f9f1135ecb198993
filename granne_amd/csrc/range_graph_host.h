// range_graph_host.h -- host side of granne_hip_range_graph* (included by granne_hip.hip after knn_graph_host.h): every
// element's exact neighbours within a radius -- exact_range with the element's own row as the query and the element struck
// out. The scan is exact_range_screened's one radius pass (ETS_RADIUS) with knn_graph's query source (ETS_Q_ROWS): a wave's
// 32 queries are read from the rows where they lie, and the score of a row with itself is -inf before the block's max, so
// an element is in neither of its lists and in none of its counts. The kernels: exact_topk_screened.hip; the method and
// the argument: DESIGN.md 3.7f. Per element, S sure rows (score >= hi), B band rows (lo <= score < hi), both without it:
//
//   A  total = S + (band rows with d <= r) <= ETS_CAP: both lists are whole; their keys within r are ranked (er_rank_kernel)
//   B  total > ETS_CAP, B <= ETS_CAP: the total is exact from the pass; the cap nearest others all lie within r: the rows
//      gathered as queries for exact_topk_screened_run(k = cap + 1), the element dropped by knn_graph's kg_drop_self
//   C  B > ETS_CAP, or a handle without a screen: the rows gathered for exact_range_run(cap + 1), which counts the element
//      exactly when d(e, e) <= r in its own arithmetic; rg_drop_self evaluates that compare once (dists_kernel on row e
//      against row e), corrects the total and drops the element
// cap + 1 may be ET_KMAX + 1: only the entries' argument checks hold k and cap to ET_KMAX -- the passes, the selection and
// the ranking take any k below ET_CAP and ET_PRIME_MIN. The call waits on its stream once for the lengths of the B and C
// lists (and wherever the runs it hands those elements to wait).
#pragma once

#include "exact_range_screened_host.h"
#include "knn_graph_host.h"

static_assert(ER_CAP_MAX + 1u < ET_CAP && ER_CAP_MAX + 1u < ET_PRIME_MIN, "cap + 1 is a k the scans can be asked for");

static int range_graph_args(const granne_hip_index* ix, uint64_t first, uint64_t count, uint32_t cap, bool buffers) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "range_graph: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "range_graph");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "range_graph");
    if (first > ix->n_elements || count > ix->n_elements - first)
        return fail(GRANNE_HIP_ERR_INVALID, "range_graph: first + count (%llu + %llu) is beyond the %llu elements", (unsigned long long)first,
                    (unsigned long long)count, (unsigned long long)ix->n_elements);
    if (count == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "range_graph: null buffer");
    if (cap == 0 || cap > ER_CAP_MAX) return fail(GRANNE_HIP_ERR_INVALID, "range_graph: cap (%u) must be in [1, %u]", cap, ER_CAP_MAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "range_graph takes up to 2^32 - 1 elements");
    return GRANNE_HIP_OK;
}

// Path C: the elements first + p (p = d_list[f], or f where d_list is null; f < m) by exact_range's own scan, a round of
// ET_CHUNK at a time: rows and radii gathered, d(e, e) from dists_kernel, the answer for cap + 1, the element struck out on
// the way to place p of the outputs. d_radii: the call's, by place. d_xs: exact_range's status words. d_filter with
// d_allowed, its id list (graph_filtered_host.h): the elements are the ids at the list's positions first + p, the scan runs
// under the filter -- which allows the element, so it is counted exactly when d(e, e) <= r, as without one.
static int rg_by_scan(const granne_hip_index* ix, uint64_t first, const uint32_t* d_list, uint32_t m, const float* d_radii, uint32_t cap,
                      uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_xs, hipStream_t s,
                      const uint32_t* d_filter = nullptr, const uint32_t* d_allowed = nullptr) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qbytes = ix->dim * query_elem_size(ix->dtype);
    const uint32_t mc_max = m < ET_CHUNK ? m : ET_CHUNK, cap1 = cap + 1u;
    const size_t w = up((size_t)mc_max * 4), o_r = up((size_t)mc_max * qbytes), o_sid = o_r + w, o_self = o_sid + w, o_c = o_self + w, o_t = o_c + w;
    const size_t o_ids = o_t + w, o_d = o_ids + up((size_t)mc_max * cap1 * 8);
    PfStreamMem mem;
    HIP_TRY(mem.alloc(o_d + (size_t)mc_max * cap1 * 4, s));
    uint8_t* const buf = mem.as<uint8_t>();
    for (uint32_t c0 = 0; c0 < m; c0 += ET_CHUNK) {
        const uint32_t mc = m - c0 < ET_CHUNK ? m - c0 : ET_CHUNK;
        const uint32_t* const list = d_list ? d_list + c0 : nullptr;
        HIP_TRY(ets_gather_rows(ix->d_elements.as<uint8_t>(), ix->row_stride, qbytes, first, list, c0, mc, buf, s, d_allowed));
        HIP_TRY(rg_self(first, list, c0, mc, d_radii, (uint32_t*)(buf + o_sid), (float*)(buf + o_r), s, d_allowed));
        if (const int rc = dists_launch(ix, buf, nullptr, 1u, (const uint32_t*)(buf + o_sid), mc, (float*)(buf + o_self), nullptr, s)) return rc;
        if (const int rc = exact_range_run(ix, buf, mc, (const float*)(buf + o_r), cap1, d_filter, 0, (uint64_t*)(buf + o_ids), (float*)(buf + o_d),
                                           (uint32_t*)(buf + o_c), (uint32_t*)(buf + o_t), d_xs, s))
            return rc;
        HIP_TRY(rg_drop_self(first, list, c0, mc, cap, (const uint64_t*)(buf + o_ids), (const float*)(buf + o_d), (const uint32_t*)(buf + o_c),
                             (const uint32_t*)(buf + o_t), (const float*)(buf + o_self), (const float*)(buf + o_r), d_out_ids, d_out_dists,
                             d_out_counts, d_out_totals, s, d_allowed));
    }
    return GRANNE_HIP_OK;
}

// Path B: the elements first + d_list[f], f < m, whose totals the pass has made: their cap nearest others by the screened
// selection over their gathered rows with k = cap + 1, the element dropped (kg_drop_self). An answer of count 0 is an
// element voided by exact_topk's overflow. d_filter, d_allowed: as rg_by_scan's -- the selection is then the screened
// filtered one.
static int rg_by_topk(const granne_hip_index* ix, uint64_t first, const uint32_t* d_list, uint32_t m, uint32_t cap, uint64_t* d_out_ids,
                      float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, hipStream_t s, const uint32_t* d_filter = nullptr,
                      const uint32_t* d_allowed = nullptr) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qbytes = ix->dim * query_elem_size(ix->dtype);
    const uint32_t mc_max = m < ET_CHUNK ? m : ET_CHUNK, cap1 = cap + 1u;
    const size_t o_c = up((size_t)mc_max * qbytes), o_ids = o_c + up((size_t)mc_max * 4), o_d = o_ids + up((size_t)mc_max * cap1 * 8);
    PfStreamMem mem;
    HIP_TRY(mem.alloc(o_d + (size_t)mc_max * cap1 * 4, s));
    uint8_t* const buf = mem.as<uint8_t>();
    for (uint32_t c0 = 0; c0 < m; c0 += ET_CHUNK) {
        const uint32_t mc = m - c0 < ET_CHUNK ? m - c0 : ET_CHUNK;
        HIP_TRY(ets_gather_rows(ix->d_elements.as<uint8_t>(), ix->row_stride, qbytes, first, d_list + c0, c0, mc, buf, s, d_allowed));
        if (const int rc = exact_topk_screened_run(ix, buf, mc, cap1, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c), nullptr, s,
                                                   d_filter))
            return rc;
        HIP_TRY(kg_drop_self(first, d_list + c0, c0, mc, cap, (const uint64_t*)(buf + o_ids), (const float*)(buf + o_d), (const uint32_t*)(buf + o_c),
                             d_out_ids, d_out_dists, d_out_counts, s, d_allowed));
        if (d_status) HIP_TRY(ers_voided((const uint32_t*)(buf + o_c), mc, d_status, s));
    }
    return GRANNE_HIP_OK;
}

// The call on stream s, arguments checked, nq = count > 0. d_radii: one per element of the window. d_status optional.
// d_filter (graph_filtered_host.h; null: all rows, and nothing below differs): one shared bitmap that the
// caller has compacted -- d_allowed is its id list of allowed_m >= 2 ids -- and the window is the list's POSITIONS first ..
// first + nq - 1 (within allowed_m): the pass scans the list with its queries read through it (ETS_LIST with ETS_Q_ROWS,
// the diagonal a compare of positions), the listed positions become ids in ers_pad, dists_kernel gets the round's query
// rows gathered dense, and paths B and C run under the filter and strike out the id at the position.
static int range_graph_run(const granne_hip_index* ix, uint64_t first, uint32_t nq, const float* d_radii, uint32_t cap, uint64_t* d_out_ids,
                           float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status, hipStream_t s,
                           const uint32_t* d_filter = nullptr, const uint32_t* d_allowed = nullptr, uint64_t allowed_m = 0) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    uint32_t form = ETS_FORM_ROUTED;
    if (const int rc = ets_form(ix, s, &form, false)) return rc;
    const bool i8 = ix->dtype == GRANNE_HIP_I8;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    if (form == ETS_FORM_ROUTED) { // no screen for the handle: every element is path C's
        PfStreamMem xs;
        HIP_TRY(xs.alloc(16, s));
        HIP_TRY(ets_clear(xs.as<uint32_t>(), 4u, s));
        if (const int rc = rg_by_scan(ix, first, nullptr, nq, d_radii, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, xs.as<uint32_t>(), s,
                                      d_filter, d_allowed))
            return rc;
        if (d_status) HIP_TRY(ers_status(d_status, xs.as<uint32_t>(), nq, (uint32_t)ETS_FORM_ROUTED, s));
        return GRANNE_HIP_OK;
    }
    const uint64_t n = d_allowed ? allowed_m : ix->n_elements; // the rows, or the list's positions, the pass scans
    const uint32_t qc_max = nq < ET_CHUNK ? nq : ET_CHUNK;
    const uint32_t qbytes = ix->dim * query_elem_size(ix->dtype);
    // scratch as exact_range_screened_run's: the numbers of B and C elements and er_rank_kernel's bitmap over the window
    // (cleared together); the two lists; a round's thresholds, counters and totals, its id lists [qc][2][ET_CAP], their
    // distances, the keys
    const size_t o_n = 0, o_dense = 256, o_lb = o_dense + up((size_t)filter_words(nq) * 4), o_lc = o_lb + up((size_t)nq * 4);
    const size_t o_lo = o_lc + up((size_t)nq * 4), w = up((size_t)qc_max * 4), o_hi = o_lo + w, o_sure = o_hi + w, o_cnt = o_sure + w;
    const size_t o_bcnt = o_cnt + w, o_tot = o_bcnt + w, o_cand = o_tot + w, o_dist = o_cand + (size_t)qc_max * 2 * ET_CAP * 4;
    const size_t o_keys = o_dist + (size_t)qc_max * 2 * ET_CAP * 4, o_q = o_keys + (size_t)qc_max * ET_CAP * 8;
    const size_t total = o_q + (d_allowed ? (size_t)qc_max * qbytes : 0); // (a list: a round's query rows, dense)
    PfStreamMem mem;
    HIP_TRY(mem.alloc(total, s));
    uint8_t* const scratch = mem.as<uint8_t>();
    HIP_TRY(ets_clear((uint32_t*)(scratch + o_n), 64u + (uint32_t)filter_words(nq), s));
    if (i8)
        if (const int rc = ets_scan_norms(ix, s)) return rc;
    const uint64_t tile = ets_tile_rows(form);
    EtsParams P;
    P.elements = ix->d_elements.as<uint8_t>();
    P.n = n;
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
    P.queries = nullptr;
    P.inv_norm = i8 ? ix->d_inv_norm.as<float>() : nullptr;
    P.inv_gmax = i8 ? P.inv_norm + ((ix->n_elements + 31u) & ~31ull) : nullptr;
    P.lo = (const float*)(scratch + o_lo);
    P.hi = (const float*)(scratch + o_hi);
    P.hist = nullptr;
    P.sure = (uint32_t*)(scratch + o_sure);
    P.cnt = (uint32_t*)(scratch + o_cnt);
    P.bcnt = (uint32_t*)(scratch + o_bcnt);
    P.cand = (uint32_t*)(scratch + o_cand);
    P.eps2 = 0.0f;
    P.list = d_allowed;
    const ErsLists lists{(uint32_t*)(scratch + o_n), (uint32_t*)(scratch + o_lb), (uint32_t*)(scratch + o_lc)};
    float* const dist = (float*)(scratch + o_dist);
    uint64_t* const keys = (uint64_t*)(scratch + o_keys);
    for (uint32_t c0 = 0; c0 < nq; c0 += ET_CHUNK) {
        const uint32_t qc = nq - c0 < ET_CHUNK ? nq - c0 : ET_CHUNK;
        const uint32_t tiles = (qc + ETS_QT - 1) / ETS_QT;
        P.q_first = first + c0;
        P.nq = qc;
        // the ranges of exact_topk_screened_run's passes: one block per compute unit, four rounds of them, a multiple of 8
        uint64_t G = (n + tile - 1) / tile;
        const uint64_t most = 1024u / tiles;
        if (G > most) G = most;
        if (G >= 8) G &= ~7ull;
        if (G < 1) G = 1;
        P.per_range = ((n + G - 1) / G + tile - 1) / tile * tile;
        HIP_TRY(ers_radius(i8, nullptr, d_radii + c0, qc, ix->dim, ets_epsilon(i8, ix->dim), (float*)(scratch + o_lo), (float*)(scratch + o_hi),
                           P.sure, P.cnt, P.bcnt, s));
        HIP_TRY(d_allowed ? ets_scan_radius_rows_list(form, tiles, (uint32_t)G, P, s) : ets_scan_radius_rows(form, tiles, (uint32_t)G, P, s));
        HIP_TRY(ers_pad(P.cand, P.sure, P.bcnt, P.list, qc, s));
        // the listed rows' distances in the reference's arithmetic, the queries read where the rows lie (a list: they lie
        // apart, and are gathered as rg_by_scan gathers them)
        const uint8_t* dq = P.elements + P.q_first * ix->row_stride;
        if (d_allowed) {
            HIP_TRY(ets_gather_rows(P.elements, ix->row_stride, qbytes, P.q_first, nullptr, 0u, qc, scratch + o_q, s, d_allowed));
            dq = scratch + o_q;
        }
        if (const int rc = dists_launch(ix, dq, nullptr, 2u * ET_CAP, P.cand, (uint64_t)qc * 2u * ET_CAP, dist, nullptr, s,
                                        d_allowed ? 0u : ix->row_stride))
            return rc;
        HIP_TRY(ers_keys(P.cand, dist, d_radii + c0, P.lo, P.hi, P.sure, P.bcnt, qc, c0, keys, (uint32_t*)(scratch + o_tot), lists, d_status, s));
        hipLaunchKernelGGL(er_rank_kernel, dim3(qc), dim3(ET_RANK_THREADS), 0, s, (const uint64_t*)keys, (const uint32_t*)(scratch + o_tot), c0, cap,
                           d_out_ids, d_out_dists, d_out_counts, d_out_totals, (uint32_t*)(scratch + o_dense), (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (d_status) HIP_TRY(ers_status(d_status, nullptr, 0u, form, s));
    uint32_t np[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(np, lists.n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // the entry's one wait of its own
    if (np[0]) // path B; er_rank_kernel has written the totals
        if (const int rc = rg_by_topk(ix, first, lists.b, np[0], cap, d_out_ids, d_out_dists, d_out_counts, d_status, s, d_filter, d_allowed))
            return rc;
    if (np[1]) { // path C, totals included
        uint32_t* const xs = (uint32_t*)(scratch + o_lo); // (the rounds are over: their thresholds' place)
        HIP_TRY(ets_clear(xs, 4u, s));
        if (const int rc = rg_by_scan(ix, first, lists.c, np[1], d_radii, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, xs, s, d_filter,
                                      d_allowed))
            return rc;
        if (d_status) HIP_TRY(ers_status(d_status, xs, 0u, 0u, s));
    }
    return GRANNE_HIP_OK;
}

// For e in [first, first + count): the elements x != e with dist(element e, x) <= d_radii[e - first] -- their exact number
// and the nearest min(total, cap) by (distance bits, id) -- into row e - first of the outputs. Ordered on `stream`.
extern "C" int granne_hip_range_graph_device(const granne_hip_index* ix, uint64_t first, uint64_t count, const float* d_radii, uint32_t cap,
                                             uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_totals,
                                             uint32_t* d_status, void* stream) {
    if (const int rc = range_graph_args(ix, first, count, cap, d_radii && d_out_ids && d_out_dists && d_out_counts && d_out_totals)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    return range_graph_run(ix, first, (uint32_t)count, d_radii, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, d_status,
                           (hipStream_t)stream);
}

// the same with host buffers in and out (synchronous); a NaN radius is refused here, where it can be seen;
// GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where exact_range itself gives it
extern "C" int granne_hip_range_graph(const granne_hip_index* ix, uint64_t first, uint64_t count, const float* radii, uint32_t cap,
                                      uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_totals, uint32_t* out_status) {
    if (const int rc = range_graph_args(ix, first, count, cap, radii && out_ids && out_dists && out_counts && out_totals)) return rc;
    if (count == 0) return GRANNE_HIP_OK;
    const uint32_t nq = (uint32_t)count;
    if (const uint32_t bad = range_first_nan(radii, nq); bad < nq)
        return fail(GRANNE_HIP_ERR_INVALID, "range_graph: the radius of element %llu is NaN", (unsigned long long)(first + bad));
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_ids = up((size_t)nq * 4), o_d = o_ids + up((size_t)nq * cap * 8), o_c = o_d + up((size_t)nq * cap * 4);
    const size_t o_t = o_c + up((size_t)nq * 4), o_st = o_t + up((size_t)nq * 4);
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the call left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, radii, (size_t)nq * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = range_graph_run(ix, first, nq, (const float*)buf, cap, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                       (uint32_t*)(buf + o_t), (uint32_t*)(buf + o_st), nullptr))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * cap * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_totals, buf + o_t, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "range_graph: %u elements have more than %u rows inside one second-level bin at their cap-th distance",
                    st[0], ET_CAP);
    return GRANNE_HIP_OK;
}
