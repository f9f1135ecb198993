// exact_range_screened_host.h -- granne_hip_exact_range_screened*: exact_range's answer with the matrix cores screening
// the rows first (included by granne_hip.hip after exact_topk_screened_filtered_host.h; the scan is exact_topk_screened.h's
// with its third epilogue, ETS_RADIUS). A radius is a floor known before the scan: one pass over the rows,
// no priming prefixes, no histogram. Per query the pass leaves S, the exact number of rows whose score vouches for d <= r,
// the first ETS_CAP of their ids, and the B rows of the band, which only the reference's arithmetic can decide.
//
//   A  total = S + (band rows with d <= r) <= ETS_CAP: both lists are whole; their keys within r are ranked (er_rank_kernel)
//   B  total > ETS_CAP, B <= ETS_CAP: the total is exact without a second scan, and the cap nearest rows all lie within r:
//      they are exact_topk_screened's answer for k = cap under the same filter
//   C  B > ETS_CAP (masses of copies at the border) or an f32 query outside the norm bound: exact_range_run
// A is exact_range's own phase A condition and B its phase B, so a query is voided by exact_topk's overflow here exactly
// when exact_range voids it. The call waits on its stream once for two words, the numbers of B and C queries (a shared
// bitmap: once more at its start, for the length of its id list, as exact_topk_screened_filtered).
#pragma once

#include "exact_topk_screened_filtered_host.h"

static_assert(GRANNE_HIP_ETS_FORM_ROUTED == ETS_FORM_ROUTED && GRANNE_HIP_ETS_FORM_B16_7x4 == ETS_FORM_B16_7x4 &&
                  GRANNE_HIP_ETS_FORM_B16_13x2 == ETS_FORM_B16_13x2 && GRANNE_HIP_ETS_FORM_I8 == ETS_FORM_I8 && GRANNE_HIP_ETS_FORM_B16_LONG == ETS_FORM_B16_LONG &&
                  GRANNE_HIP_ETS_FORM_I8_LONG == ETS_FORM_I8_LONG && GRANNE_HIP_ETS_VOIDED == ETS_VOIDED,
              "the status words granne_hip.h declares");

// exact_range_args under this entry's name
static int exact_range_screened_args(const granne_hip_index* ix, uint32_t nq, uint32_t cap, bool buffers, const void* filter,
                                     uint64_t filter_stride_words) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_range_screened");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_range_screened");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened: null buffer");
    if (cap == 0 || cap > ER_CAP_MAX) return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened: cap (%u) must be in [1, %u]", cap, ER_CAP_MAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened takes up to 2^32 - 1 elements");
    if (filter && filter_stride_words && filter_stride_words < filter_words(ix->n_elements))
        return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened: filter_stride_words (%llu) must be 0 or at least ceil(n_elements / 32) = %llu",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(ix->n_elements));
    return GRANNE_HIP_OK;
}

// run(first, count, filter, stride) over the np queries listed in d_list (dense, in the list's order), under the call's
// filter: null or one shared bitmap in one call; one bitmap per query: the listed queries' bitmaps gathered a bounded
// number (256 MiB) at a time, as exact_range_run's phase B gathers them
template <class Run>
static int ers_under_filter(const granne_hip_index* ix, const uint32_t* d_filter, uint64_t filter_stride_words, const uint32_t* d_list, uint32_t np,
                            hipStream_t s, Run run) {
    if (!d_filter || filter_stride_words == 0) return run(0u, np, d_filter, (uint64_t)0);
    const uint64_t words = filter_words(ix->n_elements);
    uint64_t chunk = (256ull << 20) / (words * 4u);
    if (chunk < 1) chunk = 1;
    if (chunk > np) chunk = np;
    PfStreamMem maps;
    HIP_TRY(maps.alloc((size_t)chunk * words * 4, s));
    for (uint32_t c0 = 0; c0 < np; c0 += (uint32_t)chunk) {
        const uint32_t qc = np - c0 < chunk ? np - c0 : (uint32_t)chunk;
        if (const int rc = pf_gather_rows(d_filter, filter_stride_words * 4u, d_list + c0, qc, words * 4u, maps.p, s)) return rc;
        if (const int rc = run(c0, qc, maps.as<uint32_t>(), words)) return rc;
    }
    return GRANNE_HIP_OK;
}

static int ers_scatter(const uint8_t* f, size_t o_d, size_t o_c, const uint32_t* d_found, const uint32_t* d_list, uint32_t np, uint32_t cap,
                       uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_found, hipStream_t s) {
    uint64_t blocks = ((uint64_t)np * cap + 255u) / 256u;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(er_scatter_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint64_t*)f, (const float*)(f + o_d), (const uint32_t*)(f + o_c),
                       d_found, d_list, np, cap, d_out_ids, d_out_dists, d_out_counts, d_out_found, (uint32_t*)nullptr, 0u, (const uint32_t*)nullptr, 0u,
                       (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// The call on stream s, arguments checked, nq > 0; the filter as exact_range_run's. d_status optional.
static int exact_range_screened_run(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii, uint32_t cap,
                                    const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists,
                                    uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status, hipStream_t s) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    uint32_t form = ETS_FORM_ROUTED;
    if (const int rc = ets_form(ix, s, &form, true)) return rc;
    const bool i8 = ix->dtype == GRANNE_HIP_I8;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    if (form == ETS_FORM_ROUTED) { // no screen for the handle: the whole call is exact_range's
        PfStreamMem xs;
        HIP_TRY(xs.alloc(16, s));
        HIP_TRY(ets_clear(xs.as<uint32_t>(), 4u, s));
        if (const int rc = exact_range_run(ix, d_queries, nq, d_radii, cap, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts,
                                           d_out_totals, xs.as<uint32_t>(), s))
            return rc;
        if (d_status) HIP_TRY(ers_status(d_status, xs.as<uint32_t>(), nq, (uint32_t)ETS_FORM_ROUTED, s));
        return GRANNE_HIP_OK;
    }
    const int src = !d_filter ? ETS_ALL : filter_stride_words == 0 ? ETS_LIST : ETS_BITS;
    const bool list = src == ETS_LIST;
    uint64_t n = ix->n_elements; // ETS_LIST: the list's length, once it is known
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    const uint32_t qc_max = nq < ET_CHUNK ? nq : ET_CHUNK;
    // scratch: the numbers of B and C queries and er_rank_kernel's bitmap over the call's queries (cleared together); the
    // two lists; a round's thresholds, counters and totals, its id lists [qc][2][ET_CAP], their distances, the keys; the
    // shared bitmap's list (length, block counts, ids)
    const size_t o_n = 0, o_dense = 256, o_lb = o_dense + up((size_t)filter_words(nq) * 4), o_lc = o_lb + up((size_t)nq * 4);
    const size_t o_lo = o_lc + up((size_t)nq * 4), w = up((size_t)qc_max * 4), o_hi = o_lo + w, o_sure = o_hi + w, o_cnt = o_sure + w;
    const size_t o_bcnt = o_cnt + w, o_tot = o_bcnt + w, o_cand = o_tot + w, o_dist = o_cand + (size_t)qc_max * 2 * ET_CAP * 4;
    const size_t o_keys = o_dist + (size_t)qc_max * 2 * ET_CAP * 4, o_m = o_keys + (size_t)qc_max * ET_CAP * 8, o_blk = o_m + 256;
    const size_t o_list = o_blk + up(list ? (size_t)fl_blocks(n) * 4 : 0), total = o_list + (list ? (size_t)n * 4 : 0);
    PfStreamMem mem;
    HIP_TRY(mem.alloc(total, s));
    uint8_t* const scratch = mem.as<uint8_t>();
    HIP_TRY(ets_clear((uint32_t*)(scratch + o_n), 64u + (uint32_t)filter_words(nq), s));
    if (list) {
        if (const int rc = filter_compact<uint32_t>(d_filter, n, (uint32_t*)(scratch + o_blk), (uint32_t*)(scratch + o_list),
                                                    (uint64_t*)(scratch + o_m), nullptr, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(&n, scratch + o_m, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n == 0) { // nothing is allowed: no scan
            HIP_TRY(ets_empty(nq, cap, d_out_ids, d_out_dists, d_out_counts, s));
            HIP_TRY(ets_clear(d_out_totals, nq, s));
            if (d_status) HIP_TRY(ers_status(d_status, nullptr, 0u, form, s));
            return GRANNE_HIP_OK;
        }
    }
    if (i8)
        if (const int rc = ets_scan_norms(ix, s)) return rc;
    const uint64_t tile = ets_tile_rows(form);
    EtsParams P;
    P.elements = ix->d_elements.as<uint8_t>();
    P.n = n;
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
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
    P.list = list ? (const uint32_t*)(scratch + o_list) : nullptr;
    P.filter_stride = filter_stride_words;
    const ErsLists lists{(uint32_t*)(scratch + o_n), (uint32_t*)(scratch + o_lb), (uint32_t*)(scratch + o_lc)};
    float* const dist = (float*)(scratch + o_dist);
    uint64_t* const keys = (uint64_t*)(scratch + o_keys);
    for (uint32_t c0 = 0; c0 < nq; c0 += ET_CHUNK) {
        const uint32_t qc = nq - c0 < ET_CHUNK ? nq - c0 : ET_CHUNK;
        const uint32_t tiles = (qc + ETS_QT - 1) / ETS_QT;
        P.queries = (const uint8_t*)d_queries + (size_t)c0 * qbytes;
        P.nq = qc;
        P.filter = src == ETS_BITS ? d_filter + (size_t)c0 * filter_stride_words : nullptr;
        // the ranges of exact_topk_screened_run's passes: one block per compute unit, four rounds of them, a multiple of 8
        uint64_t G = (n + tile - 1) / tile;
        const uint64_t most = 1024u / tiles;
        if (G > most) G = most;
        if (G >= 8) G &= ~7ull;
        if (G < 1) G = 1;
        P.per_range = ((n + G - 1) / G + tile - 1) / tile * tile;
        HIP_TRY(ers_radius(i8, P.queries, d_radii + c0, qc, ix->dim, ets_epsilon_of(form, i8, ix->dim), (float*)(scratch + o_lo), (float*)(scratch + o_hi),
                           P.sure, P.cnt, P.bcnt, s));
        HIP_TRY(ets_scan_radius(form, src, tiles, (uint32_t)G, P, s));
        HIP_TRY(ers_pad(P.cand, P.sure, P.bcnt, P.list, qc, s));
        if (const int rc = dists_launch(ix, P.queries, nullptr, 2u * ET_CAP, P.cand, (uint64_t)qc * 2u * ET_CAP, dist, nullptr, s)) return rc;
        HIP_TRY(ers_keys(P.cand, dist, d_radii + c0, P.lo, P.hi, P.sure, P.bcnt, qc, c0, keys, (uint32_t*)(scratch + o_tot), lists, d_status, s));
        hipLaunchKernelGGL(er_rank_kernel, dim3(qc), dim3(ET_RANK_THREADS), 0, s, (const uint64_t*)keys, (const uint32_t*)(scratch + o_tot), c0, cap,
                           d_out_ids, d_out_dists, d_out_counts, d_out_totals, (uint32_t*)(scratch + o_dense), (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (d_status) HIP_TRY(ers_status(d_status, nullptr, 0u, form, s));
    uint32_t np[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(np, lists.n, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // the entry's one wait
    if (np[0]) { // path B: exact_topk_screened(k = cap); er_rank_kernel has written the totals
        const uint32_t nb = np[0];
        const size_t o_d = up((size_t)nb * cap * 8), o_c = o_d + up((size_t)nb * cap * 4), o_q = o_c + up((size_t)nb * 4);
        PfStreamMem fb;
        HIP_TRY(fb.alloc(o_q + (size_t)nb * qbytes, s));
        uint8_t* const f = fb.as<uint8_t>();
        if (const int rc = pf_gather_rows(d_queries, qbytes, lists.b, nb, qbytes, f + o_q, s)) return rc;
        if (const int rc = ers_under_filter(ix, d_filter, filter_stride_words, lists.b, nb, s,
                                            [&](uint32_t c0, uint32_t qc, const uint32_t* filter, uint64_t stride) {
                                                return exact_topk_screened_run(ix, f + o_q + (size_t)c0 * qbytes, qc, cap, (uint64_t*)f + (size_t)c0 * cap,
                                                                               (float*)(f + o_d) + (size_t)c0 * cap, (uint32_t*)(f + o_c) + c0, nullptr, s,
                                                                               filter, stride);
                                            }))
            return rc;
        if (const int rc = ers_scatter(f, o_d, o_c, nullptr, lists.b, nb, cap, d_out_ids, d_out_dists, d_out_counts, nullptr, s)) return rc;
        // at least cap rows lie within the radius: a count of 0 is a query voided by exact_topk's overflow
        if (d_status) HIP_TRY(ers_voided((const uint32_t*)(f + o_c), nb, d_status, s));
    }
    if (np[1]) { // path C: exact_range's own scan, totals included
        const uint32_t nc = np[1];
        const size_t o_d = up((size_t)nc * cap * 8), o_c = o_d + up((size_t)nc * cap * 4), o_t = o_c + up((size_t)nc * 4);
        const size_t o_r = o_t + up((size_t)nc * 4), o_xs = o_r + up((size_t)nc * 4), o_q = o_xs + 256;
        PfStreamMem fb;
        HIP_TRY(fb.alloc(o_q + (size_t)nc * qbytes, s));
        uint8_t* const f = fb.as<uint8_t>();
        HIP_TRY(ets_clear((uint32_t*)(f + o_xs), 4u, s));
        if (const int rc = pf_gather_rows(d_queries, qbytes, lists.c, nc, qbytes, f + o_q, s)) return rc;
        if (const int rc = pf_gather_rows(d_radii, 4, lists.c, nc, 4, f + o_r, s)) return rc;
        if (const int rc = ers_under_filter(ix, d_filter, filter_stride_words, lists.c, nc, s,
                                            [&](uint32_t c0, uint32_t qc, const uint32_t* filter, uint64_t stride) {
                                                return exact_range_run(ix, f + o_q + (size_t)c0 * qbytes, qc, (const float*)(f + o_r) + c0, cap, filter, stride,
                                                                       (uint64_t*)f + (size_t)c0 * cap, (float*)(f + o_d) + (size_t)c0 * cap,
                                                                       (uint32_t*)(f + o_c) + c0, (uint32_t*)(f + o_t) + c0, (uint32_t*)(f + o_xs), s);
                                            }))
            return rc;
        if (const int rc = ers_scatter(f, o_d, o_c, (const uint32_t*)(f + o_t), lists.c, nc, cap, d_out_ids, d_out_dists, d_out_counts, d_out_totals, s))
            return rc;
        if (d_status) HIP_TRY(ers_status(d_status, (const uint32_t*)(f + o_xs), 0u, 0u, s));
    }
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_exact_range_screened_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii,
                                                      uint32_t cap, const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids,
                                                      float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status,
                                                      void* stream) {
    if (const int rc = exact_range_screened_args(ix, nq, cap, d_queries && d_radii && d_out_ids && d_out_dists && d_out_counts && d_out_totals,
                                                 d_filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_range_screened_run(ix, d_queries, nq, d_radii, cap, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts,
                                    d_out_totals, d_status, (hipStream_t)stream);
}

// the same with host buffers in and out (synchronous); a NaN radius is refused here, where it can be seen;
// GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where exact_range itself gives it
extern "C" int granne_hip_exact_range_screened(const granne_hip_index* ix, const void* queries, uint32_t nq, const float* radii, uint32_t cap,
                                               const uint32_t* filter, uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists,
                                               uint32_t* out_counts, uint32_t* out_totals, uint32_t* out_status) {
    if (const int rc = exact_range_screened_args(ix, nq, cap, queries && radii && out_ids && out_dists && out_counts && out_totals, filter,
                                                 filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (const uint32_t bad = range_first_nan(radii, nq); bad < nq)
        return fail(GRANNE_HIP_ERR_INVALID, "exact_range_screened: the radius of query %u is NaN", bad);
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t fb = !filter ? 0 : (filter_stride_words ? (size_t)nq * filter_stride_words : (size_t)filter_words(ix->n_elements)) * 4;
    const size_t o_r = up(qb), o_f = o_r + up((size_t)nq * 4), o_ids = o_f + up(fb), o_d = o_ids + up((size_t)nq * cap * 8);
    const size_t o_c = o_d + up((size_t)nq * cap * 4), o_t = o_c + up((size_t)nq * 4), o_st = o_t + up((size_t)nq * 4), total = o_st + 16;
    DevBuf block;
    HIP_TRY(block.alloc(total));
    struct Settle { // (declared after the block: whatever the call left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(buf + o_r, radii, (size_t)nq * 4, hipMemcpyHostToDevice));
    if (filter) HIP_TRY(hipMemcpy(buf + o_f, filter, fb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = exact_range_screened_run(ix, buf, nq, (const float*)(buf + o_r), cap, filter ? (const uint32_t*)(buf + o_f) : nullptr,
                                                filter_stride_words, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
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
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_range_screened: %u queries have more than %u rows inside one second-level bin at their cap-th "
                    "distance", st[0], ET_CAP);
    return GRANNE_HIP_OK;
}
