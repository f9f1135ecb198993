// exact_topk_screened_host.h -- host side of the screened exact selection (included by granne_hip.hip after
// exact_topk_host.h): granne_hip_exact_topk_screened*, granne_hip_exact_topk_screen_epsilon[_long],
// granne_hip_index_screen_long_rows. The kernels and the method:
// exact_topk_screened.h; DESIGN.md 3.7b.
#pragma once

#include "exact_topk_screened.h"

static_assert(ETS_CAP == ET_CAP && sizeof(EtSel) == 16 && offsetof(EtSel, over) == 12, "ets_pad_kernel writes exact_topk's EtSel; one cap");

extern "C" float granne_hip_exact_topk_screen_epsilon(int dtype, uint32_t dim) {
    if (dtype != GRANNE_HIP_F32 && dtype != GRANNE_HIP_I8) return 0.0f;
    return ets_epsilon(dtype == GRANNE_HIP_I8, dim);
}

extern "C" float granne_hip_exact_topk_screen_epsilon_long(int dtype, uint32_t dim) {
    if (dtype != GRANNE_HIP_F32 && dtype != GRANNE_HIP_I8) return 0.0f;
    return ets_epsilon_long(dtype == GRANNE_HIP_I8, dim);
}

// the handle's dense-query screened entries screen long rows too (ets_form); a handle without such rows: accepted, no effect
extern "C" int granne_hip_index_screen_long_rows(granne_hip_index* ix, int on) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "screen_long_rows: index is null");
    ix->screen_long.store(on ? 1 : 0);
    return GRANNE_HIP_OK;
}

static int exact_topk_screened_args(const granne_hip_index* ix, uint32_t nq, uint32_t k, bool buffers) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_topk_screened");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_topk_screened");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened: null buffer");
    if (k == 0 || k > ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened: k must be in [1, %u]", ET_KMAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_screened takes up to 2^32 - 1 elements");
    return GRANNE_HIP_OK;
}

// The form that screens the handle's rows, or ETS_FORM_ROUTED: rows too long for the register forms, or f32 rows beyond
// the norm the bound is proven for. The largest squared norm is looked up once per handle (one pass over the rows and one
// wait on s, under norm_mu); every later call reads the verdict.
// Rows beyond the register forms: the long-row forms where the handle has asked for them
// (granne_hip_index_screen_long_rows) and the call's queries are dense (`dense_queries`; the graphs have no long-row form
// yet: they pass false and stay routed); ETS_FORM_ROUTED otherwise, as before.
static int ets_form(const granne_hip_index* ix, hipStream_t s, uint32_t* form, bool dense_queries) {
    *form = ETS_FORM_ROUTED;
    const bool long_ok = dense_queries && ix->screen_long.load() != 0 && ix->dim <= ETS_LONG_DIM_MAX;
    if (ix->dtype == GRANNE_HIP_I8) {
        if (ix->dim <= ETS_I8_DIM_MAX && ix->row_bytes <= 128u) *form = ETS_FORM_I8;
        else if (long_ok && ix->dim > ETS_I8_DIM_MAX && ix->row_bytes % ETS_LONG_CHUNK == 0u) *form = ETS_FORM_I8_LONG;
        return GRANNE_HIP_OK;
    }
    if (ix->dim > ETS_F32_DIM_MAX && !long_ok) return GRANNE_HIP_OK;
    granne_hip_index* mix = const_cast<granne_hip_index*>(ix);
    int verdict = mix->screen_rows.load();
    if (verdict == 0) {
        std::lock_guard<std::mutex> lk(mix->norm_mu);
        verdict = mix->screen_rows.load();
        if (verdict == 0) {
            uint32_t* d_max = nullptr;
            uint32_t bits = 0;
            HIP_TRY(hipMallocAsync((void**)&d_max, 4, s));
            hipError_t e = ets_clear(d_max, 1u, s);
            if (e == hipSuccess) e = ets_max_norm2(ix->d_elements.as<uint8_t>(), ix->n_elements, ix->row_bytes, ix->row_stride, d_max, s);
            if (e == hipSuccess) e = hipMemcpyAsync(&bits, d_max, 4, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            (void)hipFreeAsync(d_max, s);
            HIP_TRY(e);
            float worst;
            memcpy(&worst, &bits, 4);
            verdict = worst <= ets_norm2_test(ix->dim) ? 1 : 2; // (a NaN compares false)
            mix->screen_rows.store(verdict);
        }
    }
    if (verdict == 1) *form = ix->dim <= 112u ? ETS_FORM_B16_7x4 : ix->dim <= ETS_F32_DIM_MAX ? ETS_FORM_B16_13x2 : ETS_FORM_B16_LONG;
    return GRANNE_HIP_OK;
}

// int8: the rows' 1 / |x| are made with the index (make_scan_norms); a handle that has none yet gets them here, and the call
// waits for them once, since other streams may scan the handle next
static int ets_scan_norms(const granne_hip_index* ix, hipStream_t s) {
    if (ix->d_inv_norm) return GRANNE_HIP_OK;
    if (const int rc = make_scan_norms(const_cast<granne_hip_index*>(ix), s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return GRANNE_HIP_OK;
}

// the fallback list's queries under their own bitmaps (exact_topk_screened_filtered_host.h)
static int ets_fallback_bits(const granne_hip_index* ix, const uint8_t* d_fb_queries, const uint32_t* d_fb_list, uint32_t nfb, uint32_t k,
                             const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_ids, float* d_dists, uint32_t* d_counts,
                             uint32_t* d_xs, hipStream_t s, const float* d_fb_after_dists = nullptr, const uint64_t* d_fb_after_ids = nullptr);
// the handle's own rows first + p (p = d_list[f], or f where d_list is null; f < m) by exact_topk's scan with k + 1, the
// row itself dropped (knn_graph_host.h)
static int kg_by_scan(const granne_hip_index* ix, uint64_t first, const uint32_t* d_list, uint32_t m, uint32_t k, uint64_t* d_out_ids,
                      float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_xs, hipStream_t s, const uint32_t* d_filter = nullptr,
                      const uint32_t* d_allowed = nullptr);

// The selection on stream s, arguments checked, nq > 0. Everything is ordered on s; the call waits on s once, after the
// last round, for one word: the number of queries on the fallback list (and runs exact_topk's scan over them if any).
// d_filter (exact_topk_screened_filtered_host.h; null: all rows, and nothing below differs from the unfiltered call):
// filter_stride_words == 0 is one bitmap for every query, compacted here to its ascending id list, whose length m the call
// reads back once, at its start -- the prefixes and the grids are then made from m as they are made from n, and the
// kernels scan list positions (ETS_LIST); any other stride is one bitmap per query, tested in the kernels (ETS_BITS).
// What is handed to exact_topk_run, routed or on the fallback list, goes there with its filter.
// own_first (knn_graph_host.h; null: the caller's queries, and nothing below differs): the queries are the handle's own
// rows *own_first .. + nq - 1, d_queries and the filter are null, and the answer is every row's k nearest OTHER rows --
// the scans read their queries where the rows lie and take the diagonal out (ETS_Q_ROWS), dists_kernel strides over the
// rows, and what exact_topk's scan answers is asked for k + 1 and has the row itself dropped (kg_by_scan).
// own_first WITH one shared bitmap (graph_filtered_host.h): the caller has compacted the bitmap already --
// d_allowed is its id list of allowed_m >= 2 ids, nothing is compacted or read back here -- and the queries are the rows
// at the list's POSITIONS *own_first .. + nq - 1 (within allowed_m): the scans run over the list with their queries read
// through it (ETS_LIST with ETS_Q_ROWS, the diagonal a compare of positions), dists_kernel gets the round's query rows
// gathered dense, and kg_by_scan runs under the filter and drops the id at the position.
// d_after_ids (exact_topk_after_host.h; null: no cursor, and nothing below differs; never with own_first):
// with d_after_dists the queries' cursors. ets_init_after makes two more words per query, top_sure and top_any; the
// counting passes histogram the rows surely beyond the cursor, the collecting pass lists up to top_any, ets_keys_after
// keeps the candidates the exact arithmetic puts beyond the cursor, and whatever goes to exact_topk_run goes with its cursor.
static int exact_topk_screened_run(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_ids,
                                   float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, hipStream_t s,
                                   const uint32_t* d_filter = nullptr, uint64_t filter_stride_words = 0, const uint64_t* own_first = nullptr,
                                   const uint32_t* d_allowed = nullptr, uint64_t allowed_m = 0, const float* d_after_dists = nullptr,
                                   const uint64_t* d_after_ids = nullptr) {
    const bool after = d_after_ids != nullptr;
    GRANNE_HIP_ON_DEVICE(ix->device);
    uint32_t form = ETS_FORM_ROUTED;
    if (const int rc = ets_form(ix, s, &form, !own_first)) return rc;
    const int src = !d_filter ? ETS_ALL : filter_stride_words == 0 ? ETS_LIST : ETS_BITS;
    const bool list = src == ETS_LIST && form != ETS_FORM_ROUTED;
    uint64_t n = ix->n_elements; // ETS_LIST: the list's length, once it is known
    const bool i8 = ix->dtype == GRANNE_HIP_I8;
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qc_max = nq < ET_CHUNK ? nq : ET_CHUNK;
    // scratch: xs (exact_topk's status words for what is handed to it) and the fallback count; the fallback list; then a
    // round's floors, histograms, counts, EtSel words, candidates, their distances and their keys
    const size_t o_xs = 0, o_fbn = 16, o_fbl = 256, o_lo = o_fbl + up((size_t)nq * 4), o_hist = o_lo + up((size_t)qc_max * 4);
    const size_t o_cnt = o_hist + up((size_t)qc_max * ETS_BUCKETS * 4), o_sel = o_cnt + up((size_t)qc_max * 4);
    const size_t o_cand = o_sel + up((size_t)qc_max * sizeof(EtSel)), o_dist = o_cand + (size_t)qc_max * ET_CAP * 4;
    const size_t o_keys = o_dist + (size_t)qc_max * ET_CAP * 4;
    // ETS_LIST: the list's length (u64), the compaction's block counts, the list
    const size_t o_top = o_keys + (size_t)qc_max * ET_CAP * 8; // a cursor call: top_sure [qc], top_any [qc]
    const size_t o_m = o_top + up(after ? (size_t)qc_max * 8 : 0), o_blk = o_m + 256, o_list = o_blk + up(list ? (size_t)fl_blocks(n) * 4 : 0);
    // (the caller's list: a round's query rows, dense for dists_kernel, where the compaction's words would be)
    const size_t total = form == ETS_FORM_ROUTED ? 256 : d_allowed ? o_m + up((size_t)qc_max * qbytes) : list ? o_list + (size_t)n * 4 : o_m;
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, total, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() {
            if (p) (void)hipFreeAsync(p, s);
        }
    } release{scratch, s};
    uint32_t* const xs = (uint32_t*)(scratch + o_xs);
    HIP_TRY(ets_clear(xs, 8u, s)); // words 0..3: xs; word 4 (o_fbn = 16 bytes): the fallback count
    if (form == ETS_FORM_ROUTED) {
        if (own_first) {
            if (const int rc = kg_by_scan(ix, *own_first, nullptr, nq, k, d_out_ids, d_out_dists, d_out_counts, xs, s, d_filter, d_allowed)) return rc;
        } else if (const int rc = exact_topk_run(ix, d_queries, nq, k, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts, xs, s,
                                                 nullptr, nullptr, d_after_dists, d_after_ids))
            return rc;
        if (d_status) HIP_TRY(ets_status(d_status, nq, (uint32_t)ETS_FORM_ROUTED, xs, s));
        return GRANNE_HIP_OK;
    }
    if (d_allowed) n = allowed_m;
    else if (list) {
        if (const int rc = filter_compact<uint32_t>(d_filter, n, (uint32_t*)(scratch + o_blk), (uint32_t*)(scratch + o_list),
                                                    (uint64_t*)(scratch + o_m), nullptr, s))
            return rc;
        HIP_TRY(hipMemcpyAsync(&n, scratch + o_m, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n == 0) { // nothing is allowed: no scan
            HIP_TRY(ets_empty(nq, k, d_out_ids, d_out_dists, d_out_counts, s));
            if (d_status) HIP_TRY(ets_status(d_status, 0u, form, nullptr, s));
            return GRANNE_HIP_OK;
        }
    }
    if (i8)
        if (const int rc = ets_scan_norms(ix, s)) return rc;
    const uint64_t tile = ets_tile_rows(form);
    // the prefixes the floor is raised over, shortest first, the last one all rows (exact_topk's); one stage: counted twice
    uint64_t prefix[17];
    uint32_t stages = 0;
    {
        uint64_t rev[16], p = n;
        uint32_t m = 0;
        rev[m++] = p;
        while (p > 2ull * ET_PRIME_MIN && m < 16) {
            p /= ET_PRIME_STEP;
            if (p < ET_PRIME_MIN) p = ET_PRIME_MIN;
            rev[m++] = p;
        }
        while (m) prefix[stages++] = rev[--m];
        if (stages == 1) prefix[stages++] = n;
    }
    EtsParams P;
    P.elements = ix->d_elements.as<uint8_t>();
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
    P.inv_norm = i8 ? ix->d_inv_norm.as<float>() : nullptr;
    P.inv_gmax = i8 ? P.inv_norm + ((ix->n_elements + 31u) & ~31ull) : nullptr;
    P.lo = (const float*)(scratch + o_lo);
    P.hist = (uint32_t*)(scratch + o_hist);
    P.cnt = (uint32_t*)(scratch + o_cnt);
    P.cand = (uint32_t*)(scratch + o_cand);
    P.eps2 = 2.0f * ets_epsilon_of(form, i8, ix->dim);
    P.list = d_allowed ? d_allowed : list ? (const uint32_t*)(scratch + o_list) : nullptr;
    P.filter_stride = filter_stride_words;
    uint32_t* const fb_count = (uint32_t*)(scratch + o_fbn);
    uint32_t* const fb_list = (uint32_t*)(scratch + o_fbl);
    float* const top_sure = (float*)(scratch + o_top);
    float* const top_any = top_sure + qc_max;
    const float eps = ets_epsilon_of(form, i8, ix->dim);
    for (uint32_t c0 = 0; c0 < nq; c0 += ET_CHUNK) {
        const uint32_t qc = nq - c0 < ET_CHUNK ? nq - c0 : ET_CHUNK;
        const uint32_t tiles = (qc + ETS_QT - 1) / ETS_QT;
        P.queries = own_first ? nullptr : (const uint8_t*)d_queries + (size_t)c0 * qbytes;
        P.q_first = own_first ? *own_first + c0 : 0;
        P.nq = qc;
        P.filter = src == ETS_BITS ? d_filter + (size_t)c0 * filter_stride_words : nullptr;
        auto pass = [&](bool collect, uint64_t rows) -> int {
            // one block per compute unit (the tile and the histogram fill its LDS), four rounds of them; a multiple of 8
            // ranges so that the tiles of a range share an XCD (bf_block)
            uint64_t G = (rows + tile - 1) / tile;
            const uint64_t most = 1024u / tiles;
            if (G > most) G = most;
            if (G >= 8) G &= ~7ull;
            if (G < 1) G = 1;
            P.n = rows;
            P.per_range = ((rows + G - 1) / G + tile - 1) / tile * tile;
            P.tops = !after ? nullptr : collect ? top_any : top_sure;
            HIP_TRY(after       ? ets_scan_after(form, collect, src, tiles, (uint32_t)G, P, s)
                    : !own_first ? ets_scan_src(form, collect, src, tiles, (uint32_t)G, P, s)
                    : d_allowed ? ets_scan_rows_list(form, collect, tiles, (uint32_t)G, P, s)
                                : ets_scan_rows(form, collect, tiles, (uint32_t)G, P, s));
            return GRANNE_HIP_OK;
        };
        HIP_TRY(after ? ets_init_after(i8, P.queries, qc, ix->dim, eps, d_after_dists + c0, d_after_ids + c0, (float*)(scratch + o_lo), top_sure,
                                       top_any, P.hist, P.cnt, s)
                      : ets_init(i8, P.queries, qc, ix->dim, (float*)(scratch + o_lo), P.hist, P.cnt, s));
        for (uint32_t st = 0; st < stages; ++st) {
            if (const int rc = pass(false, prefix[st])) return rc;
            HIP_TRY(after ? ets_select_after(P.hist, qc, k, (float*)(scratch + o_lo), top_sure, s)
                          : ets_select(P.hist, qc, k, (float*)(scratch + o_lo), s));
        }
        if (const int rc = pass(true, n)) return rc;
        // the survivors' distances in the reference's arithmetic, then exact_topk's ranking by (distance bits, id)
        HIP_TRY(ets_pad(P.cand, P.cnt, P.lo, qc, c0, (uint32_t*)(scratch + o_sel), fb_count, fb_list, d_status, s));
        const uint8_t* dq = own_first ? P.elements + P.q_first * ix->row_stride : P.queries; // (a row is a prepared query)
        if (own_first && d_allowed) { // the rows at the round's positions lie apart: gathered, as kg_by_scan gathers them
            HIP_TRY(ets_gather_rows(P.elements, ix->row_stride, (uint32_t)qbytes, P.q_first, nullptr, 0u, qc, scratch + o_m, s, d_allowed));
            dq = scratch + o_m;
        }
        if (const int rc = dists_launch(ix, dq, nullptr, ET_CAP, P.cand, (uint64_t)qc * ET_CAP, (float*)(scratch + o_dist), nullptr, s,
                                        own_first && !d_allowed ? ix->row_stride : 0u))
            return rc;
        HIP_TRY(after ? ets_keys_after(P.cand, (const float*)(scratch + o_dist), P.cnt, qc, d_after_dists + c0, d_after_ids + c0,
                                       (uint64_t*)(scratch + o_keys), s)
                      : ets_keys(P.cand, (const float*)(scratch + o_dist), P.cnt, qc, (uint64_t*)(scratch + o_keys), s));
        hipLaunchKernelGGL(et_rank_kernel, dim3(qc), dim3(ET_RANK_THREADS), 0, s, (const uint64_t*)(scratch + o_keys), (const uint32_t*)P.cnt,
                           (const EtSel*)(scratch + o_sel), k, d_out_ids + (size_t)c0 * k, d_out_dists + (size_t)c0 * k, d_out_counts + c0,
                           (uint32_t*)nullptr, (uint32_t*)nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (d_status) HIP_TRY(ets_status(d_status, 0u, form, nullptr, s));
    uint32_t nfb = 0;
    HIP_TRY(hipMemcpyAsync(&nfb, fb_count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (nfb == 0) return GRANNE_HIP_OK;
    if (own_first) {
        if (const int rc = kg_by_scan(ix, *own_first, fb_list, nfb, k, d_out_ids, d_out_dists, d_out_counts, xs, s, d_filter, d_allowed)) return rc;
        if (d_status) HIP_TRY(ets_status(d_status, 0u, form, xs, s)); // (ETS_VOIDED where exact_topk voided one of them)
        return GRANNE_HIP_OK;
    }
    // the fallback: the listed queries by exact_topk's own scan (under their filter), the answers into their places
    const size_t f_ids = up((size_t)nfb * qbytes), f_d = f_ids + (size_t)nfb * k * 8, f_c = f_d + up((size_t)nfb * k * 4);
    const size_t f_ai = up(f_c + (size_t)nfb * 4), f_ad = f_ai + (size_t)nfb * 8; // their cursors, gathered alongside
    uint8_t* fb = nullptr;
    HIP_TRY(hipMallocAsync((void**)&fb, after ? f_ad + (size_t)nfb * 4 : f_c + (size_t)nfb * 4, s));
    Release release_fb{fb, s};
    HIP_TRY(ets_gather((const uint8_t*)d_queries, (uint32_t)qbytes, fb_list, nfb, fb, s));
    const float* fb_ad = nullptr;
    const uint64_t* fb_ai = nullptr;
    if (after) {
        HIP_TRY(ets_gather((const uint8_t*)d_after_ids, 8u, fb_list, nfb, fb + f_ai, s));
        HIP_TRY(ets_gather((const uint8_t*)d_after_dists, 4u, fb_list, nfb, fb + f_ad, s));
        fb_ad = (const float*)(fb + f_ad), fb_ai = (const uint64_t*)(fb + f_ai);
    }
    if (src != ETS_BITS) {
        if (const int rc = exact_topk_run(ix, fb, nfb, k, d_filter, 0, (uint64_t*)(fb + f_ids), (float*)(fb + f_d), (uint32_t*)(fb + f_c), xs, s,
                                          nullptr, nullptr, fb_ad, fb_ai))
            return rc;
    } else if (const int rc = ets_fallback_bits(ix, fb, fb_list, nfb, k, d_filter, filter_stride_words, (uint64_t*)(fb + f_ids), (float*)(fb + f_d),
                                                (uint32_t*)(fb + f_c), xs, s, fb_ad, fb_ai))
        return rc;
    HIP_TRY(ets_scatter(fb_list, nfb, k, (const uint64_t*)(fb + f_ids), (const float*)(fb + f_d), (const uint32_t*)(fb + f_c), xs, d_out_ids,
                        d_out_dists, d_out_counts, d_status, s));
    return GRANNE_HIP_OK;
}

// exact_topk's answer, the matrix cores screening the rows first (exact_topk_screened.h)
extern "C" int granne_hip_exact_topk_screened_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                                     uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status,
                                                     void* stream) {
    if (const int rc = exact_topk_screened_args(ix, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_screened_run(ix, d_queries, nq, k, d_out_ids, d_out_dists, d_out_counts, d_status, (hipStream_t)stream);
}

// host buffers in and out; GRANNE_HIP_ERR_OVERFLOW (outputs and status still written) where exact_topk itself would give it
extern "C" int granne_hip_exact_topk_screened(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k, uint64_t* out_ids,
                                              float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = exact_topk_screened_args(ix, nq, k, queries && out_ids && out_dists && out_counts)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t o_ids = up(qb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4), o_st = o_c + up((size_t)nq * 4);
    DevBuf block;
    HIP_TRY(block.alloc(o_st + 16));
    struct Settle { // (declared after the block: whatever the passes left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    if (const int rc = exact_topk_screened_run(ix, buf, nq, k, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c),
                                               (uint32_t*)(buf + o_st), nullptr))
        return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[3] & ETS_VOIDED)
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_topk_screened: exact_topk's own selection overflowed for a query handed to it (more than %u rows "
                    "inside one second-level bin at its k-th distance)", ET_CAP);
    return GRANNE_HIP_OK;
}
