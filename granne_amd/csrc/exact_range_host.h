// exact_range_host.h -- host side of the exact range search (included by granne_hip.hip after postfilter_host.h):
// granne_hip_exact_range* give every element within a radius of every query -- the exact count and the nearest `cap` of
// them -- over all rows or the rows an id bitmap allows (exact_range.h). One driver (exact_range_run) and
// one host staging serve both entries; range_host.h's exact fallback calls the driver too.
//
// Phase A is stream-ordered. The entry then WAITS on the stream ONCE: the number of queries with more than ET_CAP rows
// within their radius (one u32) comes back; 0 ends the call, otherwise phase B runs exact_topk_run(k = cap) for them.
#pragma once

#include "exact_range.h"

// The argument checks, in exact_topk_args' order. `buffers`: every required pointer is there.
static int exact_range_args(const granne_hip_index* ix, uint32_t nq, uint32_t cap, bool buffers, const void* filter, uint64_t filter_stride_words) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "exact_range: index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_range");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_range");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "exact_range: null buffer");
    if (cap == 0 || cap > ER_CAP_MAX) return fail(GRANNE_HIP_ERR_INVALID, "exact_range: cap (%u) must be in [1, %u]", cap, ER_CAP_MAX);
    if (ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "exact_range takes up to 2^32 - 1 elements");
    if (filter && filter_stride_words && filter_stride_words < filter_words(ix->n_elements))
        return fail(GRANNE_HIP_ERR_INVALID, "exact_range: filter_stride_words (%llu) must be 0 or at least ceil(n_elements / 32) = %llu",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(ix->n_elements));
    return GRANNE_HIP_OK;
}

// the first NaN among nq host radii, or nq
static uint32_t range_first_nan(const float* radii, uint32_t nq) {
    for (uint32_t q = 0; q < nq; ++q)
        if (radii[q] != radii[q]) return q;
    return nq;
}

// The call on stream s, arguments checked, nq > 0. The filter as exact_topk_run's: null, one bitmap (stride 0) or one per
// query. d_status optional.
static int exact_range_run(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii, uint32_t cap,
                           const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists,
                           uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status, hipStream_t s) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    const uint64_t n = ix->n_elements;
    const bool i8 = ix->dtype == GRANNE_HIP_I8;
    const EtSrc src = !d_filter ? ET_ALL : filter_stride_words == 0 ? ET_LIST : ET_BITS;
    const bool list = src == ET_LIST;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qc_max = nq < ET_CHUNK ? nq : ET_CHUNK;
    // scratch: the candidates [qc][ET_CAP], totals [qc] and slots [qc] (zeroed together); the shared bitmap's list (length,
    // block counts, ids); the dense bitmap over the call's queries, its compaction's block counts, list and count
    const size_t o_tot = (size_t)qc_max * ET_CAP * 8, o_cnt = o_tot + (size_t)qc_max * 4, o_m = up(o_cnt + (size_t)qc_max * 4);
    const size_t o_blk = o_m + 256, o_list = o_blk + up(list ? (size_t)fl_blocks(n) * 4 : 0), o_dense = o_list + up(list ? (size_t)n * 4 : 0);
    const size_t o_dblk = o_dense + up((size_t)filter_words(nq) * 4), o_dlist = o_dblk + up((size_t)fl_blocks(nq) * 4);
    const size_t o_dcnt = o_dlist + up((size_t)nq * 4), total = o_dcnt + 16;
    PfStreamMem mem;
    HIP_TRY(mem.alloc(total, s));
    uint8_t* const scratch = mem.as<uint8_t>();
    if (list)
        if (const int rc = filter_compact<uint32_t>(d_filter, n, (uint32_t*)(scratch + o_blk), (uint32_t*)(scratch + o_list),
                                                    (uint64_t*)(scratch + o_m), d_status ? d_status + 3 : nullptr, s))
            return rc;
    uint32_t* const d_dense = (uint32_t*)(scratch + o_dense);
    HIP_TRY(hipMemsetAsync(d_dense, 0, (size_t)filter_words(nq) * 4, s));
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    const bool resident = ix->row_bytes <= 1024u;
    ErParams P;
    P.elements = ix->d_elements.as<uint8_t>();
    P.rows = n;
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
    P.q_lds = resident ? ix->row_bytes : 0u;
    P.totals = (uint32_t*)(scratch + o_tot);
    P.cnt = (uint32_t*)(scratch + o_cnt);
    P.cand = (uint64_t*)scratch;
    P.list = list ? (const uint32_t*)(scratch + o_list) : nullptr;
    P.m = list ? (const uint64_t*)(scratch + o_m) : nullptr;
    P.filter_stride = filter_stride_words;
    const uint32_t lds = ET_QT * P.q_lds;
    for (uint32_t c0 = 0; c0 < nq; c0 += ET_CHUNK) { // phase A
        const uint32_t qc = nq - c0 < ET_CHUNK ? nq - c0 : ET_CHUNK;
        const uint32_t tiles = (qc + ET_QT - 1) / ET_QT;
        uint64_t G = (n + ET_GROUPS - 1) / ET_GROUPS; // the row ranges, as exact_topk_run's passes
        const uint64_t most = 2048u / tiles ? 2048u / tiles : 1u;
        if (G > most) G = most;
        if (G < 1) G = 1;
        P.per_range = ((n + G - 1) / G + ET_GROUPS - 1) / ET_GROUPS * ET_GROUPS;
        if (P.per_range < ET_GROUPS) P.per_range = ET_GROUPS;
        P.queries = (const uint8_t*)d_queries + (size_t)c0 * qbytes;
        P.nq = qc;
        P.radii = d_radii + c0;
        P.filter = src == ET_BITS ? d_filter + (size_t)c0 * filter_stride_words : nullptr;
        HIP_TRY(hipMemsetAsync(scratch + o_tot, 0, (size_t)qc_max * 8, s)); // totals and slots
        hipLaunchKernelGGL(er_scan_fn(i8, ix->row_bytes, src), dim3(tiles, (uint32_t)G), dim3(ET_THREADS), lds, s, P);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(er_rank_kernel, dim3(qc), dim3(ET_RANK_THREADS), 0, s, (const uint64_t*)scratch, (const uint32_t*)(scratch + o_tot), c0, cap,
                           d_out_ids, d_out_dists, d_out_counts, d_out_totals, d_dense, d_status);
        HIP_TRY(hipGetLastError());
    }
    uint32_t* const d_list = (uint32_t*)(scratch + o_dlist);
    if (const int rc = filter_compact<uint32_t>(d_dense, nq, (uint32_t*)(scratch + o_dblk), d_list, (uint64_t*)(scratch + o_dcnt),
                                                (uint32_t*)(scratch + o_dcnt + 8), s))
        return rc;
    uint32_t np = 0;
    HIP_TRY(hipMemcpyAsync(&np, scratch + o_dcnt + 8, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // the entry's one wait
    if (np == 0) return GRANNE_HIP_OK;
    // phase B: exact_topk_run(k = cap) for the np dense queries of d_list, answers scattered to their rows
    const size_t o_fd = up((size_t)np * cap * 8), o_fc = o_fd + up((size_t)np * cap * 4), o_fs = o_fc + up((size_t)np * 4);
    const size_t o_fq = o_fs + 256, fb_total = o_fq + (size_t)np * qbytes;
    PfStreamMem fb;
    HIP_TRY(fb.alloc(fb_total, s));
    uint8_t* const f = fb.as<uint8_t>();
    HIP_TRY(hipMemsetAsync(f + o_fs, 0, 16, s));
    if (const int rc = pf_gather_rows(d_queries, qbytes, d_list, np, qbytes, f + o_fq, s)) return rc;
    if (src != ET_BITS) {
        if (const int rc = exact_topk_run(ix, f + o_fq, np, cap, d_filter, 0, (uint64_t*)f, (float*)(f + o_fd), (uint32_t*)(f + o_fc),
                                          (uint32_t*)(f + o_fs), s))
            return rc;
    } else { // one bitmap per query: the dense queries' bitmaps, gathered a bounded number (256 MiB) at a time
        const uint64_t words = filter_words(n);
        uint64_t chunk = (256ull << 20) / (words * 4u);
        if (chunk < 1) chunk = 1;
        if (chunk > np) chunk = np;
        PfStreamMem maps;
        HIP_TRY(maps.alloc((size_t)chunk * words * 4, s));
        for (uint32_t c0 = 0; c0 < np; c0 += (uint32_t)chunk) {
            const uint32_t qc = np - c0 < chunk ? np - c0 : (uint32_t)chunk;
            if (const int rc = pf_gather_rows(d_filter, filter_stride_words * 4u, d_list + c0, qc, words * 4u, maps.p, s)) return rc;
            if (const int rc = exact_topk_run(ix, f + o_fq + (size_t)c0 * qbytes, qc, cap, maps.as<uint32_t>(), words, (uint64_t*)f + (size_t)c0 * cap,
                                              (float*)(f + o_fd) + (size_t)c0 * cap, (uint32_t*)(f + o_fc) + c0, (uint32_t*)(f + o_fs), s))
                return rc;
        }
    }
    uint64_t blocks = ((uint64_t)np * cap + 255u) / 256u;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(er_scatter_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint64_t*)f, (const float*)(f + o_fd),
                       (const uint32_t*)(f + o_fc), (const uint32_t*)nullptr, (const uint32_t*)d_list, np, cap, d_out_ids, d_out_dists, d_out_counts,
                       (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (const uint32_t*)(f + o_fs), 1u, d_status);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_exact_range_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii, uint32_t cap,
                                             const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists,
                                             uint32_t* d_out_counts, uint32_t* d_out_totals, uint32_t* d_status, void* stream) {
    if (const int rc = exact_range_args(ix, nq, cap, d_queries && d_radii && d_out_ids && d_out_dists && d_out_counts && d_out_totals, d_filter,
                                        filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_range_run(ix, d_queries, nq, d_radii, cap, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts, d_out_totals,
                           d_status, (hipStream_t)stream);
}

// the same with host buffers in and out (synchronous); a NaN radius is refused here, where it can be seen
extern "C" int granne_hip_exact_range(const granne_hip_index* ix, const void* queries, uint32_t nq, const float* radii, uint32_t cap,
                                      const uint32_t* filter, uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists,
                                      uint32_t* out_counts, uint32_t* out_totals, uint32_t* out_status) {
    if (const int rc = exact_range_args(ix, nq, cap, queries && radii && out_ids && out_dists && out_counts && out_totals, filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (const uint32_t bad = range_first_nan(radii, nq); bad < nq)
        return fail(GRANNE_HIP_ERR_INVALID, "exact_range: the radius of query %u is NaN", bad);
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
    const int rc = exact_range_run(ix, buf, nq, (const float*)(buf + o_r), cap, filter ? (const uint32_t*)(buf + o_f) : nullptr, filter_stride_words,
                                   (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c), (uint32_t*)(buf + o_t),
                                   (uint32_t*)(buf + o_st), nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * cap * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_totals, buf + o_t, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "exact_range: %u queries have more than %u rows inside one second-level bin at their cap-th distance",
                    st[0], ET_CAP);
    return GRANNE_HIP_OK;
}
