// exact_topk_host.h -- host side of the exact selection (included by granne_hip.hip): granne_hip_exact_topk* over all rows,
// granne_hip_exact_topk_filtered* over the rows an id bitmap allows -- the compacted list for one shared bitmap, all rows
// under a bit test for per-query bitmaps (exact_topk.h, sources) -- and
// granne_hip_filter_to_ids_device, the compaction alone (filter.h, fl_*). One driver (exact_topk_run) and one host staging
// (exact_topk_staged) serve the four entries; a null filter means all rows.
#pragma once

#include "exact_topk.h"

// bitmap -> ids on stream s: counts (u32[fl_blocks(n)], scratch) end as the blocks' offsets; *d_count the number of ids
template <typename ID>
static int filter_compact(const uint32_t* d_filter, uint64_t n, uint32_t* d_counts, ID* d_out, uint64_t* d_count, uint32_t* d_count32,
                          hipStream_t s) {
    const uint32_t blocks = (uint32_t)fl_blocks(n);
    hipLaunchKernelGGL(fl_count_kernel, dim3(blocks), dim3(FL_THREADS), 0, s, d_filter, n, d_counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fl_scan_kernel, dim3(1), dim3(FL_SCAN_THREADS), 0, s, d_counts, blocks, d_count, d_count32);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fl_scatter_kernel<ID>, dim3(blocks), dim3(FL_THREADS), 0, s, d_filter, n, (const uint32_t*)d_counts, d_out);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_filter_to_ids_device(const uint32_t* d_filter, uint64_t n_elements, uint64_t* d_out_ids, uint64_t* d_out_count,
                                               int device_id, void* stream) {
    if (!d_out_count) return fail(GRANNE_HIP_ERR_INVALID, "filter_to_ids: out_count is null");
    if (n_elements && (!d_filter || !d_out_ids)) return fail(GRANNE_HIP_ERR_INVALID, "filter_to_ids: null buffer");
    if (n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "filter_to_ids takes bitmaps over up to 2^32 - 1 ids");
    static_assert(((0xFFFFFFFFull + 31u) / 32u + FL_BLOCK_WORDS - 1) / FL_BLOCK_WORDS <= FL_MAX_BLOCKS, "one block scans the block counts");
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = (hipStream_t)stream;
    if (n_elements == 0) {
        HIP_TRY(hipMemsetAsync(d_out_count, 0, 8, s));
        return GRANNE_HIP_OK;
    }
    uint32_t* counts = nullptr;
    HIP_TRY(hipMallocAsync((void**)&counts, (size_t)fl_blocks(n_elements) * 4, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() { (void)hipFreeAsync(p, s); }
    } release{counts, s};
    return filter_compact<uint64_t>(d_filter, n_elements, counts, d_out_ids, d_out_count, nullptr, s);
}

// The four entries' argument checks. `filtered`: the entry takes a filter (its name in the messages is
// exact_topk_filtered, and the two filter checks apply).
static int exact_topk_args(const granne_hip_index* ix, uint32_t nq, uint32_t k, bool buffers, bool filtered, const void* filter,
                           uint64_t filter_stride_words) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, filtered ? "exact_topk_filtered: index is null" : "index is null");
    if (filtered) {
        GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_topk_filtered");
        GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_topk_filtered");
    } else {
        GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "exact_topk");
        GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "exact_topk");
    }
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (k == 0 || k > ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "k must be in [1, %u]", ET_KMAX);
    if (ix->n_elements > 0xFFFFFFFFull)
        return fail(GRANNE_HIP_ERR_INVALID, "%s takes up to 2^32 - 1 elements", filtered ? "exact_topk_filtered" : "exact_topk");
    if (!filtered) return GRANNE_HIP_OK;
    if (!filter) return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_filtered: the filter is null");
    if (filter_stride_words && filter_stride_words < filter_words(ix->n_elements))
        return fail(GRANNE_HIP_ERR_INVALID, "exact_topk_filtered: filter_stride_words (%llu) must be 0 or at least ceil(n_elements / 32) = %llu",
                    (unsigned long long)filter_stride_words, (unsigned long long)filter_words(ix->n_elements));
    return GRANNE_HIP_OK;
}

// The selection's scratch: the candidates [qc][ET_CAP] u64 -- the two histograms live in the same bytes, dead before the
// keys are collected -- then bound [qc], sel [qc], cnt [qc]; then, for the list source, the list's length (u64), the
// compaction's block counts and the list itself (u32 [n]). qc: the queries of one chunk.
struct EtScratch {
    size_t o_big, o_bound, o_sel, o_cnt, o_m, o_blk, o_list, total;
};
static EtScratch et_scratch(uint64_t n, uint32_t nq, bool list) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const uint32_t qc_max = nq < ET_CHUNK ? nq : ET_CHUNK;
    static_assert((ET_BINS1 + ET_BINS2) * 4u <= ET_CAP * 8u, "the histograms fit in the candidates' bytes");
    EtScratch o;
    o.o_big = 0;
    o.o_bound = (size_t)qc_max * ET_CAP * 8;
    o.o_sel = o.o_bound + (size_t)qc_max * 4;
    o.o_cnt = o.o_sel + (size_t)qc_max * sizeof(EtSel);
    o.o_m = up(o.o_cnt + (size_t)qc_max * 4);
    o.o_blk = o.o_m + 256;
    o.o_list = o.o_blk + up(list ? (size_t)fl_blocks(n) * 4 : 0);
    o.total = o.o_list + (list ? (size_t)n * 4 : 0);
    return o;
}

// The selection on stream s, arguments checked, nq > 0. d_filter null: all rows (ET_ALL); else filter_stride_words == 0:
// one bitmap for every query, compacted here to its ids (ET_LIST); else one bitmap per query (ET_BITS). d_over (optional,
// u32[nq]): 1 where the selection overflowed and the query was voided, else 0. d_scratch (optional): et_scratch(..).total
// bytes of the caller's on the index's device, free for this call on s; null: taken from the stream-ordered allocator.
static int exact_topk_run(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_filter,
                          uint64_t filter_stride_words, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status,
                          hipStream_t s, uint32_t* d_over = nullptr, uint8_t* d_scratch = nullptr) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    const uint64_t n = ix->n_elements;
    const bool i8 = ix->dtype == GRANNE_HIP_I8;
    const EtSrc src = !d_filter ? ET_ALL : filter_stride_words == 0 ? ET_LIST : ET_BITS;
    const bool list = src == ET_LIST;
    // the prefixes the selection runs over, shortest first, the last one all rows (exact_topk.h, priming): a function of n
    // alone -- the list source clips them to the list's length on the device
    uint64_t prefix[16];
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
    }
    const EtScratch lay = et_scratch(n, nq, list);
    const size_t o_big = lay.o_big, o_bound = lay.o_bound, o_sel = lay.o_sel, o_cnt = lay.o_cnt, o_m = lay.o_m, o_blk = lay.o_blk, o_list = lay.o_list;
    uint8_t* scratch = d_scratch;
    if (!scratch) HIP_TRY(hipMallocAsync((void**)&scratch, lay.total, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() {
            if (p) (void)hipFreeAsync(p, s);
        }
    } release{d_scratch ? nullptr : scratch, s};
    if (list)
        if (const int rc = filter_compact<uint32_t>(d_filter, n, (uint32_t*)(scratch + o_blk), (uint32_t*)(scratch + o_list),
                                                    (uint64_t*)(scratch + o_m), d_status ? d_status + 3 : nullptr, s))
            return rc;
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    const bool resident = ix->row_bytes <= 1024u;
    EtParams P;
    P.elements = ix->d_elements.as<uint8_t>();
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
    P.q_lds = resident ? ix->row_bytes : 0u;
    P.list = list ? (const uint32_t*)(scratch + o_list) : nullptr;
    P.m = list ? (const uint64_t*)(scratch + o_m) : nullptr;
    P.filter_stride = filter_stride_words;
    P.bound = (const uint32_t*)(scratch + o_bound);
    P.sel = (const EtSel*)(scratch + o_sel);
    P.cnt = (uint32_t*)(scratch + o_cnt);
    P.cand = (uint64_t*)(scratch + o_big);
    uint32_t* const hist1 = (uint32_t*)(scratch + o_big);
    const uint32_t lds = ET_QT * P.q_lds;
    for (uint32_t c0 = 0; c0 < nq; c0 += ET_CHUNK) {
        const uint32_t qc = nq - c0 < ET_CHUNK ? nq - c0 : ET_CHUNK;
        uint32_t* const hist2 = hist1 + (size_t)qc * ET_BINS1;
        const uint32_t tiles = (qc + ET_QT - 1) / ET_QT;
        P.queries = (const uint8_t*)d_queries + (size_t)c0 * qbytes;
        P.nq = qc;
        P.filter = src == ET_BITS ? d_filter + (size_t)c0 * filter_stride_words : nullptr;
        // a counting pass (1, 2) and its select, or the collecting pass (3), over the prefix `rows` that follows `prev`
        auto pass = [&](int which, uint64_t rows, uint64_t prev, uint32_t final) -> int {
            uint64_t G = (rows + ET_GROUPS - 1) / ET_GROUPS;
            const uint64_t most = 2048u / tiles ? 2048u / tiles : 1u; // ~8 blocks per compute unit
            if (G > most) G = most;
            if (G < 1) G = 1;
            P.rows = rows;
            P.per_range = ((rows + G - 1) / G + ET_GROUPS - 1) / ET_GROUPS * ET_GROUPS;
            if (P.per_range < ET_GROUPS) P.per_range = ET_GROUPS;
            P.prev_rows = prev;
            P.hist = which == 1 ? hist1 : hist2;
            hipLaunchKernelGGL(et_scan_fn(i8, ix->row_bytes, which, src), dim3(tiles, (uint32_t)G), dim3(ET_THREADS), lds, s, P);
            HIP_TRY(hipGetLastError());
            if (which == 3) return GRANNE_HIP_OK;
            hipLaunchKernelGGL(et_select_fn(which, src), dim3(qc), dim3(256), 0, s, (const uint32_t*)P.hist, k, rows, prev, P.m, n,
                               (uint32_t*)(scratch + o_bound), (EtSel*)(scratch + o_sel), final, d_status);
            HIP_TRY(hipGetLastError());
            return GRANNE_HIP_OK;
        };
        HIP_TRY(hipMemsetAsync(scratch + o_bound, 0xFF, (size_t)qc * 4, s));
        for (uint32_t st = 0; st < stages; ++st) {
            const uint32_t final = st + 1 == stages ? 1u : 0u; // (ET_BITS; the list rule decides on the device)
            const uint64_t prev = st ? prefix[st - 1] : 0;
            HIP_TRY(hipMemsetAsync(hist1, 0, (size_t)qc * (ET_BINS1 + ET_BINS2) * 4, s));
            if (const int rc = pass(1, prefix[st], prev, final)) return rc;
            if (const int rc = pass(2, prefix[st], prev, final)) return rc;
        }
        HIP_TRY(hipMemsetAsync(scratch + o_cnt, 0, (size_t)qc * 4, s));
        if (const int rc = pass(3, n, 0, 0)) return rc;
        hipLaunchKernelGGL(et_rank_kernel, dim3(qc), dim3(ET_RANK_THREADS), 0, s, (const uint64_t*)(scratch + o_big),
                           (const uint32_t*)(scratch + o_cnt), (const EtSel*)(scratch + o_sel), k, d_out_ids + (size_t)c0 * k,
                           d_out_dists + (size_t)c0 * k, d_out_counts + c0, d_status, d_over ? d_over + c0 : nullptr);
        HIP_TRY(hipGetLastError());
    }
    return GRANNE_HIP_OK;
}

// Host buffers in and out around exact_topk_run: the queries and the filter's words (ceil(n_elements / 32), or
// nq * stride; none for a null filter) go up, the answer and the status words come back. `name`: the entry's, for the
// overflow message.
static int exact_topk_staged(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k, const uint32_t* filter,
                             uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_status,
                             const char* name) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t fb = !filter ? 0 : (filter_stride_words ? (size_t)nq * filter_stride_words : (size_t)filter_words(ix->n_elements)) * 4;
    const size_t o_f = up(qb), o_ids = o_f + up(fb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4);
    const size_t o_st = o_c + up((size_t)nq * 4), total = o_st + 16;
    DevBuf block;
    HIP_TRY(block.alloc(total));
    struct Settle { // (declared after the block: whatever the passes left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    if (filter) HIP_TRY(hipMemcpy(buf + o_f, filter, fb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    const int rc = exact_topk_run(ix, buf, nq, k, filter ? (const uint32_t*)(buf + o_f) : nullptr, filter_stride_words, (uint64_t*)(buf + o_ids),
                                  (float*)(buf + o_d), (uint32_t*)(buf + o_c), (uint32_t*)(buf + o_st), nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "%s: %u queries have more than %u rows inside one second-level bin at their k-th distance", name,
                    st[0], ET_CAP);
    return GRANNE_HIP_OK;
}

// exact k nearest elements in the reference's arithmetic, selected by (distance bits, id)
extern "C" int granne_hip_exact_topk_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                            uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status,
                                            void* stream) {
    if (const int rc = exact_topk_args(ix, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, false, nullptr, 0)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_run(ix, d_queries, nq, k, nullptr, 0, d_out_ids, d_out_dists, d_out_counts, d_status, (hipStream_t)stream);
}

extern "C" int granne_hip_exact_topk(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k, uint64_t* out_ids,
                                     float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = exact_topk_args(ix, nq, k, queries && out_ids && out_dists && out_counts, false, nullptr, 0)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_staged(ix, queries, nq, k, nullptr, 0, out_ids, out_dists, out_counts, out_status, "exact_topk");
}

// the same among the ids a bitmap allows: one bitmap for every query (filter_stride_words == 0) or one per query
extern "C" int granne_hip_exact_topk_filtered_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                                     const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids,
                                                     float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = exact_topk_args(ix, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, true, d_filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_run(ix, d_queries, nq, k, d_filter, filter_stride_words, d_out_ids, d_out_dists, d_out_counts, d_status,
                          (hipStream_t)stream);
}

extern "C" int granne_hip_exact_topk_filtered(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k, const uint32_t* filter,
                                              uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                              uint32_t* out_status) {
    if (const int rc = exact_topk_args(ix, nq, k, queries && out_ids && out_dists && out_counts, true, filter, filter_stride_words)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return exact_topk_staged(ix, queries, nq, k, filter, filter_stride_words, out_ids, out_dists, out_counts, out_status, "exact_topk_filtered");
}
