// range_host.h -- host side of range search by the walk (included by granne_hip.hip after exact_range_host.h):
// granne_hip_search_range_batch* run the ordinary search -- search_launch, whatever walker its plan picks -- with
// max_search = num_neighbors = E_s stage after stage, cut every list at its query's radius (range.h) and hand the queries
// whose list never reached past the radius to the exact range scan (exact_range_run) or leave them their short answer. The
// model is in include/granne_hip.h; DESIGN.md 3.10e.
//
// The device entry is stream-ordered, but it WAITS on the stream once per stage it goes beyond: the number of pending
// queries comes back to the host (one u32), which sizes the next stage's launches and ends the call early at 0. After the
// last stage nothing is read back with GRANNE_HIP_RG_FALLBACK_SHORT; with _EXACT one count sizes the scan, which waits once
// more itself.
#pragma once

#include "range.h"

// what both entries check, in this order: the arguments that need no handle, the handle, what depends on the handle.
// host_radii: the host entry's radii (null for the device entry, which cannot see them).
static int range_check(const granne_hip_index* ix, uint32_t nq, uint32_t cap, const uint32_t* stages, uint32_t n_stages, int fallback,
                       bool buffers, const float* host_radii) {
    if (n_stages == 0 || n_stages > GRANNE_HIP_RG_MAX_STAGES)
        return fail(GRANNE_HIP_ERR_INVALID, "search_range: n_stages (%u) must be in [1, %d]", n_stages, GRANNE_HIP_RG_MAX_STAGES);
    if (!stages) return fail(GRANNE_HIP_ERR_INVALID, "search_range: stages is null");
    for (uint32_t s = 0; s < n_stages; ++s) {
        if (stages[s] == 0) return fail(GRANNE_HIP_ERR_INVALID, "search_range: stages[%u] is 0 (a stage is a max_search > 0)", s);
        if (s && stages[s] <= stages[s - 1])
            return fail(GRANNE_HIP_ERR_INVALID, "search_range: stages must be strictly ascending (stages[%u] = %u after %u)", s, stages[s],
                        stages[s - 1]);
    }
    if (cap == 0 || cap > ER_CAP_MAX) return fail(GRANNE_HIP_ERR_INVALID, "search_range: cap (%u) must be in [1, %u]", cap, ER_CAP_MAX);
    if (fallback != GRANNE_HIP_RG_FALLBACK_SHORT && fallback != GRANNE_HIP_RG_FALLBACK_EXACT)
        return fail(GRANNE_HIP_ERR_INVALID, "search_range: fallback (%d) must be GRANNE_HIP_RG_FALLBACK_SHORT or _EXACT", fallback);
    if (nq && !buffers) return fail(GRANNE_HIP_ERR_INVALID, "search_range: null buffer");
    if (host_radii)
        if (const uint32_t bad = range_first_nan(host_radii, nq); bad < nq)
            return fail(GRANNE_HIP_ERR_INVALID, "search_range: the radius of query %u is NaN", bad);
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "search_range: index is null");
    if (fallback == GRANNE_HIP_RG_FALLBACK_EXACT) {
        if (ix->dtype == GRANNE_HIP_F16)
            return fail(GRANNE_HIP_ERR_INVALID, "search_range: GRANNE_HIP_RG_FALLBACK_EXACT has no form for GRANNE_HIP_F16 (angular_f16) handles: the exact scan refuses them; use GRANNE_HIP_RG_FALLBACK_SHORT");
        if (ix->se)
            return fail(GRANNE_HIP_ERR_INVALID, "search_range: GRANNE_HIP_RG_FALLBACK_EXACT has no form for compact SumEmbeddings handles: the exact scan needs dense rows; use GRANNE_HIP_RG_FALLBACK_SHORT");
        if (ix->n_elements > 0xFFFFFFFFull)
            return fail(GRANNE_HIP_ERR_INVALID, "search_range: GRANNE_HIP_RG_FALLBACK_EXACT takes up to 2^32 - 1 elements");
    }
    return GRANNE_HIP_OK;
}

// the call on stream s, arguments checked, nq > 0
static int range_run(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii, uint32_t cap, const uint32_t* stages,
                     uint32_t n_stages, int fallback, uint64_t scratch_bytes, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                     uint32_t* d_out_found, uint32_t* d_out_stage, uint32_t* d_status, hipStream_t s) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    const SearchTarget T(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size());
    const size_t qbytes = (size_t)ix->dim * query_elem_size(ix->dtype);
    if (scratch_bytes == 0) scratch_bytes = 256ull << 20;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    // the call's bookkeeping, as postfiltered_run's: the pending bitmap, the compaction's block counts, the two pending
    // lists, the list's length (u64, then u32)
    const size_t o_blk = up((size_t)filter_words(nq) * 4), o_la = o_blk + up((size_t)fl_blocks(nq) * 4), o_lb = o_la + up((size_t)nq * 4);
    const size_t o_cnt = o_lb + up((size_t)nq * 4), book_total = o_cnt + 16;
    PfStreamMem book;
    HIP_TRY(book.alloc(book_total, s));
    uint8_t* const bk = book.as<uint8_t>();
    uint32_t* const d_pending = (uint32_t*)bk;
    uint32_t* list_cur = nullptr; // null: every query of the call, in order (stage 0)
    uint32_t* list_next = (uint32_t*)(bk + o_la);
    uint32_t np = nq;
    for (uint32_t st = 0; st < n_stages; ++st) {
        const uint32_t E = stages[st];
        const bool last = st + 1 == n_stages;
        uint64_t chunk = scratch_bytes / (12ull * E); // a list is E ids (u64) and E distances (f32)
        if (chunk < 1) chunk = 1;
        if (chunk > np) chunk = np;
        const size_t o_d = up((size_t)chunk * E * 8), o_c = o_d + up((size_t)chunk * E * 4), lists_total = o_c + up((size_t)chunk * 4);
        PfStreamMem lists, rows;
        HIP_TRY(lists.alloc(lists_total, s));
        const uint8_t* q_src = (const uint8_t*)d_queries;
        if (list_cur) { // the pending queries' rows, dense
            HIP_TRY(rows.alloc((size_t)np * qbytes, s));
            if (const int rc = pf_gather_rows(d_queries, qbytes, list_cur, np, qbytes, rows.p, s)) return rc;
            q_src = rows.as<uint8_t>();
        }
        HIP_TRY(hipMemsetAsync(d_pending, 0, (size_t)filter_words(nq) * 4, s));
        uint8_t* const lb = lists.as<uint8_t>();
        for (uint32_t c0 = 0; c0 < np; c0 += (uint32_t)chunk) {
            const uint32_t qc = np - c0 < chunk ? np - c0 : (uint32_t)chunk;
            if (const int rc = search_launch(T, index_call(q_src + (size_t)c0 * qbytes, qc, E, E, (uint64_t*)lb, (float*)(lb + o_d),
                                                           (uint32_t*)(lb + o_c), nullptr, d_status, s)))
                return rc;
            RgTake P;
            P.ids = (const uint64_t*)lb;
            P.dists = (const float*)(lb + o_d);
            P.counts = (const uint32_t*)(lb + o_c);
            P.np = qc;
            P.E = E;
            P.orig = list_cur ? list_cur + c0 : nullptr;
            P.row0 = c0;
            P.cap = cap;
            P.stage = st;
            P.last_short = last && fallback == GRANNE_HIP_RG_FALLBACK_SHORT ? 1u : 0u;
            P.last = last ? 1u : 0u;
            P.radii = d_radii;
            P.out_ids = d_out_ids;
            P.out_dists = d_out_dists;
            P.out_counts = d_out_counts;
            P.out_found = d_out_found;
            P.out_stage = d_out_stage;
            P.pending = d_pending;
            P.status = d_status;
            hipLaunchKernelGGL(rg_take_kernel, dim3((qc + RG_TAKE_WAVES - 1) / RG_TAKE_WAVES), dim3(64 * RG_TAKE_WAVES), 0, s, P);
            HIP_TRY(hipGetLastError());
        }
        if (last && fallback == GRANNE_HIP_RG_FALLBACK_SHORT) return GRANNE_HIP_OK; // every query has its answer: nothing to read back
        if (const int rc = filter_compact<uint32_t>(d_pending, nq, (uint32_t*)(bk + o_blk), list_next, (uint64_t*)(bk + o_cnt),
                                                    (uint32_t*)(bk + o_cnt + 8), s))
            return rc;
        uint32_t pending = 0;
        HIP_TRY(hipMemcpyAsync(&pending, bk + o_cnt + 8, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // the one wait of the stage
        if (pending == 0) return GRANNE_HIP_OK;
        np = pending;
        uint32_t* const t = list_cur ? list_cur : (uint32_t*)(bk + o_lb);
        list_cur = list_next;
        list_next = t;
    }
    // GRANNE_HIP_RG_FALLBACK_EXACT: the exact range scan for the np queries of list_cur, with their radii
    const size_t o_fd = up((size_t)np * cap * 8), o_fc = o_fd + up((size_t)np * cap * 4), o_ft = o_fc + up((size_t)np * 4);
    const size_t o_fr = o_ft + up((size_t)np * 4), o_fs = o_fr + up((size_t)np * 4), o_fq = o_fs + 256, fb_total = o_fq + (size_t)np * qbytes;
    PfStreamMem fb;
    HIP_TRY(fb.alloc(fb_total, s));
    uint8_t* const f = fb.as<uint8_t>();
    HIP_TRY(hipMemsetAsync(f + o_fs, 0, 16, s));
    if (const int rc = pf_gather_rows(d_queries, qbytes, list_cur, np, qbytes, f + o_fq, s)) return rc;
    if (const int rc = pf_gather_rows(d_radii, 4, list_cur, np, 4, f + o_fr, s)) return rc;
    if (const int rc = exact_range_run(ix, f + o_fq, np, (const float*)(f + o_fr), cap, nullptr, 0, (uint64_t*)f, (float*)(f + o_fd),
                                       (uint32_t*)(f + o_fc), (uint32_t*)(f + o_ft), (uint32_t*)(f + o_fs), s))
        return rc;
    uint64_t blocks = ((uint64_t)np * cap + 255u) / 256u;
    if (blocks > 65536u) blocks = 65536u;
    hipLaunchKernelGGL(er_scatter_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, (const uint64_t*)f, (const float*)(f + o_fd),
                       (const uint32_t*)(f + o_fc), (const uint32_t*)(f + o_ft), (const uint32_t*)list_cur, np, cap, d_out_ids, d_out_dists,
                       d_out_counts, d_out_found, d_out_stage, RG_STAGE_EXACT, (const uint32_t*)(f + o_fs), 0u, d_status);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_search_range_batch_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, const float* d_radii,
                                                    uint32_t cap, const uint32_t* stages, uint32_t n_stages, int fallback, uint64_t scratch_bytes,
                                                    uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_out_found,
                                                    uint32_t* d_out_stage, uint32_t* d_status, void* stream) {
    if (const int rc = range_check(ix, nq, cap, stages, n_stages, fallback, d_queries && d_radii && d_out_ids && d_out_dists && d_out_counts, nullptr))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return range_run(ix, d_queries, nq, d_radii, cap, stages, n_stages, fallback, scratch_bytes, d_out_ids, d_out_dists, d_out_counts, d_out_found,
                     d_out_stage, d_status, (hipStream_t)stream);
}

// the same with host buffers in and out (synchronous); a NaN radius is refused; never part of a GRANNE_HIP_OPT_COALESCE group
extern "C" int granne_hip_search_range_batch(const granne_hip_index* ix, const void* queries, uint32_t nq, const float* radii, uint32_t cap,
                                             const uint32_t* stages, uint32_t n_stages, int fallback, uint64_t scratch_bytes, uint64_t* out_ids,
                                             float* out_dists, uint32_t* out_counts, uint32_t* out_found, uint32_t* out_stage,
                                             uint32_t* out_status) {
    const bool buffers = queries && radii && out_ids && out_dists && out_counts;
    const int rc0 = range_check(ix, nq, cap, stages, n_stages, fallback, buffers, nq && buffers ? radii : nullptr);
    if (out_status && !rc0) out_status[0] = out_status[1] = out_status[2] = out_status[3] = 0;
    if (rc0 || nq == 0) return rc0;
    GRANNE_HIP_ON_DEVICE(ix->device);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t o_r = up(qb), o_ids = o_r + up((size_t)nq * 4), o_d = o_ids + up((size_t)nq * cap * 8), o_c = o_d + up((size_t)nq * cap * 4);
    const size_t o_fn = o_c + up((size_t)nq * 4), o_sg = o_fn + up((size_t)nq * 4), o_st = o_sg + up((size_t)nq * 4), total = o_st + 16;
    DevBuf block;
    HIP_TRY(block.alloc(total));
    struct Settle { // (declared after the block: whatever the stages left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(buf + o_r, radii, (size_t)nq * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(buf + o_st, 0, 16));
    const int rc = range_run(ix, buf, nq, (const float*)(buf + o_r), cap, stages, n_stages, fallback, scratch_bytes, (uint64_t*)(buf + o_ids),
                             (float*)(buf + o_d), (uint32_t*)(buf + o_c), (uint32_t*)(buf + o_fn), (uint32_t*)(buf + o_sg),
                             (uint32_t*)(buf + o_st), nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    uint32_t st[4];
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * cap * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * cap * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    if (out_found) HIP_TRY(hipMemcpy(out_found, buf + o_fn, (size_t)nq * 4, hipMemcpyDeviceToHost));
    if (out_stage) HIP_TRY(hipMemcpy(out_stage, buf + o_sg, (size_t)nq * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(st, buf + o_st, 16, hipMemcpyDeviceToHost));
    if (out_status) memcpy(out_status, st, 16);
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "search_range: a walk ran out of exact-search scratch (raise GRANNE_HIP_OPT_SLOW_SLOTS) or the fallback's selection overflowed");
    return GRANNE_HIP_OK;
}
