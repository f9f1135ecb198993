// sharded_ops_host.h -- filtered search and the exact selection on a partitioned index (included by granne_hip.hip after
// the single index's entries). The driver is sharded_host.h's: a ShardedOp rides through the same slots,
// exchange and merge as `search`. What is here: the shard's slice of the caller's bitmap(s), the per-shard calls, the
// fold / finishing step after the merge, and the entries.
//
// A global filter covers granne_hip_sharded_id_span bits on the merge device. Shard s needs the bits
// [offset_s, offset_s + n_elements_s) as a bitmap of its own, on its device:
//     the merge device's group, offset_s % 32 == 0   a pointer into the caller's words: nothing is copied (the bits past the
//                                                    shard's last id in its last word are another shard's, and never read)
//     the merge device's group, otherwise            one slice launch (filter.h)
//     another group, offset_s % 32 == 0              the covering words copied to the shard's device: the copy is the slice
//     another group, otherwise                       the covering words copied there, then one slice launch there
// All of it on the shard's stream, after the slot's `ready`: nothing new is waited for.
#pragma once

extern "C" uint64_t granne_hip_sharded_id_span(const granne_hip_sharded* sh) {
    uint64_t span = 0;
    if (sh)
        for (auto& S : sh->shards) span = std::max(span, S.offset + granne_hip_index_num_elements(S.ix));
    return span;
}

// shard s's bitmap(s) for this batch: *f / *f_stride are what its filtered call takes
static int sharded_local_filter(granne_hip_sharded* sh, granne_hip_sharded::Slot& L, uint32_t s, const ShardedOp& op, uint32_t nq,
                                const uint32_t** f, uint64_t* f_stride) {
    auto& S = sh->shards[s];
    const uint64_t n = S.ix->n_elements, first = S.offset & 31u, w0 = S.offset >> 5;
    const uint64_t words = filter_words(n), cover = filter_words(first + n); // the shard's own; the caller's words that hold them
    const uint32_t nf = op.filter_stride ? nq : 1u;
    const bool here = S.dev == 0;
    if (n == 0 || (here && first == 0)) {
        *f = op.d_filter + w0;
        *f_stride = op.filter_stride;
        return GRANNE_HIP_OK;
    }
    // [the slice: nf x words][the covering words: nf x cover (another group, unaligned)]
    const size_t slice_bytes = (size_t)nf * words * 4, cover_bytes = (!here && first) ? (size_t)nf * cover * 4 : 0;
    if (const int rc = slot_grow(&L.d_filt[s], &L.filt_cap[s], slice_bytes + cover_bytes)) return rc;
    uint32_t* const d_slice = (uint32_t*)L.d_filt[s];
    uint32_t* const d_cover = (uint32_t*)(L.d_filt[s] + slice_bytes);
    *f = d_slice;
    *f_stride = op.filter_stride ? words : 0;
    if (here)
        return granne_hip_filter_slice_device(op.d_filter, granne_hip_sharded_id_span(sh), op.filter_stride, nf, S.offset, n, d_slice, words,
                                              S.ix->device, S.stream);
    uint32_t* const dst = first ? d_cover : d_slice; // (aligned: cover == words)
    if (nf == 1)
        HIP_TRY(hipMemcpyPeerAsync(dst, S.ix->device, op.d_filter + w0, sh->merge_device, (size_t)cover * 4, S.stream));
    else // one strided copy for all the queries' bitmaps
        HIP_TRY(hipMemcpy2DAsync(dst, (size_t)cover * 4, op.d_filter + w0, (size_t)op.filter_stride * 4, (size_t)cover * 4, nf,
                                 hipMemcpyDeviceToDevice, S.stream));
    if (!first) return GRANNE_HIP_OK;
    return granne_hip_filter_slice_device(d_cover, first + n, nf == 1 ? 0 : cover, nf, first, n, d_slice, words, S.ix->device, S.stream);
}

// the shard's part of a batch on its stream (the driver has set the device and zeroed the block's tail)
static int sharded_op_enqueue(granne_hip_sharded* sh, granne_hip_sharded::Slot& L, uint32_t s, const ShardedOp& op, const void* q_here,
                              uint32_t nq, uint32_t max_search, uint32_t k, uint8_t* blk, size_t pb) {
    auto& S = sh->shards[s];
    const uint32_t* f = nullptr;
    uint64_t f_stride = 0;
    if (op.d_filter)
        if (const int rc = sharded_local_filter(sh, L, s, op, nq, &f, &f_stride)) return rc;
    uint64_t* const ids = (uint64_t*)blk;
    float* const dists = (float*)(blk + packed_dists_off(nq, k));
    uint32_t* const counts = (uint32_t*)(blk + packed_counts_off(nq, k));
    uint32_t* const status = (uint32_t*)(blk + pb);
    if (op.kind == ShardedOp::FILTERED)
        return granne_hip_search_filtered_batch_device(S.ix, q_here, nq, max_search, k, f, f_stride, op.max_expand, ids, dists, counts, nullptr,
                                                       status, S.stream);
    // The selection's scratch is the slot's, not the stream-ordered allocator's: the shards of a batch allocate and free on
    // streams of their own while all of them are still running, and blocks handed from one stream's free to another
    // stream's allocation were seen shared by two running selections (a shard's candidates zeroed by its neighbour).
    const size_t want = et_scratch(S.ix->n_elements, nq, op.d_filter && !op.filter_stride).total;
    if (const int rc = slot_grow(&L.d_scan[s], &L.scan_cap[s], want)) return rc;
    return exact_topk_run(S.ix, q_here, nq, k, f, f_stride, ids, dists, counts, status, S.stream, status + 4, L.d_scan[s]);
}

// after the merge, on the merge stream
static int sharded_op_finish(granne_hip_sharded* sh, granne_hip_sharded::Slot& L, const ShardedOp& op, uint32_t nq, uint32_t k, size_t pb,
                             uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status) {
    const uint32_t G = (uint32_t)sh->shards.size();
    if (op.kind == ShardedOp::FILTERED) {
        if (d_status)
            hipLaunchKernelGGL(fold_status4_kernel, dim3(1), dim3(64), 0, sh->merge_stream, (const uint8_t*)L.d_recv[0], (uint64_t)L.stride,
                               (uint64_t)pb, G, d_status);
    } else {
        hipLaunchKernelGGL(sharded_exact_finish_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, sh->merge_stream, (const uint8_t*)L.d_recv[0],
                           (uint64_t)L.stride, (uint64_t)pb, (uint64_t)(pb + SHARD_STATUS_BYTES), G, nq, k, d_out_ids, d_out_dists, d_out_counts,
                           d_status);
    }
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// ---- argument checks: the single index's refusals, before anything is enqueued -----------------------------------------
static int sharded_filter_args(granne_hip_sharded* sh, const char* name, const void* filter, uint64_t filter_stride_words) {
    if (!filter) return fail(GRANNE_HIP_ERR_INVALID, "%s: the filter is null", name);
    const uint64_t words = filter_words(granne_hip_sharded_id_span(sh));
    if (filter_stride_words && filter_stride_words < words)
        return fail(GRANNE_HIP_ERR_INVALID, "%s: filter_stride_words (%llu) must be 0 or at least ceil(id_span / 32) = %llu", name,
                    (unsigned long long)filter_stride_words, (unsigned long long)words);
    return GRANNE_HIP_OK;
}

static int sharded_filtered_args(granne_hip_sharded* sh, uint32_t nq, uint32_t max_search, uint32_t num_neighbors, const void* filter,
                                 uint64_t filter_stride_words) {
    if (const int rc = sharded_check_args(sh, max_search, num_neighbors)) return rc;
    for (auto& S : sh->shards)
        if (S.ix->se) return fail(GRANNE_HIP_ERR_INVALID, "sharded_search_filtered: compact SumEmbeddings shards have no filtered walk");
    if (nq == 0) return GRANNE_HIP_OK;
    return sharded_filter_args(sh, "sharded_search_filtered", filter, filter_stride_words);
}

static int sharded_exact_args(granne_hip_sharded* sh, uint32_t nq, uint32_t k, bool buffers, bool filtered, const void* filter,
                              uint64_t filter_stride_words) {
    const char* name = filtered ? "sharded_exact_topk_filtered" : "sharded_exact_topk";
    if (!sh) return fail(GRANNE_HIP_ERR_INVALID, "sharded index is null");
    for (auto& S : sh->shards) {
        GRANNE_HIP_COMPACT_UNSUPPORTED(S.ix, "sharded_exact_topk");
        if (S.ix->n_elements > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "%s takes shards of up to 2^32 - 1 elements", name);
    }
    if (nq == 0) return GRANNE_HIP_OK;
    if (!buffers) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (k == 0 || k > ET_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "k must be in [1, %u]", ET_KMAX);
    if ((uint64_t)sh->shards.size() * k > 4096) return fail(GRANNE_HIP_ERR_INVALID, "n_shards * k must be <= 4096");
    return filtered ? sharded_filter_args(sh, name, filter, filter_stride_words) : GRANNE_HIP_OK;
}

// one full call: begin + end on the caller's stream (arguments checked, nq > 0, k > 0)
static int sharded_op_device(granne_hip_sharded* sh, const ShardedOp& op, const void* d_queries, uint32_t nq, uint32_t max_search, uint32_t k,
                             uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    uint64_t ticket = 0;
    {
        std::lock_guard<std::mutex> lk(sh->mu);
        const int rc = sharded_begin_locked(sh, op, d_queries, nq, max_search, k, d_out_ids, d_out_dists, d_out_counts, d_status,
                                            (hipStream_t)stream, &ticket);
        if (rc) {
            sharded_quiesce(sh); // an error return leaves nothing running on the caller's buffers
            return rc;
        }
    }
    return granne_hip_sharded_end_device(sh, ticket, stream);
}

// The same with host buffers (synchronous): [queries | filter | ids | dists | counts | status] on the merge device. The
// queries and the results are staged through the handle's pinned HostIO like granne_hip_sharded_search_batch's; the
// filter's words, which may be many megabytes, go up from the caller's memory as they are.
static int sharded_op_host(granne_hip_sharded* sh, ShardedOp op, const void* queries, uint32_t nq, uint32_t max_search, uint32_t k,
                           const uint32_t* filter, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    std::lock_guard<std::mutex> hk(sh->host_mu);
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t qb = (size_t)nq * sh->dim * elem_size(sh->dtype);
    const size_t fb = !filter ? 0 : (op.filter_stride ? (size_t)nq * op.filter_stride : (size_t)filter_words(granne_hip_sharded_id_span(sh))) * 4;
    const size_t o_ids = up(qb), o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + up((size_t)nq * k * 4), o_st = o_c + up((size_t)nq * 4);
    const size_t o_f = o_st + 256, total = o_f + fb;
    GRANNE_HIP_ON_DEVICE(sh->merge_device);
    auto& H = sh->host_io[0];
    if (!H.h_done) HIP_TRY(hipEventCreateWithFlags(&H.h_done, hipEventDisableTiming));
    if (H.h_pin.capacity() < o_f) HIP_TRY(H.h_pin.reserve(o_f + (o_f >> 2), hipHostMallocDefault));
    if (const int rc = slot_grow(&H.d_io, &H.io_cap, total)) return rc;
    struct Quiesce { // whatever way this call ends, nothing it enqueued is still running when it returns
        granne_hip_sharded* sh;
        bool armed = true;
        ~Quiesce() {
            if (armed) sharded_quiesce(sh);
        }
    } quiesce{sh};
    uint8_t* const h_pin = H.h_pin.as<uint8_t>();
    memcpy(h_pin, queries, qb);
    HIP_TRY(hipMemcpyAsync(H.d_io, h_pin, qb, hipMemcpyHostToDevice, sh->io_stream));
    if (fb) HIP_TRY(hipMemcpyAsync(H.d_io + o_f, filter, fb, hipMemcpyHostToDevice, sh->io_stream));
    HIP_TRY(hipMemsetAsync(H.d_io + o_st, 0, 16, sh->io_stream));
    if (filter) op.d_filter = (const uint32_t*)(H.d_io + o_f);
    if (const int rc = sharded_op_device(sh, op, H.d_io, nq, max_search, k, (uint64_t*)(H.d_io + o_ids), (float*)(H.d_io + o_d),
                                         (uint32_t*)(H.d_io + o_c), (uint32_t*)(H.d_io + o_st), sh->io_stream))
        return rc;
    HIP_TRY(hipMemcpyAsync(h_pin + o_ids, H.d_io + o_ids, o_st + 16 - o_ids, hipMemcpyDeviceToHost, sh->io_stream));
    HIP_TRY(hipEventRecord(H.h_done, sh->io_stream));
    HIP_TRY(hipEventSynchronize(H.h_done));
    quiesce.armed = false; // everything has been waited for
    memcpy(out_ids, h_pin + o_ids, (size_t)nq * k * 8);
    memcpy(out_dists, h_pin + o_d, (size_t)nq * k * 4);
    memcpy(out_counts, h_pin + o_c, (size_t)nq * 4);
    const uint32_t* st = (const uint32_t*)(h_pin + o_st);
    if (out_status) memcpy(out_status, st, 16);
    if (st[0] && op.kind == ShardedOp::FILTERED)
        return fail(GRANNE_HIP_ERR_OVERFLOW, "a shard's exact-search scratch is exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
    if (st[0])
        return fail(GRANNE_HIP_ERR_OVERFLOW, "sharded_exact_topk: %u queries have more than %u rows of one shard inside one second-level bin at their k-th distance",
                    st[0], ET_CAP);
    return GRANNE_HIP_OK;
}

// ---- filtered search: every shard's granne_hip_search_filtered_batch_device under its slice, merged by (dist, global id)
extern "C" int granne_hip_sharded_search_filtered_batch_device(granne_hip_sharded* sh, const void* d_queries, uint32_t nq, uint32_t max_search,
                                                               uint32_t num_neighbors, const uint32_t* d_filter, uint64_t filter_stride_words,
                                                               uint64_t max_expand, uint64_t* d_out_ids, float* d_out_dists,
                                                               uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = sharded_filtered_args(sh, nq, max_search, num_neighbors, d_filter, filter_stride_words)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    if (num_neighbors == 0) { // .take(0), src/index/mod.rs:974-977
        if (!d_out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
        DeviceGuard g(sh->merge_device);
        HIP_TRY(hipMemsetAsync(d_out_counts, 0, (size_t)nq * 4, (hipStream_t)stream));
        return GRANNE_HIP_OK;
    }
    if (!d_queries || !d_out_ids || !d_out_dists || !d_out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    ShardedOp op;
    op.kind = ShardedOp::FILTERED;
    op.d_filter = d_filter;
    op.filter_stride = filter_stride_words;
    op.max_expand = max_expand;
    return sharded_op_device(sh, op, d_queries, nq, max_search, num_neighbors, d_out_ids, d_out_dists, d_out_counts, d_status, stream);
}

extern "C" int granne_hip_sharded_search_filtered_batch(granne_hip_sharded* sh, const void* queries, uint32_t nq, uint32_t max_search,
                                                        uint32_t num_neighbors, const uint32_t* filter, uint64_t filter_stride_words,
                                                        uint64_t max_expand, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                                        uint32_t* out_status) {
    const int rc = sharded_filtered_args(sh, nq, max_search, num_neighbors, filter, filter_stride_words);
    if (out_status && !rc) out_status[0] = out_status[1] = out_status[2] = out_status[3] = 0;
    if (rc || nq == 0) return rc;
    if (num_neighbors == 0) {
        if (!out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
        memset(out_counts, 0, (size_t)nq * 4);
        return GRANNE_HIP_OK;
    }
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    ShardedOp op;
    op.kind = ShardedOp::FILTERED;
    op.filter_stride = filter_stride_words;
    op.max_expand = max_expand;
    return sharded_op_host(sh, op, queries, nq, max_search, num_neighbors, filter, out_ids, out_dists, out_counts, out_status);
}

// ---- the exact selection: every shard's exact_topk(_filtered), merged; a query that overflowed in any shard is voided ----
static ShardedOp sharded_exact_op(uint32_t nq, const uint32_t* d_filter, uint64_t filter_stride_words) {
    ShardedOp op;
    op.kind = ShardedOp::EXACT;
    op.d_filter = d_filter;
    op.filter_stride = filter_stride_words;
    op.extra = ((size_t)nq * 4 + 15) & ~(size_t)15; // the shard's overflow flags, after its status words
    return op;
}

extern "C" int granne_hip_sharded_exact_topk_device(granne_hip_sharded* sh, const void* d_queries, uint32_t nq, uint32_t k, uint64_t* d_out_ids,
                                                    float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = sharded_exact_args(sh, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, false, nullptr, 0)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return sharded_op_device(sh, sharded_exact_op(nq, nullptr, 0), d_queries, nq, 1, k, d_out_ids, d_out_dists, d_out_counts, d_status, stream);
}

extern "C" int granne_hip_sharded_exact_topk(granne_hip_sharded* sh, const void* queries, uint32_t nq, uint32_t k, uint64_t* out_ids,
                                             float* out_dists, uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = sharded_exact_args(sh, nq, k, queries && out_ids && out_dists && out_counts, false, nullptr, 0)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return sharded_op_host(sh, sharded_exact_op(nq, nullptr, 0), queries, nq, 1, k, nullptr, out_ids, out_dists, out_counts, out_status);
}

extern "C" int granne_hip_sharded_exact_topk_filtered_device(granne_hip_sharded* sh, const void* d_queries, uint32_t nq, uint32_t k,
                                                             const uint32_t* d_filter, uint64_t filter_stride_words, uint64_t* d_out_ids,
                                                             float* d_out_dists, uint32_t* d_out_counts, uint32_t* d_status, void* stream) {
    if (const int rc = sharded_exact_args(sh, nq, k, d_queries && d_out_ids && d_out_dists && d_out_counts, true, d_filter, filter_stride_words))
        return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return sharded_op_device(sh, sharded_exact_op(nq, d_filter, filter_stride_words), d_queries, nq, 1, k, d_out_ids, d_out_dists, d_out_counts,
                             d_status, stream);
}

extern "C" int granne_hip_sharded_exact_topk_filtered(granne_hip_sharded* sh, const void* queries, uint32_t nq, uint32_t k,
                                                      const uint32_t* filter, uint64_t filter_stride_words, uint64_t* out_ids, float* out_dists,
                                                      uint32_t* out_counts, uint32_t* out_status) {
    if (const int rc = sharded_exact_args(sh, nq, k, queries && out_ids && out_dists && out_counts, true, filter, filter_stride_words)) return rc;
    if (nq == 0) return GRANNE_HIP_OK;
    return sharded_op_host(sh, sharded_exact_op(nq, nullptr, filter_stride_words), queries, nq, 1, k, filter, out_ids, out_dists, out_counts,
                           out_status);
}
