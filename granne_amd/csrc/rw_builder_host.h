// rw_builder_host.h -- RwGranneBuilder on the GPU (included by granne_hip.hip).
// Restates the reference's src/index/rw/mod.rs:15-224 over a dense f32 / int8 granne_hip_builder: `new` (:32-61),
// `write` (:70-97), `insert` / `insert_batch` (:99-182), `search` (:184-207), the accessors (:209-223). The per-element
// work is the bulk builder's (builder_kernels.h: select_kernel and apply_kernel restate index_element), searched by the
// walkers every other search uses; what is new is the object that keeps capacity and layers the reference's way, and a
// phase B sized for the sub-batches this API receives (sort_ops_small_kernel).
//
// index_element under Rw differs from the bulk builder's use in three ways:
//   * num_neighbors is the config's value on every layer, never halved: rw/mod.rs:162 passes `self.config` where
//     index_elements passes a config with the halved value (mod.rs:665-668) -- m_layer = cap below;
//   * there is no final per-row limit pass: mod.rs:795-797 belongs to index_elements, which Rw never calls
//     (rw/mod.rs:159-169 calls index_element directly) -- final_prune_kernel is not launched;
//   * there is no reinsertion: mod.rs:692-710 belongs to index_elements_in_last_layer, likewise not reached.
// The `selected` byte per row (BuildParams::selected) SURVIVES from one insert call to the next: only apply_kernel
// writes rows of the current layer, and it keeps the byte in step with every row it writes. It is cleared when the
// handle is made (the bulk build's rows are taken as unknown) and carried over, row for row, when a layer is promoted
// (the new current layer starts as a copy of the old one).
#pragma once

#include <condition_variable>
#include <shared_mutex>

#include "rw_tombstone.h"

// bitmap -> ascending ids (exact_topk_host.h, included after this file)
template <typename ID>
static int filter_compact(const uint32_t* d_filter, uint64_t n, uint32_t* d_counts, ID* d_out, uint64_t* d_count, uint32_t* d_count32,
                          hipStream_t s);

static_assert(RW_SMALL_OPS == GRANNE_HIP_RW_SMALL_OPS, "the header quotes the kernel's constant");

// The handle's reader-writer lock. Writers go first: a search that arrives while an insert waits queues behind it, so
// searching threads that overlap without a gap cannot keep an insert out (std::shared_mutex makes no such promise).
struct RwGate {
    std::mutex m;
    std::condition_variable cv;
    uint32_t readers = 0, writers_waiting = 0;
    bool writing = false;
    void lock_shared() {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return !writing && writers_waiting == 0; });
        ++readers;
    }
    void unlock_shared() {
        std::unique_lock<std::mutex> l(m);
        if (--readers == 0) cv.notify_all();
    }
    void lock() {
        std::unique_lock<std::mutex> l(m);
        ++writers_waiting;
        cv.wait(l, [&] { return !writing && readers == 0; });
        --writers_waiting;
        writing = true;
    }
    void unlock() {
        std::unique_lock<std::mutex> l(m);
        writing = false;
        cv.notify_all();
    }
};

struct granne_hip_rw_builder {
    // the consumed builder: config, device, element rows (allocated once for elem_cap rows) and the layers -- the
    // previous layers followed by the CURRENT one, whose len is the number of elements and cap_rows its capacity
    granne_hip_builder* b = nullptr;
    uint64_t max_elements = 0;
    uint64_t elem_cap = 0;
    // insert / promotion / remove / restore hold it exclusively, everything that reads holds it shared, for the whole call
    RwGate mu;
    hipStream_t stream = nullptr; // inserts
    BuildScratch S;               // sized for batch_cap members (d_layers and selected stay empty in it: they are below)
    uint64_t batch_cap = 0;
    DevBuf d_layers; // LayerDev [64]
    DevBuf selected; // uint8_t [current layer's cap_rows]
    DevBuf d_stage;  // dense rows of an insert call on their way into the element rows
    uint64_t opt_small_ops = RW_SMALL_OPS;
    std::atomic<uint64_t> small_launches{0}, sorted_launches{0};
    // tombstones (rw_tombstone.h): one bit per element slot, one = alive, all ones when the handle is
    // made. `removed` counts the zero bits below len; while it is 0 a search is the unfiltered launch it always was.
    // The insert path never looks at either.
    DevBuf alive;     // uint32_t [filter_words(elem_cap)]
    DevBuf d_mark;    // a remove / restore call's counters (u64 [4]), then its ids
    uint64_t removed = 0;
    std::atomic<uint64_t> filtered_searches{0};
    hipEvent_t alive_read = nullptr; // rw_builder_alive: the caller's copy of the bitmap, which the next writer waits for
    // host-pointer searches: a stream and a device buffer per concurrent caller, kept for the life of the handle
    std::mutex call_mu;
    std::vector<granne_hip_index::HostCall*> call_free;
};

static void rw_destroy(granne_hip_rw_builder* rw) {
    if (!rw) return;
    const int device = rw->b ? rw->b->device : 0;
    {
        DeviceGuard g(device);
        if (rw->stream) {
            (void)hipStreamSynchronize(rw->stream);
            (void)hipStreamDestroy(rw->stream);
        }
        if (rw->alive_read) (void)hipEventDestroy(rw->alive_read);
        for (auto* c : rw->call_free) {
            if (c->stream) (void)hipStreamDestroy(c->stream);
            delete c;
        }
        granne_hip_builder* b = rw->b;
        delete rw; // (its memory goes here, under the guard, after the streams)
        destroy_builder(b);
    }
}

// the layer table the walkers read: previous layers, then the current one with all its (UNUSED-filled) capacity --
// rows past len are linked from nowhere, as in the bulk builder's layer in the making
static int rw_upload_layers(granne_hip_rw_builder* rw) {
    const granne_hip_builder* b = rw->b;
    std::vector<LayerDev> h(b->layers.size());
    for (size_t l = 0; l < h.size(); ++l) {
        h[l].adj = b->layers[l].d_adj.as<uint32_t>();
        h[l].len = l + 1 < h.size() ? b->layers[l].len : b->layers[l].cap_rows;
        h[l].width = b->W;
        h[l].flags = 0; // connect_nodes never lists a neighbor twice (mod.rs:913-917)
        h[l].adjx = nullptr;
        h[l].adjx_stride = 0;
        h[l].reserved = 0;
    }
    HIP_TRY(hipMemcpyAsync(rw->d_layers.get(), h.data(), sizeof(LayerDev) * h.size(), hipMemcpyHostToDevice, rw->stream));
    HIP_TRY(hipStreamSynchronize(rw->stream));
    return GRANNE_HIP_OK;
}

// a current layer of `rows` rows: the first `keep` rows of `from` (may be null), the rest UNUSED; `selected` likewise
static int rw_make_current(granne_hip_rw_builder* rw, const BuilderLayer* from, uint64_t keep, uint64_t rows,
                           BuilderLayer* out) {
    granne_hip_builder* b = rw->b;
    hipStream_t s = rw->stream;
    DevBuf adj, sel;
    const size_t bytes = (size_t)rows * b->W * 4;
    SettleStream settle{s}; // (declared after the two: the stream is idle before an early return frees them)
    HIP_TRY(adj.alloc(bytes));
    HIP_TRY(sel.alloc(rows));
    if (bytes) HIP_TRY(hipMemsetAsync(adj.get(), 0xFF, bytes, s));
    HIP_TRY(hipMemsetAsync(sel.get(), 0, rows ? rows : 1, s));
    if (keep) {
        HIP_TRY(hipMemcpyAsync(adj.get(), from->d_adj.get(), (size_t)keep * b->W * 4, hipMemcpyDeviceToDevice, s));
        if (rw->selected) HIP_TRY(hipMemcpyAsync(sel.get(), rw->selected.get(), keep, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    rw->selected = std::move(sel);
    out->d_adj = std::move(adj);
    out->len = keep;
    out->cap_rows = rows;
    b->hbm_bytes += bytes;
    return GRANNE_HIP_OK;
}

// RwGranneBuilder::new, rw/mod.rs:32-61
extern "C" int granne_hip_rw_builder_create(granne_hip_rw_builder** out, granne_hip_builder* b, uint64_t max_elements) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!b) return fail(GRANNE_HIP_ERR_INVALID, "builder is null");
    if (max_elements == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_elements must be > 0");
    if (max_elements >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "max_elements must be < 2^32 - 1 (src/index/mod.rs:420)");
    if (b->d_half) return fail(GRANNE_HIP_ERR_INVALID, "rw_builder_create has no form for GRANNE_HIP_F16 (angular_f16) rows: use f32 or int8 rows");
    if (b->se)
        return fail(GRANNE_HIP_ERR_INVALID, "an RwGranneBuilder over a SumEmbeddings container is not supported: make the "
                    "builder from dense rows (granne_hip_builder_create)");
    GRANNE_HIP_ON_DEVICE(b->device);

    // builder.config.expected_num_elements = Some(max_elements); builder.build(), :34-36
    const uint64_t expected_before = b->cfg.expected_num_elements;
    b->cfg.expected_num_elements = max_elements;
    int rc = granne_hip_builder_build(b, GRANNE_HIP_BUILD_ALL);
    if (rc) {
        b->cfg.expected_num_elements = expected_before;
        return rc;
    }
    granne_hip_rw_builder* rw = new granne_hip_rw_builder();
    const uint64_t n = b->n_elements;
    BuilderLayer cur;
    DevBuf grown;
    auto body = [&]() -> int { // (a commit point: the builder becomes the handle's only once all of this has been made)
        HIP_TRY(hipStreamCreateWithFlags(&rw->stream, hipStreamNonBlocking));
        HIP_TRY(rw->d_layers.alloc(sizeof(LayerDev) * 64));
        // element storage for max(max_elements, n) rows, once: an insert writes its rows in place
        rw->elem_cap = max_elements > n ? max_elements : n;
        const size_t eb = (size_t)rw->elem_cap * b->row_stride;
        HIP_TRY(grown.alloc(eb));
        HIP_TRY(hipMemsetAsync(grown.get(), 0, eb, rw->stream));
        HIP_TRY(rw->alive.alloc((size_t)filter_words(rw->elem_cap) * 4));
        HIP_TRY(hipMemsetAsync(rw->alive.get(), 0xFF, (size_t)filter_words(rw->elem_cap) * 4, rw->stream));
        HIP_TRY(hipEventCreateWithFlags(&rw->alive_read, hipEventDisableTiming));
        if (n) HIP_TRY(hipMemcpyAsync(grown.get(), b->d_elements.get(), (size_t)n * b->row_stride, hipMemcpyDeviceToDevice, rw->stream));
        HIP_TRY(hipStreamSynchronize(rw->stream));
        // builder.layers.pop() or an empty layer, resized to max(len, compute_num_elements_in_layer(max_elements,
        // multiplier, layers.len())) rows of UNUSED, :38-48
        const bool has = !b->layers.empty();
        const uint64_t len = has ? b->layers.back().len : 0;
        const uint64_t n_prev = has ? b->layers.size() - 1 : 0;
        uint64_t rows = num_elements_in_layer(max_elements, b->cfg.layer_multiplier, n_prev);
        if (rows < len) rows = len;
        rw->b = b; // (rw_make_current reads the row width and the stream through it)
        int r = rw_make_current(rw, has ? &b->layers.back() : nullptr, len, rows, &cur);
        rw->b = nullptr;
        return r;
    };
    rc = body();
    if (rc) {
        b->cfg.expected_num_elements = expected_before;
        rw_destroy(rw); // (rw->b is null: the builder stays the caller's)
        return rc;
    }
    // from here on the builder is the handle's
    rw->b = b;
    rw->max_elements = max_elements;
    b->hbm_bytes += (size_t)(rw->elem_cap - n) * b->row_stride + (size_t)filter_words(rw->elem_cap) * 4;
    b->d_elements = std::move(grown);
    if (!b->layers.empty()) {
        b->hbm_bytes -= (size_t)b->layers.back().cap_rows * b->W * 4;
        b->layers.pop_back();
    }
    b->layers.push_back(std::move(cur));
    rc = rw_upload_layers(rw);
    if (rc) { // (a failed copy of a few hundred bytes: the device is gone; the handle owns the builder by now)
        rw_destroy(rw);
        return rc;
    }
    *out = rw;
    return GRANNE_HIP_OK;
}

extern "C" void granne_hip_rw_builder_destroy(granne_hip_rw_builder* rw) { rw_destroy(rw); }

// scratch for sub-batches of up to `members` elements
static int rw_ensure_scratch(granne_hip_rw_builder* rw, uint64_t members) {
    if (members <= rw->batch_cap) return GRANNE_HIP_OK;
    const granne_hip_builder* b = rw->b;
    uint64_t cap = rw->batch_cap ? rw->batch_cap : 64;
    while (cap < members) cap *= 2;
    if (cap > b->cfg.batch_max) cap = b->cfg.batch_max;
    if (cap < members) cap = members;
    HIP_TRY(hipStreamSynchronize(rw->stream));
    rw->S = BuildScratch(); // (the smaller blocks go first)
    rw->batch_cap = 0;
    int rc = alloc_batch_scratch(rw->S, cap, b->cfg.max_search, cap * b->cfg.num_neighbors * 2, rw->stream);
    if (rc) return rc;
    rw->batch_cap = cap;
    return GRANNE_HIP_OK;
}

// the sub-batch size of the batched schedule: clamp(nodes in the layer / batch_div, 1, batch_max)
static uint64_t rw_sub_batch(const granne_hip_builder* b, uint64_t n_in_layer) {
    uint64_t B = n_in_layer / b->cfg.batch_div;
    if (B < 1) B = 1;
    if (B > b->cfg.batch_max) B = b->cfg.batch_max;
    return B;
}

// GranneBuilder::index_element (mod.rs:805-846) for elements first .. first + count - 1, whose rows are in place and
// whose layer rows are UNUSED, under the batched schedule: rw/mod.rs:159-169
static int rw_index_elements(granne_hip_rw_builder* rw, uint64_t first, uint64_t count) {
    granne_hip_builder* b = rw->b;
    hipStream_t s = rw->stream;
    BuilderLayer& L = b->layers.back();
    const uint32_t cap = b->cfg.num_neighbors;
    const uint32_t max_search = b->cfg.max_search;
    {
        uint64_t need = rw_sub_batch(b, first + count);
        if (need > count) need = count;
        int rc = rw_ensure_scratch(rw, need);
        if (rc) return rc;
    }
    BuildScratch& S = rw->S;
    BuildPlan plan;
    {
        // num_neighbors is the config's on every layer (rw/mod.rs:162 passes self.config): m_layer = cap
        int rc = make_build_plan(b, L, cap, max_search, S, rw->selected.as<uint8_t>(), &plan);
        if (rc) return rc;
    }
    BuildParams& P = plan.P;
    P.layer_len = L.cap_rows;
    P.idx_step = 1;

    const SearchTarget T(b, rw->d_layers.as<LayerDev>(), (uint32_t)b->layers.size());
    SearchCall call; // entry through the previous layers at (1, 1), or id 0; search_for_neighbors on the current layer
    call.ef = call.k = max_search;
    call.ids = S.s_ids.as<uint64_t>();
    call.dists = S.s_dists.as<float>();
    call.counts = S.s_counts.as<uint32_t>();
    call.status = P.n_seg + 1;
    call.stream = s;
    call.q_stride = (int64_t)b->row_stride;

    uint64_t pos = 0;
    while (pos < count) {
        uint64_t B = rw_sub_batch(b, first + pos);
        if (B > count - pos) B = count - pos;
        // phase A: every member searches the graph as it stands now, then select_neighbors
        call.queries = P.elements + (size_t)(first + pos) * b->row_stride;
        call.nq = (uint32_t)B;
        int rc = search_launch(T, call);
        if (rc) return rc;
        P.first_idx = (int64_t)(first + pos);
        P.batch = (uint32_t)B;
        P.n_ops = (uint32_t)(B * cap * 2);
        hipLaunchKernelGGL(plan.K.select, dim3((uint32_t)B), dim3(64), plan.lds, s, P);
        HIP_TRY(hipGetLastError());
        // phase B: the link updates, sorted by (target row, order), replayed one wave per target row
        if (rw->opt_small_ops && P.n_ops <= rw->opt_small_ops) {
            uint32_t threads = 64;
            while (threads < 1024 && threads * 2 < P.n_ops) threads <<= 1;
            hipLaunchKernelGGL(sort_ops_small_kernel, dim3(1), dim3(threads), 0, s, P.op_keys, P.op_vals, P.n_ops,
                               S.sorted_keys.as<uint64_t>(), S.sorted_vals.as<uint64_t>(), P.seg_start, P.n_seg);
            HIP_TRY(hipGetLastError());
            rw->small_launches.fetch_add(1);
        } else {
            size_t tmp_bytes = S.sort_tmp_bytes;
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(S.sort_tmp.get(), tmp_bytes, P.op_keys, S.sorted_keys.as<uint64_t>(), P.op_vals,
                                                       S.sorted_vals.as<uint64_t>(), (int)P.n_ops, 0, OP_KEY_BITS, s));
            HIP_TRY(hipMemsetAsync(P.n_seg, 0, 4, s));
            hipLaunchKernelGGL(mark_heads_kernel, dim3(grid_for(P.n_ops, 256)), dim3(256), 0, s, P.sorted_keys, P.n_ops,
                               P.seg_start, P.n_seg);
            HIP_TRY(hipGetLastError());
            rw->sorted_launches.fetch_add(1);
        }
        const uint32_t grid = P.n_ops < 4096 ? P.n_ops : 4096;
        hipLaunchKernelGGL(plan.K.apply, dim3(grid), dim3(64), plan.lds_rows, s, P);
        HIP_TRY(hipGetLastError());
        pos += B;
    }
    // no final per-row limit pass (mod.rs:795-797 is index_elements', not reached from rw/mod.rs:159-169), no reinsertion
    uint32_t hc[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(hc, P.n_seg, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hc[1]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted during insert");
    return GRANNE_HIP_OK;
}

// the full current layer becomes the last previous layer, a clone resized to the next layer's size the current one,
// rw/mod.rs:118-135
static int rw_promote(granne_hip_rw_builder* rw) {
    granne_hip_builder* b = rw->b;
    if (b->layers.size() >= 64) return fail(GRANNE_HIP_ERR_INVALID, "too many layers");
    BuilderLayer& full = b->layers.back();
    const uint64_t rows = num_elements_in_layer(rw->max_elements, b->cfg.layer_multiplier, b->layers.size());
    if (rows < full.len) // assert!(current_layer.len() >= elements.len()), rw/mod.rs:137
        return fail(GRANNE_HIP_ERR_INVALID, "the next layer holds %llu rows but %llu elements exist (the reference panics, rw/mod.rs:137)",
                    (unsigned long long)rows, (unsigned long long)full.len);
    BuilderLayer cur;
    int rc = rw_make_current(rw, &full, full.len, rows, &cur);
    if (rc) return rc;
    b->layers.push_back(std::move(cur));
    return rw_upload_layers(rw);
}

// RwGranneBuilder::insert_batch, rw/mod.rs:103-182 (the recursion as a loop)
extern "C" int granne_hip_rw_builder_insert_batch(granne_hip_rw_builder* rw, const void* rows, uint64_t n_new,
                                                  uint64_t* out_ids, uint64_t* out_count) {
    if (out_count) *out_count = 0;
    if (!rw || !out_count) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (n_new == 0) return GRANNE_HIP_OK;
    if (!rows) return fail(GRANNE_HIP_ERR_INVALID, "rows is null");
    if (!out_ids) return fail(GRANNE_HIP_ERR_INVALID, "out_ids is null");
    std::unique_lock<RwGate> lk(rw->mu);
    granne_hip_builder* b = rw->b;
    GRANNE_HIP_ON_DEVICE(b->device);
    hipStream_t s = rw->stream;
    const size_t dense = (size_t)b->dim * elem_size(b->dtype);
    const uint8_t* src = (const uint8_t*)rows;
    uint64_t remaining = n_new, written = 0;
    while (remaining) {
        const uint64_t len = b->n_elements;
        if (len >= rw->max_elements) break; // :104-106 -- what is left is dropped
        if (len >= b->layers.back().cap_rows) { // time to create a new layer, :118
            int rc = rw_promote(rw);
            if (rc) return rc;
        }
        BuilderLayer& L = b->layers.back();
        const uint64_t take = std::min<uint64_t>(remaining, L.cap_rows - len); // :141
        // elements.push, :146-148: the rows go where they stay
        if (dense == b->row_stride) {
            HIP_TRY(hipMemcpyAsync(b->d_elements.as<uint8_t>() + (size_t)len * b->row_stride, src, take * dense, hipMemcpyHostToDevice, s));
        } else {
            if (rw->d_stage.capacity() < take * dense) {
                HIP_TRY(hipStreamSynchronize(s)); // (the previous round's relayout still reads the smaller block)
                HIP_TRY(rw->d_stage.reserve(take * dense < 4096 ? 4096 : take * dense));
            }
            HIP_TRY(hipMemcpyAsync(rw->d_stage.get(), src, take * dense, hipMemcpyHostToDevice, s));
            const uint64_t units = take * (b->row_stride / 16);
            hipLaunchKernelGGL(relayout_rows_kernel, dim3(grid_for(units, 256)), dim3(256), 0, s, rw->d_stage.as<uint8_t>(),
                               b->d_elements.as<uint8_t>() + (size_t)len * b->row_stride, take, (uint32_t)dense, b->row_stride);
            HIP_TRY(hipGetLastError());
        }
        b->n_elements = len + take;
        L.len = len + take;
        int rc = rw_index_elements(rw, len, take);
        if (rc) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        for (uint64_t i = 0; i < take; ++i) out_ids[written + i] = len + i; // :142
        written += take;
        *out_count = written;
        src += take * dense;
        remaining -= take;
    }
    return GRANNE_HIP_OK;
}

static granne_hip_index::HostCall* rw_call_acquire(granne_hip_rw_builder* rw) {
    {
        std::lock_guard<std::mutex> lk(rw->call_mu);
        if (!rw->call_free.empty()) {
            auto* c = rw->call_free.back();
            rw->call_free.pop_back();
            return c;
        }
    }
    auto* c = new granne_hip_index::HostCall();
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return nullptr;
    }
    return c;
}

// RwGranneBuilder::search, rw/mod.rs:184-207, for nq queries
extern "C" int granne_hip_rw_builder_search_batch(granne_hip_rw_builder* rw, const void* queries, uint32_t nq,
                                                  uint32_t max_search, uint32_t num_neighbors, uint64_t* out_ids,
                                                  float* out_dists, uint32_t* out_counts, uint64_t* out_stats) {
    if (!rw) return fail(GRANNE_HIP_ERR_INVALID, "rw builder is null");
    if (max_search == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (num_neighbors == 0) { // .take(0)
        memset(out_counts, 0, (size_t)nq * 4);
        return GRANNE_HIP_OK;
    }
    if (!queries || !out_ids || !out_dists) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    std::shared_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    const size_t k = num_neighbors;
    if (b->layers.size() < 2) {
        // index.search(&element, 1, 1).first() is None without a previous layer: vec![], rw/mod.rs:198-206 -- also
        // when the current layer holds elements
        memset(out_counts, 0, (size_t)nq * 4);
        for (size_t i = 0; i < (size_t)nq * k; ++i) {
            out_ids[i] = UINT64_MAX;
            out_dists[i] = INFINITY;
        }
        if (out_stats) memset(out_stats, 0, (size_t)nq * 24);
        return GRANNE_HIP_OK;
    }
    GRANNE_HIP_ON_DEVICE(b->device);
    const size_t qb = (size_t)nq * b->dim * elem_size(b->dtype);
    const size_t o_ids = (qb + 255) & ~(size_t)255;
    const size_t o_d = o_ids + (size_t)nq * k * 8;
    const size_t o_c = o_d + (((size_t)nq * k * 4 + 15) & ~(size_t)15);
    const size_t o_s = o_c + (((size_t)nq * 4 + 15) & ~(size_t)15);
    const size_t o_st = o_s + (size_t)nq * 24;
    const size_t total = o_st + 16;
    granne_hip_index::HostCall* c = rw_call_acquire(rw);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // back to the pool once the stream is idle (an error return may leave work on it)
        granne_hip_rw_builder* rw;
        granne_hip_index::HostCall* c;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            std::lock_guard<std::mutex> lk(rw->call_mu);
            rw->call_free.push_back(c);
        }
    } release{rw, c};
    HIP_TRY(c->d_buf.reserve(total));
    hipStream_t s = c->stream;
    uint8_t* buf = c->d_buf.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(buf, queries, qb, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(buf + o_st, 0, 16, s));
    // index.search(q, 1, 1) over the previous layers, then search_for_neighbors on the current layer from its result
    // (:198-199) is Granne::search over previous + current: the ordinary walk, over the rows where they are
    const SearchTarget T(b, rw->d_layers.as<LayerDev>(), (uint32_t)b->layers.size());
    SearchCall call;
    call.queries = buf;
    call.nq = nq;
    call.ef = max_search;
    call.k = num_neighbors;
    call.ids = (uint64_t*)(buf + o_ids);
    call.dists = (float*)(buf + o_d);
    call.counts = (uint32_t*)(buf + o_c);
    call.stats = (uint64_t*)(buf + o_s);
    call.status = (uint32_t*)(buf + o_st);
    call.stream = s;
    if (rw->removed != 0) { // the walk under the tombstones (filter.h): removed nodes are traversed, never returned
        call.filter = rw->alive.as<uint32_t>();
        rw->filtered_searches.fetch_add(1);
    }
    int r = search_launch(T, call);
    if (r) return r;
    uint32_t st[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(st, buf + o_st, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, buf + o_s, (size_t)nq * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st[0]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted");
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_rw_builder_search(granne_hip_rw_builder* rw, const void* query, uint32_t max_search,
                                            uint32_t num_neighbors, uint64_t* out_ids, float* out_dists, uint32_t* out_count) {
    if (!out_count) return fail(GRANNE_HIP_ERR_INVALID, "out_count is null");
    return granne_hip_rw_builder_search_batch(rw, query, 1, max_search, num_neighbors, out_ids, out_dists, out_count, nullptr);
}

// ---- accessors, rw/mod.rs:209-223 ------------------------------------------------------------------
extern "C" uint64_t granne_hip_rw_builder_len(granne_hip_rw_builder* rw) {
    if (!rw) return 0;
    std::shared_lock<RwGate> lk(rw->mu);
    return rw->b->n_elements;
}
extern "C" uint64_t granne_hip_rw_builder_max_elements(granne_hip_rw_builder* rw) { return rw ? rw->max_elements : 0; }
extern "C" uint32_t granne_hip_rw_builder_num_layers(granne_hip_rw_builder* rw) {
    if (!rw) return 0;
    std::shared_lock<RwGate> lk(rw->mu);
    return (uint32_t)rw->b->layers.size();
}
extern "C" uint64_t granne_hip_rw_builder_layer_len(granne_hip_rw_builder* rw, uint32_t layer) {
    if (!rw) return 0;
    std::shared_lock<RwGate> lk(rw->mu);
    return layer < rw->b->layers.size() ? rw->b->layers[layer].len : 0;
}
extern "C" int granne_hip_rw_builder_get_layer(granne_hip_rw_builder* rw, uint32_t layer, uint32_t* out_rows) {
    if (!rw) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    std::shared_lock<RwGate> lk(rw->mu);
    if (layer < rw->b->layers.size() && rw->b->layers[layer].len == 0) return GRANNE_HIP_OK; // nothing to copy
    return granne_hip_builder_get_layer(rw->b, layer, out_rows);
}
extern "C" int granne_hip_rw_builder_get_element(granne_hip_rw_builder* rw, uint64_t idx, void* out) {
    if (!rw || !out) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    std::shared_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    if (idx >= b->n_elements) return fail(GRANNE_HIP_ERR_INVALID, "element index out of range");
    DeviceGuard g(b->device);
    HIP_TRY(hipMemcpy(out, b->d_elements.as<uint8_t>() + idx * b->row_stride, (size_t)b->dim * elem_size(b->dtype), hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

// ---- tombstones (no reference counterpart) -----------------------------------------
// remove (clear the bits) or restore (set them): out_counts = changed, already so, out of range
static int rw_mark(granne_hip_rw_builder* rw, const uint64_t* ids, uint64_t n, uint64_t* out_counts, bool remove) {
    const char* name = remove ? "rw_builder_remove" : "rw_builder_restore";
    if (!rw) return fail(GRANNE_HIP_ERR_INVALID, "%s: rw builder is null", name);
    if (!out_counts) return fail(GRANNE_HIP_ERR_INVALID, "%s: out_counts is null", name);
    out_counts[0] = out_counts[1] = out_counts[2] = 0;
    if (n == 0) return GRANNE_HIP_OK;
    if (!ids) return fail(GRANNE_HIP_ERR_INVALID, "%s: ids is null", name);
    if (n > (1ull << 40)) return fail(GRANNE_HIP_ERR_INVALID, "%s: at most 2^40 ids per call", name);
    std::unique_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    GRANNE_HIP_ON_DEVICE(b->device);
    hipStream_t s = rw->stream;
    constexpr size_t head = 32; // the counters
    if (rw->d_mark.capacity() < head + (size_t)n * 8) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(rw->d_mark.reserve(head + (size_t)n * 8));
    }
    unsigned long long* d_counters = rw->d_mark.as<unsigned long long>();
    uint64_t* d_ids = (uint64_t*)(rw->d_mark.as<uint8_t>() + head);
    HIP_TRY(hipMemsetAsync(d_counters, 0, head, s));
    HIP_TRY(hipMemcpyAsync(d_ids, ids, (size_t)n * 8, hipMemcpyHostToDevice, s));
    auto kernel = remove ? tomb_mark_kernel<true> : tomb_mark_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint64_t*)d_ids, n, b->n_elements, rw->alive.as<uint32_t>(),
                       d_counters);
    HIP_TRY(hipGetLastError());
    unsigned long long hc[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(hc, d_counters, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    rw->removed = remove ? rw->removed + hc[0] : rw->removed - hc[0];
    out_counts[0] = hc[0], out_counts[1] = hc[1], out_counts[2] = hc[2];
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_rw_builder_remove(granne_hip_rw_builder* rw, const uint64_t* ids, uint64_t n, uint64_t* out_counts) {
    return rw_mark(rw, ids, n, out_counts, true);
}
extern "C" int granne_hip_rw_builder_restore(granne_hip_rw_builder* rw, const uint64_t* ids, uint64_t n, uint64_t* out_counts) {
    return rw_mark(rw, ids, n, out_counts, false);
}
extern "C" uint64_t granne_hip_rw_builder_removed_count(granne_hip_rw_builder* rw) {
    if (!rw) return 0;
    std::shared_lock<RwGate> lk(rw->mu);
    return rw->removed;
}

// a copy of the bitmap's first filter_words(len) words, ordered on the caller's stream
extern "C" int granne_hip_rw_builder_alive(granne_hip_rw_builder* rw, uint32_t* d_filter_out, void* stream) {
    if (!rw || !d_filter_out) return fail(GRANNE_HIP_ERR_INVALID, "rw_builder_alive: null argument");
    std::shared_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    if (b->n_elements == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(b->device);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(d_filter_out, rw->alive.get(), (size_t)filter_words(b->n_elements) * 4, hipMemcpyDeviceToDevice, s));
    // the copy may still be waiting on the caller's stream when the gate opens: whatever the handle's own stream runs next
    // -- a remove or restore among it -- waits for it
    std::lock_guard<std::mutex> ev(rw->call_mu);
    HIP_TRY(hipEventRecord(rw->alive_read, s));
    HIP_TRY(hipStreamWaitEvent(rw->stream, rw->alive_read, 0));
    return GRANNE_HIP_OK;
}

// the surviving rows, ascending by old id, as a new handle built by the bulk path under this one's config
extern "C" int granne_hip_rw_builder_compact(granne_hip_rw_builder* rw, uint64_t max_elements, granne_hip_rw_builder** out_rw,
                                             uint64_t* out_old_ids, uint64_t* out_count) {
    if (out_rw) *out_rw = nullptr;
    if (out_count) *out_count = 0;
    if (!rw || !out_rw || !out_old_ids || !out_count) return fail(GRANNE_HIP_ERR_INVALID, "rw_builder_compact: null argument");
    if (max_elements == 0) return fail(GRANNE_HIP_ERR_INVALID, "rw_builder_compact: max_elements must be > 0");
    if (max_elements >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "rw_builder_compact: max_elements must be < 2^32 - 1 (src/index/mod.rs:420)");
    std::shared_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    GRANNE_HIP_ON_DEVICE(b->device);
    const granne_hip_build_config cfg = b->cfg; // (rw_builder_create sets expected_num_elements to the new max_elements)
    const uint32_t dim = b->dim;
    const int dtype = b->dtype, device = b->device;
    const uint64_t n = b->n_elements;
    const uint32_t dense = dim * (uint32_t)elem_size(dtype);
    granne_hip_index::HostCall* c = rw_call_acquire(rw);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // (as search_batch's)
        granne_hip_rw_builder* rw;
        granne_hip_index::HostCall* c;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            std::lock_guard<std::mutex> lk(rw->call_mu);
            rw->call_free.push_back(c);
        }
    } release{rw, c};
    hipStream_t s = c->stream;
    DevBuf d_ids, d_counts, d_count, d_dense;
    SettleStream settle{s}; // (declared after the four: the stream is idle before an early return frees them)
    uint64_t m = 0;
    std::vector<uint32_t> h_ids;
    if (n) {
        HIP_TRY(d_ids.alloc((size_t)n * 4));
        HIP_TRY(d_counts.alloc((size_t)fl_blocks(n) * 4));
        HIP_TRY(d_count.alloc(8));
        int rc = filter_compact<uint32_t>(rw->alive.as<uint32_t>(), n, d_counts.as<uint32_t>(), d_ids.as<uint32_t>(), d_count.as<uint64_t>(), nullptr, s);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(&m, d_count.get(), 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (m > n) return fail(GRANNE_HIP_ERR_HIP, "rw_builder_compact: %llu survivors of %llu elements", (unsigned long long)m, (unsigned long long)n);
    }
    if (m) {
        HIP_TRY(d_dense.alloc((size_t)m * dense));
        const uint8_t* rows = b->d_elements.as<uint8_t>();
        const uint32_t* ids = d_ids.as<uint32_t>();
        uint8_t* out = d_dense.as<uint8_t>();
        if (dense % 16u == 0)
            hipLaunchKernelGGL(gather_dense_rows_kernel<uint4>, dim3(grid_for(m * (dense / 16u), 256)), dim3(256), 0, s, rows, b->row_stride, ids, m, dense, out);
        else if (dense % 4u == 0)
            hipLaunchKernelGGL(gather_dense_rows_kernel<uint32_t>, dim3(grid_for(m * (dense / 4u), 256)), dim3(256), 0, s, rows, b->row_stride, ids, m, dense, out);
        else
            hipLaunchKernelGGL(gather_dense_rows_kernel<uint8_t>, dim3(grid_for(m * dense, 256)), dim3(256), 0, s, rows, b->row_stride, ids, m, dense, out);
        HIP_TRY(hipGetLastError());
        h_ids.resize(m);
        HIP_TRY(hipMemcpyAsync(h_ids.data(), ids, (size_t)m * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    lk.unlock(); // the rows are gathered: the source goes on while the new graph is built
    granne_hip_builder* nb = nullptr;
    int rc = granne_hip_builder_create_device(&nb, &cfg, m ? d_dense.get() : nullptr, m, dim, dtype, device, s); // synchronises
    if (rc) return rc;
    d_dense.reset();
    granne_hip_rw_builder* made = nullptr;
    rc = granne_hip_rw_builder_create(&made, nb, max_elements);
    if (rc) {
        destroy_builder(nb);
        return rc;
    }
    for (uint64_t i = 0; i < m; ++i) out_old_ids[i] = h_ids[i];
    *out_count = m;
    *out_rw = made;
    return GRANNE_HIP_OK;
}

// RwGranneBuilder::write, rw/mod.rs:70-97: the elements, then previous layers + the current layer's first len rows
// (no layers at all while there are no elements, :85-93)
extern "C" int granne_hip_rw_builder_save(granne_hip_rw_builder* rw, const char* index_path, const char* elements_path) {
    if (!rw || !index_path || !elements_path) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    std::shared_lock<RwGate> lk(rw->mu); // inserts wait (the reference's write_lock), searches go on
    const granne_hip_builder* b = rw->b;
    GRANNE_HIP_ON_DEVICE(b->device);
    const uint64_t n = b->n_elements;
    const size_t dense = (size_t)b->dim * elem_size(b->dtype);
    std::vector<uint8_t> el((size_t)n * dense);
    if (n) HIP_TRY(hipMemcpy2D(el.data(), dense, b->d_elements.get(), b->row_stride, dense, n, hipMemcpyDeviceToHost));
    int rc = granne_hip_write_elements_file(elements_path, el.data(), n, b->dim, b->dtype);
    if (rc) return rc;
    const uint32_t nn = b->cfg.num_neighbors;
    const size_t nl = n ? b->layers.size() : 0;
    std::vector<std::vector<uint32_t>> rows(nl);
    std::vector<uint64_t> lens(nl);
    std::vector<const uint32_t*> ptrs(nl);
    std::vector<uint32_t> widths(nl, nn);
    for (size_t l = 0; l < nl; ++l) {
        rows[l].resize((size_t)b->layers[l].len * nn);
        rc = granne_hip_builder_get_layer(b, (uint32_t)l, rows[l].data());
        if (rc) return rc;
        lens[l] = b->layers[l].len;
        ptrs[l] = rows[l].data();
    }
    return granne_hip_write_index_file(index_path, (uint32_t)nl, lens.data(), ptrs.data(), widths.data());
}

// a static snapshot: elements 0..len and previous layers + current rows 0..len, copied device to device
extern "C" int granne_hip_rw_builder_get_index(granne_hip_rw_builder* rw, granne_hip_index** out) {
    if (!rw || !out) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    *out = nullptr;
    std::shared_lock<RwGate> lk(rw->mu);
    const granne_hip_builder* b = rw->b;
    if (b->n_elements == 0) // no layers (as `write`, rw/mod.rs:85-93)
        return granne_hip_index_create(out, nullptr, 0, b->dim, b->dtype, 0, nullptr, nullptr, nullptr, b->device);
    return granne_hip_builder_get_index(b, out);
}

extern "C" int granne_hip_rw_builder_set_option(granne_hip_rw_builder* rw, int option, uint64_t value) {
    if (!rw) return fail(GRANNE_HIP_ERR_INVALID, "rw builder is null");
    if (option != GRANNE_HIP_RW_OPT_SMALL_OPS) return fail(GRANNE_HIP_ERR_INVALID, "unknown or read-only option %d", option);
    std::unique_lock<RwGate> lk(rw->mu);
    rw->opt_small_ops = value == 1 ? RW_SMALL_OPS : value > RW_SMALL_OPS ? RW_SMALL_OPS : value;
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_rw_builder_get_option(granne_hip_rw_builder* rw, int option, uint64_t* value) {
    if (!rw || !value) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    std::shared_lock<RwGate> lk(rw->mu);
    switch (option) {
    case GRANNE_HIP_RW_OPT_SMALL_OPS: *value = rw->opt_small_ops; return GRANNE_HIP_OK;
    case GRANNE_HIP_RW_OPT_SMALL_LAUNCHES: *value = rw->small_launches.load(); return GRANNE_HIP_OK;
    case GRANNE_HIP_RW_OPT_SORTED_LAUNCHES: *value = rw->sorted_launches.load(); return GRANNE_HIP_OK;
    case GRANNE_HIP_RW_OPT_REMOVED: *value = rw->removed; return GRANNE_HIP_OK;
    case GRANNE_HIP_RW_OPT_FILTERED_SEARCHES: *value = rw->filtered_searches.load(); return GRANNE_HIP_OK;
    }
    return fail(GRANNE_HIP_ERR_INVALID, "unknown option %d", option);
}
