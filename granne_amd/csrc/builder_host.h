// builder_host.h -- host side of the GPU GranneBuilder (included by granne_hip.hip).
// Restates the control flow of /root/reference/src/index/mod.rs:364-402 (build_partial),
// :634-643 (compute_num_elements_in_layer), :646-713 (index_elements_in_last_layer) and :715-802
// (index_elements) around the batched device kernels of builder_kernels.h.
#pragma once

#include <hipcub/hipcub.hpp>

#include <cmath>

#include "builder_kernels.h"

struct BuilderLayer {
    uint64_t len = 0;      // rows in use
    uint64_t cap_rows = 0; // rows allocated
    DevBuf d_adj;          // uint32_t [cap_rows][W]
};

struct granne_hip_builder {
    int device = 0;
    granne_hip_build_config cfg;
    uint32_t dim = 0;
    int dtype = 0;
    uint64_t n_elements = 0;
    uint32_t row_bytes = 0, row_stride = 0; // data bytes of a device row; bytes from one row to the next
    DevBuf d_elements;
    uint32_t W = 32; // device row width
    std::vector<BuilderLayer> layers;
    uint64_t hbm_bytes = 0;
    ScratchCache scratch; // the build's searches (search_launch)
    std::shared_ptr<SeDev> se; // made by granne_hip_builder_create_sum_embeddings: the container d_elements was materialised from
    // made with GRANNE_HIP_F16: the halves as an index keeps them (half_stride bytes apart). d_elements holds the rows they
    // stand for -- normalize(widen(row)), f32 -- and the build is the f32 build over those; get_index hands out the halves.
    DevBuf d_half;
    uint32_t half_bytes = 0, half_stride = 0;
};

extern "C" void granne_hip_build_config_default(granne_hip_build_config* c) {
    if (!c) return;
    c->layer_multiplier = 15.0f;
    c->expected_num_elements = 0;
    c->num_neighbors = 30;
    c->max_search = 200;
    c->reinsert_elements = 1;
    c->show_progress = 0;
    c->batch_max = 0;
    c->batch_div = 0;
}

// compute_num_elements_in_layer, src/index/mod.rs:634-643
static uint64_t num_elements_in_layer(uint64_t total, float layer_multiplier, uint64_t layer_idx) {
    double m = (double)layer_multiplier;
    double t = (double)total;
    double e = std::floor(std::log(t) / std::log(m)) - (double)layer_idx;
    double v = std::ceil(t / std::pow(m, e));
    uint64_t r;
    if (!(v >= 0.0)) r = 0;
    else if (v >= 18446744073709551615.0) r = UINT64_MAX;
    else r = (uint64_t)v;
    return r < total ? r : total;
}

static void destroy_builder(granne_hip_builder* b) {
    if (!b) return;
    DeviceGuard g(b->device);
    delete b;
}

static int builder_validate(granne_hip_builder** out, const granne_hip_build_config* cfg, uint64_t n, uint32_t dim,
                            int dtype) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!cfg) return fail(GRANNE_HIP_ERR_INVALID, "config is null");
    if (!known_dtype(dtype)) return fail(GRANNE_HIP_ERR_INVALID, "unknown dtype %d", dtype);
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many elements (src/index/mod.rs:420)");
    if (cfg->num_neighbors < 1 || cfg->num_neighbors > BUILD_MAX_NEIGHBORS)
        return fail(GRANNE_HIP_ERR_INVALID, "num_neighbors must be in [1, %u] on the GPU builder", BUILD_MAX_NEIGHBORS);
    if (cfg->max_search < 1 || cfg->max_search > BUILD_MAX_CAND)
        return fail(GRANNE_HIP_ERR_INVALID, "max_search must be in [1, %u] on the GPU builder", BUILD_MAX_CAND);
    if (!(cfg->layer_multiplier > 1.0f)) return fail(GRANNE_HIP_ERR_INVALID, "layer_multiplier must be > 1");
    if (cfg->batch_max > (1u << 20)) return fail(GRANNE_HIP_ERR_INVALID, "batch_max must be <= 2^20");
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_builder_create_device(granne_hip_builder** out, const granne_hip_build_config* cfg,
                                                const void* d_elements, uint64_t n_elements, uint32_t dim, int dtype,
                                                int device_id, void* stream) {
    int rc = builder_validate(out, cfg, n_elements, dim, dtype);
    if (rc) return rc;
    if (n_elements && !d_elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    GRANNE_HIP_ON_DEVICE(device_id);
    if (dtype == GRANNE_HIP_F16) {
        // rows of halves: R = normalize(widen(rows)) is made once, the f32 builder runs over R, and the halves are kept
        // in an index's layout for get_index. R lives as long as the builder.
        hipStream_t s = (hipStream_t)stream;
        DevBuf d_R;
        HIP_TRY(d_R.alloc((size_t)n_elements * dim * 4));
        rc = f16_rows_to_f32((const uint8_t*)d_elements, (uint64_t)dim * 2u, d_R.as<float>(), n_elements, dim, 1, s);
        if (rc == 0) rc = granne_hip_builder_create_device(out, cfg, d_R.get(), n_elements, dim, GRANNE_HIP_F32, device_id, stream); // synchronises
        else (void)hipStreamSynchronize(s);
        d_R.reset();
        if (rc) return rc;
        granne_hip_builder* b = *out;
        granne_hip_index tmp;
        tmp.device = device_id;
        tmp.dim = dim;
        tmp.dtype = GRANNE_HIP_F16;
        tmp.n_elements = n_elements;
        tmp.row_bytes = device_row_bytes(dim, GRANNE_HIP_F16);
        tmp.row_stride = device_row_stride(dim, GRANNE_HIP_F16);
        rc = upload_elements_from_device(&tmp, d_elements, s);
        if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "sync failed");
        b->d_half = std::move(tmp.d_elements);
        b->half_bytes = tmp.row_bytes;
        b->half_stride = tmp.row_stride;
        b->hbm_bytes += tmp.hbm_bytes;
        if (rc) {
            destroy_builder(b);
            *out = nullptr;
        }
        return rc;
    }
    granne_hip_builder* b = new granne_hip_builder();
    b->device = device_id;
    b->cfg = *cfg;
    if (b->cfg.batch_max == 0) b->cfg.batch_max = 65536;
    if (b->cfg.batch_div == 0) b->cfg.batch_div = 8;
    b->dim = dim;
    b->dtype = dtype;
    b->n_elements = n_elements;
    b->row_bytes = device_row_bytes(dim, dtype);
    b->row_stride = device_row_stride(dim, dtype);
    b->W = (cfg->num_neighbors + 31u) & ~31u;
    // reuse the index's element upload (re-layout to the padded device rows)
    granne_hip_index tmp;
    tmp.device = device_id;
    tmp.dim = dim;
    tmp.dtype = dtype;
    tmp.n_elements = n_elements;
    tmp.row_bytes = b->row_bytes;
    tmp.row_stride = b->row_stride;
    rc = upload_elements_from_device(&tmp, d_elements, (hipStream_t)stream);
    if (rc == 0 && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "sync failed");
    b->d_elements = std::move(tmp.d_elements);
    b->hbm_bytes = tmp.hbm_bytes;
    if (rc) {
        destroy_builder(b);
        return rc;
    }
    *out = b;
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_builder_create(granne_hip_builder** out, const granne_hip_build_config* cfg,
                                         const void* elements, uint64_t n_elements, uint32_t dim, int dtype,
                                         int device_id) {
    int rc = builder_validate(out, cfg, n_elements, dim, dtype);
    if (rc) return rc;
    if (n_elements && !elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    GRANNE_HIP_ON_DEVICE(device_id);
    DevBuf d;
    size_t bytes = (size_t)n_elements * dim * elem_size(dtype);
    HIP_TRY(d.alloc(bytes));
    hipError_t e = bytes ? hipMemcpy(d.get(), elements, bytes, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "element upload failed: %s", hipGetErrorString(e));
    return granne_hip_builder_create_device(out, cfg, d.get(), n_elements, dim, dtype, device_id, nullptr);
}

// Builder::push for a batch of rows (src/index/mod.rs:303-315, dense_vector.rs push): the element
// container grows, nothing is indexed until the next build.
extern "C" int granne_hip_builder_append(granne_hip_builder* b, const void* elements, uint64_t n_new) {
    if (!b) return fail(GRANNE_HIP_ERR_INVALID, "builder is null");
    if (n_new == 0) return GRANNE_HIP_OK;
    if (!elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    if (b->n_elements + n_new >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many elements (src/index/mod.rs:420)");
    if (b->d_half) return fail(GRANNE_HIP_ERR_INVALID, "builder_append has no form for GRANNE_HIP_F16 (angular_f16) rows: make a new builder over all the rows");
    GRANNE_HIP_ON_DEVICE(b->device);
    const size_t dense = (size_t)b->dim * elem_size(b->dtype);
    const size_t old_bytes = (size_t)b->n_elements * b->row_stride, add_bytes = (size_t)n_new * b->row_stride;
    DevBuf grown, staged;
    HIP_TRY(grown.alloc(old_bytes + add_bytes));
    HIP_TRY(staged.alloc(n_new * dense));
    HIP_TRY(hipMemcpy(staged.get(), elements, n_new * dense, hipMemcpyHostToDevice));
    if (old_bytes) HIP_TRY(hipMemcpyAsync(grown.get(), b->d_elements.get(), old_bytes, hipMemcpyDeviceToDevice, nullptr));
    if (dense == b->row_stride) {
        HIP_TRY(hipMemcpyAsync(grown.as<uint8_t>() + old_bytes, staged.get(), add_bytes, hipMemcpyDeviceToDevice, nullptr));
    } else {
        const uint64_t units = n_new * (b->row_stride / 16);
        hipLaunchKernelGGL(relayout_rows_kernel, dim3(grid_for(units, 256)), dim3(256), 0, nullptr,
                           staged.as<uint8_t>(), grown.as<uint8_t>() + old_bytes, n_new, (uint32_t)dense, b->row_stride);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipDeviceSynchronize());
    b->d_elements = std::move(grown);
    b->n_elements += n_new;
    b->hbm_bytes += add_bytes;
    return GRANNE_HIP_OK;
}

extern "C" void granne_hip_builder_destroy(granne_hip_builder* b) { destroy_builder(b); }
extern "C" uint64_t granne_hip_builder_len(const granne_hip_builder* b) {
    return (b && !b->layers.empty()) ? b->layers.back().len : 0;
}
extern "C" uint64_t granne_hip_builder_num_elements(const granne_hip_builder* b) { return b ? b->n_elements : 0; }
extern "C" uint32_t granne_hip_builder_num_layers(const granne_hip_builder* b) { return b ? (uint32_t)b->layers.size() : 0; }
extern "C" uint64_t granne_hip_builder_layer_len(const granne_hip_builder* b, uint32_t l) {
    return (b && l < b->layers.size()) ? b->layers[l].len : 0;
}

// ------------------------------------------------------------------------------------------------
// one index_elements pass (first insertion or reinsertion) over the last layer
// ------------------------------------------------------------------------------------------------
typedef void (*build_fn)(const BuildParams);
struct BuildKernels {
    build_fn select, apply, final_prune;
};
template <int DT, int DIM>
static BuildKernels build_kernels_of() {
    return {select_kernel<DT, DIM>, apply_kernel<DT, DIM>, final_prune_kernel<DT, DIM>};
}
static BuildKernels pick_build_kernels(int dtype, uint32_t dim) {
    if (dtype == GRANNE_HIP_I8) return build_kernels_of<DT_I8, 0>();
    switch (dim) {
    case 100: return build_kernels_of<DT_F32, 100>();
    case 200: return build_kernels_of<DT_F32, 200>();
    default: return build_kernels_of<DT_F32, 0>();
    }
}

struct BuildScratch {
    DevBuf s_ids, op_keys, op_vals, sorted_keys, sorted_vals; // uint64_t
    DevBuf s_dists;                                           // float
    DevBuf s_counts, seg_start, counters; // uint32_t; counters: [0]=n_seg [1]=status [2]=slow count
    DevBuf sort_tmp;
    size_t sort_tmp_bytes = 0;
    DevBuf d_layers; // LayerDev
    DevBuf selected; // uint8_t per row of the layer being built: BuildParams::selected
};

// the blocks of a BuildScratch that are sized by a batch: `members` elements searched with `max_search`, `n_ops_max`
// link updates sorted on `s`
static int alloc_batch_scratch(BuildScratch& S, uint64_t members, uint32_t max_search, uint64_t n_ops_max, hipStream_t s) {
    HIP_TRY(S.s_ids.alloc(members * max_search * 8));
    HIP_TRY(S.s_dists.alloc(members * max_search * 4));
    HIP_TRY(S.s_counts.alloc(members * 4));
    HIP_TRY(S.op_keys.alloc(n_ops_max * 8));
    HIP_TRY(S.op_vals.alloc(n_ops_max * 8));
    HIP_TRY(S.sorted_keys.alloc(n_ops_max * 8));
    HIP_TRY(S.sorted_vals.alloc(n_ops_max * 8));
    HIP_TRY(S.seg_start.alloc(n_ops_max * 4));
    HIP_TRY(S.counters.alloc(32));
    HIP_TRY(hipMemsetAsync(S.counters.get(), 0, 32, s));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, S.sort_tmp_bytes, S.op_keys.as<uint64_t>(), S.sorted_keys.as<uint64_t>(),
                                               S.op_vals.as<uint64_t>(), S.sorted_vals.as<uint64_t>(), (int)n_ops_max, 0, OP_KEY_BITS, s));
    HIP_TRY(S.sort_tmp.alloc(S.sort_tmp_bytes));
    return GRANNE_HIP_OK;
}

// What every launch of the three build kernels over one layer shares: the kernels of the row shape, the LDS carve-up
// and its sizes, and the BuildParams that do not change from one batch to the next.
struct BuildPlan {
    BuildKernels K;
    uint32_t lds = 0, lds_rows = 0; // dynamic LDS of select_kernel; of apply_kernel / final_prune_kernel (<= lds)
    BuildParams P;
};
static int make_build_plan(const granne_hip_builder* b, const BuilderLayer& L, uint32_t m_layer, uint32_t max_search,
                           const BuildScratch& S, uint8_t* selected, BuildPlan* out) {
    const uint32_t cap = b->cfg.num_neighbors;
    const uint32_t lrow = ((b->row_bytes / 16) | 1u) * 16u;
    const BuildKernels K = pick_build_kernels(b->dtype, b->dim);
    // (apply / final_prune only ever see cap + 1 candidates: their arrays keep the minimum size)
    const uint32_t cand_cap = build_cand_cap(max_search);
    // long rows stage fewer candidates per gather round (same results, more rounds): 32 up to 640-d f32, 16 at 768-d
    uint32_t sel_lds = cap; // the rows select_neighbors has selected stay in LDS -- all of them, unless they are too long for that
    uint32_t chunk = build_chunk_for(lrow, cap, cand_cap, 160u * 1024u);
    if (chunk == 0) {
        sel_lds = build_sel_lds_for(lrow, cap, cand_cap, 160u * 1024u);
        if (sel_lds >= cap)
            return fail(GRANNE_HIP_ERR_INVALID, "dimension too large for the GPU builder: select_neighbors stages the node's row and at "
                        "least 4 candidate rows of %u bytes in LDS (%u bytes, a CU has 163840)", lrow,
                        build_lds_bytes(lrow, cap, cand_cap, 4, 0u));
        chunk = 4;
    }
    const uint32_t lds = build_lds_bytes(lrow, cap, cand_cap, chunk, sel_lds);
    const uint32_t lds_rows = build_lds_bytes_rows(lrow, cap, cand_cap, chunk, sel_lds); // apply / final_prune (<= lds)
    if (lds > 64u * 1024u) {
        HIP_TRY(hipFuncSetAttribute((const void*)K.select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(hipFuncSetAttribute((const void*)K.apply, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIP_TRY(hipFuncSetAttribute((const void*)K.final_prune, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    out->K = K;
    out->lds = lds;
    out->lds_rows = lds_rows;
    BuildParams& P = out->P;
    P.elements = b->d_elements.as<uint8_t>();
    P.row_bytes = b->row_bytes;
    P.row_stride = b->row_stride;
    P.dim = b->dim;
    P.lrow = lrow;
    P.adj = L.d_adj.as<uint32_t>();
    P.W = b->W;
    P.cap = cap;
    P.m_layer = m_layer;
    P.layer_len = L.len;
    P.efc = max_search;
    P.s_ids = S.s_ids.as<uint64_t>();
    P.s_dists = S.s_dists.as<float>();
    P.s_counts = S.s_counts.as<uint32_t>();
    P.op_keys = S.op_keys.as<uint64_t>();
    P.op_vals = S.op_vals.as<uint64_t>();
    P.sorted_keys = S.sorted_keys.as<uint64_t>();
    P.sorted_vals = S.sorted_vals.as<uint64_t>();
    P.seg_start = S.seg_start.as<uint32_t>();
    P.n_seg = S.counters.as<uint32_t>();
    P.selected = selected;
    P.cand_cap = cand_cap;
    P.chunk = chunk;
    P.sel_lds = sel_lds;
    return GRANNE_HIP_OK;
}

static int index_elements_pass(granne_hip_builder* b, uint32_t m_layer, uint32_t max_search, bool reinsert,
                               uint64_t already, BuildScratch& S, hipStream_t s) {
    const uint32_t last = (uint32_t)b->layers.size() - 1;
    BuilderLayer& L = b->layers[last];
    const uint64_t layer_len = L.len;
    const uint32_t cap = b->cfg.num_neighbors;
    const uint64_t total = reinsert ? layer_len : layer_len - already;
    const uint32_t bmax = b->cfg.batch_max;
    BuildPlan plan;
    {
        int rc = make_build_plan(b, L, m_layer, max_search, S, S.selected.as<uint8_t>(), &plan);
        if (rc) return rc;
    }
    const BuildKernels K = plan.K;
    const uint32_t lds = plan.lds, lds_rows = plan.lds_rows;
    BuildParams& P = plan.P;

    const SearchTarget T(b, S.d_layers.as<LayerDev>(), last + 1);
    SearchCall call; // phase A's searches: max_search neighbors of each batch's rows, from the rows themselves
    call.ef = call.k = max_search;
    call.ids = S.s_ids.as<uint64_t>();
    call.dists = S.s_dists.as<float>();
    call.counts = S.s_counts.as<uint32_t>();
    call.status = P.n_seg + 1;
    call.stream = s;

    HIP_TRY(hipMemsetAsync(S.selected.get(), 0, layer_len ? layer_len : 1, s)); // nothing is known about the rows of a pass

    const bool debug = getenv("GRANNE_HIP_DEBUG") != nullptr;
    auto dbg = [&](const char* what, uint64_t pos_, uint64_t B_) {
        if (!debug) return;
        hipError_t e = hipStreamSynchronize(s);
        fprintf(stderr, "[granne_hip build] layer %u %s pos %llu batch %llu: %s\n", last, what,
                (unsigned long long)pos_, (unsigned long long)B_, hipGetErrorString(e));
        fflush(stderr);
    };
    uint64_t pos = 0;
    while (pos < total) {
        const uint64_t n_in_graph = reinsert ? layer_len : already + pos;
        uint64_t B = n_in_graph / b->cfg.batch_div;
        if (B < 1) B = 1;
        if (B > bmax) B = bmax;
        if (B > total - pos) B = total - pos;
        const int64_t first = reinsert ? (int64_t)(layer_len - 1 - pos) : (int64_t)(already + pos);
        const int64_t step = reinsert ? -1 : 1;

        // phase A: entry search through the previous layers + search_for_neighbors on this layer
        call.queries = P.elements + (size_t)first * b->row_stride;
        call.q_stride = step * (int64_t)b->row_stride;
        call.nq = (uint32_t)B;
        int rc = search_launch(T, call);
        if (rc) return rc;
        dbg("search", pos, B);
        P.first_idx = first;
        P.idx_step = step;
        P.batch = (uint32_t)B;
        P.n_ops = (uint32_t)(B * cap * 2);
        hipLaunchKernelGGL(K.select, dim3((uint32_t)B), dim3(64), lds, s, P);
        HIP_TRY(hipGetLastError());
        dbg("select", pos, B);

        // phase B: sort the ops by (target row, order), one wave per target row replays them
        size_t tmp_bytes = S.sort_tmp_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(S.sort_tmp.get(), tmp_bytes, P.op_keys, S.sorted_keys.as<uint64_t>(), P.op_vals,
                                                   S.sorted_vals.as<uint64_t>(), (int)P.n_ops, 0, OP_KEY_BITS, s));
        dbg("sort", pos, B);
        HIP_TRY(hipMemsetAsync(P.n_seg, 0, 4, s));
        hipLaunchKernelGGL(mark_heads_kernel, dim3(grid_for(P.n_ops, 256)), dim3(256), 0, s, P.sorted_keys, P.n_ops,
                           P.seg_start, P.n_seg);
        HIP_TRY(hipGetLastError());
        uint32_t grid = P.n_ops < 4096 ? P.n_ops : 4096;
        hipLaunchKernelGGL(K.apply, dim3(grid), dim3(64), lds_rows, s, P);
        HIP_TRY(hipGetLastError());
        dbg("apply", pos, B);
        pos += B;
    }
    // limit number of neighbors, src/index/mod.rs:795-797
    uint32_t grid = layer_len < 8192 ? (uint32_t)layer_len : 8192u;
    hipLaunchKernelGGL(K.final_prune, dim3(grid ? grid : 1), dim3(64), lds_rows, s, P);
    HIP_TRY(hipGetLastError());
    dbg("final_prune", total, 0);
    return GRANNE_HIP_OK;
}

// index_elements_in_last_layer, src/index/mod.rs:646-713
static int index_elements_in_last_layer(granne_hip_builder* b, uint64_t max_num_elements, hipStream_t s) {
    const uint64_t total = b->cfg.expected_num_elements ? b->cfg.expected_num_elements : b->n_elements;
    const uint64_t t2 = total > b->n_elements ? total : b->n_elements;
    const uint32_t last = (uint32_t)b->layers.size() - 1;
    BuilderLayer& L = b->layers[last];
    const uint64_t ideal = num_elements_in_layer(t2, b->cfg.layer_multiplier, last);
    if (ideal <= L.len) return GRANNE_HIP_OK; // nothing to index in this layer, :654-657
    const uint64_t num_in_layer = max_num_elements < ideal ? max_num_elements : ideal;
    uint32_t m_layer = b->cfg.num_neighbors;
    if (ideal < total) m_layer = m_layer / 2 > 1 ? m_layer / 2 : 1; // half num_neighbors on upper layers, :665-668
    uint32_t max_search = b->cfg.max_search;
    if (b->cfg.show_progress) {
        printf("Building layer %u with %llu elements...\n", last, (unsigned long long)num_in_layer);
        fflush(stdout);
    }

    // layer.resize(num_elements, UNUSED), :730 (capacity: `ideal` rows, :670)
    const uint64_t already = L.len;
    if (num_in_layer > L.cap_rows) {
        DevBuf nrows;
        size_t bytes = (size_t)ideal * b->W * 4;
        HIP_TRY(nrows.alloc(bytes));
        HIP_TRY(hipMemsetAsync(nrows.get(), 0xFF, bytes, s));
        if (L.len) HIP_TRY(hipMemcpyAsync(nrows.get(), L.d_adj.get(), (size_t)L.len * b->W * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
        b->hbm_bytes += bytes;
        if (L.d_adj) b->hbm_bytes -= (size_t)L.cap_rows * b->W * 4;
        L.d_adj = std::move(nrows);
        L.cap_rows = ideal;
    }
    L.len = num_in_layer;

    // scratch sized for the largest batch of this pass
    BuildScratch S;
    const uint64_t bmaxu = std::min<uint64_t>(b->cfg.batch_max, num_in_layer);
    const uint64_t n_ops_max = bmaxu * b->cfg.num_neighbors * 2;
    SettleStream settle{s}; // (declared after S: the stream is idle before an early return frees the scratch)
    int rc = alloc_batch_scratch(S, bmaxu, max_search, n_ops_max, s);
    if (rc) return rc;
    HIP_TRY(S.selected.alloc(num_in_layer));
    // layer table: finished layers + the one being built
    std::vector<LayerDev> h(last + 1);
    for (uint32_t l = 0; l <= last; ++l) {
        h[l].adj = b->layers[l].d_adj.as<uint32_t>();
        h[l].len = b->layers[l].len;
        h[l].width = b->W;
        h[l].flags = 0; // connect_nodes never lists a neighbor twice (mod.rs:913-917)
    }
    HIP_TRY(S.d_layers.alloc(sizeof(LayerDev) * h.size()));
    HIP_TRY(hipMemcpyAsync(S.d_layers.get(), h.data(), sizeof(LayerDev) * h.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));

    rc = index_elements_pass(b, m_layer, max_search, false, already, S, s);
    if (rc) return rc;
    if (b->cfg.reinsert_elements) { // :692-710
        if (b->cfg.show_progress) {
            printf("Reinserting elements...\n");
            fflush(stdout);
        }
        uint32_t ms2 = max_search / 2 > 1 ? max_search / 2 : 1;
        rc = index_elements_pass(b, m_layer, ms2, true, 0, S, s);
        if (rc) return rc;
    }
    uint32_t hc[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(hc, S.counters.get(), 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (hc[1]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted during build");
    return GRANNE_HIP_OK;
}

// build_partial, src/index/mod.rs:374-402
extern "C" int granne_hip_builder_build(granne_hip_builder* b, uint64_t num_elements) {
    if (!b) return fail(GRANNE_HIP_ERR_INVALID, "builder is null");
    if (num_elements == GRANNE_HIP_BUILD_ALL) num_elements = b->n_elements; // Builder::build(), mod.rs:370-372
    if (num_elements == 0) return GRANNE_HIP_OK; // build_partial(0) is a no-op, mod.rs:375
    if (num_elements > b->n_elements) return fail(GRANNE_HIP_ERR_INVALID, "Cannot index more elements than exist.");
    if (!b->layers.empty() && num_elements < b->layers.back().len)
        return fail(GRANNE_HIP_ERR_INVALID, "Cannot index fewer elements than already in index.");
    GRANNE_HIP_ON_DEVICE(b->device);
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    int rc = GRANNE_HIP_OK;
    if (!b->layers.empty()) rc = index_elements_in_last_layer(b, num_elements, s);
    while (rc == 0 && granne_hip_builder_len(b) < num_elements) {
        BuilderLayer nl; // with_width(num_neighbors) or prev_layer.clone(), :393-398
        if (!b->layers.empty()) {
            const BuilderLayer& pl = b->layers.back();
            size_t bytes = (size_t)pl.len * b->W * 4;
            hipError_t e = nl.d_adj.alloc(bytes);
            // on the builder's own stream: a device-to-device hipMemcpy on the null stream is
            // asynchronous and a non-blocking stream would not wait for it
            if (e == hipSuccess && bytes) e = hipMemcpyAsync(nl.d_adj.get(), pl.d_adj.get(), bytes, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) {
                rc = fail(GRANNE_HIP_ERR_HIP, "layer clone failed: %s", hipGetErrorString(e));
                break;
            }
            nl.len = pl.len;
            nl.cap_rows = pl.len;
        }
        if (b->layers.size() >= 64) {
            rc = fail(GRANNE_HIP_ERR_INVALID, "too many layers");
            break;
        }
        b->hbm_bytes += (size_t)nl.cap_rows * b->W * 4; // (counted once the clone is the builder's)
        b->layers.push_back(std::move(nl));
        rc = index_elements_in_last_layer(b, num_elements, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    return rc;
}

extern "C" int granne_hip_builder_get_layer(const granne_hip_builder* b, uint32_t layer, uint32_t* out_rows) {
    if (!b || !out_rows) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (layer >= b->layers.size()) return fail(GRANNE_HIP_ERR_INVALID, "layer out of range");
    DeviceGuard g(b->device);
    const BuilderLayer& L = b->layers[layer];
    const uint32_t nn = b->cfg.num_neighbors;
    HIP_TRY(hipMemcpy2D(out_rows, (size_t)nn * 4, L.d_adj.get(), (size_t)b->W * 4, (size_t)nn * 4, L.len, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_builder_get_index(const granne_hip_builder* b, granne_hip_index** out) {
    if (!b || !out) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    *out = nullptr;
    GRANNE_HIP_ON_DEVICE(b->device);
    IndexPtr made(new granne_hip_index());
    granne_hip_index* ix = made.get();
    ix->device = b->device;
    ix->dim = b->dim;
    ix->dtype = b->d_half ? GRANNE_HIP_F16 : b->dtype;
    ix->n_elements = b->n_elements;
    ix->row_bytes = b->d_half ? b->half_bytes : b->row_bytes;
    ix->row_stride = b->d_half ? b->half_stride : b->row_stride;
    size_t eb = (size_t)b->n_elements * ix->row_stride;
    HIP_TRY(ix->d_elements.alloc(eb));
    ix->hbm_bytes += eb;
    if (eb) HIP_TRY(hipMemcpy(ix->d_elements.get(), (b->d_half ? b->d_half : b->d_elements).get(), eb, hipMemcpyDeviceToDevice));
    for (const auto& BL : b->layers) {
        LayerHost L;
        L.len = BL.len;
        L.width = b->cfg.num_neighbors;
        L.dev_width = b->W;
        size_t bytes = (size_t)BL.len * b->W * 4;
        HIP_TRY(L.d_adj.alloc(bytes));
        ix->hbm_bytes += bytes;
        ix->layers.push_back(std::move(L));
        if (bytes) HIP_TRY(hipMemcpy(ix->layers.back().d_adj.get(), BL.d_adj.get(), bytes, hipMemcpyDeviceToDevice));
    }
    int rc = finish_layers(ix, nullptr);
    if (rc) return rc;
    *out = made.release();
    return GRANNE_HIP_OK;
}
