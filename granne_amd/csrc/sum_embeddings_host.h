// sum_embeddings_host.h -- embeddings::SumEmbeddings (/root/reference/src/elements/embeddings/mod.rs:41-216) on the host
// side (included by granne_hip.hip): the container handle, its two files, and the indexes and builders made from it.
//
//   elements file    src/slice_vector/mod.rs:623-634, 660-676 (VariableWidthSliceVector<ThreeByteInt, FiveByteInt>,
//                    odd_byte_int.rs:3-36): [u64 LE n][(n + 1) offsets, 5 bytes LE each, counted in ids, the first 0]
//                    [ids, 3 bytes LE each]
//   embeddings file  an ordinary f32 Vectors file ([u64 LE dim][rows], fileformat_host.h), rows NOT normalised
//
// The container keeps its table and term lists on the host (files, get_terms and append need no device) and uploads them
// once, when a device entry point first needs them (SeDev). A materialised index turns every element into its dense
// normalised row and is from there on an ordinary f32 index; a compact index keeps the SeDev instead of rows.
#pragma once

namespace granne_file {

constexpr uint64_t SE_MAX_EMBEDDINGS = 1ull << 24; // ThreeByteInt
constexpr uint64_t SE_MAX_OFFSET = 1ull << 40;     // FiveByteInt

static int se_decode_elements(const uint8_t* buf, uint64_t len, std::vector<uint64_t>* off, std::vector<uint32_t>* ids,
                              std::string* err) {
    if (len < 8) return *err = "elements file too small", -1;
    const uint64_t n = rd_u64(buf);
    if (n >= 0xFFFFFFFFull || (len - 8) / 5 < n + 1) return *err = "elements file: truncated offsets", -1;
    const uint8_t* po = buf + 8;
    off->resize(n + 1);
    for (uint64_t i = 0; i <= n; ++i) {
        uint64_t v = 0;
        for (int b = 4; b >= 0; --b) v = (v << 8) | po[i * 5 + b];
        (*off)[i] = v;
        if (i == 0 ? v != 0 : v < (*off)[i - 1]) return *err = "elements file: offsets must start at 0 and never decrease", -1;
    }
    const uint64_t rest = len - 8 - (n + 1) * 5, total = off->back();
    if (rest / 3 < total) return *err = "elements file: truncated ids", -1;
    const uint8_t* pi = po + (n + 1) * 5;
    ids->resize(total);
    for (uint64_t t = 0; t < total; ++t) (*ids)[t] = (uint32_t)pi[t * 3] | ((uint32_t)pi[t * 3 + 1] << 8) | ((uint32_t)pi[t * 3 + 2] << 16);
    return 0;
}

static void se_encode_elements(const std::vector<uint64_t>& off, const std::vector<uint32_t>& ids, std::vector<uint8_t>* out) {
    const uint64_t n = off.size() - 1;
    out->resize(8 + (n + 1) * 5 + ids.size() * 3);
    uint8_t* p = out->data();
    wr_u64(p, n);
    p += 8;
    for (uint64_t v : off)
        for (int b = 0; b < 5; ++b) *p++ = (uint8_t)(v >> (8 * b));
    for (uint32_t v : ids)
        for (int b = 0; b < 3; ++b) *p++ = (uint8_t)(v >> (8 * b));
}

} // namespace granne_file

struct granne_hip_sum_embeddings {
    int device = 0;
    uint32_t dim = 0;
    uint64_t n_embeddings = 0;
    std::vector<float> table;     // [V][dim]
    std::vector<uint64_t> offsets; // [n + 1]
    std::vector<uint32_t> terms;
    std::mutex mu;
    std::shared_ptr<SeDev> dev; // made at the first device use, dropped by append
};

// offsets[0] == 0, never decreasing; every term id < V
static int se_validate_csr(const uint64_t* offsets, const uint32_t* terms, uint64_t n, uint64_t n_embeddings) {
    if (!offsets) return fail(GRANNE_HIP_ERR_INVALID, "offsets is null");
    if (offsets[0] != 0) return fail(GRANNE_HIP_ERR_INVALID, "the first offset must be 0");
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(GRANNE_HIP_ERR_INVALID, "offsets decrease at element %llu", (unsigned long long)i);
    if (offsets[n] && !terms) return fail(GRANNE_HIP_ERR_INVALID, "terms is null");
    for (uint64_t t = 0; t < offsets[n]; ++t)
        if (terms[t] >= n_embeddings)
            return fail(GRANNE_HIP_ERR_INVALID, "term id %u is not below the number of embeddings (%llu)", terms[t], (unsigned long long)n_embeddings);
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_sum_embeddings_create(granne_hip_sum_embeddings** out, const float* table, uint64_t n_embeddings,
                                                uint32_t dim, const uint64_t* offsets, const uint32_t* terms,
                                                uint64_t n_elements, int device_id) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n_embeddings && !table) return fail(GRANNE_HIP_ERR_INVALID, "table is null");
    if (n_embeddings > 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many embeddings");
    if (n_elements >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many elements (reference limit, src/index/mod.rs:420)");
    const uint64_t zero = 0;
    if (n_elements == 0 && !offsets) offsets = &zero;
    int rc = se_validate_csr(offsets, terms, n_elements, n_embeddings);
    if (rc) return rc;
    auto* se = new granne_hip_sum_embeddings();
    se->device = device_id;
    se->dim = dim;
    se->n_embeddings = n_embeddings;
    se->table.assign(table, table + (size_t)n_embeddings * dim);
    se->offsets.assign(offsets, offsets + n_elements + 1);
    se->terms.assign(terms, terms + offsets[n_elements]);
    *out = se;
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_sum_embeddings_create_device(granne_hip_sum_embeddings** out, const float* d_table,
                                                       uint64_t n_embeddings, uint32_t dim, const uint64_t* d_offsets,
                                                       const uint32_t* d_terms, uint64_t n_elements, int device_id,
                                                       void* stream) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if ((n_embeddings && !d_table) || !d_offsets) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (n_embeddings > 0xFFFFFFFFull || n_elements >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many embeddings or elements");
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = (hipStream_t)stream;
    // the term lists are checked on the host before any kernel indexes the table with them
    std::vector<float> table((size_t)n_embeddings * dim);
    std::vector<uint64_t> offsets(n_elements + 1);
    HIP_TRY(hipMemcpyAsync(offsets.data(), d_offsets, offsets.size() * 8, hipMemcpyDeviceToHost, s));
    if (!table.empty()) HIP_TRY(hipMemcpyAsync(table.data(), d_table, table.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint32_t> terms(offsets[n_elements] < (1ull << 40) ? offsets[n_elements] : 0);
    if (offsets[n_elements] != terms.size()) return fail(GRANNE_HIP_ERR_INVALID, "offsets out of range");
    if (!terms.empty()) {
        if (!d_terms) return fail(GRANNE_HIP_ERR_INVALID, "terms is null");
        HIP_TRY(hipMemcpy(terms.data(), d_terms, terms.size() * 4, hipMemcpyDeviceToHost));
    }
    return granne_hip_sum_embeddings_create(out, table.data(), n_embeddings, dim, offsets.data(), terms.data(), n_elements, device_id);
}

// SumEmbeddings::from_files' element half: the bytes of an elements file over a table the caller holds
extern "C" int granne_hip_sum_embeddings_load(granne_hip_sum_embeddings** out, const float* table, uint64_t n_embeddings,
                                              uint32_t dim, const void* elements_bytes, uint64_t elements_len, int device_id) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!elements_bytes) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    std::vector<uint64_t> off;
    std::vector<uint32_t> ids;
    std::string err;
    if (granne_file::se_decode_elements((const uint8_t*)elements_bytes, elements_len, &off, &ids, &err))
        return fail(GRANNE_HIP_ERR_INVALID, "%s", err.c_str());
    return granne_hip_sum_embeddings_create(out, table, n_embeddings, dim, off.data(), ids.data(), off.size() - 1, device_id);
}

extern "C" int granne_hip_sum_embeddings_load_files(granne_hip_sum_embeddings** out, const char* embeddings_path,
                                                    const char* elements_path, int device_id) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!embeddings_path || !elements_path) return fail(GRANNE_HIP_ERR_INVALID, "null path");
    granne_file::MappedFile fe, fl;
    if (!fe.open_ro(embeddings_path)) return fail(GRANNE_HIP_ERR_IO, "Could not open embeddings file %s", embeddings_path);
    if (!fl.open_ro(elements_path)) return fail(GRANNE_HIP_ERR_IO, "Could not open elements file %s", elements_path);
    if (fe.len < 8) return fail(GRANNE_HIP_ERR_INVALID, "embeddings file too small");
    const uint64_t dim = granne_file::rd_u64(fe.data), payload = fe.len - 8;
    if (dim == 0 || dim > 0xFFFFFFFFull || payload % 4 != 0 || (payload / 4) % dim != 0)
        return fail(GRANNE_HIP_ERR_INVALID, "embeddings file: width %llu does not divide the data", (unsigned long long)dim);
    std::vector<float> table(payload / 4); // (the mapping's payload starts 8 bytes in: copied for alignment's sake)
    if (payload) memcpy(table.data(), fe.data + 8, payload);
    return granne_hip_sum_embeddings_load(out, table.data(), payload / 4 / dim, (uint32_t)dim, fl.data, fl.len, device_id);
}

extern "C" int granne_hip_sum_embeddings_save_elements(const granne_hip_sum_embeddings* se, const char* path) {
    if (!se || !path) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (se->n_embeddings > granne_file::SE_MAX_EMBEDDINGS)
        return fail(GRANNE_HIP_ERR_INVALID, "the elements file holds 3-byte term ids: at most 2^24 embeddings");
    if (se->offsets.back() >= granne_file::SE_MAX_OFFSET) return fail(GRANNE_HIP_ERR_INVALID, "the elements file holds 5-byte offsets: fewer than 2^40 ids");
    std::vector<uint8_t> buf;
    granne_file::se_encode_elements(se->offsets, se->terms, &buf);
    if (!granne_file::write_file(path, buf.data(), buf.size(), nullptr, 0)) return fail(GRANNE_HIP_ERR_IO, "Could not write %s", path);
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_sum_embeddings_save_embeddings(const granne_hip_sum_embeddings* se, const char* path) {
    if (!se || !path) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    return granne_hip_write_elements_file(path, se->table.data(), se->n_embeddings, se->dim, GRANNE_HIP_F32);
}

extern "C" void granne_hip_sum_embeddings_destroy(granne_hip_sum_embeddings* se) { delete se; }
extern "C" uint64_t granne_hip_sum_embeddings_len(const granne_hip_sum_embeddings* se) { return se ? se->offsets.size() - 1 : 0; }
extern "C" uint64_t granne_hip_sum_embeddings_num_embeddings(const granne_hip_sum_embeddings* se) { return se ? se->n_embeddings : 0; }
extern "C" uint32_t granne_hip_sum_embeddings_dim(const granne_hip_sum_embeddings* se) { return se ? se->dim : 0; }
extern "C" uint64_t granne_hip_sum_embeddings_hbm_bytes(const granne_hip_sum_embeddings* se) {
    if (!se) return 0;
    return se->n_embeddings * device_row_bytes(se->dim, GRANNE_HIP_F32) + se->offsets.size() * 8u + se->terms.size() * 4u;
}

extern "C" int granne_hip_sum_embeddings_get_terms(const granne_hip_sum_embeddings* se, uint64_t idx, uint32_t* out_terms,
                                                   uint32_t cap, uint32_t* out_count) {
    if (!se || !out_count) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (idx + 1 >= se->offsets.size()) return fail(GRANNE_HIP_ERR_INVALID, "element index out of range");
    const uint64_t b = se->offsets[idx], n = se->offsets[idx + 1] - b;
    *out_count = (uint32_t)(n < 0xFFFFFFFFull ? n : 0xFFFFFFFFull);
    for (uint64_t t = 0; t < n && t < cap && out_terms; ++t) out_terms[t] = se->terms[b + t];
    return GRANNE_HIP_OK;
}

// ExtendableElementContainer::push (embeddings/mod.rs:180-182) for n_new elements: offsets[n_new + 1] from 0
extern "C" int granne_hip_sum_embeddings_append(granne_hip_sum_embeddings* se, const uint64_t* offsets, const uint32_t* terms,
                                                uint64_t n_new) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    if (n_new == 0) return GRANNE_HIP_OK;
    if (se->offsets.size() - 1 + n_new >= 0xFFFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many elements (src/index/mod.rs:420)");
    int rc = se_validate_csr(offsets, terms, n_new, se->n_embeddings);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(se->mu);
    const uint64_t base = se->offsets.back();
    for (uint64_t i = 1; i <= n_new; ++i) se->offsets.push_back(base + offsets[i]);
    se->terms.insert(se->terms.end(), terms, terms + offsets[n_new]);
    se->dev.reset(); // (indexes and builders made before keep the copy they were made from)
    return GRANNE_HIP_OK;
}

// the container's device copy, uploaded once
static int se_device(const granne_hip_sum_embeddings* cse, std::shared_ptr<SeDev>* out) {
    auto* se = const_cast<granne_hip_sum_embeddings*>(cse);
    std::lock_guard<std::mutex> lk(se->mu);
    if (se->dev) return *out = se->dev, GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(se->device);
    auto d = std::make_shared<SeDev>();
    d->device = se->device;
    d->dim = se->dim;
    d->tstride = device_row_bytes(se->dim, GRANNE_HIP_F32) / 4u;
    d->n_embeddings = se->n_embeddings;
    d->n = se->offsets.size() - 1;
    d->n_terms = se->terms.size();
    const size_t tb = (size_t)d->n_embeddings * d->tstride * 4u;
    HIP_TRY(d->d_table.alloc(tb));
    HIP_TRY(d->d_offsets.alloc(se->offsets.size() * 8));
    HIP_TRY(d->d_terms.alloc(d->n_terms * 4));
    if (tb) {
        HIP_TRY(hipMemset(d->d_table.get(), 0, tb));
        HIP_TRY(hipMemcpy2D(d->d_table.get(), (size_t)d->tstride * 4u, se->table.data(), (size_t)se->dim * 4u, (size_t)se->dim * 4u,
                            d->n_embeddings, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(d->d_offsets.get(), se->offsets.data(), se->offsets.size() * 8, hipMemcpyHostToDevice));
    if (d->n_terms) HIP_TRY(hipMemcpy(d->d_terms.get(), se->terms.data(), d->n_terms * 4, hipMemcpyHostToDevice));
    se->dev = d;
    *out = d;
    return GRANNE_HIP_OK;
}

// sum_embeddings_rows_kernel over the term lists (d_offsets, d_terms) and the container's table
static int se_rows_launch(const SeDev& d, const uint64_t* d_offsets, const uint32_t* d_terms, uint64_t first, uint64_t count,
                          int normalised, float* d_out, uint64_t stride, hipStream_t s) {
    if (count == 0) return GRANNE_HIP_OK;
    if (!d_out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    if (stride < d.dim) return fail(GRANNE_HIP_ERR_INVALID, "the row stride (%llu floats) is below dim (%u)", (unsigned long long)stride, d.dim);
    const uint32_t lstride = d.dim | 1u;
    uint32_t rpp = (60u * 1024u) / (lstride * 4u);
    if (rpp > 64) rpp = 64;
    if (rpp < 1) return fail(GRANNE_HIP_ERR_INVALID, "dim too large");
    uint64_t blocks = (count + rpp - 1) / rpp;
    if (blocks > 256u * 32u) blocks = 256u * 32u;
    const SeView v{d.d_table.as<float>(), d_offsets, d_terms, d.tstride, (uint32_t)d.n_embeddings};
    hipLaunchKernelGGL(sum_embeddings_rows_kernel, dim3((uint32_t)blocks), dim3(64), rpp * lstride * 4u, s, v, first, count, d.dim,
                       normalised, d_out, stride, rpp, lstride);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

static int se_rows_to_host(const SeDev& d, uint64_t first, uint64_t count, int normalised, float* out) {
    if (count == 0) return GRANNE_HIP_OK;
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    GRANNE_HIP_ON_DEVICE(d.device);
    DevBuf d_out;
    const size_t bytes = (size_t)count * d.dim * 4u;
    HIP_TRY(d_out.alloc(bytes));
    int rc = se_rows_launch(d, d.d_offsets.as<uint64_t>(), d.d_terms.as<uint32_t>(), first, count, normalised, d_out.as<float>(), d.dim, nullptr);
    if (rc == 0 && hipMemcpy(out, d_out.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMemcpy failed");
    return rc;
}

// get_embedding (normalised = 0, embeddings/mod.rs:113-115) / ElementContainer::get (normalised = 1, :164-166) of elements
// first .. first + count - 1 as dense device rows of `stride` floats
extern "C" int granne_hip_sum_embeddings_materialize_device(const granne_hip_sum_embeddings* se, uint64_t first, uint64_t count,
                                                            int normalised, float* d_out, uint64_t stride, void* stream) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    const uint64_t n = se->offsets.size() - 1;
    if (first > n || count > n - first) return fail(GRANNE_HIP_ERR_INVALID, "elements out of range");
    if (count == 0) return GRANNE_HIP_OK;
    std::shared_ptr<SeDev> d;
    int rc = se_device(se, &d);
    if (rc) return rc;
    DeviceGuard g(d->device);
    return se_rows_launch(*d, d->d_offsets.as<uint64_t>(), d->d_terms.as<uint32_t>(), first, count, normalised, d_out, stride, (hipStream_t)stream);
}

extern "C" int granne_hip_sum_embeddings_materialize(const granne_hip_sum_embeddings* se, uint64_t first, uint64_t count,
                                                     int normalised, float* out) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    const uint64_t n = se->offsets.size() - 1;
    if (first > n || count > n - first) return fail(GRANNE_HIP_ERR_INVALID, "elements out of range");
    if (count == 0) return GRANNE_HIP_OK;
    std::shared_ptr<SeDev> d;
    int rc = se_device(se, &d);
    if (rc) return rc;
    return se_rows_to_host(*d, first, count, normalised, out);
}

// create_embedding (embeddings/mod.rs:118-120) for nq caller-supplied term lists (device CSR: d_offsets[nq + 1] from 0).
// The ids index the container's table: one that is not below num_embeddings contributes nothing.
extern "C" int granne_hip_sum_embeddings_embed_device(const granne_hip_sum_embeddings* se, const uint64_t* d_offsets,
                                                      const uint32_t* d_terms, uint64_t nq, int normalised, float* d_out,
                                                      uint64_t stride, void* stream) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_offsets || !d_terms) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    std::shared_ptr<SeDev> d;
    int rc = se_device(se, &d);
    if (rc) return rc;
    DeviceGuard g(d->device);
    return se_rows_launch(*d, d_offsets, d_terms, 0, nq, normalised, d_out, stride, (hipStream_t)stream);
}

// the same with host buffers in and out (synchronous); the term lists are checked like the container's own
extern "C" int granne_hip_sum_embeddings_embed(const granne_hip_sum_embeddings* se, const uint64_t* offsets, const uint32_t* terms,
                                               uint64_t nq, int normalised, float* out) {
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    int rc = se_validate_csr(offsets, terms, nq, se->n_embeddings);
    if (rc) return rc;
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    DeviceGuard g(d->device);
    DevBuf d_off, d_terms, d_out;
    const size_t nt = (size_t)offsets[nq], bytes = (size_t)nq * d->dim * 4u;
    HIP_TRY(d_off.alloc((nq + 1) * 8));
    HIP_TRY(d_terms.alloc(nt * 4));
    HIP_TRY(d_out.alloc(bytes));
    HIP_TRY(hipMemcpy(d_off.get(), offsets, (nq + 1) * 8, hipMemcpyHostToDevice));
    if (nt) HIP_TRY(hipMemcpy(d_terms.get(), terms, nt * 4, hipMemcpyHostToDevice));
    rc = se_rows_launch(*d, d_off.as<uint64_t>(), d_terms.as<uint32_t>(), 0, nq, normalised, d_out.as<float>(), d->dim, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, d_out.get(), bytes, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

// An index over a container from layers in DEVICE memory ([len][width] u32 rows, UNUSED padded). Materialised: the
// normalised rows are made on the device and granne_hip_index_create_device takes over. Compact: the index keeps the
// container's device copy in place of rows; its layers are laid out and checked the same way.
static int se_index_from_device_layers(granne_hip_index** out, const std::shared_ptr<SeDev>& d, uint32_t n_layers,
                                       const uint64_t* layer_len, const uint32_t* const* d_layer_rows, const uint32_t* layer_width,
                                       int mode, hipStream_t s) {
    int rc = validate_common(out, d->n, d->dim, GRANNE_HIP_F32, n_layers, layer_len);
    if (rc) return rc;
    if (n_layers && (!d_layer_rows || !layer_width)) return fail(GRANNE_HIP_ERR_INVALID, "layer arrays are null");
    if (mode != GRANNE_HIP_SE_MATERIALIZED && mode != GRANNE_HIP_SE_COMPACT) return fail(GRANNE_HIP_ERR_INVALID, "unknown mode %d", mode);
    GRANNE_HIP_ON_DEVICE(d->device);
    if (mode == GRANNE_HIP_SE_MATERIALIZED) {
        DevBuf d_rows;
        HIP_TRY(d_rows.alloc((size_t)d->n * d->dim * 4u));
        rc = se_rows_launch(*d, d->d_offsets.as<uint64_t>(), d->d_terms.as<uint32_t>(), 0, d->n, 1, d_rows.as<float>(), d->dim, s);
        if (rc == 0)
            rc = granne_hip_index_create_device(out, d_rows.get(), d->n, d->dim, GRANNE_HIP_F32, n_layers, layer_len, d_layer_rows,
                                                layer_width, d->device, s); // synchronises s
        else
            (void)hipStreamSynchronize(s);
        return rc;
    }
    granne_hip_index* ix = new granne_hip_index();
    ix->device = d->device;
    ix->dim = d->dim;
    ix->dtype = GRANNE_HIP_F32;
    ix->n_elements = d->n;
    ix->row_bytes = d->tstride * 4u; // the table's row pitch: what the walkers stage a vector in
    ix->row_stride = ix->row_bytes;
    ix->se = d;
    ix->hbm_bytes += d->bytes();
    DevBuf bad_buf; // neighbor ids outside their layer, as granne_hip_index_create_device looks for them
    if (bad_buf.alloc(4) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMalloc failed");
    uint32_t* const d_bad = bad_buf.as<uint32_t>();
    if (rc == 0 && hipMemsetAsync(d_bad, 0, 4, s) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMemsetAsync failed");
    for (uint32_t l = 0; rc == 0 && l < n_layers; ++l) {
        rc = add_layer_from_device_rows(ix, layer_len[l], layer_width[l], d_layer_rows[l], s);
        const uint64_t total = layer_len[l] * layer_width[l];
        if (rc == 0 && total)
            hipLaunchKernelGGL(check_adj_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, d_layer_rows[l], total, layer_len[l], d_bad);
    }
    if (rc == 0) rc = finish_layers(ix, s); // synchronises s
    uint32_t bad = 0;
    if (rc == 0 && hipMemcpy(&bad, d_bad, 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMemcpy failed");
    if (rc == 0 && bad) rc = fail(GRANNE_HIP_ERR_INVALID, "%u neighbor ids lie outside their layer", bad);
    if (rc) {
        destroy_index(ix);
        return rc;
    }
    *out = ix;
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_index_create_sum_embeddings(granne_hip_index** out, const granne_hip_sum_embeddings* se,
                                                      uint32_t n_layers, const uint64_t* layer_len,
                                                      const uint32_t* const* layer_rows, const uint32_t* layer_width, int mode) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    if (n_layers && (!layer_len || !layer_rows || !layer_width)) return fail(GRANNE_HIP_ERR_INVALID, "layer arrays are null");
    if (mode != GRANNE_HIP_SE_MATERIALIZED && mode != GRANNE_HIP_SE_COMPACT) return fail(GRANNE_HIP_ERR_INVALID, "unknown mode %d", mode);
    int rc = validate_common(out, se->offsets.size() - 1, se->dim, GRANNE_HIP_F32, n_layers, layer_len);
    if (rc) return rc;
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    DeviceGuard g(d->device);
    std::vector<DevBuf> staged(n_layers);
    std::vector<const uint32_t*> d_rows(n_layers, nullptr);
    hipError_t e = hipSuccess;
    for (uint32_t l = 0; e == hipSuccess && l < n_layers; ++l) {
        const size_t b = (size_t)layer_len[l] * layer_width[l] * 4;
        e = staged[l].alloc(b);
        d_rows[l] = staged[l].as<uint32_t>();
        if (e == hipSuccess && b) e = hipMemcpy(staged[l].get(), layer_rows[l], b, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "staging upload failed: %s", hipGetErrorString(e));
    return se_index_from_device_layers(out, d, n_layers, layer_len, d_rows.data(), layer_width, mode, nullptr);
}

// Granne::from_file over a SumEmbeddings container: index file + embeddings file + elements file
extern "C" int granne_hip_index_load_files_sum_embeddings(granne_hip_index** out, const char* index_path,
                                                          const char* embeddings_path, const char* elements_path, int mode,
                                                          int device_id) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!index_path) return fail(GRANNE_HIP_ERR_INVALID, "null path");
    granne_hip_sum_embeddings* se = nullptr;
    int rc = granne_hip_sum_embeddings_load_files(&se, embeddings_path, elements_path, device_id);
    if (rc) return rc;
    std::unique_ptr<granne_hip_sum_embeddings> owner(se);
    granne_file::MappedFile fi;
    if (!fi.open_ro(index_path)) return fail(GRANNE_HIP_ERR_IO, "Could not open index file %s", index_path);
    std::vector<granne_file::DecodedLayer> layers;
    std::string err;
    if (granne_file::decode_index(fi.data, fi.len, &layers, &err)) return fail(GRANNE_HIP_ERR_IO, "index file: %s", err.c_str());
    // the decoded neighbor lists as fixed-width rows, UNUSED padded (what a builder holds)
    const size_t nl = layers.size();
    std::vector<uint64_t> lens(nl);
    std::vector<uint32_t> widths(nl);
    std::vector<std::vector<uint32_t>> rows(nl);
    std::vector<const uint32_t*> ptrs(nl);
    for (size_t l = 0; l < nl; ++l) {
        const auto& L = layers[l];
        lens[l] = L.offsets.size() - 1;
        uint64_t w = 0;
        for (uint64_t i = 0; i < lens[l]; ++i) w = std::max<uint64_t>(w, L.offsets[i + 1] - L.offsets[i]);
        if (w > 0xFFFF) return fail(GRANNE_HIP_ERR_IO, "index file: degree too large");
        widths[l] = (uint32_t)w;
        rows[l].assign((size_t)lens[l] * w, GRANNE_HIP_UNUSED);
        for (uint64_t i = 0; i < lens[l]; ++i)
            for (uint64_t t = L.offsets[i]; t < L.offsets[i + 1]; ++t) rows[l][i * w + (t - L.offsets[i])] = L.ids[t];
        ptrs[l] = rows[l].data();
    }
    return granne_hip_index_create_sum_embeddings(out, se, (uint32_t)nl, lens.data(), ptrs.data(), widths.data(), mode);
}

// GranneBuilder::new(config, sum_embeddings): the existing builder over the materialised (normalised) rows; the builder
// remembers the container's device copy so that granne_hip_builder_get_index_compact can hand it on
extern "C" int granne_hip_builder_create_sum_embeddings(granne_hip_builder** out, const granne_hip_build_config* config,
                                                        const granne_hip_sum_embeddings* se) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!se) return fail(GRANNE_HIP_ERR_INVALID, "container is null");
    int rc = builder_validate(out, config, se->offsets.size() - 1, se->dim, GRANNE_HIP_F32);
    if (rc) return rc;
    std::shared_ptr<SeDev> d;
    rc = se_device(se, &d);
    if (rc) return rc;
    DeviceGuard g(d->device);
    DevBuf d_rows;
    HIP_TRY(d_rows.alloc((size_t)d->n * d->dim * 4u));
    rc = se_rows_launch(*d, d->d_offsets.as<uint64_t>(), d->d_terms.as<uint32_t>(), 0, d->n, 1, d_rows.as<float>(), d->dim, nullptr);
    if (rc == 0) rc = granne_hip_builder_create_device(out, config, d_rows.get(), d->n, d->dim, GRANNE_HIP_F32, d->device, nullptr); // synchronises
    else (void)hipDeviceSynchronize();
    if (rc == 0) (*out)->se = d;
    return rc;
}

// GranneBuilder::get_index as a COMPACT index over the builder's current layers: the layers are copied, the container's
// device copy is shared, the builder keeps everything it holds
extern "C" int granne_hip_builder_get_index_compact(const granne_hip_builder* b, granne_hip_index** out) {
    if (!b || !out) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!b->se) return fail(GRANNE_HIP_ERR_INVALID, "the builder was not made from a SumEmbeddings container");
    if (b->se->n != b->n_elements) return fail(GRANNE_HIP_ERR_INVALID, "rows were appended to the builder: its container no longer describes them");
    std::vector<uint64_t> lens;
    std::vector<uint32_t> widths;
    std::vector<const uint32_t*> ptrs;
    for (const auto& L : b->layers) {
        lens.push_back(L.len);
        widths.push_back(b->W); // (the builder's rows are W ids wide, UNUSED beyond num_neighbors)
        ptrs.push_back(L.d_adj.as<uint32_t>());
    }
    return se_index_from_device_layers(out, b->se, (uint32_t)lens.size(), lens.data(), ptrs.data(), widths.data(), GRANNE_HIP_SE_COMPACT, nullptr);
}
