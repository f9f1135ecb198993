// granne.hpp -- C++17 host-side mirror of granne's Rust API for the search path, over the C ABI of
// include/granne_hip.h. The reference is Rust (no toolchain in this environment); this header
// keeps its names, argument meaning and error behaviour so that code -- and tests -- read like the
// reference's:
//
//   granne::angular::Vector / Vectors          src/elements/angular.rs, dense_vector.rs
//   granne::angular_int::Vector / Vectors      src/elements/angular_int.rs
//   granne::BuildConfig                        src/index/mod.rs:198-291 (fluent setters)
//   granne::GranneBuilder<Elements>            src/index/mod.rs:293-531   (build, build_partial, get_index, ...)
//   granne::Granne<Elements>                   src/index/mod.rs:38-185    (search, len, num_layers, ...)
//
// Where the reference panics (max_search == 0, malformed files) these throw std::runtime_error
// carrying granne_hip_last_error(). Vectors own host copies of their rows (like the Rust
// `Vectors<'static>`); a Granne/GranneBuilder owns the device copies.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include <type_traits>

#include "granne_hip.h"

namespace granne {

inline void check(int rc) {
    if (rc != GRANNE_HIP_OK) throw std::runtime_error(std::string("granne_hip: ") + granne_hip_last_error());
}

// One IEEE binary16 value of an "angular_f16" element set (GRANNE_HIP_F16): its bits. The element a row of them stands for
// is angular::Vector::from(widen(row)), normalised where it is read.
struct f16 {
    uint16_t bits;
};

namespace detail {
// a GranneBuilder's handle, until an RwGranneBuilder takes it over
struct BuilderDeleter {
    bool armed = true;
    void operator()(granne_hip_builder* b) const { if (armed) granne_hip_builder_destroy(b); }
};
template <class Scalar> struct dtype_of;
template <> struct dtype_of<float> { static constexpr int value = GRANNE_HIP_F32; };
template <> struct dtype_of<int8_t> { static constexpr int value = GRANNE_HIP_I8; };
template <> struct dtype_of<f16> { static constexpr int value = GRANNE_HIP_F16; };

// dense_vector! (src/elements/dense_vector.rs): Vector = one row, Vectors = row-major collection
template <class Scalar>
struct Vector {
    std::vector<Scalar> data;
    size_t len() const { return data.size(); }
    const Scalar* as_slice() const { return data.data(); }
};

template <class Scalar>
class Vectors {
public:
    using Element = Vector<Scalar>;
    Vectors() = default;
    // Vectors::from_vec(vec, dim): rows are taken as stored (already normalised / quantised)
    static Vectors from_vec(std::vector<Scalar> v, size_t dim) {
        if (dim == 0 || v.size() % dim != 0) throw std::runtime_error("dim must be non-zero and divide the length");
        Vectors r;
        r.dim_ = dim;
        r.data_ = std::move(v);
        return r;
    }
    void push(const Element& e) { // the dimension is set by the first vector pushed
        if (dim_ == 0) dim_ = e.len();
        if (e.len() != dim_) throw std::runtime_error("dimension mismatch");
        data_.insert(data_.end(), e.data.begin(), e.data.end());
    }
    size_t len() const { return dim_ ? data_.size() / dim_ : 0; }
    size_t dim() const { return dim_; }
    Element get_element(size_t i) const { return Element{std::vector<Scalar>(data_.begin() + i * dim_, data_.begin() + (i + 1) * dim_)}; }
    const Scalar* as_slice() const { return data_.data(); }

private:
    size_t dim_ = 0;
    std::vector<Scalar> data_;
};
} // namespace detail

namespace angular {
using Vector = detail::Vector<float>;
using Vectors = detail::Vectors<float>;
// impl From<Vec<f32>> for Vector (angular.rs:55-61): normalised on construction, on the device
inline Vector from(std::vector<float> v, int device = 0) {
    if (!v.empty()) check(granne_hip_normalize_f32(v.data(), 1, (uint32_t)v.size(), device));
    return Vector{std::move(v)};
}
} // namespace angular

namespace angular_int {
using Vector = detail::Vector<int8_t>;
using Vectors = detail::Vectors<int8_t>;
// Vector::quantize (angular_int.rs:27-45)
inline Vector from(const std::vector<float>& v, int device = 0) {
    Vector r{std::vector<int8_t>(v.size())};
    if (!v.empty()) check(granne_hip_quantize_f32(v.data(), r.data.data(), 1, (uint32_t)v.size(), device));
    return r;
}
} // namespace angular_int

// Rows of halves: the conversions. There is deliberately no angular_f16::Vectors: the class templates below take their
// queries in the element type of their Elements, and the queries of an F16 index are prepared f32 rows (angular::Vector),
// so Granne / GranneBuilder / RefinedGranne / ShardedGranne over f16 elements are rejected at compile time. An F16 index is
// made and searched through the C entry points with detail::dtype_of<f16>::value (GRANNE_HIP_F16) and f32 queries.
namespace angular_f16 {
// f32 rows [n][dim] -> halves, rounded to nearest even, on the device
inline std::vector<f16> to_f16(const std::vector<float>& rows, size_t dim, int device = 0) {
    std::vector<f16> out(rows.size());
    if (!rows.empty()) check(granne_hip_f32_to_f16(rows.data(), reinterpret_cast<uint16_t*>(out.data()), rows.size() / dim, (uint32_t)dim, device));
    return out;
}
// halves -> the f32 rows they stand for: widened exactly, then (normalised) angular::Vector::from per row
inline std::vector<float> from_f16(const std::vector<f16>& rows, size_t dim, bool normalised = true, int device = 0) {
    std::vector<float> out(rows.size());
    if (!rows.empty())
        check(granne_hip_f16_to_f32(reinterpret_cast<const uint16_t*>(rows.data()), out.data(), rows.size() / dim, (uint32_t)dim, normalised ? 1 : 0, device));
    return out;
}
} // namespace angular_f16

// BuildConfig (src/index/mod.rs:198-291)
class BuildConfig {
public:
    BuildConfig() { granne_hip_build_config_default(&c_); }
    static BuildConfig new_() { return BuildConfig(); }
    BuildConfig num_neighbors(size_t n) const { BuildConfig r = *this; r.c_.num_neighbors = (uint32_t)n; return r; }
    BuildConfig max_search(size_t n) const { BuildConfig r = *this; r.c_.max_search = (uint32_t)n; return r; }
    BuildConfig expected_num_elements(size_t n) const { BuildConfig r = *this; r.c_.expected_num_elements = n; return r; }
    BuildConfig layer_multiplier(float m) const { BuildConfig r = *this; r.c_.layer_multiplier = m; return r; }
    BuildConfig reinsert_elements(bool yes) const { BuildConfig r = *this; r.c_.reinsert_elements = yes; return r; }
    BuildConfig show_progress(bool yes) const { BuildConfig r = *this; r.c_.show_progress = yes; return r; }
    const granne_hip_build_config& raw() const { return c_; }

private:
    granne_hip_build_config c_;
};

namespace detail {
// device memory of the library's allocator, freed with the object
class DeviceMem {
public:
    DeviceMem(size_t bytes, int device) : device_(device) { check(granne_hip_device_malloc(&p_, bytes, device)); }
    DeviceMem(DeviceMem&& o) noexcept : p_(o.p_), device_(o.device_) { o.p_ = nullptr; }
    DeviceMem(const DeviceMem&) = delete;
    DeviceMem& operator=(const DeviceMem&) = delete;
    ~DeviceMem() { granne_hip_device_free(p_, device_); }
    void* get() const { return p_; }
    void upload(const void* src, size_t bytes) const {
        check(granne_hip_copy_to_device(p_, src, bytes, device_, nullptr));
        check(granne_hip_stream_synchronize(nullptr, device_));
    }
    void download(void* dst, size_t bytes, size_t offset = 0) const {
        check(granne_hip_copy_to_host(dst, (const char*)p_ + offset, bytes, device_, nullptr));
        check(granne_hip_stream_synchronize(nullptr, device_));
    }

private:
    void* p_ = nullptr;
    int device_;
};
} // namespace detail

template <class Elements>
class RwGranneBuilder;

// An id bitmap in device memory for Granne::search_filtered (granne_hip.h, "filtered search"): bit (id & 31) of u32 word
// (id >> 5) over the ids 0..n-1, made and counted by the library's kernels.
class Filter {
public:
    // the bits of `ids` set; duplicates are harmless, ids >= n are left out and counted in *bad
    static Filter from_ids(const std::vector<uint64_t>& ids, size_t n, int device = 0, uint32_t* bad = nullptr) {
        Filter f(n, device);
        detail::DeviceMem d_ids(ids.size() * 8 + 8, device), d_bad(4, device);
        const uint32_t zero = 0;
        d_ids.upload(ids.data(), ids.size() * 8);
        d_bad.upload(&zero, 4);
        check(granne_hip_filter_from_ids_device((const uint64_t*)d_ids.get(), ids.size(), n, f.words(), (uint32_t*)d_bad.get(), device, nullptr));
        uint32_t b = 0;
        d_bad.download(&b, 4);
        if (bad) *bad = b;
        return f;
    }
    // one entry per id, true = allowed
    static Filter from_mask(const std::vector<bool>& mask, int device = 0) {
        Filter f(mask.size(), device);
        std::vector<uint8_t> bytes(mask.begin(), mask.end());
        detail::DeviceMem d_mask(bytes.size() + 1, device);
        d_mask.upload(bytes.data(), bytes.size());
        check(granne_hip_filter_from_mask_device((const uint8_t*)d_mask.get(), mask.size(), f.words(), device, nullptr));
        check(granne_hip_stream_synchronize(nullptr, device));
        return f;
    }
    // number of allowed ids
    uint64_t count() const {
        detail::DeviceMem d_out(8, device_);
        check(granne_hip_filter_count_device(words(), n_, (uint64_t*)d_out.get(), device_, nullptr));
        uint64_t c = 0;
        d_out.download(&c, 8);
        return c;
    }
    // the allowed ids, ascending: what from_ids would take back
    std::vector<uint64_t> ids() const {
        detail::DeviceMem d_ids(n_ * 8 + 8, device_), d_count(8, device_);
        check(granne_hip_filter_to_ids_device(words(), n_, (uint64_t*)d_ids.get(), (uint64_t*)d_count.get(), device_, nullptr));
        uint64_t m = 0;
        d_count.download(&m, 8);
        std::vector<uint64_t> out((size_t)m);
        if (m) d_ids.download(out.data(), (size_t)m * 8);
        return out;
    }
    size_t len() const { return n_; }
    int device() const { return device_; }
    uint32_t* words() const { return (uint32_t*)mem_.get(); } // device pointer

private:
    template <class> friend class RwGranneBuilder; // (alive_filter)
    Filter(size_t n, int device) : n_(n), device_(device), mem_(words_of(n) * 4, device) {}
    Filter(size_t n, size_t room, int device) : n_(n), device_(device), mem_(words_of(room > n ? room : n) * 4, device) {}
    static size_t words_of(size_t n) {
        uint64_t w = 0;
        check(granne_hip_filter_words(n, &w));
        return (size_t)w;
    }
    size_t n_;
    int device_;
    detail::DeviceMem mem_;
};

// Granne (src/index/mod.rs:38-185): search + the Index trait
template <class Elements>
class Granne {
public:
    using Element = typename Elements::Element;
    static_assert(!std::is_same<typename decltype(Element::data)::value_type, f16>::value,
                  "an index over f16 rows takes f32 queries: use the C entry points with GRANNE_HIP_F16");
    explicit Granne(granne_hip_index* h) : h_(h, granne_hip_index_destroy) {}

    // Granne::from_file (mod.rs:122-135) over Vectors::from_file
    static Granne from_file(const std::string& index_path, const std::string& elements_path, int device = 0) {
        granne_hip_index* h = nullptr;
        check(granne_hip_index_load_files(&h, index_path.c_str(), elements_path.c_str(), dtype(), device));
        return Granne(h);
    }
    // from_file through the device codec: read in pieces into a pinned ring of staging_bytes (0: the library's default),
    // decoded on the GPU; info (optional, u64[4]): layers on the device / host codec, peak device scratch, peak host staging
    static Granne load_files_on_device(const std::string& index_path, const std::string& elements_path, int device = 0,
                                       uint64_t staging_bytes = 0, uint64_t* info = nullptr) {
        granne_hip_index* h = nullptr;
        check(granne_hip_index_load_files_on_device(&h, index_path.c_str(), elements_path.c_str(), dtype(), device, staging_bytes, info));
        return Granne(h);
    }
    // Granne::from_bytes (mod.rs:106-113)
    static Granne from_bytes(const void* index, size_t index_len, const void* elements, size_t elements_len, int device = 0) {
        granne_hip_index* h = nullptr;
        check(granne_hip_index_load(&h, index, index_len, elements, elements_len, dtype(), device));
        return Granne(h);
    }

    // Granne::search(&element, max_search, num_neighbors) -> Vec<(usize, f32)> (mod.rs:140-150)
    std::vector<std::pair<size_t, float>> search(const Element& element, size_t max_search, size_t num_neighbors) const {
        return std::move(search_batch(&element, 1, max_search, num_neighbors)[0]);
    }
    // nq independent searches in one launch
    std::vector<std::vector<std::pair<size_t, float>>> search_batch(const Element* elements, size_t nq, size_t max_search,
                                                                    size_t num_neighbors) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        std::vector<uint64_t> ids(nq * num_neighbors);
        std::vector<float> ds(nq * num_neighbors);
        std::vector<uint32_t> counts(nq);
        check(granne_hip_search_batch(h_.get(), q.data(), (uint32_t)nq, (uint32_t)max_search, (uint32_t)num_neighbors,
                                      ids.data(), ds.data(), counts.data(), nullptr));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * num_neighbors + j], ds[i * num_neighbors + j]);
        return out;
    }

    // `search` among the ids `allowed` lets through (granne_hip.h, "filtered search"): ascending by (distance, id), fewer than
    // num_neighbors when the walk met fewer allowed ids; max_expand > 0 caps the bottom layer's expansions
    std::vector<std::pair<size_t, float>> search_filtered(const Element& element, const Filter& allowed, size_t max_search,
                                                          size_t num_neighbors, uint64_t max_expand = 0) const {
        return std::move(search_filtered_batch(&element, 1, allowed, max_search, num_neighbors, max_expand)[0]);
    }
    std::vector<std::vector<std::pair<size_t, float>>> search_filtered_batch(const Element* elements, size_t nq, const Filter& allowed,
                                                                             size_t max_search, size_t num_neighbors,
                                                                             uint64_t max_expand = 0) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        const int device = granne_hip_index_device(h_.get());
        if (allowed.len() != len() || allowed.device() != device) throw std::runtime_error("the filter must cover the index's ids on its device");
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        const size_t k = num_neighbors, qb = q.size() * sizeof(q[0]);
        const size_t o_d = nq * k * 8, o_c = o_d + nq * k * 4, o_st = o_c + nq * 4, total = o_st + 16;
        detail::DeviceMem d_q(qb + 16, device), d_out(total, device);
        std::vector<uint8_t> host(total, 0);
        d_q.upload(q.data(), qb);
        d_out.upload(host.data(), total);
        int rc = granne_hip_search_filtered_batch_device(h_.get(), d_q.get(), (uint32_t)nq, (uint32_t)max_search, (uint32_t)k, allowed.words(), 0,
                                                         max_expand, (uint64_t*)d_out.get(), (float*)((char*)d_out.get() + o_d),
                                                         (uint32_t*)((char*)d_out.get() + o_c), nullptr, (uint32_t*)((char*)d_out.get() + o_st), nullptr);
        check(granne_hip_stream_synchronize(nullptr, device));
        check(rc);
        d_out.download(host.data(), total);
        const uint64_t* ids = (const uint64_t*)host.data();
        const float* ds = (const float*)(host.data() + o_d);
        const uint32_t* counts = (const uint32_t*)(host.data() + o_c);
        if (*(const uint32_t*)(host.data() + o_st)) throw std::runtime_error("exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }

    // The exact k nearest elements of every query by a scan of all elements on the matrix cores (k <= 16): what
    // ElementContainer::dists over every index + a sort would give (src/elements/mod.rs:35-39); the recall ground truth.
    std::vector<std::vector<std::pair<size_t, float>>> brute_force(const Element* elements, size_t nq, size_t k) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        std::vector<uint64_t> ids(nq * k);
        std::vector<float> ds(nq * k);
        std::vector<uint32_t> counts(nq);
        check(granne_hip_brute_force(h_.get(), q.data(), (uint32_t)nq, (uint32_t)k, ids.data(), ds.data(), counts.data()));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }

    // The k (up to 1024) nearest elements of every query by a scan of all rows in the reference's own arithmetic,
    // selected by (distance bits, id): exact by construction, ties included (granne_hip_exact_topk). Throws when a query
    // overflowed the selection (thousands of copies of one row at its k-th distance).
    std::vector<std::vector<std::pair<size_t, float>>> exact_topk(const Element* elements, size_t nq, size_t k) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        std::vector<uint64_t> ids(nq * k);
        std::vector<float> ds(nq * k);
        std::vector<uint32_t> counts(nq);
        check(granne_hip_exact_topk(h_.get(), q.data(), (uint32_t)nq, (uint32_t)k, ids.data(), ds.data(), counts.data(), nullptr));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }

    // exact_topk among the ids `allowed` lets through (granne_hip_exact_topk_filtered_device; one bitmap for all queries,
    // over num_elements() ids): the scan walks the bitmap's id list -- the tool for a selective filter, where
    // search_filtered steps over many disallowed nodes per allowed one. A result holds fewer than k ids when fewer are allowed.
    std::vector<std::vector<std::pair<size_t, float>>> exact_topk_filtered(const Element* elements, size_t nq, size_t k,
                                                                           const Filter& allowed) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        const int device = granne_hip_index_device(h_.get());
        if (allowed.len() != num_elements() || allowed.device() != device)
            throw std::runtime_error("the filter must cover the index's elements on its device");
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        const size_t qb = q.size() * sizeof(q[0]);
        const size_t o_d = nq * k * 8, o_c = o_d + nq * k * 4, o_st = o_c + nq * 4, total = o_st + 16;
        detail::DeviceMem d_q(qb + 16, device), d_out(total, device);
        std::vector<uint8_t> host(total, 0);
        d_q.upload(q.data(), qb);
        d_out.upload(host.data(), total);
        int rc = granne_hip_exact_topk_filtered_device(h_.get(), d_q.get(), (uint32_t)nq, (uint32_t)k, allowed.words(), 0, (uint64_t*)d_out.get(),
                                                       (float*)((char*)d_out.get() + o_d), (uint32_t*)((char*)d_out.get() + o_c),
                                                       (uint32_t*)((char*)d_out.get() + o_st), nullptr);
        check(granne_hip_stream_synchronize(nullptr, device));
        check(rc);
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        if (nq == 0) return out;
        d_out.download(host.data(), total);
        const uint64_t* ids = (const uint64_t*)host.data();
        const float* ds = (const float*)(host.data() + o_d);
        const uint32_t* counts = (const uint32_t*)(host.data() + o_c);
        if (*(const uint32_t*)(host.data() + o_st)) throw std::runtime_error("exact_topk_filtered: a query has too many rows inside one second-level bin at its k-th distance");
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }

    // The num_neighbors nearest ALLOWED ids by the ordinary search with a long list and a filter of its result
    // (granne_hip.h, "post-filtered search"): a query's list of stages[s] entries answers it once it holds min_allowed
    // allowed ids or the walk ran out of graph, else the query goes on to the next stage; what no stage finishes gets the
    // exact scan under the filter (GRANNE_HIP_PF_FALLBACK_EXACT) or its short answer (_SHORT). out_stage (optional): the
    // stage that answered each query, or GRANNE_HIP_PF_STAGE_EXACT / _SHORT.
    std::vector<std::vector<std::pair<size_t, float>>> search_postfiltered(const Element* elements, size_t nq, size_t num_neighbors,
                                                                           const Filter& allowed, size_t min_allowed,
                                                                           const std::vector<uint32_t>& stages,
                                                                           int fallback = GRANNE_HIP_PF_FALLBACK_EXACT,
                                                                           std::vector<uint32_t>* out_stage = nullptr,
                                                                           uint64_t scratch_bytes = 0) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        const int device = granne_hip_index_device(h_.get());
        if (allowed.len() != num_elements() || allowed.device() != device)
            throw std::runtime_error("the filter must cover the index's elements on its device");
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        const size_t k = num_neighbors, qb = q.size() * sizeof(q[0]);
        const size_t o_d = nq * k * 8, o_c = o_d + nq * k * 4, o_sg = o_c + nq * 4, o_st = o_sg + nq * 4, total = o_st + 16;
        detail::DeviceMem d_q(qb + 16, device), d_out(total, device);
        std::vector<uint8_t> host(total, 0);
        d_q.upload(q.data(), qb);
        d_out.upload(host.data(), total);
        char* const o = (char*)d_out.get();
        int rc = granne_hip_search_postfiltered_batch_device(h_.get(), d_q.get(), (uint32_t)nq, (uint32_t)k, (uint32_t)min_allowed, stages.data(),
                                                             (uint32_t)stages.size(), fallback, allowed.words(), 0, scratch_bytes, (uint64_t*)o,
                                                             (float*)(o + o_d), (uint32_t*)(o + o_c), (uint32_t*)(o + o_sg), (uint32_t*)(o + o_st),
                                                             nullptr);
        check(granne_hip_stream_synchronize(nullptr, device));
        check(rc);
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        if (out_stage) out_stage->assign(nq, 0);
        if (nq == 0) return out;
        d_out.download(host.data(), total);
        const uint64_t* ids = (const uint64_t*)host.data();
        const float* ds = (const float*)(host.data() + o_d);
        const uint32_t* counts = (const uint32_t*)(host.data() + o_c);
        if (*(const uint32_t*)(host.data() + o_st))
            throw std::runtime_error("search_postfiltered: a walk ran out of exact-search scratch or the fallback's selection overflowed");
        if (out_stage) std::memcpy(out_stage->data(), host.data() + o_sg, nq * 4);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }

    // Every element within radii[i] of query i, exact by construction (granne_hip.h, "range search"): the nearest cap (up to
    // GRANNE_HIP_RANGE_CAP_MAX) of them ascending by (distance, id); out_totals (optional): the exact number within the
    // radius, also beyond cap. allowed: null for all rows, else the rows one bitmap allows.
    std::vector<std::vector<std::pair<size_t, float>>> exact_range(const Element* elements, size_t nq, const float* radii, size_t cap,
                                                                   const Filter* allowed = nullptr,
                                                                   std::vector<uint32_t>* out_totals = nullptr) const {
        if (allowed && (allowed->len() != num_elements() || allowed->device() != granne_hip_index_device(h_.get())))
            throw std::runtime_error("the filter must cover the index's elements on its device");
        return range_call(elements, nq, radii, cap, out_totals, nullptr, "exact_range: a query has too many rows inside one second-level bin at its cap-th distance",
                          [&](const void* q, const float* r, uint64_t* ids, float* ds, uint32_t* counts, uint32_t* found, uint32_t*, uint32_t* status) {
                              return granne_hip_exact_range_device(h_.get(), q, (uint32_t)nq, r, (uint32_t)cap, allowed ? allowed->words() : nullptr, 0, ids,
                                                                   ds, counts, found, status, nullptr);
                          });
    }

    // The elements within radii[i] of query i by the ordinary search with lists of stages[s] entries, cut at the radius
    // (granne_hip.h, "range search"): a list answers its query once it holds an entry beyond the radius or the walk ran out
    // of graph, else the query goes on to the next stage; what no stage finishes gets the exact scan
    // (GRANNE_HIP_RG_FALLBACK_EXACT) or its short answer (_SHORT). out_found / out_stage (optional): the entries within the
    // radius (the exact total after the scan), and the stage that answered, or GRANNE_HIP_RG_STAGE_EXACT / _SHORT.
    std::vector<std::vector<std::pair<size_t, float>>> search_range(const Element* elements, size_t nq, const float* radii, size_t cap,
                                                                    const std::vector<uint32_t>& stages,
                                                                    int fallback = GRANNE_HIP_RG_FALLBACK_EXACT,
                                                                    std::vector<uint32_t>* out_found = nullptr,
                                                                    std::vector<uint32_t>* out_stage = nullptr,
                                                                    uint64_t scratch_bytes = 0) const {
        return range_call(elements, nq, radii, cap, out_found, out_stage, "search_range: a walk ran out of exact-search scratch or the fallback's selection overflowed",
                          [&](const void* q, const float* r, uint64_t* ids, float* ds, uint32_t* counts, uint32_t* found, uint32_t* stage, uint32_t* status) {
                              return granne_hip_search_range_batch_device(h_.get(), q, (uint32_t)nq, r, (uint32_t)cap, stages.data(), (uint32_t)stages.size(),
                                                                          fallback, scratch_bytes, ids, ds, counts, found, stage, status, nullptr);
                          });
    }

    // A handle over the rows alone (no layers): what RefinedGranne re-ranks by; get_element and the distance operators work
    static Granne from_elements(const Elements& elements, int device = 0) {
        granne_hip_index* h = nullptr;
        check(granne_hip_index_create(&h, elements.as_slice(), elements.len(), (uint32_t)(elements.dim() ? elements.dim() : 1), dtype(),
                                      0, nullptr, nullptr, nullptr, device));
        return Granne(h);
    }

    // Index trait (mod.rs:54-71)
    size_t len() const { return granne_hip_index_len(h_.get()); }
    size_t num_elements() const { return granne_hip_index_num_elements(h_.get()); } // rows of the element set (>= len())
    size_t num_layers() const { return granne_hip_index_num_layers(h_.get()); }
    size_t layer_len(size_t layer) const { return granne_hip_index_layer_len(h_.get(), (uint32_t)layer); }
    std::vector<size_t> get_neighbors(size_t index, size_t layer) const {
        uint32_t buf[512], n = 0;
        check(granne_hip_index_get_neighbors(h_.get(), index, (uint32_t)layer, buf, 512, &n));
        return std::vector<size_t>(buf, buf + n);
    }
    Element get_element(size_t index) const {
        Element e;
        e.data.resize(granne_hip_index_dim(h_.get()));
        check(granne_hip_index_get_element(h_.get(), index, e.data.data()));
        return e;
    }
    // Granne::reorder / reorder_by_keys (src/index/reorder.rs:59-133): returns the permutation
    std::vector<size_t> reorder(bool /*show_progress*/ = false) {
        std::vector<uint64_t> order(len());
        check(granne_hip_index_reorder(h_.get(), order.data()));
        return std::vector<size_t>(order.begin(), order.end());
    }
    std::vector<size_t> reorder_by_keys(const std::vector<uint64_t>& keys, bool /*show_progress*/ = false) {
        if (keys.size() != len()) throw std::runtime_error("need one key per element"); // reorder.rs:91
        std::vector<uint64_t> order(len());
        check(granne_hip_index_reorder_by_keys(h_.get(), keys.data(), order.data()));
        return std::vector<size_t>(order.begin(), order.end());
    }
    void write_index(const std::string& path) const { check(granne_hip_index_save(h_.get(), path.c_str(), nullptr)); }
    void write_elements(const std::string& path) const { check(granne_hip_index_save(h_.get(), nullptr, path.c_str())); }
    // write_index + write_elements through the device codec (either path may be empty: not written); the same bytes
    void save_on_device(const std::string& index_path, const std::string& elements_path, uint64_t staging_bytes = 0,
                        uint64_t* info = nullptr) const {
        check(granne_hip_index_save_on_device(h_.get(), index_path.empty() ? nullptr : index_path.c_str(),
                                              elements_path.empty() ? nullptr : elements_path.c_str(), staging_bytes, info));
    }
    // Index::write_index into a writer (src/index/mod.rs:67-70): the bytes of the index file
    std::vector<uint8_t> index_bytes() const {
        void* p = nullptr;
        uint64_t n = 0;
        check(granne_hip_index_encode(h_.get(), &p, &n));
        std::vector<uint8_t> out(static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + n);
        granne_hip_bytes_free(p);
        return out;
    }
    // the walkers' copy of the layers with the neighbors' row tails next to the ids (f32 100-d / 200-d: whole-line reads)
    void set_inline_tails(bool keep) { check(granne_hip_index_set_option(h_.get(), GRANNE_HIP_OPT_INLINE_TAILS, keep ? 1 : 0)); }
    // from how many walks per launch revisits are skipped before their rows are fetched (f32; 0 = always)
    void set_seen_min(uint64_t walks) { check(granne_hip_index_set_option(h_.get(), GRANNE_HIP_OPT_SEEN_MIN, walks)); }
    // search() calls that host threads make at the same moment share search launches (GRANNE_HIP_OPT_COALESCE: the
    // reference's par_iter over Granne::search). Off by default; results do not depend on it; nothing for one thread
    void set_coalesce(bool on) { check(granne_hip_index_set_option(h_.get(), GRANNE_HIP_OPT_COALESCE, on ? 1 : 0)); }
    bool coalesce() const { return get_option(GRANNE_HIP_OPT_COALESCE) != 0; }
    // the cap of queries per grouped launch (1..1024) and how long a new leader waits for its group to fill (0 = never)
    void set_coalesce_max(uint64_t queries) { check(granne_hip_index_set_option(h_.get(), GRANNE_HIP_OPT_COALESCE_MAX, queries)); }
    void set_coalesce_wait_us(uint64_t us) { check(granne_hip_index_set_option(h_.get(), GRANNE_HIP_OPT_COALESCE_WAIT_US, us)); }
    // launches made for groups since the index was created, and the queries they served
    uint64_t coalesced_launches() const { return get_option(GRANNE_HIP_OPT_COALESCED_LAUNCHES); }
    uint64_t coalesced_queries() const { return get_option(GRANNE_HIP_OPT_COALESCED_QUERIES); }
    // whether the last search launch ran the compacted row stage of the sketched walkers (GRANNE_HIP_OPT_LAST_COMPACT_ROWS)
    bool last_compact_rows() const { return get_option(GRANNE_HIP_OPT_LAST_COMPACT_ROWS) != 0; }
    // whether the last search launch ran its tail blocks as a kernel of their own (GRANNE_HIP_OPT_LAST_SPLIT_TAIL)
    bool last_split_tail() const { return get_option(GRANNE_HIP_OPT_LAST_SPLIT_TAIL) != 0; }
    // what the last exact scan ran (GRANNE_HIP_OPT_LAST_SCAN): the kernel form, the ranges, whether the priming pass ran
    struct LastScan {
        unsigned form, ranges, prime_ranges, kk; // GRANNE_HIP_SCAN_*, G, Gs, min(k + 6, 16)
        bool primed;
    };
    LastScan last_scan() const {
        const uint64_t w = get_option(GRANNE_HIP_OPT_LAST_SCAN);
        return {GRANNE_HIP_LAST_SCAN_FORM(w), GRANNE_HIP_LAST_SCAN_RANGES(w), GRANNE_HIP_LAST_SCAN_PRIME_RANGES(w),
                GRANNE_HIP_LAST_SCAN_KK(w), GRANNE_HIP_LAST_SCAN_PRIMED(w) != 0};
    }
    uint64_t get_option(int option) const {
        uint64_t v = 0;
        check(granne_hip_index_get_option(h_.get(), option, &v));
        return v;
    }
    granne_hip_index* raw() const { return h_.get(); }

private:
    static constexpr int dtype() { return detail::dtype_of<typename decltype(Element::data)::value_type>::value; }
    // what exact_range and search_range share: queries and radii up, `call` on device buffers (ids, dists, counts, found,
    // stage, status), the answer down; out_found / out_stage optional; a non-zero status[0] throws `overflow`
    template <class Call>
    std::vector<std::vector<std::pair<size_t, float>>> range_call(const Element* elements, size_t nq, const float* radii, size_t cap,
                                                                  std::vector<uint32_t>* out_found, std::vector<uint32_t>* out_stage,
                                                                  const char* overflow, Call call) const {
        const size_t dim = granne_hip_index_dim(h_.get());
        const int device = granne_hip_index_device(h_.get());
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            if (radii[i] != radii[i]) throw std::runtime_error("range search: a radius is NaN");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        const size_t qb = q.size() * sizeof(q[0]);
        const size_t o_d = nq * cap * 8, o_c = o_d + nq * cap * 4, o_fn = o_c + nq * 4, o_sg = o_fn + nq * 4, o_st = o_sg + nq * 4, total = o_st + 16;
        detail::DeviceMem d_q(qb + 16, device), d_r(nq * 4 + 16, device), d_out(total, device);
        std::vector<uint8_t> host(total, 0);
        d_q.upload(q.data(), qb);
        d_r.upload(radii, nq * 4);
        d_out.upload(host.data(), total);
        char* const o = (char*)d_out.get();
        int rc = call((const void*)d_q.get(), (const float*)d_r.get(), (uint64_t*)o, (float*)(o + o_d), (uint32_t*)(o + o_c), (uint32_t*)(o + o_fn),
                      (uint32_t*)(o + o_sg), (uint32_t*)(o + o_st));
        check(granne_hip_stream_synchronize(nullptr, device));
        check(rc);
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        if (out_found) out_found->assign(nq, 0);
        if (out_stage) out_stage->assign(nq, 0);
        if (nq == 0) return out;
        d_out.download(host.data(), total);
        const uint64_t* ids = (const uint64_t*)host.data();
        const float* ds = (const float*)(host.data() + o_d);
        const uint32_t* counts = (const uint32_t*)(host.data() + o_c);
        if (out_found) std::memcpy(out_found->data(), host.data() + o_fn, nq * 4);
        if (out_stage) std::memcpy(out_stage->data(), host.data() + o_sg, nq * 4);
        if (*(const uint32_t*)(host.data() + o_st)) throw std::runtime_error(overflow);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * cap + j], ds[i * cap + j]);
        return out;
    }
    std::shared_ptr<granne_hip_index> h_;
};

// Refined search (granne_hip_search_refined_batch): walk one index, give the walk's refine_from best candidates their
// distances under ANOTHER index's rows -- the same elements under the same ids, e.g. int8 rows walked and f32 rows
// re-ranked -- and return the num_neighbors best by (distance, id). Both handles are shared with the Grannes they came from.
template <class WalkElements, class RefineElements>
class RefinedGranne {
public:
    using WalkElement = typename WalkElements::Element;
    using RefineElement = typename RefineElements::Element;
    RefinedGranne(const Granne<WalkElements>& walk, const Granne<RefineElements>& refine) : walk_(walk), refine_(refine) {}

    // refine_from = 0 means max_search; 1 <= refine_from <= min(max_search, 1024)
    std::vector<std::pair<size_t, float>> search(const WalkElement& walk_element, const RefineElement& refine_element, size_t max_search,
                                                 size_t num_neighbors, size_t refine_from = 0) const {
        return std::move(search_batch(&walk_element, &refine_element, 1, max_search, num_neighbors, refine_from)[0]);
    }
    std::vector<std::vector<std::pair<size_t, float>>> search_batch(const WalkElement* walk_elements, const RefineElement* refine_elements,
                                                                    size_t nq, size_t max_search, size_t num_neighbors,
                                                                    size_t refine_from = 0) const {
        const size_t wdim = granne_hip_index_dim(walk_.raw()), rdim = granne_hip_index_dim(refine_.raw());
        std::vector<typename decltype(WalkElement::data)::value_type> qw(nq * wdim);
        std::vector<typename decltype(RefineElement::data)::value_type> qr(nq * rdim);
        for (size_t i = 0; i < nq; ++i) {
            if (walk_elements[i].len() != wdim || refine_elements[i].len() != rdim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(qw.data() + i * wdim, walk_elements[i].as_slice(), wdim * sizeof(qw[0]));
            std::memcpy(qr.data() + i * rdim, refine_elements[i].as_slice(), rdim * sizeof(qr[0]));
        }
        std::vector<uint64_t> ids(nq * num_neighbors);
        std::vector<float> ds(nq * num_neighbors);
        std::vector<uint32_t> counts(nq);
        check(granne_hip_search_refined_batch(walk_.raw(), refine_.raw(), qw.data(), qr.data(), (uint32_t)nq, (uint32_t)max_search,
                                              (uint32_t)(refine_from ? refine_from : max_search), (uint32_t)num_neighbors, ids.data(),
                                              ds.data(), counts.data(), nullptr, nullptr));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * num_neighbors + j], ds[i * num_neighbors + j]);
        return out;
    }

private:
    Granne<WalkElements> walk_;
    Granne<RefineElements> refine_;
};

// A partitioned index: shard s is a Granne of its own over the elements [offsets[s], offsets[s] + shard.len()) of the
// whole set -- how the reference's shard helper cuts an element file (src/elements/embeddings/parsing.rs:63-100). A search
// asks every shard and keeps the best by (distance, global id); ids in the results are global. One host process drives
// all shards (granne_hip_sharded_*); batches are pipelined inside the library.
template <class Elements>
class ShardedGranne {
public:
    using Element = typename Elements::Element;
    ShardedGranne(std::vector<Granne<Elements>> shards, const std::vector<uint64_t>& offsets) : shards_(std::move(shards)) {
        if (shards_.empty() || shards_.size() != offsets.size()) throw std::runtime_error("need one offset per shard");
        std::vector<granne_hip_index*> hs;
        for (auto& s : shards_) hs.push_back(s.raw());
        granne_hip_sharded* h = nullptr;
        check(granne_hip_sharded_create(&h, hs.data(), offsets.data(), (uint32_t)hs.size()));
        h_.reset(h, granne_hip_sharded_destroy); // destroyed before shards_ (declared after it): the handle borrows them
    }
    // the whole element set in, a searchable partitioned index out (granne_hip_sharded_build): n_shards id ranges
    // (src/elements/embeddings/parsing.rs:72-98), each built with the GPU builder under `config`; the handle owns its shards
    static ShardedGranne build(const BuildConfig& config, const Elements& elements, size_t n_shards, const std::vector<int>& devices = {0}) {
        using Scalar = typename decltype(Elements::Element::data)::value_type;
        granne_hip_sharded* h = nullptr;
        check(granne_hip_sharded_build(&h, &config.raw(), elements.as_slice(), elements.len(), (uint32_t)(elements.dim() ? elements.dim() : 1),
                                       detail::dtype_of<Scalar>::value, (uint32_t)n_shards, devices.data(), (uint32_t)devices.size()));
        ShardedGranne s;
        s.h_.reset(h, granne_hip_sharded_destroy);
        return s;
    }
    size_t len() const { return granne_hip_sharded_len(h_.get()); }
    size_t num_shards() const { return granne_hip_sharded_num_shards(h_.get()); }
    // the exchange step as ONE RCCL all-gather over the shard devices instead of peer copies (librccl by dlopen)
    void use_rccl_all_gather() { check(granne_hip_sharded_set_option(h_.get(), GRANNE_HIP_SHARDED_OPT_EXCHANGE, GRANNE_HIP_SHARDED_EXCHANGE_RCCL)); }
    void set_depth(size_t depth) { check(granne_hip_sharded_set_option(h_.get(), GRANNE_HIP_SHARDED_OPT_DEPTH, depth)); }

    std::vector<std::pair<size_t, float>> search(const Element& element, size_t max_search, size_t num_neighbors) const {
        return search_batches(&element, 1, 1, max_search, num_neighbors)[0];
    }
    // n_batches batches of nq queries each (elements: n_batches * nq of them), pipelined inside the library
    std::vector<std::vector<std::pair<size_t, float>>> search_batches(const Element* elements, size_t n_batches, size_t nq,
                                                                      size_t max_search, size_t num_neighbors) const {
        const size_t total = n_batches * nq, dim = granne_hip_index_dim(granne_hip_sharded_shard(h_.get(), 0));
        std::vector<typename decltype(Element::data)::value_type> q(total * dim);
        for (size_t i = 0; i < total; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        std::vector<uint64_t> ids(total * num_neighbors);
        std::vector<float> ds(total * num_neighbors);
        std::vector<uint32_t> counts(total);
        check(granne_hip_sharded_search_batches(h_.get(), q.data(), (uint32_t)n_batches, (uint32_t)nq, (uint32_t)max_search,
                                                (uint32_t)num_neighbors, ids.data(), ds.data(), counts.data()));
        std::vector<std::vector<std::pair<size_t, float>>> out(total);
        for (size_t i = 0; i < total; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * num_neighbors + j], ds[i * num_neighbors + j]);
        return out;
    }

    // the bits of a global filter: max over the shards of offset + rows (granne_hip_sharded_id_span)
    size_t id_span() const { return (size_t)granne_hip_sharded_id_span(h_.get()); }

    // `search` among the GLOBAL ids `allowed` lets through (a Filter over id_span() ids on the handle's device): every
    // shard walks under its slice of the bitmap, the results are merged by (distance, global id); max_expand > 0 caps each
    // shard's walk
    std::vector<std::vector<std::pair<size_t, float>>> search_filtered(const Element* elements, size_t nq, const Filter& allowed,
                                                                       size_t max_search, size_t num_neighbors,
                                                                       uint64_t max_expand = 0) const {
        check_filter(allowed);
        return run(elements, nq, num_neighbors, "a shard's exact-search scratch is exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)",
                   [&](const void* q, uint64_t* ids, float* ds, uint32_t* counts, uint32_t* st) {
                       return granne_hip_sharded_search_filtered_batch_device(h_.get(), q, (uint32_t)nq, (uint32_t)max_search, (uint32_t)num_neighbors,
                                                                              allowed.words(), 0, max_expand, ids, ds, counts, st, nullptr);
                   });
    }
    // the k (up to 1024, n_shards * k up to 4096) nearest rows of the whole partitioned set, exact
    // (granne_hip_sharded_exact_topk_device); throws when a query overflowed the selection in a shard
    std::vector<std::vector<std::pair<size_t, float>>> exact_topk(const Element* elements, size_t nq, size_t k) const {
        return run(elements, nq, k, "sharded exact_topk: a query overflowed the selection in a shard",
                   [&](const void* q, uint64_t* ids, float* ds, uint32_t* counts, uint32_t* st) {
                       return granne_hip_sharded_exact_topk_device(h_.get(), q, (uint32_t)nq, (uint32_t)k, ids, ds, counts, st, nullptr);
                   });
    }
    // the same among the global ids `allowed` lets through
    std::vector<std::vector<std::pair<size_t, float>>> exact_topk_filtered(const Element* elements, size_t nq, size_t k,
                                                                           const Filter& allowed) const {
        check_filter(allowed);
        return run(elements, nq, k, "sharded exact_topk_filtered: a query overflowed the selection in a shard",
                   [&](const void* q, uint64_t* ids, float* ds, uint32_t* counts, uint32_t* st) {
                       return granne_hip_sharded_exact_topk_filtered_device(h_.get(), q, (uint32_t)nq, (uint32_t)k, allowed.words(), 0, ids, ds,
                                                                            counts, st, nullptr);
                   });
    }

private:
    // queries up, one device call (queries, ids, dists, counts, status), results down as lists; `overflow`: status[0] != 0
    template <class Call>
    std::vector<std::vector<std::pair<size_t, float>>> run(const Element* elements, size_t nq, size_t k, const char* overflow, Call call) const {
        const size_t dim = granne_hip_index_dim(granne_hip_sharded_shard(h_.get(), 0));
        const int device = granne_hip_sharded_device(h_.get());
        std::vector<typename decltype(Element::data)::value_type> q(nq * dim);
        for (size_t i = 0; i < nq; ++i) {
            if (elements[i].len() != dim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(q.data() + i * dim, elements[i].as_slice(), dim * sizeof(q[0]));
        }
        const size_t qb = q.size() * sizeof(q[0]);
        const size_t o_d = nq * k * 8, o_c = o_d + nq * k * 4, o_st = o_c + nq * 4, total = o_st + 16;
        detail::DeviceMem d_q(qb + 16, device), d_out(total, device);
        std::vector<uint8_t> host(total, 0);
        d_q.upload(q.data(), qb);
        d_out.upload(host.data(), total);
        char* const o = (char*)d_out.get();
        const int rc = call(d_q.get(), (uint64_t*)o, (float*)(o + o_d), (uint32_t*)(o + o_c), (uint32_t*)(o + o_st));
        check(granne_hip_stream_synchronize(nullptr, device));
        check(rc);
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        if (nq == 0) return out;
        d_out.download(host.data(), total);
        const uint64_t* ids = (const uint64_t*)host.data();
        const float* ds = (const float*)(host.data() + o_d);
        const uint32_t* counts = (const uint32_t*)(host.data() + o_c);
        if (*(const uint32_t*)(host.data() + o_st)) throw std::runtime_error(overflow);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * k + j], ds[i * k + j]);
        return out;
    }
    void check_filter(const Filter& allowed) const {
        if (allowed.len() != id_span() || allowed.device() != granne_hip_sharded_device(h_.get()))
            throw std::runtime_error("the filter must cover the partitioned index's id_span() ids on its device");
    }
    ShardedGranne() = default;
    std::vector<Granne<Elements>> shards_; // empty when the handle owns its shards (build)
    std::shared_ptr<granne_hip_sharded> h_;
};

// GranneBuilder (src/index/mod.rs:293-531) + the Builder trait (:303-315)
template <class Elements>
class GranneBuilder {
public:
    static_assert(!std::is_same<typename decltype(Elements::Element::data)::value_type, f16>::value,
                  "a builder over f16 rows hands out an index that takes f32 queries: use the C entry points with GRANNE_HIP_F16");
    GranneBuilder(const BuildConfig& config, const Elements& elements, int device = 0) {
        granne_hip_builder* b = nullptr;
        using Scalar = typename decltype(Elements::Element::data)::value_type;
        check(granne_hip_builder_create(&b, &config.raw(), elements.as_slice(), elements.len(),
                                        (uint32_t)(elements.dim() ? elements.dim() : 1), detail::dtype_of<Scalar>::value, device));
        b_.reset(b, detail::BuilderDeleter{});
    }
    // GranneBuilder::from_bytes (mod.rs:430-461): a builder resuming from a written index
    static GranneBuilder from_bytes(const BuildConfig& config, const void* index, size_t index_len, const Elements& elements,
                                    int device = 0) {
        GranneBuilder b(config, elements, device);
        check(granne_hip_builder_load_index(b.b_.get(), index, index_len));
        return b;
    }
    // Builder::push (mod.rs:303-315): indexed by the next build()
    void push(const typename Elements::Element& element) {
        check(granne_hip_builder_append(b_.get(), element.as_slice(), 1));
    }
    void build() { check(granne_hip_builder_build(b_.get(), GRANNE_HIP_BUILD_ALL)); }
    void build_partial(size_t num_elements) {
        if (num_elements == 0) return; // mod.rs:375-377
        check(granne_hip_builder_build(b_.get(), num_elements));
    }
    size_t len() const { return granne_hip_builder_len(b_.get()); }
    size_t num_elements() const { return granne_hip_builder_num_elements(b_.get()); }
    size_t num_layers() const { return granne_hip_builder_num_layers(b_.get()); }
    size_t layer_len(size_t layer) const { return granne_hip_builder_layer_len(b_.get(), (uint32_t)layer); }
    Granne<Elements> get_index() const {
        granne_hip_index* h = nullptr;
        check(granne_hip_builder_get_index(b_.get(), &h));
        return Granne<Elements>(h);
    }

private:
    template <class> friend class RwGranneBuilder;
    // hands the handle over (RwGranneBuilder consumes it); every copy of this GranneBuilder is empty afterwards
    granne_hip_builder* release() {
        std::get_deleter<detail::BuilderDeleter>(b_)->armed = false;
        granne_hip_builder* p = b_.get();
        b_.reset();
        return p;
    }
    std::shared_ptr<granne_hip_builder> b_;
};

// RwGranneBuilder (src/index/rw/mod.rs:15-224): inserts and searches on one live graph. Member functions are const as
// the reference's take &self: the library serialises inserts against searches with a reader-writer lock held per call
// (a search sees the graph after a whole number of insert calls). Without a previous layer search returns nothing
// (rw/mod.rs:198-206).
template <class Elements>
class RwGranneBuilder {
public:
    using Element = typename Elements::Element;
    // RwGranneBuilder::new(builder, max_elements, _) (rw/mod.rs:32-61): consumes the builder (no other copy of it may
    // be in use)
    RwGranneBuilder(GranneBuilder<Elements>&& builder, size_t max_elements) {
        granne_hip_rw_builder* h = nullptr;
        check(granne_hip_rw_builder_create(&h, builder.b_.get(), max_elements));
        builder.release();
        h_.reset(h, granne_hip_rw_builder_destroy);
    }
    // insert (rw/mod.rs:99-101): the element's id, or -1 when the builder is full
    long long insert(const Element& element) const {
        uint64_t id = 0, count = 0;
        check(granne_hip_rw_builder_insert_batch(h_.get(), element.as_slice(), 1, &id, &count));
        return count ? (long long)id : -1;
    }
    // insert_batch (rw/mod.rs:103-182)
    std::vector<size_t> insert_batch(const Elements& elements) const {
        std::vector<uint64_t> ids(elements.len());
        uint64_t count = 0;
        check(granne_hip_rw_builder_insert_batch(h_.get(), elements.as_slice(), elements.len(), ids.data(), &count));
        return std::vector<size_t>(ids.begin(), ids.begin() + count);
    }
    // search (rw/mod.rs:184-207)
    std::vector<std::pair<size_t, float>> search(const Element& element, size_t max_search, size_t num_neighbors) const {
        std::vector<uint64_t> ids(num_neighbors);
        std::vector<float> dists(num_neighbors);
        uint32_t count = 0;
        check(granne_hip_rw_builder_search(h_.get(), element.as_slice(), (uint32_t)max_search, (uint32_t)num_neighbors,
                                           ids.data(), dists.data(), &count));
        std::vector<std::pair<size_t, float>> out(count);
        for (uint32_t i = 0; i < count; ++i) out[i] = {(size_t)ids[i], dists[i]};
        return out;
    }
    size_t len() const { return granne_hip_rw_builder_len(h_.get()); }
    bool is_empty() const { return len() == 0; }
    size_t max_elements() const { return granne_hip_rw_builder_max_elements(h_.get()); }
    size_t num_layers() const { return granne_hip_rw_builder_num_layers(h_.get()); }
    size_t layer_len(size_t layer) const { return granne_hip_rw_builder_layer_len(h_.get(), (uint32_t)layer); }
    // save_index_and_elements_to_disk (rw/mod.rs:63-68)
    void save_index_and_elements_to_disk(const std::string& index_path, const std::string& elements_path) const {
        check(granne_hip_rw_builder_save(h_.get(), index_path.c_str(), elements_path.c_str()));
    }
    Granne<Elements> get_index() const {
        granne_hip_index* h = nullptr;
        check(granne_hip_rw_builder_get_index(h_.get(), &h));
        return Granne<Elements>(h);
    }
    void set_option(int option, uint64_t value) const { check(granne_hip_rw_builder_set_option(h_.get(), option, value)); }
    uint64_t get_option(int option) const {
        uint64_t v = 0;
        check(granne_hip_rw_builder_get_option(h_.get(), option, &v));
        return v;
    }

    // ---- removing elements (granne_hip.h, "removing elements"; no reference counterpart) ----
    struct MarkCounts {
        uint64_t changed, already, out_of_range; // ids this call removed (restored); in that state already; >= len, ignored
    };
    // search never returns a removed element again; it stays in the graph (traversed, linked to), its slot is not reused
    MarkCounts remove(const std::vector<uint64_t>& ids) const {
        uint64_t c[3] = {0, 0, 0};
        check(granne_hip_rw_builder_remove(h_.get(), ids.data(), ids.size(), c));
        return {c[0], c[1], c[2]};
    }
    MarkCounts restore(const std::vector<uint64_t>& ids) const {
        uint64_t c[3] = {0, 0, 0};
        check(granne_hip_rw_builder_restore(h_.get(), ids.data(), ids.size(), c));
        return {c[0], c[1], c[2]};
    }
    size_t removed_count() const { return granne_hip_rw_builder_removed_count(h_.get()); } // (= GRANNE_HIP_RW_OPT_REMOVED)
    // search calls that ran under the tombstone bitmap so far: one per call made while removed_count() was not 0
    uint64_t filtered_searches() const { return get_option(GRANNE_HIP_RW_OPT_FILTERED_SEARCHES); }
    // a copy of the bitmap of the elements that are not removed, over the ids 0..len-1 (`device`: the handle's): the filter
    // for Granne::search_filtered on a get_index() snapshot taken with no insert in between
    Filter alive_filter(int device = 0) const {
        Filter f(len(), max_elements(), device); // (room for whatever a concurrent insert adds)
        check(granne_hip_rw_builder_alive(h_.get(), f.words(), nullptr));
        check(granne_hip_stream_synchronize(nullptr, device));
        return f;
    }
    // a new, independent builder over the elements that are not removed, in ascending old-id order, built afresh under
    // this one's config; (*old_ids)[new_id] = the element's id here. This builder is left as it is.
    RwGranneBuilder compact(size_t max_elements, std::vector<uint64_t>* old_ids = nullptr) const {
        std::vector<uint64_t> old(std::max(len(), this->max_elements()) + 1);
        granne_hip_rw_builder* h = nullptr;
        uint64_t count = 0;
        check(granne_hip_rw_builder_compact(h_.get(), max_elements, &h, old.data(), &count));
        old.resize((size_t)count);
        if (old_ids) old_ids->swap(old);
        return RwGranneBuilder(h);
    }

private:
    explicit RwGranneBuilder(granne_hip_rw_builder* h) : h_(h, granne_hip_rw_builder_destroy) {}
    std::shared_ptr<granne_hip_rw_builder> h_;
};

// granne::embeddings::SumEmbeddings (src/elements/embeddings/mod.rs:41-216): elements are lists of term ids, their
// vectors sums of rows of an embedding table. index() makes a searchable index over given layers: materialised (dense
// normalised rows on the device) or compact (the container in place of rows; search only).
namespace embeddings {
class SumEmbeddings {
public:
    SumEmbeddings(const std::vector<float>& table, uint32_t dim, const std::vector<std::vector<uint32_t>>& elements, int device = 0) {
        std::vector<uint64_t> off(1, 0);
        std::vector<uint32_t> terms;
        for (const auto& e : elements) {
            terms.insert(terms.end(), e.begin(), e.end());
            off.push_back(terms.size());
        }
        granne_hip_sum_embeddings* h = nullptr;
        check(granne_hip_sum_embeddings_create(&h, table.data(), dim ? table.size() / dim : 0, dim, off.data(), terms.data(),
                                               elements.size(), device));
        h_.reset(h, granne_hip_sum_embeddings_destroy);
    }
    static SumEmbeddings from_files(const std::string& embeddings_path, const std::string& elements_path, int device = 0) {
        granne_hip_sum_embeddings* h = nullptr;
        check(granne_hip_sum_embeddings_load_files(&h, embeddings_path.c_str(), elements_path.c_str(), device));
        return SumEmbeddings(h);
    }
    size_t len() const { return granne_hip_sum_embeddings_len(h_.get()); }
    size_t num_embeddings() const { return granne_hip_sum_embeddings_num_embeddings(h_.get()); }
    size_t dim() const { return granne_hip_sum_embeddings_dim(h_.get()); }
    void push(const std::vector<uint32_t>& element) {
        const uint64_t off[2] = {0, element.size()};
        check(granne_hip_sum_embeddings_append(h_.get(), off, element.data(), 1));
    }
    std::vector<size_t> get_terms(size_t idx) const {
        uint32_t n = 0;
        check(granne_hip_sum_embeddings_get_terms(h_.get(), idx, nullptr, 0, &n));
        std::vector<uint32_t> t(n);
        check(granne_hip_sum_embeddings_get_terms(h_.get(), idx, t.data(), n, &n));
        return std::vector<size_t>(t.begin(), t.end());
    }
    std::vector<float> get_embedding(size_t idx) const { // the raw sum
        std::vector<float> v(dim());
        check(granne_hip_sum_embeddings_materialize(h_.get(), idx, 1, 0, v.data()));
        return v;
    }
    std::vector<float> create_embedding(const std::vector<uint32_t>& terms, bool normalised = false) const {
        const uint64_t off[2] = {0, terms.size()};
        std::vector<float> v(dim());
        check(granne_hip_sum_embeddings_embed(h_.get(), off, terms.data(), 1, normalised ? 1 : 0, v.data()));
        return v;
    }
    void save_elements(const std::string& path) const { check(granne_hip_sum_embeddings_save_elements(h_.get(), path.c_str())); }
    void save_embeddings(const std::string& path) const { check(granne_hip_sum_embeddings_save_embeddings(h_.get(), path.c_str())); }
    // the C handles of an index / a builder over this container (owned by the caller: granne_hip_index_destroy / _builder_destroy)
    granne_hip_index* index(uint32_t n_layers, const uint64_t* layer_len, const uint32_t* const* layer_rows,
                            const uint32_t* layer_width, bool compact) const {
        granne_hip_index* ix = nullptr;
        check(granne_hip_index_create_sum_embeddings(&ix, h_.get(), n_layers, layer_len, layer_rows, layer_width,
                                                     compact ? GRANNE_HIP_SE_COMPACT : GRANNE_HIP_SE_MATERIALIZED));
        return ix;
    }
    granne_hip_builder* builder(const granne_hip_build_config& config) const {
        granne_hip_builder* b = nullptr;
        check(granne_hip_builder_create_sum_embeddings(&b, &config, h_.get()));
        return b;
    }
    // elements first .. first + count - 1 as prepared int8 rows (normalised, then quantised): the rows of the index that
    // RefinedSumEmbeddingsGranne walks (granne_hip_sum_embeddings_rows, GRANNE_HIP_I8)
    std::vector<int8_t> rows_i8(size_t first, size_t count) const {
        std::vector<int8_t> rows(count * dim());
        check(granne_hip_sum_embeddings_rows(h_.get(), first, count, GRANNE_HIP_I8, rows.data()));
        return rows;
    }
    granne_hip_sum_embeddings* handle() const { return h_.get(); }
    std::shared_ptr<granne_hip_sum_embeddings> shared() const { return h_; }

private:
    explicit SumEmbeddings(granne_hip_sum_embeddings* h) : h_(h, granne_hip_sum_embeddings_destroy) {}
    std::shared_ptr<granne_hip_sum_embeddings> h_;
};
} // namespace embeddings

// RefinedGranne's sibling over a container (granne_hip_search_refined_sum_embeddings_batch): walk one index -- typically
// the int8 rows of SumEmbeddings::rows_i8 with their graph -- and re-rank the walk's refine_from best candidates by the
// container's own vectors, made from their terms inside the kernel: f32 SumEmbeddings distances without dense f32 rows.
// A refine query is dim() prepared (normalised) floats. Both handles are shared with the objects they came from.
template <class WalkElements>
class RefinedSumEmbeddingsGranne {
public:
    using WalkElement = typename WalkElements::Element;
    RefinedSumEmbeddingsGranne(const Granne<WalkElements>& walk, const embeddings::SumEmbeddings& refine) : walk_(walk), se_(refine.shared()) {}

    // refine_from = 0 means max_search; 1 <= refine_from <= min(max_search, 1024)
    std::vector<std::vector<std::pair<size_t, float>>> search_batch(const WalkElement* walk_elements,
                                                                    const std::vector<float>* refine_queries, size_t nq,
                                                                    size_t max_search, size_t num_neighbors,
                                                                    size_t refine_from = 0) const {
        const size_t wdim = granne_hip_index_dim(walk_.raw()), rdim = granne_hip_sum_embeddings_dim(se_.get());
        std::vector<typename decltype(WalkElement::data)::value_type> qw(nq * wdim);
        std::vector<float> qr(nq * rdim);
        for (size_t i = 0; i < nq; ++i) {
            if (walk_elements[i].len() != wdim || refine_queries[i].size() != rdim) throw std::runtime_error("query dimension mismatch");
            std::memcpy(qw.data() + i * wdim, walk_elements[i].as_slice(), wdim * sizeof(qw[0]));
            std::memcpy(qr.data() + i * rdim, refine_queries[i].data(), rdim * sizeof(float));
        }
        std::vector<uint64_t> ids(nq * num_neighbors);
        std::vector<float> ds(nq * num_neighbors);
        std::vector<uint32_t> counts(nq);
        check(granne_hip_search_refined_sum_embeddings_batch(walk_.raw(), se_.get(), qw.data(), qr.data(), (uint32_t)nq,
                                                             (uint32_t)max_search, (uint32_t)(refine_from ? refine_from : max_search),
                                                             (uint32_t)num_neighbors, ids.data(), ds.data(), counts.data(), nullptr, nullptr));
        std::vector<std::vector<std::pair<size_t, float>>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) out[i].emplace_back((size_t)ids[i * num_neighbors + j], ds[i * num_neighbors + j]);
        return out;
    }
    std::vector<std::pair<size_t, float>> search(const WalkElement& walk_element, const std::vector<float>& refine_query, size_t max_search,
                                                 size_t num_neighbors, size_t refine_from = 0) const {
        return std::move(search_batch(&walk_element, &refine_query, 1, max_search, num_neighbors, refine_from)[0]);
    }

private:
    Granne<WalkElements> walk_;
    std::shared_ptr<granne_hip_sum_embeddings> se_;
};

} // namespace granne
