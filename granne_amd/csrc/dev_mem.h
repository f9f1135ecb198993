// dev_mem.h -- the host layer's two owners of HIP memory: DevBuf (hipMalloc / hipFree) and PinBuf (hipHostMalloc /
// hipHostFree). Move-only; the destructor frees. Like combiner.h this header includes nothing from HIP: it uses
// hipMalloc, hipFree, hipHostMalloc, hipHostFree, hipError_t and hipSuccess as whoever includes it has declared them
// (tests/cpp/test_dev_mem.cpp declares counting fakes).
//
// An owner frees on the device that is current when it dies: declare a function's owners AFTER its DeviceGuard, and
// destroy a handle that holds some under one. hipFree waits for the device; where a free has to come before or after
// something else, say so with reset().
#pragma once

#include <cstddef>
#include <utility>

namespace dev_mem_detail {
struct Device {
    static hipError_t get(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static void put(void* p) { (void)hipFree(p); }
};
struct Pinned {
    static hipError_t get(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static void put(void* p) { (void)hipHostFree(p); }
};

template <class M>
class Owner {
    void* p_ = nullptr;
    size_t cap_ = 0;

  protected:
    // Frees what the owner holds, then allocates; 0 bytes ask for 16 (a kernel argument is never null). On failure the
    // owner is empty and the error is returned -- HIP's sticky error is left for the caller to read or clear.
    hipError_t alloc_(size_t bytes, unsigned flags) {
        reset();
        if (bytes == 0) bytes = 16;
        const hipError_t e = M::get(&p_, bytes, flags);
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = bytes;
        return e;
    }

  public:
    Owner() = default;
    Owner(Owner&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Owner& operator=(Owner&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    Owner(const Owner&) = delete;
    Owner& operator=(const Owner&) = delete;
    ~Owner() { reset(); }

    void reset() {
        if (p_) M::put(p_);
        p_ = nullptr, cap_ = 0;
    }
    void* release() { // the caller frees
        cap_ = 0;
        return std::exchange(p_, nullptr);
    }
    void* get() const { return p_; }
    template <class T>
    T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
    size_t capacity() const { return cap_; } // bytes asked for (16 for a request of 0), 0 when empty
};
} // namespace dev_mem_detail

// device memory
struct DevBuf : dev_mem_detail::Owner<dev_mem_detail::Device> {
    hipError_t alloc(size_t bytes) { return alloc_(bytes, 0); }
    // grow only: nothing happens while the capacity suffices (the contents do not survive a growth)
    hipError_t reserve(size_t bytes) { return capacity() >= bytes ? hipSuccess : alloc_(bytes, 0); }
};

// pinned host memory; `flags` are hipHostMalloc's
struct PinBuf : dev_mem_detail::Owner<dev_mem_detail::Pinned> {
    hipError_t alloc(size_t bytes, unsigned flags) { return alloc_(bytes, flags); }
    hipError_t reserve(size_t bytes, unsigned flags) { return capacity() >= bytes ? hipSuccess : alloc_(bytes, flags); }
};
