// The host layer's memory owners (granne_amd/csrc/dev_mem.h) on the CPU: counting fakes stand in for the four HIP calls,
// hand out malloc memory and keep the live pointers in a set. Built by tests/test_dev_mem_host.py with g++ (plain, and
// with -fsanitize=address,undefined where the machine has the runtimes). Exits 0 and prints "ok"; a failed check exits 1.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            fflush(stderr);                                                  \
            _exit(1);                                                        \
        }                                                                    \
    } while (0)

// ---- the fakes: what dev_mem.h expects its includer to have declared ------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };

struct Fake {
    std::set<void*> live;
    size_t allocs = 0, frees = 0, last_bytes = 0;
    unsigned last_flags = 0;
    long fail_at = -1; // the allocation call (counted from 0 at the time it is set) that fails
    hipError_t get(void** p, size_t bytes, unsigned flags) {
        if (fail_at == 0) {
            fail_at = -1;
            return hipErrorOutOfMemory; // (*p is left alone, as a failed hipMalloc leaves it)
        }
        if (fail_at > 0) --fail_at;
        *p = malloc(bytes);
        CHECK(*p && live.insert(*p).second);
        ++allocs, last_bytes = bytes, last_flags = flags;
        return hipSuccess;
    }
    hipError_t put(void* p) {
        CHECK(p && live.erase(p) == 1); // freed exactly once, and only what was handed out
        free(p);
        ++frees;
        return hipSuccess;
    }
};
static Fake g_dev, g_pin;
static hipError_t hipMalloc(void** p, size_t bytes) { return g_dev.get(p, bytes, 0); }
static hipError_t hipFree(void* p) { return g_dev.put(p); }
static hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) { return g_pin.get(p, bytes, flags); }
static hipError_t hipHostFree(void* p) { return g_pin.put(p); }

#include "../../granne_amd/csrc/dev_mem.h"

// the owners' protocol, the same for both: `mk(buf, bytes)` allocates, `grow(buf, bytes)` reserves
template <class Buf, class Alloc, class Reserve>
static void protocol(Fake& F, Alloc mk, Reserve grow) {
    const size_t a0 = F.allocs, f0 = F.frees;
    { // scope exit
        Buf b;
        CHECK(!b && b.get() == nullptr && b.capacity() == 0);
        CHECK(mk(b, 100) == hipSuccess && b && b.capacity() == 100 && F.last_bytes == 100 && F.live.count(b.get()));
        CHECK(b.template as<char>() == (char*)b.get());
    }
    CHECK(F.live.empty() && F.allocs == a0 + 1 && F.frees == f0 + 1);
    { // move construction: one owner afterwards, one free
        Buf a;
        CHECK(mk(a, 32) == hipSuccess);
        void* p = a.get();
        Buf b(std::move(a));
        CHECK(!a && a.capacity() == 0 && b.get() == p && b.capacity() == 32 && F.frees == f0 + 1);
    }
    CHECK(F.live.empty() && F.frees == f0 + 2);
    { // move assignment onto a non-empty owner frees what it held, once
        Buf a, b;
        CHECK(mk(a, 8) == hipSuccess && mk(b, 24) == hipSuccess);
        void *pa = a.get(), *pb = b.get();
        b = std::move(a);
        CHECK(!F.live.count(pb) && F.live.count(pa) && b.get() == pa && b.capacity() == 8 && !a && F.frees == f0 + 3);
        b = std::move(b); // (self-assignment keeps the block)
        CHECK(b.get() == pa && F.live.count(pa));
    }
    CHECK(F.live.empty() && F.frees == f0 + 4);
    { // reset, alloc onto a non-empty owner, release
        Buf b;
        CHECK(mk(b, 64) == hipSuccess);
        b.reset();
        CHECK(!b && b.capacity() == 0 && F.live.empty());
        b.reset(); // (an empty owner frees nothing)
        CHECK(F.frees == f0 + 5);
        CHECK(mk(b, 64) == hipSuccess);
        CHECK(mk(b, 128) == hipSuccess && F.live.size() == 1 && F.frees == f0 + 6 && b.capacity() == 128); // (the first block is gone)
        void* p2 = b.release();
        CHECK(!b && b.capacity() == 0 && p2 && F.live.count(p2));
    }
    CHECK(F.live.size() == 1); // the released block is the caller's: not freed
    CHECK(F.put(*F.live.begin()) == hipSuccess);
    { // a request for 0 bytes asks for 16
        Buf b;
        CHECK(mk(b, 0) == hipSuccess && F.last_bytes == 16 && b.capacity() == 16 && b);
    }
    { // a failed alloc: the owner is empty, what it held is gone, the live set untouched by the failed call
        Buf b;
        F.fail_at = 0;
        CHECK(mk(b, 40) == hipErrorOutOfMemory && !b && b.get() == nullptr && b.capacity() == 0 && F.live.empty());
        CHECK(mk(b, 40) == hipSuccess);
        const size_t a1 = F.allocs;
        F.fail_at = 0;
        CHECK(mk(b, 80) == hipErrorOutOfMemory && !b && b.capacity() == 0 && F.live.empty() && F.allocs == a1);
        F.fail_at = 1; // the second of two
        Buf c;
        CHECK(mk(b, 8) == hipSuccess && mk(c, 8) == hipErrorOutOfMemory && b && !c && F.live.size() == 1);
    }
    CHECK(F.live.empty());
    { // reserve: no call below the capacity, one free and one alloc above it
        Buf b;
        CHECK(grow(b, 100) == hipSuccess && b.capacity() == 100);
        const size_t a1 = F.allocs, f1 = F.frees;
        void* p = b.get();
        CHECK(grow(b, 100) == hipSuccess && grow(b, 1) == hipSuccess && b.get() == p && F.allocs == a1 && F.frees == f1);
        CHECK(grow(b, 101) == hipSuccess && b.capacity() == 101 && F.allocs == a1 + 1 && F.frees == f1 + 1 && F.live.size() == 1);
        F.fail_at = 0; // a failed growth leaves the owner empty: the next reserve allocates again
        CHECK(grow(b, 500) == hipErrorOutOfMemory && !b && b.capacity() == 0 && F.live.empty());
        CHECK(grow(b, 10) == hipSuccess && b.capacity() == 10);
    }
    CHECK(F.live.empty());
    { // a vector of structs that hold owners, growing through reallocation
        struct Layer {
            size_t len = 0;
            Buf adj, adjx;
        };
        std::vector<Layer> v;
        std::vector<void*> want;
        for (size_t i = 0; i < 100; ++i) {
            Layer L;
            L.len = i;
            CHECK(mk(L.adj, 16 + i) == hipSuccess);
            if (i % 3 == 0) CHECK(mk(L.adjx, 8) == hipSuccess);
            want.push_back(L.adj.get());
            v.push_back(std::move(L));
            CHECK(!L.adj && v.back().adj.get() == want.back());
        }
        CHECK(F.live.size() == 100 + 34);
        for (size_t i = 0; i < 100; ++i) CHECK(v[i].len == i && v[i].adj.get() == want[i] && v[i].adj.capacity() == 16 + i);
        v.erase(v.begin() + 10, v.begin() + 20);
        CHECK(F.live.size() == 90 + 34 - 3 && v[10].adj.get() == want[20]);
    }
    CHECK(F.live.empty() && F.allocs - a0 == F.frees - f0);
}

int main() {
    protocol<DevBuf>(g_dev, [](DevBuf& b, size_t n) { return b.alloc(n); }, [](DevBuf& b, size_t n) { return b.reserve(n); });
    CHECK(g_pin.allocs == 0 && g_pin.frees == 0); // the device owner never touches pinned memory ...
    const size_t dev_allocs = g_dev.allocs;
    protocol<PinBuf>(g_pin, [](PinBuf& b, size_t n) { return b.alloc(n, 7u); }, [](PinBuf& b, size_t n) { return b.reserve(n, 7u); });
    CHECK(g_dev.allocs == dev_allocs && g_pin.last_flags == 7u); // ... nor the pinned owner device memory; the flags arrive
    CHECK(g_dev.live.empty() && g_pin.live.empty());
    CHECK(g_dev.allocs == g_dev.frees && g_pin.allocs == g_pin.frees);
    printf("ok\n");
    return 0;
}
