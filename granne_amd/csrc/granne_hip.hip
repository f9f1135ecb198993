// granne_hip.hip -- host runtime + C ABI of libgranne_hip.so (see include/granne_hip.h).
// Compiled by hipcc for gfx950 only; there is no CPU code path for search in this library.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/granne_hip.h"
#include "search_kernel.h"
#include "walk_fast.h"
#include "slow_kernel.h"
#include "util_kernels.h"
#include "brute_force.h"
#include "exact_topk.h"
#include "combiner.h"
#include "dev_mem.h"

using namespace granne_hip;

static_assert(Combiner::DEPTH <= GRANNE_HIP_SEARCH_DEPTH && Combiner::CALL_MAX == GRANNE_HIP_COALESCE_CALL_MAX &&
                  Combiner::CAP_MAX == GRANNE_HIP_COALESCE_MAX,
              "combiner.h and granne_hip.h disagree");

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice ? GRANNE_HIP_ERR_NO_DEVICE \
                                                                            : GRANNE_HIP_ERR_HIP,  \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);   \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
// the stream is idle when the scope ends: declared AFTER the owners whose blocks the stream's work still uses, so that
// an early return does not free them under a running kernel
struct SettleStream {
    hipStream_t s;
    ~SettleStream() { (void)hipStreamSynchronize(s); }
};
// the guard of an entry point: `dev` is current until the scope ends, or the call fails here
#define GRANNE_HIP_ON_DEVICE(dev)                                                                      \
    DeviceGuard g(dev);                                                                               \
    if (!g.ok) return fail(GRANNE_HIP_ERR_NO_DEVICE, "cannot select HIP device %d", dev)

extern "C" const char* granne_hip_last_error(void) { return g_last_error.c_str(); }
extern "C" int granne_hip_abi_version(void) { return GRANNE_HIP_ABI_VERSION; }
extern "C" int granne_hip_device_count(int* out_count) {
    if (!out_count) return fail(GRANNE_HIP_ERR_INVALID, "out_count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        return fail(GRANNE_HIP_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out_count = n;
    return GRANNE_HIP_OK;
}

// experiment knobs, read once per process
struct EnvKnobs {
    int visited = 0, touch_max = -1, inline_tails = 1, seen_min = -1, bf_b16 = 1, bf_ring = 1, sketch = 1, compact_rows = 1;
    EnvKnobs() {
        auto geti = [](const char* name, int dflt) {
            const char* e = getenv(name);
            return e ? atoi(e) : dflt;
        };
        visited = geti("GRANNE_HIP_VISITED", 0); // GRANNE_HIP_OPT_VISITED16's values, where the option says auto
        inline_tails = geti("GRANNE_HIP_INLINE_TAILS", 1); // 0: no index keeps LayerDev::adjx (experiments: the layout before round 6)
        bf_ring = geti("GRANNE_HIP_BF_RING", 1); // 0: the exact scan of 128-byte int8 rows stages its tiles through registers (round 5's bf_i8_kernel)
        bf_b16 = geti("GRANNE_HIP_BF_B16", 1); // 0: the exact scan of f32 rows scores on the f32 matrix path (round 5's: 5 x slower, scores to the last bits)
        seen_min = geti("GRANNE_HIP_SEEN_MIN", -1); // launches of at least this many walks skip revisits before their rows are fetched (-1: default)
        touch_max = geti("GRANNE_HIP_TOUCH_MAX", -1); // launches of up to this many queries touch rows ahead (-1: default)
        compact_rows = geti("GRANNE_HIP_COMPACT_ROWS", 1); // 0: the sketched launches keep two lanes per neighbor slot (A/B of walk_fast.h's CR)
        sketch = geti("GRANNE_HIP_SKETCH", 1); // 0: no index makes row sketches, and no search uses them (A/B of GRANNE_HIP_OPT_SKETCH)
    }
};
static const EnvKnobs& knobs() {
    static const EnvKnobs k;
    return k;
}

// ------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------
// search_launch's scratch blocks, one per stream that has searched (see scratch_for)
struct ScratchCache {
    struct Block {
        hipStream_t stream;
        DevBuf p;
        uint64_t last_use;   // `uses` at the block's last launch
        uint32_t small_runs; // consecutive launches that needed less than a quarter of an oversized block
        std::chrono::steady_clock::time_point last_time; // wall clock of the block's last launch
    };
    std::mutex mu;
    std::vector<Block> blocks;
    uint64_t uses = 0;
    // blocks of streams that gave their place up: freed by search_launch AFTER it has released `mu` (hipFree waits for
    // the device; every concurrent searcher of the index would wait with it under the lock)
    std::vector<DevBuf> graveyard;
};

// A SumEmbeddings container's device copy (sum_embeddings_host.h): immutable once made, shared by the container and by
// every compact index and builder made from it, freed with the last of them.
struct SeDev {
    int device = 0;
    uint32_t dim = 0, tstride = 0; // floats per table row; floats from one row to the next (rows padded to 16 bytes)
    uint64_t n_embeddings = 0, n = 0, n_terms = 0;
    DevBuf d_table, d_offsets, d_terms; // float [n_embeddings][tstride], uint64_t [n + 1], uint32_t [n_terms]
    uint64_t bytes() const { return n_embeddings * tstride * 4u + (n + 1) * 8u + n_terms * 4u; }
    ~SeDev() { // (the members go after this body: freed here, under the guard)
        DeviceGuard g(device);
        d_table.reset(), d_offsets.reset(), d_terms.reset();
    }
};
#define GRANNE_HIP_COMPACT_UNSUPPORTED(ix, what)                                                                        \
    do {                                                                                                                \
        if ((ix) && (ix)->se)                                                                                           \
            return fail(GRANNE_HIP_ERR_INVALID, what " needs dense rows: make the index with GRANNE_HIP_SE_MATERIALIZED (a compact SumEmbeddings index keeps none)"); \
    } while (0)

struct LayerHost {
    uint64_t len = 0;
    uint32_t width = 0;     // caller's row width
    uint32_t dev_width = 0; // multiple of 32
    DevBuf d_adj;  // uint32_t [len][dev_width]
    DevBuf d_adjx; // the register walker's copy: ids + the neighbors' row tails (LayerDev::adjx), or empty
    uint32_t adjx_stride = 0;
};

struct granne_hip_index {
    int device = 0;
    uint32_t dim = 0;
    int dtype = 0;
    uint64_t n_elements = 0;
    uint32_t row_bytes = 0;  // data bytes of a device row (zero padded to 16)
    uint32_t row_stride = 0; // bytes from one device row to the next
    DevBuf d_elements;
    std::shared_ptr<SeDev> se; // a compact SumEmbeddings index: no d_elements, vectors are made from the term lists
    std::vector<LayerHost> layers;
    DevBuf d_layers; // LayerDev [layers.size()]
    uint64_t hbm_bytes = 0;
    uint32_t max_dev_width = 32;
    // options
    uint64_t opt_visited_slots = 0;
    uint64_t opt_force_slow = 0;
    uint64_t opt_force_general = 0; // GRANNE_HIP_OPT_FORCE_GENERAL: no register walker
    uint64_t opt_slow_slots = 1u << 18;
    uint64_t opt_slow_blocks = 16;
    uint64_t opt_overflow_slots = 0; // 0 auto, 1 off, else slots per overflow table
    uint64_t opt_visited16 = 0;      // 0 auto, 1 off, 2 always the 20-bit entries (tests)
    uint64_t opt_visited16_lg = 0;   // 0 auto, else log2(buckets)
    uint64_t opt_inline_tails = 1;   // GRANNE_HIP_OPT_INLINE_TAILS: keep LayerDev::adjx for the shapes that have one
    uint64_t opt_seen_min = 2048;    // GRANNE_HIP_OPT_SEEN_MIN: launches of at least this many walks skip revisits before their rows are fetched
    uint64_t opt_sketch = 1;         // GRANNE_HIP_OPT_SKETCH: the register walker rejects candidates by their row sketch (when d_sketch exists)
    std::atomic<uint64_t> last_slow_count{0};
    std::atomic<uint64_t> last_walker{0}; // GRANNE_HIP_OPT_LAST_WALKER
    std::atomic<uint64_t> last_compact{0}; // GRANNE_HIP_OPT_LAST_COMPACT_ROWS
    std::atomic<uint64_t> last_split{0};   // GRANNE_HIP_OPT_LAST_SPLIT_TAIL
    std::atomic<uint64_t> last_scan{0};    // GRANNE_HIP_OPT_LAST_SCAN
    // the exact scan of int8 rows (brute_force.h): 1 / |x| per row, made at the first scan
    std::mutex norm_mu;
    DevBuf d_inv_norm;
    // f32 rows of the sketched shapes: one SKETCH_LINE per row (search_kernel.h), made with the index, or null
    DevBuf d_sketch;
    // host-pointer searches (granne_hip_search / _search_batch): a stream, a device buffer and a pinned
    // staging buffer per concurrent caller, kept for the life of the index -- the reference's API is one
    // query per call (src/index/mod.rs:140-150), so a call must not pay stream creation and hipMalloc
    struct HostCall {
        hipStream_t stream = nullptr;
        DevBuf d_buf;
        PinBuf h_pin;
    };
    std::mutex call_mu;
    std::vector<HostCall*> call_free;
    // GRANNE_HIP_OPT_COALESCE: host-pointer calls of up to GRANNE_HIP_COALESCE_CALL_MAX queries that are inside the
    // library at the same moment share launches (combiner.h); each of the combiner's slots has a context of its own,
    // whose pinned block grows to what its largest group needed
    uint64_t opt_coalesce = 0;
    Combiner combiner;
    HostCall* group_call[Combiner::DEPTH] = {};
    ScratchCache scratch;
    // granne_hip_search_begin_device / _end_device: batches in flight on streams of the index's own
    struct Flight {
        hipStream_t stream = nullptr;
        hipEvent_t ready = nullptr, done = nullptr;
        bool busy = false;
        uint64_t seq = 0;
    };
    std::mutex flight_mu;
    Flight flights[GRANNE_HIP_SEARCH_DEPTH_MAX];
    uint32_t depth = GRANNE_HIP_SEARCH_DEPTH; // GRANNE_HIP_OPT_SEARCH_DEPTH
    uint32_t next_flight = 0;
    uint64_t next_seq = 1;
};

static inline uint32_t elem_size(int dtype) { return dtype == GRANNE_HIP_F32 ? 4u : dtype == GRANNE_HIP_F16 ? 2u : 1u; }
// bytes of a query component: rows of halves are searched with prepared f32 queries
static inline uint32_t query_elem_size(int dtype) { return dtype == GRANNE_HIP_I8 ? 1u : 4u; }
static inline bool known_dtype(int dtype) { return dtype == GRANNE_HIP_F32 || dtype == GRANNE_HIP_I8 || dtype == GRANNE_HIP_F16; }
// what has no form for rows of halves says so
#define GRANNE_HIP_F16_UNSUPPORTED(dt, what)                                                                            \
    do {                                                                                                                \
        if ((dt) == GRANNE_HIP_F16)                                                                                     \
            return fail(GRANNE_HIP_ERR_INVALID, what " has no form for GRANNE_HIP_F16 (angular_f16) rows: use f32 or int8 rows"); \
    } while (0)

static uint32_t next_pow2(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

// device row stride: f32 rows are padded to 16 bytes; i8 rows to a power of two (<= 1024) or a
// multiple of 1024 so that a row is split over a power-of-two number of lanes and never
// straddles more 128-byte lines than it has to (SURVEY 7 "unaligned rows").
static uint32_t device_row_bytes(uint32_t dim, int dtype) {
    if (dtype == GRANNE_HIP_F32) return (dim * 4u + 15u) & ~15u;
    if (dtype == GRANNE_HIP_F16) return f16_row_bytes(dim);
    if (dim <= 1024) return next_pow2(dim < 16 ? 16 : dim);
    return (dim + 1023u) & ~1023u;
}

// Bytes from one device row to the next. f32 rows of 256 bytes and more start on a 128-byte line: the register walker
// reads a row's 32-float chunks as whole lines, and when the layers carry the neighbors' tails next to their ids
// (LayerDev::adjx) that is all it reads of a row -- a 100-d row is three lines, not the four a 400-byte stride touches.
static uint32_t device_row_stride(uint32_t dim, int dtype) {
    const uint32_t rb = device_row_bytes(dim, dtype);
    if (dtype == GRANNE_HIP_F32 && rb >= 256u) return (rb + 127u) & ~127u;
    // rows of halves of 128 bytes and more start on a line too: a row touches ceil(bytes / 128) of them (100-d: two)
    if (dtype == GRANNE_HIP_F16 && rb >= 128u) return (rb + 127u) & ~127u;
    return rb;
}
// 16-byte units of a row's tail (the dim % 32 last floats) that LayerDev::adjx carries per neighbor; 0: the shape has no
// such copy. The unrolled f32 walkers (dims 100 and 200) read it; their layers are 32 ids wide.
static uint32_t inline_tail_units(uint32_t dim, int dtype) {
    if (dtype != GRANNE_HIP_F32 || (dim != 100u && dim != 200u)) return 0u;
    return (dim % 32u) / 4u;
}
// the scan's per-row norms: inv_norm [n_pad], then inv_gmax [n_pad / 32][2] (brute_force.h)
static inline uint64_t inv_norm_bytes(uint64_t n) {
    const uint64_t n_pad = (n + 31u) & ~31ull;
    return (n_pad + n_pad / 16 + 1 + 16) * 4; // (+16: bf_i8_ring_kernel reads a tile's eight inv_gmax entries in one scalar load, past the last block's too)
}

static int grid_for(uint64_t work, int block) {
    uint64_t g = (work + block - 1) / block;
    if (g > 256ull * 32) g = 256ull * 32;
    if (g < 1) g = 1;
    return (int)g;
}

static int validate_common(granne_hip_index** out, uint64_t n_elements, uint32_t dim, int dtype, uint32_t n_layers,
                           const uint64_t* layer_len) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!known_dtype(dtype)) return fail(GRANNE_HIP_ERR_INVALID, "unknown dtype %d", dtype);
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n_elements >= 0xFFFFFFFFull)
        return fail(GRANNE_HIP_ERR_INVALID, "too many elements (reference limit, src/index/mod.rs:420)");
    if (n_layers && !layer_len) return fail(GRANNE_HIP_ERR_INVALID, "layer_len is null");
    for (uint32_t l = 0; l < n_layers; ++l) {
        if (layer_len[l] > n_elements)
            return fail(GRANNE_HIP_ERR_INVALID, "layer %u has %llu nodes but only %llu elements", l,
                        (unsigned long long)layer_len[l], (unsigned long long)n_elements);
        if (l > 0 && layer_len[l] < layer_len[l - 1])
            return fail(GRANNE_HIP_ERR_INVALID, "layers must be prefix-nested (layer %u shrinks)", l);
        if (layer_len[l] == 0) return fail(GRANNE_HIP_ERR_INVALID, "layer %u is empty", l);
    }
    return GRANNE_HIP_OK;
}

// rows first .. first + count - 1 of a container as dense host rows [count][dim] (sum_embeddings_host.h)
static int se_rows_to_host(const SeDev& se, uint64_t first, uint64_t count, int normalised, float* out);

static void destroy_index(granne_hip_index* ix) {
    if (!ix) return;
    DeviceGuard g(ix->device);
    for (auto* c : ix->group_call)
        if (c) ix->call_free.push_back(c);
    for (auto* c : ix->call_free) {
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
    }
    for (auto& f : ix->flights) {
        if (f.stream) (void)hipStreamSynchronize(f.stream);
        if (f.ready) (void)hipEventDestroy(f.ready);
        if (f.done) (void)hipEventDestroy(f.done);
        if (f.stream) (void)hipStreamDestroy(f.stream);
    }
    delete ix; // (the memory goes here, under the guard, after the streams)
}
// an index in the making: destroyed by an early return, release()d to the caller once everything has been made
struct IndexDeleter {
    void operator()(granne_hip_index* ix) const { destroy_index(ix); }
};
using IndexPtr = std::unique_ptr<granne_hip_index, IndexDeleter>;

// src is a device pointer to dense rows; fills ix->d_elements
static int upload_elements_from_device(granne_hip_index* ix, const void* d_src, hipStream_t s) {
    uint64_t n = ix->n_elements;
    uint32_t dense = ix->dim * elem_size(ix->dtype);
    size_t bytes = (size_t)n * ix->row_stride;
    HIP_TRY(ix->d_elements.alloc(bytes));
    ix->hbm_bytes += bytes;
    if (n == 0) return GRANNE_HIP_OK;
    if (dense == ix->row_stride) {
        HIP_TRY(hipMemcpyAsync(ix->d_elements.get(), d_src, bytes, hipMemcpyDeviceToDevice, s));
    } else {
        uint64_t units = n * (ix->row_stride / 16);
        hipLaunchKernelGGL(relayout_rows_kernel, dim3(grid_for(units, 256)), dim3(256), 0, s, (const uint8_t*)d_src,
                           ix->d_elements.as<uint8_t>(), n, dense, ix->row_stride);
        HIP_TRY(hipGetLastError());
    }
    return GRANNE_HIP_OK;
}

// (Re)makes the register walker's copies of the layers (LayerDev::adjx) -- or drops them when the option is off or the
// shape has none. The layers and the elements are final when this runs (finish_layers).
static int make_inline_tails(granne_hip_index* ix, hipStream_t s) {
    for (auto& L : ix->layers) {
        if (L.d_adjx) {
            L.d_adjx.reset();
            ix->hbm_bytes -= (uint64_t)L.len * L.adjx_stride;
            L.adjx_stride = 0;
        }
    }
    const uint32_t tu = ix->se ? 0u : inline_tail_units(ix->dim, ix->dtype);
    if (!tu || !ix->opt_inline_tails || !knobs().inline_tails) return GRANNE_HIP_OK;
    for (auto& L : ix->layers)
        if (L.dev_width != 32u) return GRANNE_HIP_OK; // layers of up to 64 ids (WIDE) read their tails from the rows
    for (auto& L : ix->layers) {
        L.adjx_stride = 128u + 32u * tu * 16u;
        const size_t bytes = (size_t)L.len * L.adjx_stride;
        if (L.d_adjx.alloc(bytes) != hipSuccess) {
            // The copy is an accelerator, not part of the index: an index that fits without it (a 200M x 100-d shard: 128 GB
            // of copy) is made without it -- the walkers then read the tails from the rows' own last line.
            (void)hipGetLastError();
            for (auto& M : ix->layers) {
                if (M.d_adjx) {
                    (void)hipStreamSynchronize(s); // (inline_tails_kernel is still writing the copy)
                    M.d_adjx.reset();
                    ix->hbm_bytes -= (uint64_t)M.len * M.adjx_stride;
                }
                M.adjx_stride = 0;
            }
            return GRANNE_HIP_OK;
        }
        ix->hbm_bytes += bytes;
        if (L.len)
            hipLaunchKernelGGL(inline_tails_kernel, dim3(grid_for(L.len * 32u * (1u + tu), 256)), dim3(256), 0, s,
                               L.d_adj.as<uint32_t>(), L.len, ix->d_elements.as<uint8_t>(), ix->row_stride, (ix->dim / 32u) * 128u, tu,
                               L.d_adjx.as<uint8_t>(), L.adjx_stride);
        HIP_TRY(hipGetLastError());
    }
    return GRANNE_HIP_OK;
}

// The exact scan of int8 rows (brute_force.h) reads 1 / |x| per row and the largest of them per half block of 32: made
// here, when the index is made (and again after reorder), on the creating stream -- a scan never allocates, never
// synchronises its caller's stream and can be captured (round 5 made them lazily inside the first scan, under norm_mu).
static int make_scan_norms(granne_hip_index* ix, hipStream_t s) {
    if (ix->dtype != GRANNE_HIP_I8 || ix->n_elements == 0) return GRANNE_HIP_OK;
    std::lock_guard<std::mutex> lk(ix->norm_mu);
    if (ix->d_inv_norm) return GRANNE_HIP_OK;
    const uint64_t n = ix->n_elements, n_pad = (n + 31u) & ~31ull;
    DevBuf norms;
    HIP_TRY(norms.alloc((size_t)inv_norm_bytes(n)));
    float* dn = norms.as<float>();
    hipLaunchKernelGGL(inv_norm_rows_kernel, dim3(grid_for(n * 8, 256)), dim3(256), 0, s, ix->d_elements.as<uint8_t>(), n, ix->row_stride, dn);
    hipLaunchKernelGGL(inv_gmax_kernel, dim3(grid_for(n_pad / 16 + 1, 256)), dim3(256), 0, s, (const float*)dn, n, dn + n_pad);
    if (hipGetLastError() != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "inv_norm_rows_kernel failed");
    ix->d_inv_norm = std::move(norms); // (finish_layers synchronises s before the index is handed out)
    ix->hbm_bytes += inv_norm_bytes(n);
    return GRANNE_HIP_OK;
}

// The register walker's row sketches (search_kernel.h SKETCH_LINE, walk_fast.h FastWalker::sketch_rejects): made here
// (and again after reorder: the rows moved), never inside a search, so that searches stay capturable. Like LayerDev::adjx
// they are an accelerator, not part of the index: without room for them the index is made without (searches read every
// row, as they would with GRANNE_HIP_OPT_SKETCH = 0), and the room is judged with headroom left for what searches allocate.
static int make_row_sketch(granne_hip_index* ix, hipStream_t s) {
    if (ix->se || ix->dtype != GRANNE_HIP_F32 || !sketch_dim_ok(ix->dim) || ix->n_elements == 0 || !knobs().sketch) return GRANNE_HIP_OK;
    const uint64_t n = ix->n_elements;
    const size_t bytes = (size_t)n * SKETCH_LINE;
    if (!ix->d_sketch) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return GRANNE_HIP_OK;
        }
        if ((uint64_t)free_b < (uint64_t)bytes + total_b / 32u) return GRANNE_HIP_OK;
        if (ix->d_sketch.alloc(bytes) != hipSuccess) {
            (void)hipGetLastError();
            return GRANNE_HIP_OK;
        }
        ix->hbm_bytes += bytes;
    }
    hipLaunchKernelGGL(row_sketch_kernel, dim3(grid_for(n, 256)), dim3(256), 0, s, ix->d_elements.as<uint8_t>(), n, ix->row_stride, ix->dim,
                       ix->d_sketch.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK; // (finish_layers synchronises s before the index is handed out)
}

static int finish_layers(granne_hip_index* ix, hipStream_t s) {
    std::vector<LayerDev> h(ix->layers.size());
    ix->max_dev_width = 32;
    {
        int r = make_inline_tails(ix, s);
        if (r == 0) r = make_scan_norms(ix, s);
        if (r == 0) r = make_row_sketch(ix, s);
        if (r) return r;
    }
    // rows that name a neighbor twice (LAYER_TWIN_ROWS, walk_fast.h): looked for once, here, on the device rows
    DevBuf found_buf;
    std::vector<uint32_t> found(h.size(), 0u);
    if (!h.empty()) {
        HIP_TRY(found_buf.alloc(h.size() * 4));
        if (hipMemsetAsync(found_buf.get(), 0, h.size() * 4, s) != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "hipMemsetAsync failed");
    }
    uint32_t* const d_found = found_buf.as<uint32_t>();
    for (size_t l = 0; l < ix->layers.size(); ++l) {
        h[l].adj = ix->layers[l].d_adj.as<uint32_t>();
        h[l].len = ix->layers[l].len;
        h[l].width = ix->layers[l].dev_width;
        h[l].flags = 0;
        h[l].adjx = ix->layers[l].d_adjx.as<uint8_t>();
        h[l].adjx_stride = ix->layers[l].adjx_stride;
        h[l].reserved = 0;
        if (ix->layers[l].dev_width > ix->max_dev_width) ix->max_dev_width = ix->layers[l].dev_width;
        if (h[l].len && h[l].width <= 64)
            hipLaunchKernelGGL(twin_rows_kernel, dim3(grid_for(h[l].len * 64, 256)), dim3(256), 0, s, h[l].adj, h[l].len,
                               h[l].width, d_found + l);
    }
    if (!h.empty()) {
        hipError_t e = hipMemcpyAsync(found.data(), d_found, h.size() * 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "twin_rows_kernel: %s", hipGetErrorString(e));
        for (size_t l = 0; l < h.size(); ++l)
            if (found[l]) h[l].flags |= LAYER_TWIN_ROWS;
    }
    size_t bytes = sizeof(LayerDev) * (h.size() ? h.size() : 1);
    HIP_TRY(ix->d_layers.alloc(bytes));
    if (!h.empty()) HIP_TRY(hipMemcpyAsync(ix->d_layers.get(), h.data(), sizeof(LayerDev) * h.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GRANNE_HIP_OK;
}

static int add_layer_from_device_rows(granne_hip_index* ix, uint64_t len, uint32_t width, const uint32_t* d_rows,
                                      hipStream_t s) {
    LayerHost L;
    L.len = len;
    L.width = width;
    L.dev_width = (width + 31u) & ~31u;
    if (L.dev_width == 0) L.dev_width = 32;
    size_t bytes = (size_t)len * L.dev_width * 4;
    HIP_TRY(L.d_adj.alloc(bytes));
    ix->hbm_bytes += bytes;
    const uint32_t dev_width = L.dev_width;
    ix->layers.push_back(std::move(L));
    uint32_t* const d_adj = ix->layers.back().d_adj.as<uint32_t>();
    if (width == 0) {
        HIP_TRY(hipMemsetAsync(d_adj, 0xFF, bytes, s));
    } else {
        hipLaunchKernelGGL(relayout_adj_kernel, dim3(grid_for(len * dev_width, 256)), dim3(256), 0, s, d_rows,
                           d_adj, len, width, dev_width);
        HIP_TRY(hipGetLastError());
    }
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_index_create_device(granne_hip_index** out, const void* d_elements, uint64_t n_elements,
                                              uint32_t dim, int dtype, uint32_t n_layers, const uint64_t* layer_len,
                                              const uint32_t* const* d_layer_rows, const uint32_t* layer_width,
                                              int device_id, void* stream) {
    int rc = validate_common(out, n_elements, dim, dtype, n_layers, layer_len);
    if (rc) return rc;
    if (n_elements && !d_elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    if (n_layers && (!d_layer_rows || !layer_width)) return fail(GRANNE_HIP_ERR_INVALID, "layer arrays are null");
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = (hipStream_t)stream;
    granne_hip_index* ix = new granne_hip_index();
    ix->device = device_id;
    ix->dim = dim;
    ix->dtype = dtype;
    ix->n_elements = n_elements;
    ix->row_bytes = device_row_bytes(dim, dtype);
    ix->row_stride = device_row_stride(dim, dtype);
    rc = upload_elements_from_device(ix, d_elements, s);
    DevBuf bad_buf; // neighbor ids outside their layer (the file loader checks the same on the host)
    if (rc == 0 && bad_buf.alloc(4) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMalloc failed");
    uint32_t* const d_bad = bad_buf.as<uint32_t>();
    if (rc == 0 && hipMemsetAsync(d_bad, 0, 4, s) != hipSuccess) rc = fail(GRANNE_HIP_ERR_HIP, "hipMemsetAsync failed");
    for (uint32_t l = 0; rc == 0 && l < n_layers; ++l) {
        rc = add_layer_from_device_rows(ix, layer_len[l], layer_width[l], d_layer_rows[l], s);
        const uint64_t total = layer_len[l] * layer_width[l];
        if (rc == 0 && total)
            hipLaunchKernelGGL(check_adj_kernel, dim3(grid_for(total, 256)), dim3(256), 0, s, d_layer_rows[l], total,
                               layer_len[l], d_bad);
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

extern "C" int granne_hip_index_create(granne_hip_index** out, const void* elements, uint64_t n_elements, uint32_t dim,
                                       int dtype, uint32_t n_layers, const uint64_t* layer_len,
                                       const uint32_t* const* layer_rows, const uint32_t* layer_width, int device_id) {
    int rc = validate_common(out, n_elements, dim, dtype, n_layers, layer_len);
    if (rc) return rc;
    if (n_elements && !elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    if (n_layers && (!layer_rows || !layer_width)) return fail(GRANNE_HIP_ERR_INVALID, "layer arrays are null");
    GRANNE_HIP_ON_DEVICE(device_id);

    // stage the host buffers on the device, then share the device path
    DevBuf d_el;
    size_t el_bytes = (size_t)n_elements * dim * elem_size(dtype);
    std::vector<DevBuf> staged(n_layers);
    std::vector<const uint32_t*> d_rows(n_layers, nullptr);
    hipError_t e = d_el.alloc(el_bytes);
    if (e == hipSuccess && el_bytes) e = hipMemcpy(d_el.get(), elements, el_bytes, hipMemcpyHostToDevice);
    for (uint32_t l = 0; e == hipSuccess && l < n_layers; ++l) {
        size_t b = (size_t)layer_len[l] * layer_width[l] * 4;
        e = staged[l].alloc(b);
        d_rows[l] = staged[l].as<uint32_t>();
        if (e == hipSuccess && b) e = hipMemcpy(staged[l].get(), layer_rows[l], b, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
        return fail(e == hipErrorNoDevice ? GRANNE_HIP_ERR_NO_DEVICE : GRANNE_HIP_ERR_HIP, "staging upload failed: %s",
                    hipGetErrorString(e));
    return granne_hip_index_create_device(out, d_el.get(), n_elements, dim, dtype, n_layers, layer_len, d_rows.data(), layer_width,
                                          device_id, nullptr);
}

extern "C" int granne_hip_index_create_csr(granne_hip_index** out, const void* elements, uint64_t n_elements,
                                           uint32_t dim, int dtype, uint32_t n_layers, const uint64_t* layer_len,
                                           const uint64_t* const* layer_offsets, const uint32_t* const* layer_ids,
                                           int device_id) {
    int rc = validate_common(out, n_elements, dim, dtype, n_layers, layer_len);
    if (rc) return rc;
    if (n_elements && !elements) return fail(GRANNE_HIP_ERR_INVALID, "elements is null");
    if (n_layers && (!layer_offsets || !layer_ids)) return fail(GRANNE_HIP_ERR_INVALID, "layer arrays are null");
    GRANNE_HIP_ON_DEVICE(device_id);

    granne_hip_index* ix = new granne_hip_index();
    ix->device = device_id;
    ix->dim = dim;
    ix->dtype = dtype;
    ix->n_elements = n_elements;
    ix->row_bytes = device_row_bytes(dim, dtype);
    ix->row_stride = device_row_stride(dim, dtype);
    IndexPtr made(ix);
    DevBuf d_el;
    size_t el_bytes = (size_t)n_elements * dim * elem_size(dtype);
    HIP_TRY(d_el.alloc(el_bytes));
    if (el_bytes) HIP_TRY(hipMemcpy(d_el.get(), elements, el_bytes, hipMemcpyHostToDevice));
    rc = upload_elements_from_device(ix, d_el.get(), nullptr);
    if (rc) return rc;
    for (uint32_t l = 0; l < n_layers; ++l) {
        uint64_t len = layer_len[l];
        const uint64_t* off = layer_offsets[l];
        uint32_t maxdeg = 0;
        for (uint64_t i = 0; i < len; ++i) {
            if (off[i + 1] < off[i]) return fail(GRANNE_HIP_ERR_INVALID, "layer %u: offsets not monotone", l);
            uint64_t d = off[i + 1] - off[i];
            if (d > 0xFFFF) return fail(GRANNE_HIP_ERR_INVALID, "layer %u: degree too large", l);
            if (d > maxdeg) maxdeg = (uint32_t)d;
        }
        for (uint64_t t = 0; t < off[len]; ++t)
            if (layer_ids[l][t] >= len) return fail(GRANNE_HIP_ERR_INVALID, "layer %u: neighbor id outside the layer", l);
        LayerHost L;
        L.len = len;
        L.width = maxdeg;
        L.dev_width = ((maxdeg ? maxdeg : 1) + 31u) & ~31u;
        size_t bytes = (size_t)len * L.dev_width * 4;
        HIP_TRY(L.d_adj.alloc(bytes));
        ix->hbm_bytes += bytes;
        const uint32_t dev_width = L.dev_width;
        ix->layers.push_back(std::move(L));
        DevBuf d_off, d_ids;
        size_t nids = (size_t)off[len];
        HIP_TRY(d_off.alloc((len + 1) * 8));
        HIP_TRY(d_ids.alloc(nids * 4));
        hipError_t e1 = hipMemcpy(d_off.get(), off, (len + 1) * 8, hipMemcpyHostToDevice);
        hipError_t e2 = nids ? hipMemcpy(d_ids.get(), layer_ids[l], nids * 4, hipMemcpyHostToDevice) : hipSuccess;
        if (e1 == hipSuccess && e2 == hipSuccess) {
            hipLaunchKernelGGL(csr_to_adj_kernel, dim3(grid_for(len * dev_width, 256)), dim3(256), 0, nullptr,
                               d_off.as<uint64_t>(), d_ids.as<uint32_t>(), ix->layers.back().d_adj.as<uint32_t>(), len, dev_width);
            e1 = hipDeviceSynchronize();
        }
        if (e1 != hipSuccess || e2 != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "CSR upload failed");
    }
    rc = finish_layers(ix, nullptr);
    if (rc) return rc;
    *out = made.release();
    return GRANNE_HIP_OK;
}

extern "C" void granne_hip_index_destroy(granne_hip_index* index) { destroy_index(index); }

extern "C" uint64_t granne_hip_index_len(const granne_hip_index* ix) {
    return (ix && !ix->layers.empty()) ? ix->layers.back().len : 0; // src/index/mod.rs:76-83
}
extern "C" uint64_t granne_hip_index_num_elements(const granne_hip_index* ix) { return ix ? ix->n_elements : 0; }
extern "C" uint32_t granne_hip_index_num_layers(const granne_hip_index* ix) { return ix ? (uint32_t)ix->layers.size() : 0; }
extern "C" uint64_t granne_hip_index_layer_len(const granne_hip_index* ix, uint32_t layer) {
    return (ix && layer < ix->layers.size()) ? ix->layers[layer].len : 0;
}
extern "C" uint32_t granne_hip_index_dim(const granne_hip_index* ix) { return ix ? ix->dim : 0; }
extern "C" int granne_hip_index_dtype(const granne_hip_index* ix) { return ix ? ix->dtype : -1; }
extern "C" int granne_hip_index_device(const granne_hip_index* ix) { return ix ? ix->device : -1; }
extern "C" uint64_t granne_hip_index_hbm_bytes(const granne_hip_index* ix) { return ix ? ix->hbm_bytes : 0; }

extern "C" int granne_hip_index_get_neighbors(const granne_hip_index* ix, uint64_t node, uint32_t layer,
                                              uint32_t* out_ids, uint32_t cap, uint32_t* out_count) {
    if (!ix || !out_count) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (layer >= ix->layers.size()) return fail(GRANNE_HIP_ERR_INVALID, "layer %u out of range", layer);
    const LayerHost& L = ix->layers[layer];
    if (node >= L.len) return fail(GRANNE_HIP_ERR_INVALID, "node out of range");
    DeviceGuard g(ix->device);
    std::vector<uint32_t> row(L.dev_width);
    HIP_TRY(hipMemcpy(row.data(), L.d_adj.as<uint32_t>() + node * L.dev_width, (size_t)L.dev_width * 4, hipMemcpyDeviceToHost));
    uint32_t n = 0;
    while (n < L.dev_width && row[n] != GRANNE_HIP_UNUSED) ++n;
    *out_count = n;
    for (uint32_t i = 0; i < n && i < cap && out_ids; ++i) out_ids[i] = row[i];
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_index_get_element(const granne_hip_index* ix, uint64_t idx, void* out) {
    if (!ix || !out) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    if (idx >= ix->n_elements) return fail(GRANNE_HIP_ERR_INVALID, "element index out of range");
    if (ix->se) return se_rows_to_host(*ix->se, idx, 1, 1, (float*)out); // ElementContainer::get: the normalised vector
    DeviceGuard g(ix->device);
    HIP_TRY(hipMemcpy(out, ix->d_elements.as<uint8_t>() + idx * ix->row_stride, (size_t)ix->dim * elem_size(ix->dtype),
                      hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_index_get_sketch(const granne_hip_index* ix, uint64_t first, uint64_t count, void* out) {
    if (!ix || (!out && count)) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "get_sketch");
    if (!ix->d_sketch) return fail(GRANNE_HIP_ERR_INVALID, "the index holds no row sketches");
    if (first > ix->n_elements || count > ix->n_elements - first) return fail(GRANNE_HIP_ERR_INVALID, "rows out of range");
    if (count == 0) return GRANNE_HIP_OK;
    DeviceGuard g(ix->device);
    HIP_TRY(hipMemcpy(out, ix->d_sketch.as<uint8_t>() + first * SKETCH_LINE, (size_t)count * SKETCH_LINE, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_index_set_option(granne_hip_index* ix, int option, uint64_t value) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    switch (option) {
    case GRANNE_HIP_OPT_VISITED_SLOTS:
        {
            const uint64_t odd = value ? value >> __builtin_ctzll(value) : 1; // 2^k or 3 * 2^k
            if (value != 0 && (value < 256 || value > 32768 || (odd != 1 && odd != 3)))
                return fail(GRANNE_HIP_ERR_INVALID, "visited slots must be 0, 2^k or 3 * 2^k in [256, 32768]");
        }
        ix->opt_visited_slots = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_FORCE_SLOW:
        ix->opt_force_slow = value ? 1 : 0;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_FORCE_GENERAL:
        ix->opt_force_general = value ? 1 : 0;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SLOW_SLOTS:
        if (value < 256 || value > (1ull << 30) || (value & (value - 1)))
            return fail(GRANNE_HIP_ERR_INVALID, "slow slots must be a power of two in [256, 2^30]");
        ix->opt_slow_slots = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SLOW_BLOCKS:
        if (value < 1 || value > 1024) return fail(GRANNE_HIP_ERR_INVALID, "slow blocks must be in [1, 1024]");
        ix->opt_slow_blocks = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_OVERFLOW_SLOTS:
        if (value > 1 && (value < 512 || value > (1ull << 20) || (value & (value - 1))))
            return fail(GRANNE_HIP_ERR_INVALID, "overflow slots must be 0 (auto), 1 (off) or a power of two in [512, 2^20]");
        ix->opt_overflow_slots = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_VISITED16:
        if (value > 4) return fail(GRANNE_HIP_ERR_INVALID, "the visited-set option must be 0 (auto = none), 1..3 (the exact set) or 4 (none)");
        ix->opt_visited16 = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SEARCH_DEPTH: {
        if (value < 1 || value > GRANNE_HIP_SEARCH_DEPTH_MAX) return fail(GRANNE_HIP_ERR_INVALID, "search depth must be in [1, %d]", GRANNE_HIP_SEARCH_DEPTH_MAX);
        std::lock_guard<std::mutex> lk(ix->flight_mu);
        for (auto& f : ix->flights)
            if (f.busy) return fail(GRANNE_HIP_ERR_INVALID, "the depth cannot change while a batch is in flight");
        ix->depth = (uint32_t)value;
        ix->next_flight = 0;
        return GRANNE_HIP_OK;
    }
    case GRANNE_HIP_OPT_INLINE_TAILS: {
        if (value > 1) return fail(GRANNE_HIP_ERR_INVALID, "the inline-tails option is 0 or 1");
        GRANNE_HIP_ON_DEVICE(ix->device);
        HIP_TRY(hipDeviceSynchronize()); // (searches in flight read the copy and the layer table this replaces)
        ix->opt_inline_tails = value;
        return finish_layers(ix, nullptr);
    }
    case GRANNE_HIP_OPT_SEEN_MIN:
        ix->opt_seen_min = value > 0xFFFFFFFFull ? 0xFFFFFFFFull : value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SKETCH:
        if (value > 1) return fail(GRANNE_HIP_ERR_INVALID, "the sketch option is 0 or 1");
        ix->opt_sketch = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_VISITED16_LG: // (retired with the bucket tables it sized: accepted, ignored)
        if (value > 12) return fail(GRANNE_HIP_ERR_INVALID, "value out of range");
        ix->opt_visited16_lg = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE:
        if (value > 1) return fail(GRANNE_HIP_ERR_INVALID, "the coalesce option is 0 or 1");
        ix->opt_coalesce = value;
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE_MAX:
        if (value < 1 || value > GRANNE_HIP_COALESCE_MAX) return fail(GRANNE_HIP_ERR_INVALID, "the coalesce cap must be in [1, %d]", GRANNE_HIP_COALESCE_MAX);
        ix->combiner.set_cap((uint32_t)value);
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE_WAIT_US:
        ix->combiner.set_wait_us(value);
        return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCED_LAUNCHES:
    case GRANNE_HIP_OPT_COALESCED_QUERIES:
    case GRANNE_HIP_OPT_LAST_COMPACT_ROWS:
    case GRANNE_HIP_OPT_LAST_SPLIT_TAIL:
    case GRANNE_HIP_OPT_LAST_SCAN:
        return fail(GRANNE_HIP_ERR_INVALID, "option %d is read-only", option);
    default:
        return fail(GRANNE_HIP_ERR_INVALID, "unknown option %d", option);
    }
}

extern "C" int granne_hip_index_get_option(const granne_hip_index* ix, int option, uint64_t* value) {
    if (!ix || !value) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    switch (option) {
    case GRANNE_HIP_OPT_VISITED_SLOTS: *value = ix->opt_visited_slots; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_FORCE_SLOW: *value = ix->opt_force_slow; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_FORCE_GENERAL: *value = ix->opt_force_general; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SLOW_SLOTS: *value = ix->opt_slow_slots; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SLOW_BLOCKS: *value = ix->opt_slow_blocks; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_OVERFLOW_SLOTS: *value = ix->opt_overflow_slots; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_VISITED16: *value = ix->opt_visited16; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_VISITED16_LG: *value = ix->opt_visited16_lg; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_LAST_WALKER: *value = ix->last_walker.load(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SEARCH_DEPTH: *value = ix->depth; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_INLINE_TAILS: *value = (!ix->layers.empty() && ix->layers.back().d_adjx) ? 1 : 0; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SEEN_MIN: *value = ix->opt_seen_min; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_SKETCH: *value = (ix->opt_sketch && ix->d_sketch && knobs().sketch) ? 1 : 0; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE: *value = ix->opt_coalesce; return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE_MAX: *value = ix->combiner.cap(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCE_WAIT_US: *value = ix->combiner.wait_us(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCED_LAUNCHES: *value = ix->combiner.launches(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_COALESCED_QUERIES: *value = ix->combiner.queries(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_LAST_COMPACT_ROWS: *value = ix->last_compact.load(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_LAST_SPLIT_TAIL: *value = ix->last_split.load(); return GRANNE_HIP_OK;
    case GRANNE_HIP_OPT_LAST_SCAN: *value = ix->last_scan.load(); return GRANNE_HIP_OK;
    default: return fail(GRANNE_HIP_ERR_INVALID, "unknown option %d", option);
    }
}

extern "C" uint64_t granne_hip_index_last_slow_count(const granne_hip_index* ix) {
    return ix ? ix->last_slow_count.load() : 0;
}

// ------------------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------------------
// A search's scratch block (control words, overflow-region states, hand-over list, overflow tables, the exact
// walker's containers) is kept per (index, stream) for the life of the index: launches on one stream run in
// order, so they can share a block, and the kernels leave its control words and region states zeroed -- no
// allocator call and no memset per search.
constexpr size_t SLOW_SCRATCH_BUDGET = (size_t)1 << 30;               // bytes of exact-walker containers per scratch block
constexpr uint32_t SCRATCH_MAX_REGIONS = 16384;                       // 256 CUs x 32 waves x 2
constexpr size_t SCRATCH_STATE_OFF = CTL_WORDS * 4;                   // region states follow the control words
constexpr size_t SCRATCH_FIXED = SCRATCH_STATE_OFF + (size_t)SCRATCH_MAX_REGIONS * 4; // zero between launches

constexpr size_t SCRATCH_CACHE_STREAMS = 64;      // streams that keep a block for the life of the index
constexpr int SCRATCH_IDLE_SECONDS = 10;          // a cached stream idle this long gives its place to a newcomer when the cache is full
constexpr size_t SCRATCH_SHRINK_ABOVE = 256u << 20; // a cached block this large is let go when a launch needs < 1/4 of it

// `*transient` is set when the block was taken from the stream-ordered allocator for this launch alone (the cache is
// full: a caller with more live streams than SCRATCH_CACHE_STREAMS): the caller frees it with hipFreeAsync after its
// last use on `s`. No device-wide synchronisation anywhere.
static int scratch_for(ScratchCache* cache, hipStream_t s, size_t total, uint8_t** out, bool* transient) {
    // (the caller holds cache->mu for the enqueue)
    *transient = false;
    ScratchCache::Block* b = nullptr;
    cache->uses += 1;
    for (auto& x : cache->blocks)
        if (x.stream == s) b = &x;
    if (!b) {
        if (cache->blocks.size() >= SCRATCH_CACHE_STREAMS) {
            // a stream that has not searched for a long while (destroyed, most likely) gives its place up; while every
            // cached stream is in use the newcomer takes a block from the stream-ordered allocator for this launch alone
            ScratchCache::Block* lru = &cache->blocks[0];
            for (auto& x : cache->blocks)
                if (x.last_use < lru->last_use) lru = &x;
            // idle for SCRATCH_IDLE_SECONDS of wall clock (not "for so many launches": a live stream that pauses while others
            // search keeps its block)
            const auto idle = std::chrono::steady_clock::now() - lru->last_time;
            if (idle > std::chrono::seconds(SCRATCH_IDLE_SECONDS)) {
                if (lru->p) cache->graveyard.push_back(std::move(lru->p)); // freed once the lock is released (search_launch)
                *lru = {s, DevBuf(), cache->uses, 0, std::chrono::steady_clock::now()};
                b = lru;
            } else {
                HIP_TRY(hipMallocAsync((void**)out, total, s));
                HIP_TRY(hipMemsetAsync(*out, 0, SCRATCH_FIXED, s));
                *transient = true;
                return GRANNE_HIP_OK;
            }
        } else {
            cache->blocks.push_back({s, DevBuf(), cache->uses, 0, std::chrono::steady_clock::now()});
            b = &cache->blocks.back();
        }
    }
    b->last_use = cache->uses;
    b->last_time = std::chrono::steady_clock::now();
    // a block left oversized by one exact-walker batch is let go once eight launches in a row needed less than a quarter
    // of it (not at the first: a stream that alternates the two kinds of batches keeps its block)
    if (b->p.capacity() > SCRATCH_SHRINK_ABOVE && total < b->p.capacity() / 4) b->small_runs += 1;
    else b->small_runs = 0;
    const bool oversized = b->small_runs >= 8;
    if (b->p.capacity() < total || oversized) {
        if (b->p) {
            HIP_TRY(hipStreamSynchronize(s)); // earlier launches on this stream still use the old block
            b->p.reset();
        }
        b->small_runs = 0;
        HIP_TRY(b->p.alloc(total + (total >> 2))); // some headroom: batch sizes vary
        HIP_TRY(hipMemsetAsync(b->p.get(), 0, SCRATCH_FIXED, s));
    }
    *out = b->p.as<uint8_t>();
    return GRANNE_HIP_OK;
}

namespace { // (the planners' types stay out of the library's exports)
// what a search launch needs to know about the graph it walks: an index's, or the layers a builder has so far
struct SearchTarget {
    int device;
    const uint8_t* d_elements;
    uint64_t n_elements;
    uint32_t dim;
    int dtype;
    // stage_row_bytes: bytes of a row AS THE WALKERS STAGE IT (the query in LDS, the stage slots; SearchParams::row_bytes):
    // the device row's own for f32 and int8, the widened f32 row's for rows of halves. elem_row_bytes / row_stride: the
    // device rows themselves -- what anything that READS rows goes by.
    uint32_t stage_row_bytes, elem_row_bytes, row_stride;
    const LayerDev* d_layers;
    uint32_t n_layers;
    uint32_t max_dev_width;
    uint64_t opt_force_general = 0;
    uint64_t opt_visited_slots = 0, opt_force_slow = 0, opt_slow_slots = 1u << 18, opt_slow_blocks = 16, opt_overflow_slots = 0;
    uint64_t opt_visited16 = 0;
    uint64_t opt_seen_min = 0xFFFFFFFFull;
    const uint8_t* d_sketch = nullptr; // row sketches the register walker may use (an index's, when GRANNE_HIP_OPT_SKETCH is on)
    const SeDev* se = nullptr;         // a compact SumEmbeddings index: no dense rows (d_elements is null)
    ScratchCache* scratch;             // search_launch's per-stream scratch blocks
    std::atomic<uint64_t>* last_walker = nullptr; // which walker the last launch took (an index's read-only option)
    std::atomic<uint64_t>* last_compact = nullptr; // ... and whether it ran the compacted row stage
    std::atomic<uint64_t>* last_split = nullptr;   // ... and whether its tail blocks were a kernel of their own

    // G: granne_hip_index, or granne_hip_builder (builder_host.h) searching its `layers`. A builder's searches differ in
    // these ways only: no row sketches, seen_min never reached (its layers change between launches, its batches are its
    // own), its own scratch cache, its row width W as the widest layer's; every other option keeps its default.
    template <class G>
    SearchTarget(const G* g, const LayerDev* layers, uint32_t n_layers)
        : device(g->device), d_elements(g->d_elements.template as<uint8_t>()), n_elements(g->n_elements), dim(g->dim), dtype(g->dtype),
          stage_row_bytes(g->dtype == GRANNE_HIP_F16 ? (g->dim * 4u + 15u) & ~15u : g->row_bytes), elem_row_bytes(g->row_bytes),
          row_stride(g->row_stride),
          d_layers(layers), n_layers(n_layers), scratch(&const_cast<G*>(g)->scratch) {
        if constexpr (std::is_same<G, granne_hip_index>::value) {
            max_dev_width = g->max_dev_width;
            opt_visited_slots = g->opt_visited_slots;
            opt_force_slow = g->opt_force_slow;
            opt_force_general = g->opt_force_general;
            opt_slow_slots = g->opt_slow_slots;
            opt_slow_blocks = g->opt_slow_blocks;
            opt_overflow_slots = g->opt_overflow_slots;
            opt_visited16 = g->opt_visited16;
            opt_seen_min = g->opt_seen_min;
            d_sketch = (g->opt_sketch && knobs().sketch) ? g->d_sketch.template as<uint8_t>() : nullptr;
            last_walker = &const_cast<G*>(g)->last_walker;
            last_compact = &const_cast<G*>(g)->last_compact;
            last_split = &const_cast<G*>(g)->last_split;
            se = g->se.get();
        } else {
            max_dev_width = g->W;
        }
    }
};
} // namespace

// One search launch. Every caller sets the queries, nq, ef, k and the stream; of the rest only what it uses.
struct SearchCall {
    const void* queries = nullptr;
    int64_t q_stride = 0; // bytes from one query to the next (0: the target's row length, dim x element size)
    uint32_t nq = 0, ef = 0, k = 0;
    uint64_t* ids = nullptr;
    float* dists = nullptr;
    uint32_t* counts = nullptr;
    uint64_t* stats = nullptr;
    uint32_t* status = nullptr; // the caller's status words (d_status of the C ABI), or null
    hipStream_t stream = nullptr;
    uint32_t* slow_count = nullptr;  // u32[2] on the host: hand-overs and exhaustion (the call waits for the launch)
    uint32_t* trail = nullptr;       // [nq][8]: trail mode (Granne::reorder), no search outputs
    uint32_t trail_layers = 0;
    hipEvent_t ev_before = nullptr, ev_after = nullptr;
    uint32_t* host_status = nullptr; // u32[2], host-mapped: hand-over count and exhaustion flag, plain stores
    const BatchIO* batches = nullptr;
    uint32_t n_batches = 0;          // > 0: `nq` queries in EACH of these, one launch
    // filtered search (filter.h, filter_host.h): the bitmaps, words from one query's to the next (0: one for all), the
    // cap on bottom-layer pops (0: none). Never planned on a register walker.
    const uint32_t* filter = nullptr;
    uint64_t filter_stride = 0;
    uint32_t max_expand = 0;
};

typedef void (*search_fn)(const SlowParams);

// The general walker (search_kernel.h): run-time dims, any row width. nullptr: not instantiated.
template <int DT>
static search_fn general_kernel_s(uint32_t S) {
    switch (S) {
    case 1: return search_kernel<DT, 0, 1>;
    case 2: return search_kernel<DT, 0, 2>;
    case 4: return search_kernel<DT, 0, 4>;
    }
    return nullptr;
}
// the general walker of a compact SumEmbeddings index (sum_embeddings.h): f32, run-time dim, no trail walks
static search_fn compact_kernel_s(uint32_t S) {
    switch (S) {
    case 1: return search_kernel<DT_F32, 0, 1, false, PV_SE>;
    case 2: return search_kernel<DT_F32, 0, 2, false, PV_SE>;
    case 4: return search_kernel<DT_F32, 0, 4, false, PV_SE>;
    }
    return nullptr;
}
// the general walker over rows of halves (f16.h): f32 queries, run-time dim, no trail walks
static search_fn f16_kernel_s(uint32_t S) {
    switch (S) {
    case 1: return search_kernel<DT_F32, 0, 1, false, PV_F16>;
    case 2: return search_kernel<DT_F32, 0, 2, false, PV_F16>;
    case 4: return search_kernel<DT_F32, 0, 4, false, PV_F16>;
    }
    return nullptr;
}
// the general walker under an id bitmap (filter.h): dense f32 / int8 rows, run-time dims, no trail walks
template <int DT>
static search_fn filtered_kernel_s(uint32_t S) {
    switch (S) {
    case 1: return search_kernel<DT, 0, 1, false, PV_DENSE, true>;
    case 2: return search_kernel<DT, 0, 2, false, PV_DENSE, true>;
    case 4: return search_kernel<DT, 0, 4, false, PV_DENSE, true>;
    }
    return nullptr;
}
static search_fn general_kernel_of(int dtype, uint32_t S, bool trail) {
    const bool i8 = dtype == GRANNE_HIP_I8;
    if (trail) // Granne::reorder's trail walks (max_search 1)
        return S != 1 ? nullptr : i8 ? (search_fn)search_kernel<DT_I8, 0, 1, true> : (search_fn)search_kernel<DT_F32, 0, 1, true>;
    return i8 ? general_kernel_s<DT_I8>(S) : general_kernel_s<DT_F32>(S);
}

// The register walkers instantiated (walk_fast.h), by the values their LDS is sized from: the row shape DT, DIM (f32 rows of
// 100 / 200 dims unrolled, 0: any other f32 dim streamed; int8 rows of 128 bytes as DIM 0, of 256 / 512 bytes as DIM 256 /
// 512), the list slots S, the visited form V16, trail mode and 64-id layers (WIDE). nullptr: not instantiated.
template <int DT, int DIM, int S>
static search_fn fast_kernel_v(int v16, bool cr) {
    constexpr bool streamed = (DT == DT_F32 && DIM == 0) || (DT == DT_I8 && DIM >= 256);
    if constexpr (DT == DT_F32 && sketch_dim_ok((uint32_t)DIM) && S <= 4) { // the sketched launches: survivors' rows only (walk_fast.h, CR)
        if (v16 == 5 && cr) return fast_kernel<DT, DIM, S, false, 5, false, GRANNE_HIP_CR_G>; // (the walkers alone: tail_kernel follows, plan_walk's `split`)
    }
    if constexpr (S == 1 && !streamed) {
        if (v16 == 4) return fast_kernel<DT, DIM, S, false, 4>;
    }
    if constexpr (DT == DT_F32 && S <= 4) {
        if (v16 == 5) return fast_kernel<DT, DIM, S, false, 5>;
    }
    if (v16 == 3) return fast_kernel<DT, DIM, S, false, 3>;
    if constexpr (S <= 17 && !walk_list_is_long(S, false)) { // (longer lists: an exact set of ~40 x max_search ids fits no LDS)
        if (v16 == 0) return fast_kernel<DT, DIM, S>;
    }
    return nullptr;
}
template <int DT, int DIM>
static search_fn fast_kernel_s(uint32_t S, bool trail, int v16, bool cr) {
    if (trail) return S == 1 && v16 == 0 ? fast_kernel<DT, DIM, 1, true> : nullptr;
    switch (S) {
    case 1: return fast_kernel_v<DT, DIM, 1>(v16, cr);
    case 2: return fast_kernel_v<DT, DIM, 2>(v16, cr);
    case 4: return fast_kernel_v<DT, DIM, 4>(v16, cr);
    case 8: return fast_kernel_v<DT, DIM, 8>(v16, cr);
    }
    if constexpr (!((DT == DT_F32 && DIM == 0) || (DT == DT_I8 && DIM >= 256))) { // (streamed f32 dims, wide int8 rows: up to 17 slots)
        switch (S) {
        case 33: return fast_kernel_v<DT, DIM, 33>(v16, cr);
        case 65: return fast_kernel_v<DT, DIM, 65>(v16, cr);
        case 129: return fast_kernel_v<DT, DIM, 129>(v16, cr);
        }
    }
    return S == 17 ? fast_kernel_v<DT, DIM, 17>(v16, cr) : nullptr;
}
template <int DT, int DIM>
static search_fn fast_wide_kernel_s(uint32_t S) {
    switch (S) {
    case 1: return fast_kernel<DT, DIM, 1, false, 3, true>;
    case 2: return fast_kernel<DT, DIM, 2, false, 3, true>;
    case 4: return fast_kernel<DT, DIM, 4, false, 3, true>;
    case 8: return fast_kernel<DT, DIM, 8, false, 3, true>;
    case 17: return fast_kernel<DT, DIM, 17, false, 3, true>;
    }
    return nullptr;
}
static search_fn fast_kernel_of(const SearchTarget& T, uint32_t S, bool trail, int v16, bool wide, bool cr) {
    const bool i8 = T.dtype == GRANNE_HIP_I8;
    if (wide) { // (64-id layers: no visited set, no trail walks, int8 rows of 128 bytes)
        if (trail || v16 != 3 || (i8 && T.stage_row_bytes != 128)) return nullptr;
        if (i8) return fast_wide_kernel_s<DT_I8, 0>(S);
        return T.dim == 100 ? fast_wide_kernel_s<DT_F32, 100>(S) : T.dim == 200 ? fast_wide_kernel_s<DT_F32, 200>(S) : fast_wide_kernel_s<DT_F32, 0>(S);
    }
    if (i8 && T.stage_row_bytes == 256) return fast_kernel_s<DT_I8, 256>(S, trail, v16, cr);
    if (i8 && T.stage_row_bytes == 512) return fast_kernel_s<DT_I8, 512>(S, trail, v16, cr);
    if (i8) return T.stage_row_bytes == 128 ? fast_kernel_s<DT_I8, 0>(S, trail, v16, cr) : nullptr;
    return T.dim == 100 ? fast_kernel_s<DT_F32, 100>(S, trail, v16, cr) : T.dim == 200 ? fast_kernel_s<DT_F32, 200>(S, trail, v16, cr) : fast_kernel_s<DT_F32, 0>(S, trail, v16, cr);
}

// which walker serves a launch, its kernel, and how the launch is sized
struct WalkPlan {
    uint64_t walker = GRANNE_HIP_WALKER_GENERAL; // what GRANNE_HIP_OPT_LAST_WALKER reports
    uint32_t S = 0;         // list slots of 64 keys
    int v16 = 0;            // FastWalker's V16: 0 = the exact 32-bit table, 3 = no visited set, 4 = none + rows touched
                            // ahead, 5 = none + revisits skipped before their rows are fetched
    bool cr = false;        // FastWalker's CR: the sketched launches evaluate the surviving neighbors only, several lanes to a row
    search_fn fn = nullptr; // null: the launch cannot be planned (the error is set)
    uint32_t lds_bytes = 0; // the launch's dynamic LDS
    uint32_t grid = 0;      // blocks of 64 lanes: the walkers, then the tail blocks; or the exact walker's blocks alone
    uint32_t visited_slots = 0, upper_slots = 0, front_eighths = 7;
    uint32_t maxc = 0, lrow_bytes = 16, stage_bytes = 0, adjspec_bytes = 0;
    uint32_t ovf_slots = 0, ovf_regions = 0; // visited-set overflow tables
    uint32_t slow_blocks = 0, tail_blocks = 0; // the exact walker's containers; its blocks behind the walkers
    // The split form (the compacted launches: walk_fast.h, fast_kernel's CR): `fn` is the walkers alone on a grid of nq, and
    // tail_fn (slow_kernel.h, tail_kernel) follows it on the stream with tail_blocks blocks of tail_lds bytes. hand_all:
    // every walker hands its query over (GRANNE_HIP_OPT_FORCE_SLOW on a launch that splits).
    bool split = false, hand_all = false;
    search_fn tail_fn = nullptr;
    uint32_t tail_lds = 0;
};

// The register walker (walk_fast.h) serves the common shapes: every layer up to 64 ids wide on the device, ids within 31
// bits, f32 rows of any dim or int8 rows of 128 / 256 / 512 bytes. Its list holds 64*S keys and must hold max_search of
// them plus a few spare places: two distances of a walk tie surprisingly often (4000 candidates share 2^23 float values),
// and a tie between entry max_search-1 and an entry pushed off the end hands the walk over -- with spare places that takes
// a run of ties.
constexpr uint32_t FAST_MAX_SEARCH = 8192; // f32 rows of 100 / 200 dims and int8 rows of 128 bytes: two-level lists of up to 129 x 64 keys

// `filtered`: a filtered search -- the general walker when max_search allows it, else the exact one, never a register walker.
static WalkPlan plan_walk(const SearchTarget& T, uint32_t ef, uint32_t nq, bool trail, bool filtered = false) {
    WalkPlan P;
    const bool i8 = T.dtype == GRANNE_HIP_I8;
    const bool streamed = !i8 && T.dim != 100 && T.dim != 200; // f32: 100 and 200 fully unrolled, any other dim streamed (dims below 32: the tail alone)
    // Layers of up to 64 ids per node (graphs with num_neighbors 33..63: the GPU builder makes them, BuildConfig::num_neighbors
    // src/index/mod.rs:242) are walked in two passes of 32 pairs per expansion (FastWalker's WIDE) -- instantiated for lists of
    // up to 17 x 64 keys, without a visited set, not for Granne::reorder's trail walks, and for int8 rows of 128 bytes only.
    const bool wide = T.max_dev_width == 64;
    // (ids: 31 bits. A 2^31-element index needs 275 GB for its bottom layer's 128-byte adjacency rows alone, so the
    //  reference's 2^32 - 2 capacity, src/index/mod.rs:27-28, is out of one device's reach whatever the key layout)
    const bool shape = T.max_dev_width <= 64 && T.n_elements <= WALK_MAX_ELEMENTS &&
                       (!i8 || T.stage_row_bytes == 128 || (!wide && (T.stage_row_bytes == 256 || T.stage_row_bytes == 512))); // (int8 dims <= 512)
    // the longest max_search the register walker is instantiated for: lists of up to 17 x 64 keys for 64-id layers, int8
    // rows of 256 / 512 bytes and streamed f32 dims, else two-level lists of up to 129 x 64 keys
    const uint32_t fast_max = (wide || (i8 ? T.stage_row_bytes != 128 : streamed)) ? 1024u : FAST_MAX_SEARCH;
    // a compact SumEmbeddings index has no rows, sketches or inline tails for the register walker to read: every walk of
    // it is the general walker's (max_search up to 256) or the exact walker's
    const bool compact = T.se != nullptr;
    if (compact && (trail || i8)) {
        fail(GRANNE_HIP_ERR_INVALID, "a compact SumEmbeddings index serves searches only: make the index with GRANNE_HIP_SE_MATERIALIZED");
        return P;
    }
    // rows of halves are normalised where they are read: the general walker (max_search up to 256) or the exact walker
    // make them, never the register walker (walk_fast.h reads prepared f32 / int8 rows)
    const bool f16 = T.dtype == GRANNE_HIP_F16;
    if (f16 && trail) {
        fail(GRANNE_HIP_ERR_INVALID, "reorder has no form for GRANNE_HIP_F16 (angular_f16) rows");
        return P;
    }
    if (filtered && (compact || f16 || trail)) {
        fail(GRANNE_HIP_ERR_INVALID, "filtered search has no form for this index");
        return P;
    }
    const bool fast = !compact && !f16 && !filtered && !(T.opt_force_general && !trail) && shape && ef <= fast_max && !(wide && trail);
    const uint32_t ef_walk = fast ? ef : (ef > 256 ? 256 : ef); // what the register / general walker is sized for
    const bool all_slow = T.opt_force_slow || (!fast && ef > 256);
    P.walker = all_slow ? GRANNE_HIP_WALKER_EXACT
                        : fast ? (wide ? GRANNE_HIP_WALKER_REGISTER_WIDE : GRANNE_HIP_WALKER_REGISTER) : GRANNE_HIP_WALKER_GENERAL;
    if (fast)
        P.S = ef <= 60 ? 1u : ef <= 124 ? 2u : ef <= 252 ? 4u : ef <= 508 ? 8u : ef <= 1024 ? 17u : ef <= 2048 ? 33u : ef <= 4096 ? 65u : 129u;
    else
        P.S = ef_walk <= 64 ? 1u : ef_walk <= 128 ? 2u : 4u;

    // The register walkers walk without a visited set by default (VisitedNone, wave_prims.h: the list itself is searched for
    // a candidate's id): no table in LDS, only the query's staging area and what a tail block needs, so the registers
    // alone bound the walkers per CU. GRANNE_HIP_OPT_VISITED16 = 1..3 switches the exact set on (a 32-bit open-addressing
    // table in LDS + a global overflow table): n_dist is then the reference's count of distinct evaluated nodes.
    const int vmode = T.opt_visited16 ? (int)T.opt_visited16 : knobs().visited;
    const bool none = vmode == 4 || vmode == 0;
    const bool longest = walk_list_is_long((int)P.S, wide) || wide; // (lists of 33 / 65 / 129 slots, and 64-id layers: instantiated without a set only, whatever the options say)
    uint32_t walk_lds;
    if (fast && !trail && ((none && !T.opt_visited_slots) || longest)) {
        // a launch of a few queries leaves the chip idle: its walkers touch the next node's rows ahead (walk_fast.h, TOUCH)
        const uint32_t touch_max = knobs().touch_max >= 0 ? (uint32_t)knobs().touch_max : 256u; // (round 5: +4 % at 256 queries, -10 % at 1024: profiles/r5_touch.txt)
        const bool touch_shape = P.S == 1 && !wide && !streamed && !(i8 && T.stage_row_bytes != 128);
        P.v16 = (touch_shape && nq <= touch_max) ? 4 : 3;
        // launches of many walks are bound by bandwidth: their walkers skip revisits BEFORE the rows are fetched (walk_fast.h, SEEN)
        const uint64_t seen_min = knobs().seen_min >= 0 ? (uint64_t)knobs().seen_min : T.opt_seen_min; // (GRANNE_HIP_SEEN_MIN overrides the option: experiments)
        // (f32 rows: the walkers per CU are bound by registers there, 8 KB of cache each fit; int8 walkers are four times as many
        //  and lose more to the look-up than the few revisits of their rows cost: measured, profiles/r6_seen_ab.txt)
        if (P.S <= 4 && !wide && !i8 && nq >= seen_min) P.v16 = 5; // (every f32 dim: unrolled and streamed)
        // ... and, where they reject neighbors by the index's row sketch, read the rows of the survivors only (walk_fast.h, CR)
        P.cr = P.v16 == 5 && !i8 && sketch_dim_ok(T.dim) && T.d_sketch != nullptr && knobs().compact_rows != 0;
        // ... in a kernel that holds the walker and nothing else, built for five or six waves per SIMD: the tail blocks of these
        // launches are a kernel of their own behind it (slow_kernel.h, tail_kernel). Measured on launches of 2,048 and of 4,096
        // walks, which the chip holds whole at four waves per SIMD, as on the larger ones: the second kernel costs 5 us and
        // the walkers gain more, so every compacted launch takes this form.
        P.split = P.cr && !wide;
        walk_lds = fast_lds_bytes(i8, streamed, T.dim, T.stage_row_bytes, P.S, 0u, P.v16 == 5, wide);
        const uint32_t least = lds_query_bytes(T.stage_row_bytes) + 64u * 8u; // int8 query staging; a tail block (slow_kernel.h)
        if (walk_lds < least) walk_lds = least;
    } else {
        // The front table must hold the walk's visited ids (~40 x max_search on 10M uniform points) below its 7/8
        // load limit: 4096 slots at max_search 50. (Tables of 3 * 2^k slots are accepted as an option; 3072 slots --
        // 12 KB, twelve walkers per CU instead of nine -- measured no faster: 0.5 % of the walks spill to the
        // overflow table and a launch lasts as long as its slowest walk.)
        uint32_t want = T.opt_visited_slots ? (uint32_t)T.opt_visited_slots : next_pow2(ef_walk * 64u);
        if (!T.opt_visited_slots) {
            if (want < 1024) want = 1024;
            // larger walks spill to the global overflow table. A launch with more walkers than the chip
            // holds is better off with small tables (more walkers per CU; measured on the 10M build:
            // 37.7 s vs 45.4 s), one batch of a thousand queries with fewer spills (ef 200: 508k vs 421k q/s)
            uint32_t cap = nq >= 4096 ? 4096u : 8192u;
            // long lists (max_search > 252) walk ~20x max_search nodes: most inserts land in the overflow table
            // whatever the front table's size, and a 32 KB front table beside the list's LDS mirror leaves room
            // for only three walkers per CU (768 of a batch of 1024 resident: the batch runs in two rounds)
            if (fast && P.S >= 8) cap = 4096u;
            if (want > cap) want = cap;
        }
        P.visited_slots = want;
        P.upper_slots = want < 1024 ? want : 1024;
        if (fast) { // walk_fast.h: [query][S >= 8: 64*S keys][visited front table]
            walk_lds = fast_lds_bytes(i8, streamed, T.dim, T.stage_row_bytes, P.S, P.visited_slots, false, wide);
        } else {
            // the general walker (search_kernel.h): int8 keeps its speculative adjacency rows in registers (Walker::REGSPEC),
            // run-time-dim f32 parks them in LDS. LDS plan: the visited table dominates; the f32 stage gets what keeps four
            // walkers per CU (160 KiB / 4) when that leaves it at least 16 rows, else up to 32 rows within 64 KiB, else
            // whatever fits in the CU's 160 KiB.
            P.adjspec_bytes = i8 ? 0u : LDS_ADJSPEC_BYTES;
            const uint32_t fixed = lds_query_bytes(T.stage_row_bytes) + LDS_FIXED_BYTES + P.adjspec_bytes;
            if (!i8) {
                P.lrow_bytes = ((T.stage_row_bytes / 16) | 1u) * 16u; // odd number of 16-byte units: conflict-free ds_read_b128
                const uint32_t wmax = T.max_dev_width < 64 ? T.max_dev_width : 64;
                const uint32_t used = fixed + P.visited_slots * 4u;
                auto rows_in = [&](uint32_t budget) { return budget > used ? (budget - used) / P.lrow_bytes : 0u; };
                uint32_t maxc = rows_in(40u * 1024u);
                if (maxc < 16) maxc = rows_in(64u * 1024u) < 32u ? rows_in(64u * 1024u) : 32u;
                if (maxc < 16) maxc = rows_in(160u * 1024u) < 32u ? rows_in(160u * 1024u) : 32u;
                if (maxc > wmax) maxc = wmax;
                if (maxc < 1) maxc = 1;
                P.maxc = maxc;
                P.stage_bytes = P.maxc * P.lrow_bytes;
            }
            walk_lds = fixed + P.stage_bytes + P.visited_slots * 4u;
        }
    }
    if (walk_lds > 160u * 1024u) {
        fail(GRANNE_HIP_ERR_INVALID, "dimension too large for the LDS stage");
        return P;
    }
    // A walk that will outgrow the front table anyway (it visits ~40 x max_search nodes) freezes it at 5/8 load
    // instead of 7/8: every later lookup of a new id runs to an empty slot of the frozen table, 8 probes on average
    // at 7/8 load with the wave waiting for its slowest lane, 2.7 at 5/8 (C5-like int8 walk at max_search 200:
    // launch 2.70 -> 2.44 ms; f32 at 800: 7.75 -> 6.5 ms).
    P.front_eighths = (!P.v16 && (uint64_t)ef * 40u > (uint64_t)P.visited_slots) ? 5u : 7u;

    // visited-set overflow pool: one table per walker that can be resident at once (bounded by
    // LDS: 160 KiB per CU, and by 32 waves per CU), at most one per query
    if (!all_slow && T.opt_overflow_slots != 1 && P.v16 < 3) { // (no visited set, no overflow)
        P.ovf_slots = T.opt_overflow_slots ? next_pow2((uint32_t)T.opt_overflow_slots) : next_pow2(ef_walk * 64u);
        if (!T.opt_overflow_slots && P.ovf_slots < 4096) P.ovf_slots = 4096;
        if (P.ovf_slots < 512) P.ovf_slots = 512;
        if (P.ovf_slots > (1u << 20)) P.ovf_slots = 1u << 20;
        uint32_t per_cu = (160u * 1024u) / (walk_lds ? walk_lds : 1u);
        if (per_cu > 32) per_cu = 32;
        if (per_cu < 1) per_cu = 1;
        P.ovf_regions = 256u * per_cu * 2u; // 2x the residency bound keeps the region probe short
        if (P.ovf_regions > nq) P.ovf_regions = nq;
        if (P.ovf_regions > SCRATCH_MAX_REGIONS) P.ovf_regions = SCRATCH_MAX_REGIONS;
    }

    // The exact walker's blocks: a few as the tail of a register-walker launch (hand-overs are rare), many when the whole
    // batch is its to walk (max_search beyond the register lists, GRANNE_HIP_OPT_FORCE_SLOW): one block per query up to
    // 32x the option (512 at its default of 16). Every block owns 12 bytes x slow_slots + 8 x max_search of global scratch
    // (3 MB at the default 2^18 slots), and the scratch block is kept per (index, stream): the many-block form is bounded
    // by SLOW_SCRATCH_BUDGET bytes (never below the option itself), so that a handful of streams searching beyond the
    // register lists hold a few GB, not tens.
    P.slow_blocks = (uint32_t)T.opt_slow_blocks;
    const uint32_t slow_lds = lds_query_bytes(T.stage_row_bytes) + 64 * 8;
    if (all_slow) { // every query on the exact walker: its kernel alone
        uint32_t most = P.slow_blocks * 32u;
        const size_t per_block = (size_t)T.opt_slow_slots * 12 + (size_t)ef * 8;
        const size_t fit = SLOW_SCRATCH_BUDGET / per_block;
        if (most > fit) most = fit > P.slow_blocks ? (uint32_t)fit : P.slow_blocks;
        P.slow_blocks = nq < most ? (nq > P.slow_blocks ? nq : P.slow_blocks) : most;
        if (T.opt_force_slow && fast && P.split) {
            // the option on a launch that splits: the same two kernels, every walker hands its query over and as many tail
            // blocks as the exact walker's own launch has walk the list
            P.hand_all = true;
            P.fn = fast_kernel_of(T, P.S, trail, P.v16, wide, P.cr);
            P.tail_fn = (search_fn)tail_kernel<DT_F32>;
            if (!P.fn) {
                fail(GRANNE_HIP_ERR_INVALID, "no split walker is instantiated for this launch (list slots %u)", P.S);
                return P;
            }
            P.lds_bytes = walk_lds;
            P.tail_lds = slow_lds;
            P.tail_blocks = P.slow_blocks;
            P.grid = nq;
            return P;
        }
        P.split = false;
        P.fn = compact ? (search_fn)slow_kernel<DT_F32, PV_SE> : f16 ? (search_fn)slow_kernel<DT_F32, PV_F16>
               : filtered ? (!i8 ? (search_fn)slow_kernel<DT_F32, PV_DENSE, true> : (search_fn)slow_kernel<DT_I8, PV_DENSE, true>)
               : !i8 ? (search_fn)slow_kernel<DT_F32> : (search_fn)slow_kernel<DT_I8>;
        P.lds_bytes = slow_lds;
        P.grid = P.slow_blocks;
        return P;
    }
    if (!fast || wide) P.cr = P.split = false;
    if (fast && wide) P.v16 = 3; // (the two-pass walker exists without a visited set only; the same LDS as the touching one)
    P.fn = fast ? fast_kernel_of(T, P.S, trail, P.v16, wide, P.cr) : compact ? compact_kernel_s(P.S) : f16 ? f16_kernel_s(P.S)
           : filtered ? (i8 ? filtered_kernel_s<DT_I8>(P.S) : filtered_kernel_s<DT_F32>(P.S)) : general_kernel_of(T.dtype, P.S, trail);
    if (!P.fn) {
        fail(GRANNE_HIP_ERR_INVALID, "no walker is instantiated for this launch (list slots %u, visited form %d, trail %d, 64-id layers %d)",
             P.S, P.v16, (int)trail, (int)wide);
        return P;
    }
    P.lds_bytes = walk_lds > slow_lds ? walk_lds : slow_lds; // the tail blocks stage a query too
    if (P.lds_bytes > 160u * 1024u) {
        P.fn = nullptr;
        fail(GRANNE_HIP_ERR_INVALID, "dimension too large for the LDS stage");
        return P;
    }
    P.tail_blocks = P.slow_blocks < nq ? P.slow_blocks : nq;
    if (P.split) { // the walkers alone (the compacted f32 walkers: their LDS, not a tail block's); the tail blocks behind them
        P.tail_fn = (search_fn)tail_kernel<DT_F32>;
        P.lds_bytes = walk_lds;
        P.tail_lds = slow_lds;
        P.grid = nq;
        return P;
    }
    P.grid = nq + P.tail_blocks;
    return P;
}

static int search_launch(const SearchTarget& T, SearchCall c) {
    if (c.ef == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    if (c.nq == 0) return GRANNE_HIP_OK;
    if (c.n_batches > MAX_LAUNCH_BATCHES) return fail(GRANNE_HIP_ERR_INVALID, "at most %u batches per launch", MAX_LAUNCH_BATCHES);
    if (c.n_batches && (uint64_t)c.n_batches * c.nq > 0x7FFFFFFFull) return fail(GRANNE_HIP_ERR_INVALID, "too many queries in one launch");
    GRANNE_HIP_ON_DEVICE(T.device);
    hipStream_t s = c.stream;
    const uint32_t batch_nq = c.nq;
    uint32_t nq = c.nq; // walkers of the launch
    if (c.n_batches) {
        for (uint32_t b = 0; b < c.n_batches; ++b)
            if (!c.batches[b].queries || !c.batches[b].out_counts || (c.k && (!c.batches[b].out_ids || !c.batches[b].out_dists)))
                return fail(GRANNE_HIP_ERR_INVALID, "null buffer (batch %u)", b);
        if (c.k == 0) {
            for (uint32_t b = 0; b < c.n_batches; ++b) HIP_TRY(hipMemsetAsync(c.batches[b].out_counts, 0, (size_t)nq * 4, s));
            return GRANNE_HIP_OK;
        }
        c.queries = c.batches[0].queries;
        c.ids = c.batches[0].out_ids;
        c.dists = c.batches[0].out_dists;
        c.counts = c.batches[0].out_counts;
        c.stats = c.batches[0].out_stats;
        nq *= c.n_batches;
    }
    if (c.k == 0 && !c.trail) { // .take(0): every result is empty (src/index/mod.rs:974-977)
        if (!c.counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
        HIP_TRY(hipMemsetAsync(c.counts, 0, (size_t)nq * 4, s));
        return GRANNE_HIP_OK;
    }
    if (!c.queries || (!c.trail && (!c.ids || !c.dists || !c.counts))) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (T.row_stride < T.elem_row_bytes || (T.dtype == GRANNE_HIP_F16 && T.elem_row_bytes != f16_row_bytes(T.dim)))
        return fail(GRANNE_HIP_ERR_INVALID, "search: inconsistent row layout (row bytes %u, stride %u)", T.elem_row_bytes, T.row_stride);
    if (c.filter && (c.n_batches || c.trail)) return fail(GRANNE_HIP_ERR_INVALID, "a filtered search is one batch");
    const WalkPlan W = plan_walk(T, c.ef, nq, c.trail != nullptr, c.filter != nullptr);
    if (!W.fn) return GRANNE_HIP_ERR_INVALID;

    // scratch: [control words][region states] (zero between launches) [hand-over list][overflow tables][exact walker]
    const uint32_t slots = (uint32_t)T.opt_slow_slots;
    const size_t list_bytes = ((size_t)nq * 4 + 15) & ~(size_t)15;
    size_t off_list = SCRATCH_FIXED;
    size_t off_ovf = off_list + list_bytes;
    size_t off_vis = off_ovf + (size_t)W.ovf_regions * W.ovf_slots * 4;
    size_t off_pq = off_vis + (size_t)W.slow_blocks * slots * 4;
    size_t off_res = off_pq + (size_t)W.slow_blocks * slots * 8;
    size_t off_sex = (off_res + (size_t)W.slow_blocks * c.ef * 8 + 15) & ~(size_t)15; // compact indexes: a vector per lane of the exact walker
    const bool lane_x = T.se || T.dtype == GRANNE_HIP_F16; // (rows of halves: the widened row, likewise)
    size_t total = off_sex + (lane_x ? (size_t)W.slow_blocks * 64u * T.dim * 4u : 0u);
    // The cache's mutex covers finding (or growing) this stream's block and the enqueue -- host work of microseconds.
    // Whatever waits for the GPU (the synchronisation behind slow_count) happens after it is released: host threads
    // searching one index on streams of their own do not queue behind each other's kernels.
    // evicted blocks: declared before the lock, so freed after it is released (hipFree waits for the device: whatever
    // still used an evicted block is over)
    std::vector<DevBuf> bury;
    std::unique_lock<std::mutex> cache_lock(T.scratch->mu);
    uint8_t* scratch = nullptr;
    bool transient = false;
    {
        int r = scratch_for(T.scratch, s, total, &scratch, &transient);
        bury.swap(T.scratch->graveyard);
        if (r) return r;
    }
    struct FreeTransient { // a block of the stream-ordered allocator goes back after the launch's last use of it
        uint8_t* p;
        hipStream_t s;
        ~FreeTransient() {
            if (p) (void)hipFreeAsync(p, s);
        }
    } free_transient{transient ? scratch : nullptr, s};
    uint32_t* ctl = (uint32_t*)scratch;

    SlowParams sp;
    SearchParams& p = sp.sp;
    p.elements = T.d_elements;
    p.n_elements = T.n_elements;
    p.dim = T.dim;
    p.row_bytes = T.stage_row_bytes;
    p.row_stride = T.row_stride;
    p.layers = T.d_layers;
    p.n_layers = T.n_layers;
    p.queries = (const uint8_t*)c.queries;
    p.q_stride = c.q_stride ? c.q_stride : (int64_t)T.dim * query_elem_size(T.dtype);
    p.nq = nq;
    p.ef = c.ef;
    p.k = c.k;
    p.out_ids = c.ids;
    p.out_dists = c.dists;
    p.out_counts = c.counts;
    p.out_stats = c.stats;
    p.visited_slots = W.visited_slots;
    p.upper_slots = W.upper_slots;
    p.front_eighths = W.front_eighths;
    p.maxc = W.maxc;
    p.lrow_bytes = W.lrow_bytes;
    p.stage_bytes = W.stage_bytes;
    p.adjspec_bytes = W.adjspec_bytes;
    p.slow_count = ctl + CTL_SLOW_COUNT;
    p.slow_list = (uint32_t*)(scratch + off_list);
    p.force_slow = W.hand_all ? 1u : 0u;
    p.spec = 1;
    p.sketch = T.d_sketch;
    p.ovf.tables = (uint32_t*)(scratch + off_ovf);
    p.ovf.state = (uint32_t*)(scratch + SCRATCH_STATE_OFF);
    p.ovf.slots = W.ovf_slots;
    p.ovf.stride = W.ovf_slots;
    p.ovf.regions = W.ovf_regions;
    p.ovf.spilled = c.status ? c.status + 2 : ctl + CTL_SPILLED;
    p.trail_out = c.trail;
    p.trail_layers = c.trail_layers;
    p.n_batches = c.n_batches;
    p.batch_nq = batch_nq;
    for (uint32_t b = 0; b < c.n_batches; ++b) p.batch[b] = c.batches[b];
    sp.ctl = ctl;
    sp.vis = (uint32_t*)(scratch + off_vis);
    sp.pq = (uint64_t*)(scratch + off_pq);
    sp.res = (uint64_t*)(scratch + off_res);
    sp.slots = slots;
    sp.all = (W.walker == GRANNE_HIP_WALKER_EXACT && !W.split) ? 1u : 0u; // (a split launch walks the hand-over list, whoever filled it)
    sp.status2 = c.status;
    sp.host_status = c.host_status;
    p.se_table = T.se ? T.se->d_table.as<float>() : nullptr;
    p.se_offsets = T.se ? T.se->d_offsets.as<uint64_t>() : nullptr;
    p.se_terms = T.se ? T.se->d_terms.as<uint32_t>() : nullptr;
    sp.se_x = lane_x ? (float*)(scratch + off_sex) : nullptr;
    p.filter = c.filter;
    p.filter_stride = c.filter_stride;
    p.max_expand = c.max_expand;
    p.cut_count = c.status ? c.status + 3 : nullptr;

    if (T.last_walker) T.last_walker->store(W.walker);
    if (T.last_compact) T.last_compact->store(W.cr ? 1 : 0);
    if (T.last_split) T.last_split->store(W.split ? 1 : 0);
    if ((W.walker != GRANNE_HIP_WALKER_EXACT || W.split) && W.lds_bytes > 32u * 1024u)
        HIP_TRY(hipFuncSetAttribute((const void*)W.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)W.lds_bytes));
    if (c.ev_before) HIP_TRY(hipEventRecord(c.ev_before, s));
    hipLaunchKernelGGL(W.fn, dim3(W.grid), dim3(64), W.lds_bytes, s, sp);
    HIP_TRY(hipGetLastError());
    if (W.split) { // the tail blocks: stream order is what they wait for
        hipLaunchKernelGGL(W.tail_fn, dim3(W.tail_blocks), dim3(64), W.tail_lds, s, sp);
        HIP_TRY(hipGetLastError());
    }
    if (c.ev_after) HIP_TRY(hipEventRecord(c.ev_after, s));

    if (c.slow_count) {
        uint32_t hs[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(hs, ctl + CTL_LAST_SLOW, 8, hipMemcpyDeviceToHost, s)); // enqueued under the lock, ...
        cache_lock.unlock();
        HIP_TRY(hipStreamSynchronize(s));                                               // ... waited for outside it
        c.slow_count[0] = hs[0]; // queries served by the global-memory walker
        c.slow_count[1] = hs[1]; // its containers ran out
    }
    return GRANNE_HIP_OK;
}

// a search of the C ABI's device-pointer entry points on an index
static SearchCall index_call(const void* d_queries, uint32_t nq, uint32_t max_search, uint32_t num_neighbors, uint64_t* d_out_ids,
                             float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_stats, uint32_t* d_status, void* stream) {
    SearchCall c;
    c.queries = d_queries;
    c.nq = nq;
    c.ef = max_search;
    c.k = num_neighbors;
    c.ids = d_out_ids;
    c.dists = d_out_dists;
    c.counts = d_out_counts;
    c.stats = d_out_stats;
    c.status = d_status;
    c.stream = (hipStream_t)stream;
    return c;
}

extern "C" int granne_hip_search_batch_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq,
                                              uint32_t max_search, uint32_t num_neighbors, uint64_t* d_out_ids,
                                              float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_stats,
                                              uint32_t* d_status, void* stream) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    return search_launch(SearchTarget(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size()),
                         index_call(d_queries, nq, max_search, num_neighbors, d_out_ids, d_out_dists, d_out_counts, d_out_stats, d_status, stream));
}

extern "C" int granne_hip_search_batch_device_timed(const granne_hip_index* ix, const void* d_queries, uint32_t nq,
                                                    uint32_t max_search, uint32_t num_neighbors, uint64_t* d_out_ids,
                                                    float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_stats,
                                                    uint32_t* d_status, void* stream, void* ev_before, void* ev_after) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    SearchCall c = index_call(d_queries, nq, max_search, num_neighbors, d_out_ids, d_out_dists, d_out_counts, d_out_stats, d_status, stream);
    c.ev_before = (hipEvent_t)ev_before;
    c.ev_after = (hipEvent_t)ev_after;
    return search_launch(SearchTarget(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size()), c);
}

// A batch in flight beside the caller's stream. begin: the search is ordered after what `stream` holds (an event), runs on
// one of the index's own streams, and the call returns a ticket at once; end: `stream` waits for that search. Between
// the two the caller begins further batches -- the walks of up to GRANNE_HIP_SEARCH_DEPTH batches share the chip, which
// is what a host with a stream of independent batch-sized requests needs (one launch of 1024 walks is one wave per SIMD).
extern "C" int granne_hip_search_begin_device(const granne_hip_index* cix, const void* d_queries, uint32_t nq,
                                              uint32_t max_search, uint32_t num_neighbors, uint64_t* d_out_ids,
                                              float* d_out_dists, uint32_t* d_out_counts, uint64_t* d_out_stats,
                                              uint32_t* d_status, void* stream, uint64_t* out_ticket) {
    if (!cix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    if (!out_ticket) return fail(GRANNE_HIP_ERR_INVALID, "out_ticket is null");
    if (max_search == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    granne_hip_index* ix = const_cast<granne_hip_index*>(cix);
    GRANNE_HIP_ON_DEVICE(ix->device);
    std::lock_guard<std::mutex> lk(ix->flight_mu);
    // any flight that is free, looked for from the one after the last begun (tickets may be ended in any order)
    uint32_t fi = ix->depth;
    for (uint32_t t = 0; t < ix->depth; ++t) {
        const uint32_t c = (ix->next_flight + t) % ix->depth;
        if (!ix->flights[c].busy) {
            fi = c;
            break;
        }
    }
    if (fi == ix->depth)
        return fail(GRANNE_HIP_ERR_INVALID, "%u batches are in flight already (GRANNE_HIP_OPT_SEARCH_DEPTH): end one first", ix->depth);
    auto& F = ix->flights[fi];
    if (!F.done) { // created together or not at all: a failure leaves the flight as it was
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&e0, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&e1, hipEventDisableTiming);
        if (e != hipSuccess) {
            if (e1) (void)hipEventDestroy(e1);
            if (e0) (void)hipEventDestroy(e0);
            if (st) (void)hipStreamDestroy(st);
            return fail(GRANNE_HIP_ERR_HIP, "a stream for a batch in flight: %s", hipGetErrorString(e));
        }
        F.stream = st;
        F.ready = e0;
        F.done = e1;
    }
    HIP_TRY(hipEventRecord(F.ready, (hipStream_t)stream));
    HIP_TRY(hipStreamWaitEvent(F.stream, F.ready, 0));
    int rc = search_launch(SearchTarget(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size()),
                           index_call(d_queries, nq, max_search, num_neighbors, d_out_ids, d_out_dists, d_out_counts, d_out_stats, d_status, F.stream));
    if (rc) {
        (void)hipStreamSynchronize(F.stream); // an error return leaves nothing running
        return rc;
    }
    HIP_TRY(hipEventRecord(F.done, F.stream));
    F.busy = true;
    F.seq = ix->next_seq++;
    ix->next_flight = (fi + 1) % ix->depth;
    *out_ticket = (F.seq << 8) | fi;
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_search_end_device(const granne_hip_index* cix, uint64_t ticket, void* stream) {
    if (!cix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    granne_hip_index* ix = const_cast<granne_hip_index*>(cix);
    std::lock_guard<std::mutex> lk(ix->flight_mu);
    const uint32_t fi = (uint32_t)(ticket & 0xFF);
    if (fi >= GRANNE_HIP_SEARCH_DEPTH_MAX || !ix->flights[fi].busy || ix->flights[fi].seq != (ticket >> 8))
        return fail(GRANNE_HIP_ERR_INVALID, "no batch in flight has this ticket");
    DeviceGuard g(ix->device);
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, ix->flights[fi].done, 0));
    ix->flights[fi].busy = false;
    return GRANNE_HIP_OK;
}

// Several batches of `nq` queries in ONE launch: a grid of n_batches x nq walkers, which the dispatcher refills from as
// walks finish -- the in-flight depth a host otherwise has to provide with streams of its own (a launch of 1024 walks is
// one wave per SIMD and lasts as long as its slowest walk). More than MAX_LAUNCH_BATCHES batches go out as several
// launches on the same stream.
extern "C" int granne_hip_search_batches_device(const granne_hip_index* ix, uint32_t n_batches, const void* const* d_queries,
                                                uint32_t nq, uint32_t max_search, uint32_t num_neighbors,
                                                uint64_t* const* d_out_ids, float* const* d_out_dists,
                                                uint32_t* const* d_out_counts, uint64_t* const* d_out_stats,
                                                uint32_t* d_status, void* stream) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    if (max_search == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    if (n_batches == 0 || nq == 0) return GRANNE_HIP_OK;
    if (!d_queries || !d_out_counts || (num_neighbors && (!d_out_ids || !d_out_dists)))
        return fail(GRANNE_HIP_ERR_INVALID, "null pointer array");
    const SearchTarget T(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size());
    // as many batches per launch as keep the launch's walker count within 31 bits (and the kernel argument table)
    uint32_t per = MAX_LAUNCH_BATCHES;
    while (per > 1 && (uint64_t)per * nq > 0x7FFFFFFFull) per >>= 1;
    for (uint32_t b0 = 0; b0 < n_batches; b0 += per) {
        const uint32_t nb = n_batches - b0 < per ? n_batches - b0 : per;
        BatchIO io[MAX_LAUNCH_BATCHES];
        for (uint32_t b = 0; b < nb; ++b) {
            io[b].queries = (const uint8_t*)d_queries[b0 + b];
            io[b].out_ids = num_neighbors ? d_out_ids[b0 + b] : nullptr;
            io[b].out_dists = num_neighbors ? d_out_dists[b0 + b] : nullptr;
            io[b].out_counts = d_out_counts[b0 + b];
            io[b].out_stats = d_out_stats ? d_out_stats[b0 + b] : nullptr;
        }
        SearchCall c = index_call(nullptr, nq, max_search, num_neighbors, nullptr, nullptr, nullptr, nullptr, d_status, stream);
        c.batches = io;
        c.n_batches = nb;
        int rc = search_launch(T, c);
        if (rc) return rc;
    }
    return GRANNE_HIP_OK;
}

#if GRANNE_HIP_PHASE_TIMERS
// diagnostics build only (tools/phase_probe.py): the per-walk phase clocks of the last launches
extern "C" int granne_hip_debug_phases(uint64_t* out, uint32_t nq) {
    if (!out || nq > PHASE_QUERIES) return fail(GRANNE_HIP_ERR_INVALID, "bad argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), (size_t)nq * PHASE_SLOTS * 8));
    return GRANNE_HIP_OK;
}
#endif

extern "C" int granne_hip_device_malloc(void** out_ptr, uint64_t bytes, int device_id) {
    if (!out_ptr) return fail(GRANNE_HIP_ERR_INVALID, "out_ptr is null");
    *out_ptr = nullptr;
    GRANNE_HIP_ON_DEVICE(device_id);
    DevBuf b;
    HIP_TRY(b.alloc(bytes));
    *out_ptr = b.release(); // the caller's, until granne_hip_device_free
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_device_free(void* ptr, int device_id) {
    if (!ptr) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    HIP_TRY(hipFree(ptr));
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_copy_to_device(void* d_dst, const void* src, uint64_t bytes, int device_id, void* stream) {
    if (bytes == 0) return GRANNE_HIP_OK;
    if (!d_dst || !src) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    GRANNE_HIP_ON_DEVICE(device_id);
    HIP_TRY(hipMemcpyAsync(d_dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_copy_to_host(void* dst, const void* d_src, uint64_t bytes, int device_id, void* stream) {
    if (bytes == 0) return GRANNE_HIP_OK;
    if (!dst || !d_src) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    GRANNE_HIP_ON_DEVICE(device_id);
    HIP_TRY(hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_stream_create(void** out_stream, int device_id) {
    if (!out_stream) return fail(GRANNE_HIP_ERR_INVALID, "out_stream is null");
    *out_stream = nullptr;
    GRANNE_HIP_ON_DEVICE(device_id);
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out_stream = (void*)s;
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_stream_destroy(void* stream, int device_id) {
    if (!stream) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    HIP_TRY(hipStreamDestroy((hipStream_t)stream));
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_stream_synchronize(void* stream, int device_id) {
    GRANNE_HIP_ON_DEVICE(device_id);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_event_create(void** out_event) {
    if (!out_event) return fail(GRANNE_HIP_ERR_INVALID, "out_event is null");
    hipEvent_t e = nullptr;
    HIP_TRY(hipEventCreate(&e));
    *out_event = (void*)e;
    return GRANNE_HIP_OK;
}
extern "C" void granne_hip_event_destroy(void* event) {
    if (event) (void)hipEventDestroy((hipEvent_t)event);
}
extern "C" int granne_hip_event_elapsed_ms(void* before, void* after, float* out_ms) {
    if (!before || !after || !out_ms) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    HIP_TRY(hipEventElapsedTime(out_ms, (hipEvent_t)before, (hipEvent_t)after));
    return GRANNE_HIP_OK;
}

// borrow / return a host-call context (see granne_hip_index::HostCall)
static granne_hip_index::HostCall* host_call_acquire(granne_hip_index* ix) {
    {
        std::lock_guard<std::mutex> lk(ix->call_mu);
        if (!ix->call_free.empty()) {
            auto* c = ix->call_free.back();
            ix->call_free.pop_back();
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
static void host_call_release(granne_hip_index* ix, granne_hip_index::HostCall* c) {
    std::lock_guard<std::mutex> lk(ix->call_mu);
    ix->call_free.push_back(c);
}

// where a host-pointer call's queries and results lie in its block: [queries][ids][dists][counts][stats]; the four
// outputs are contiguous so that a small batch comes back in one copy
struct HostLayout {
    size_t qb, o_ids, o_d, o_c, o_s, total;
    HostLayout(const granne_hip_index* ix, size_t nq, size_t k) {
        qb = nq * ix->dim * query_elem_size(ix->dtype);
        o_ids = (qb + 255) & ~(size_t)255;
        o_d = o_ids + nq * k * 8;
        o_c = o_d + ((nq * k * 4 + 15) & ~(size_t)15);
        o_s = o_c + ((nq * 4 + 15) & ~(size_t)15);
        total = o_s + nq * 24;
    }
};
constexpr size_t HOST_PIN_BYTES = 256u << 10; // the pinned block of a call context (a group's grows beyond it)

// A host-pointer search on its own (the arguments are checked): one launch of nq walkers on a stream of the call's.
static int search_batch_direct(granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t max_search,
                               uint32_t num_neighbors, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                               uint64_t* out_stats) {
    GRANNE_HIP_ON_DEVICE(ix->device);

    const size_t k = num_neighbors;
    const HostLayout L(ix, nq, k);
    const size_t qb = L.qb, o_ids = L.o_ids, o_d = L.o_d, o_c = L.o_c, o_s = L.o_s, total = L.total;
    const bool staged = total <= HOST_PIN_BYTES; // small calls go through the pinned buffer: two DMA copies per call

    granne_hip_index::HostCall* c = host_call_acquire(ix);
    if (!c) return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
    struct Release { // the context goes back to the pool only once its stream is idle: on an error return kernels and
        granne_hip_index* ix; // copies of this call may still be running on it, reading and writing the caller's buffers
        granne_hip_index::HostCall* c;
        ~Release() {
            (void)hipStreamSynchronize(c->stream);
            host_call_release(ix, c);
        }
    } release{ix, c};
    if (staged) HIP_TRY(c->h_pin.reserve(HOST_PIN_BYTES + 64, hipHostMallocMapped)); // (+64: the status words behind the block)
    uint8_t* const h_pin = c->h_pin.as<uint8_t>();
    hipStream_t s = c->stream;
    const SearchTarget T(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size());
    SearchCall call = index_call(nullptr, nq, max_search, num_neighbors, nullptr, nullptr, nullptr, nullptr, nullptr, s);
    uint32_t slow[2] = {0, 0};
    if (staged) {
        // Small calls (one query per call is the reference's own shape, src/index/mod.rs:140-150): no copy
        // engine at all. The pinned block is mapped into the device's address space: the walker reads the
        // queries from it and writes results and status words into it over PCIe (a few hundred bytes), the
        // scratch block is the caller context's own. What is left on the stream: one memset of the scratch
        // header, the walker, the (normally empty) exact walker, one synchronisation.
        void* dev_pin = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dev_pin, h_pin, 0));
        uint8_t* dp = (uint8_t*)dev_pin;
        uint32_t* hst = (uint32_t*)(h_pin + total);
        memcpy(h_pin, queries, qb);
        hst[0] = hst[1] = hst[2] = hst[3] = 0;
        call.queries = dp;
        call.ids = (uint64_t*)(dp + o_ids);
        call.dists = (float*)(dp + o_d);
        call.counts = (uint32_t*)(dp + o_c);
        call.stats = (uint64_t*)(dp + o_s);
        call.host_status = (uint32_t*)(dp + total);
        int r = search_launch(T, call);
        hipError_t e = hipStreamSynchronize(s);
        if (r) return r;
        if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
        slow[0] = hst[1]; // queries served by the exact global-memory walker
        slow[1] = hst[0]; // its scratch ran out
        ix->last_slow_count.store(slow[0]);
        if (slow[1]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
        memcpy(out_ids, h_pin + o_ids, (size_t)nq * k * 8);
        memcpy(out_dists, h_pin + o_d, (size_t)nq * k * 4);
        memcpy(out_counts, h_pin + o_c, (size_t)nq * 4);
        if (out_stats) memcpy(out_stats, h_pin + o_s, (size_t)nq * 24);
        return GRANNE_HIP_OK;
    }
    HIP_TRY(c->d_buf.reserve(total));
    uint8_t* buf = c->d_buf.as<uint8_t>();
    HIP_TRY(hipMemcpyAsync(buf, queries, qb, hipMemcpyHostToDevice, s));
    call.queries = buf;
    call.ids = (uint64_t*)(buf + o_ids);
    call.dists = (float*)(buf + o_d);
    call.counts = (uint32_t*)(buf + o_c);
    call.stats = (uint64_t*)(buf + o_s);
    call.slow_count = slow;
    int r = search_launch(T, call);
    if (r) {
        (void)hipStreamSynchronize(s);
        return r;
    }
    ix->last_slow_count.store(slow[0]);
    if (slow[1]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
    HIP_TRY(hipMemcpyAsync(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, buf + o_s, (size_t)nq * 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return GRANNE_HIP_OK;
}

// The combiner's launch step (combiner.h): the n requests of one key that leader `slot` collected, nq queries in all, as
// ONE launch over the slot's pinned, device-mapped block -- what search_batch_direct does for a small call, with the
// block sized for the group: the walker reads the queries from it and writes results and status words into it. Scratch
// is search_launch's, sized there for the launch's nq (the group's) and kept for the slot's stream. Any non-zero return
// sends every member to the direct path; the slot's stream is idle when this returns.
static int search_batch_group(granne_hip_index* ix, unsigned slot, const CombineRequest* const* m, size_t n, uint32_t nq) {
    GRANNE_HIP_ON_DEVICE(ix->device);
    const size_t k = m[0]->num_neighbors;
    const size_t row = (size_t)ix->dim * query_elem_size(ix->dtype);
    const HostLayout L(ix, nq, k);
    granne_hip_index::HostCall*& c = ix->group_call[slot]; // (the slot is this leader's alone until it returns)
    if (!c) {
        c = new granne_hip_index::HostCall();
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            c = nullptr;
            return fail(GRANNE_HIP_ERR_HIP, "cannot create a stream");
        }
    }
    size_t want = HOST_PIN_BYTES;
    while (want < L.total) want <<= 1;
    HIP_TRY(c->h_pin.reserve(want + 64, hipHostMallocMapped)); // (+64: the status words behind the block)
    uint8_t* const h_pin = c->h_pin.as<uint8_t>();
    void* dev_pin = nullptr;
    HIP_TRY(hipHostGetDevicePointer(&dev_pin, h_pin, 0));
    uint8_t* dp = (uint8_t*)dev_pin;
    uint32_t* hst = (uint32_t*)(h_pin + L.total);
    size_t q0 = 0;
    for (size_t i = 0; i < n; ++i) {
        memcpy(h_pin + q0 * row, m[i]->queries, m[i]->nq * row);
        q0 += m[i]->nq;
    }
    hst[0] = hst[1] = hst[2] = hst[3] = 0;
    const SearchTarget T(ix, ix->d_layers.as<LayerDev>(), (uint32_t)ix->layers.size());
    SearchCall call = index_call(dp, nq, m[0]->max_search, (uint32_t)k, (uint64_t*)(dp + L.o_ids), (float*)(dp + L.o_d),
                                 (uint32_t*)(dp + L.o_c), (uint64_t*)(dp + L.o_s), nullptr, c->stream);
    call.host_status = (uint32_t*)(dp + L.total);
    int r = search_launch(T, call);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (r) return r;
    if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    ix->last_slow_count.store(hst[1]); // (the group's count)
    if (hst[0]) return fail(GRANNE_HIP_ERR_OVERFLOW, "exact-search scratch exhausted (raise GRANNE_HIP_OPT_SLOW_SLOTS)");
    q0 = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t mq = m[i]->nq;
        memcpy(m[i]->ids, h_pin + L.o_ids + q0 * k * 8, mq * k * 8);
        memcpy(m[i]->dists, h_pin + L.o_d + q0 * k * 4, mq * k * 4);
        memcpy(m[i]->counts, h_pin + L.o_c + q0 * 4, mq * 4);
        if (m[i]->stats) memcpy(m[i]->stats, h_pin + L.o_s + q0 * 24, mq * 24);
        q0 += mq;
    }
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_search_batch(const granne_hip_index* cix, const void* queries, uint32_t nq, uint32_t max_search,
                                       uint32_t num_neighbors, uint64_t* out_ids, float* out_dists, uint32_t* out_counts,
                                       uint64_t* out_stats) {
    if (!cix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    granne_hip_index* ix = const_cast<granne_hip_index*>(cix);
    if (max_search == 0) return fail(GRANNE_HIP_ERR_INVALID, "max_search must be > 0 (the reference panics, src/index/mod.rs:1019)");
    if (nq == 0) return GRANNE_HIP_OK;
    if (num_neighbors == 0) { // .take(0), src/index/mod.rs:974-977
        if (!out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
        memset(out_counts, 0, (size_t)nq * 4);
        return GRANNE_HIP_OK;
    }
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    // GRANNE_HIP_OPT_COALESCE: a small call shares a launch with the calls of its key that are in here at the same moment
    if (ix->opt_coalesce && ix->combiner.takes(nq)) {
        CombineRequest req;
        req.queries = queries;
        req.nq = nq;
        req.ids = out_ids;
        req.dists = out_dists;
        req.counts = out_counts;
        req.stats = out_stats;
        req.max_search = max_search;
        req.num_neighbors = num_neighbors;
        return ix->combiner.submit(
            req,
            [ix](unsigned slot, const CombineRequest* const* m, size_t n, uint32_t group_nq) {
                return search_batch_group(ix, slot, m, n, group_nq);
            },
            [ix](const CombineRequest& r) {
                return search_batch_direct(ix, r.queries, r.nq, r.max_search, r.num_neighbors, r.ids, r.dists, r.counts, r.stats);
            });
    }
    return search_batch_direct(ix, queries, nq, max_search, num_neighbors, out_ids, out_dists, out_counts, out_stats);
}

extern "C" int granne_hip_search(const granne_hip_index* ix, const void* query, uint32_t max_search,
                                 uint32_t num_neighbors, uint64_t* out_ids, float* out_dists, uint32_t* out_count) {
    if (!out_count) return fail(GRANNE_HIP_ERR_INVALID, "out_count is null");
    return granne_hip_search_batch(ix, query, 1, max_search, num_neighbors, out_ids, out_dists, out_count, nullptr);
}

// ------------------------------------------------------------------------------------------------
// element preparation / Dist operator / synthetic data
// ------------------------------------------------------------------------------------------------
extern "C" int granne_hip_normalize_f32_device(float* d_rows, uint64_t n, uint32_t dim, int device_id, void* stream) {
    if (!d_rows && n) return fail(GRANNE_HIP_ERR_INVALID, "rows is null");
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    uint32_t lstride = dim | 1u;
    uint32_t rpb = (60u * 1024u) / (lstride * 4u);
    if (rpb > 256) rpb = 256;
    if (rpb < 1) return fail(GRANNE_HIP_ERR_INVALID, "dim too large");
    uint64_t blocks = (n + rpb - 1) / rpb;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(normalize_rows_kernel, dim3((uint32_t)blocks), dim3(256), rpb * lstride * 4, (hipStream_t)stream,
                       d_rows, n, dim, rpb, lstride);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_quantize_f32_device(const float* d_rows, int8_t* d_out, uint64_t n, uint32_t dim,
                                              int device_id, void* stream) {
    if ((!d_rows || !d_out) && n) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    hipLaunchKernelGGL(quantize_rows_kernel, dim3(grid_for(n * 64, 256)), dim3(256), 0, (hipStream_t)stream, d_rows,
                       d_out, n, dim);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// f32 rows -> halves (round to nearest even) and back (exact; optionally normalised as angular::Vector::from does):
// the conversions of angular_f16 elements (f16.h). Dense rows on both sides.
extern "C" int granne_hip_f32_to_f16_device(const float* d_rows, uint16_t* d_out, uint64_t n, uint32_t dim, int device_id,
                                            void* stream) {
    if ((!d_rows || !d_out) && n) return fail(GRANNE_HIP_ERR_INVALID, "f32_to_f16: null buffer");
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    hipLaunchKernelGGL(f32_to_f16_kernel, dim3(grid_for(n * dim, 256)), dim3(256), 0, (hipStream_t)stream, d_rows, d_out, n * dim);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// rows of halves `in_stride` bytes apart -> dense f32 rows (checked arguments, the device selected)
static int f16_rows_to_f32(const uint8_t* d_rows16, uint64_t in_stride, float* d_out, uint64_t n, uint32_t dim, int normalised,
                           hipStream_t s) {
    if (n == 0) return GRANNE_HIP_OK;
    const uint32_t lstride = dim | 1u;
    uint32_t rpb = (60u * 1024u) / (lstride * 4u);
    if (rpb > 256) rpb = 256;
    if (rpb < 1) return fail(GRANNE_HIP_ERR_INVALID, "f16_to_f32: dim too large");
    uint64_t blocks = (n + rpb - 1) / rpb;
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(f16_to_f32_kernel, dim3((uint32_t)blocks), dim3(256), rpb * lstride * 4, s, d_rows16, in_stride, d_out, n, dim,
                       normalised, rpb, lstride);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_f16_to_f32_device(const uint16_t* d_rows16, float* d_out, uint64_t n, uint32_t dim, int normalised,
                                            int device_id, void* stream) {
    if ((!d_rows16 || !d_out) && n) return fail(GRANNE_HIP_ERR_INVALID, "f16_to_f32: null buffer");
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    GRANNE_HIP_ON_DEVICE(device_id);
    return f16_rows_to_f32((const uint8_t*)d_rows16, (uint64_t)dim * 2u, d_out, n, dim, normalised, (hipStream_t)stream);
}

// host conveniences: copy in, convert, copy out
static int f16_convert_host(const void* in, size_t in_bytes, void* out, size_t out_bytes, uint64_t n, uint32_t dim, int to_half,
                            int normalised, int device_id) {
    if ((!in || !out) && n) return fail(GRANNE_HIP_ERR_INVALID, "f16 conversion: null buffer");
    if (dim == 0) return fail(GRANNE_HIP_ERR_INVALID, "dim must be > 0");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    DevBuf di, dout;
    HIP_TRY(di.alloc(in_bytes));
    HIP_TRY(dout.alloc(out_bytes));
    HIP_TRY(hipMemcpy(di.get(), in, in_bytes, hipMemcpyHostToDevice));
    const int rc = to_half ? granne_hip_f32_to_f16_device(di.as<float>(), dout.as<uint16_t>(), n, dim, device_id, nullptr)
                           : granne_hip_f16_to_f32_device(di.as<uint16_t>(), dout.as<float>(), n, dim, normalised, device_id, nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, dout.get(), out_bytes, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}
extern "C" int granne_hip_f32_to_f16(const float* rows, uint16_t* out, uint64_t n, uint32_t dim, int device_id) {
    return f16_convert_host(rows, (size_t)n * dim * 4, out, (size_t)n * dim * 2, n, dim, 1, 0, device_id);
}
extern "C" int granne_hip_f16_to_f32(const uint16_t* rows16, float* out, uint64_t n, uint32_t dim, int normalised, int device_id) {
    return f16_convert_host(rows16, (size_t)n * dim * 2, out, (size_t)n * dim * 4, n, dim, 0, normalised, device_id);
}

static int dists_launch(const granne_hip_index* ix, const void* d_queries, const uint32_t* d_qidx, uint32_t m,
                        const uint32_t* d_ids, uint64_t n_pairs, float* d_out, uint32_t* d_status, void* stream) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "dists");
    if (n_pairs == 0) return GRANNE_HIP_OK;
    if (!d_queries || !d_ids || !d_out) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    GRANNE_HIP_ON_DEVICE(ix->device);
    uint32_t* st = d_status; // optional: count of out-of-range ids
    // eight lanes per pair, 32 pairs per 256-thread block; enough blocks to cover the chip many times
    uint64_t blocks = (n_pairs + 31) / 32;
    if (blocks > 256u * 64u) blocks = 256u * 64u;
    if (ix->dtype == GRANNE_HIP_F16)
        hipLaunchKernelGGL(dists_kernel<DT_F16>, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, ix->d_elements.as<uint8_t>(),
                           ix->n_elements, ix->row_bytes, ix->row_stride, ix->dim, (const uint8_t*)d_queries, d_qidx, m, d_ids, n_pairs,
                           d_out, st);
    else if (ix->dtype == GRANNE_HIP_F32)
        hipLaunchKernelGGL(dists_kernel<0>, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, ix->d_elements.as<uint8_t>(),
                           ix->n_elements, ix->row_bytes, ix->row_stride, ix->dim, (const uint8_t*)d_queries, d_qidx, m, d_ids, n_pairs,
                           d_out, st);
    else
        hipLaunchKernelGGL(dists_kernel<1>, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)stream, ix->d_elements.as<uint8_t>(),
                           ix->n_elements, ix->row_bytes, ix->row_stride, ix->dim, (const uint8_t*)d_queries, d_qidx, m, d_ids, n_pairs,
                           d_out, st);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_dist_pairs_device(const granne_hip_index* ix, const void* d_queries, const uint32_t* d_qidx,
                                            const uint32_t* d_ids, uint64_t n_pairs, float* d_out, void* stream) {
    if (n_pairs && !d_qidx) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    return dists_launch(ix, d_queries, d_qidx, 1, d_ids, n_pairs, d_out, nullptr, stream);
}

extern "C" int granne_hip_dists_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq,
                                       const uint32_t* d_ids, uint32_t m, float* d_out, uint32_t* d_status,
                                       void* stream) {
    if (nq && m == 0) return GRANNE_HIP_OK;
    return dists_launch(ix, d_queries, nullptr, m ? m : 1, d_ids, (uint64_t)nq * m, d_out, d_status, stream);
}

static int merge_launch(const uint8_t* ids, const uint8_t* dists, const uint8_t* counts, uint64_t ids_stride,
                        uint64_t dists_stride, uint64_t counts_stride, const uint64_t* shard_offsets, uint32_t n_shards,
                        uint32_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                        int device_id, void* stream);

// which scan kernel serves an index's rows (brute_force.h), and how it is launched
struct ScanPlan {
    uint64_t form; // GRANNE_HIP_SCAN_*: what GRANNE_HIP_OPT_LAST_SCAN reports
    void (*fn)(const BruteParams);
    void (*prime)(const BruteParams); // the same scan keeping only the best score per (range, query)
    BfGeometry geo, prime_geo;
    uint64_t max_ranges = 64; // element ranges: their lists are merged (a range is a whole number of tiles)
};
static ScanPlan plan_scan(const granne_hip_index* ix, uint32_t nq) {
    if (ix->dtype == GRANNE_HIP_I8) {
        if (ix->row_bytes > 128u) // rows of any length: in chunks of 128 bytes (brute_force.h, bf_i8_chunked_kernel)
            return {GRANNE_HIP_SCAN_I8_CHUNKED, bf_i8_chunked_kernel<4>, bf_i8_chunked_kernel<4, true>, bf_i8_chunked_geometry<4>(), bf_i8_chunked_geometry<4>()};
        if (knobs().bf_ring && ix->row_bytes == 128u && ix->row_stride == 128u && ix->n_elements < (1ull << 29)) {
            // tiles by LDS-DMA into a ring, 64 queries per wave (brute_force.h, bf_i8_ring_kernel); the priming pass stays
            ScanPlan P{GRANNE_HIP_SCAN_RING, bf_i8_ring_kernel, bf_i8_kernel<4, true>, bf_ring_geometry(), bf_i8_geometry<4>()};
            // 512 queries per block: half as many blocks per range, so twice the ranges fill the chip (merged in two steps)
            if ((uint64_t)((nq + P.geo.qt - 1) / P.geo.qt) * 64u < 256u) P.max_ranges = 128;
            return P;
        }
        return {GRANNE_HIP_SCAN_I8, bf_i8_kernel<4>, bf_i8_kernel<4, true>, bf_i8_geometry<4>(), bf_i8_geometry<4>()};
    }
    // f32 rows on the bf16 matrix path, three instructions per product (brute_force.h)
    if (knobs().bf_b16 && ix->dim <= 112) return {GRANNE_HIP_SCAN_B16_7_4, bf_b16_kernel<7, 4>, bf_b16_kernel<7, 4, true>, bf_b16_geometry<7, 4>(), bf_b16_geometry<7, 4>()};
    if (knobs().bf_b16 && ix->dim <= 208) return {GRANNE_HIP_SCAN_B16_13_2, bf_b16_kernel<13, 2>, bf_b16_kernel<13, 2, true>, bf_b16_geometry<13, 2>(), bf_b16_geometry<13, 2>()};
    // rows of any length: the vector in chunks of 128 components (brute_force.h, bf_b16_chunked_kernel; tiles of 64 rows:
    // 128 take 256 registers and spill)
    if (ix->dim > 256) return {GRANNE_HIP_SCAN_B16_CHUNKED, bf_b16_chunked_kernel<2>, bf_b16_chunked_kernel<2, true>, bf_b16_chunked_geometry<2>(), bf_b16_chunked_geometry<2>()};
    if (knobs().bf_b16) return {GRANNE_HIP_SCAN_B16_16_1, bf_b16_kernel<16, 1>, bf_b16_kernel<16, 1, true>, bf_b16_geometry<16, 1>(), bf_b16_geometry<16, 1>()};
    if (ix->dim <= 104) return {GRANNE_HIP_SCAN_F32_52_4, bf_f32_kernel<52, 4>, bf_f32_kernel<52, 4, true>, bf_f32_geometry<52, 4>(), bf_f32_geometry<52, 4>()};
    if (ix->dim <= 200) return {GRANNE_HIP_SCAN_F32_100_2, bf_f32_kernel<100, 2>, bf_f32_kernel<100, 2, true>, bf_f32_geometry<100, 2>(), bf_f32_geometry<100, 2>()};
    return {GRANNE_HIP_SCAN_F32_128_1, bf_f32_kernel<128, 1>, bf_f32_kernel<128, 1, true>, bf_f32_geometry<128, 1>(), bf_f32_geometry<128, 1>()};
}

// the scan's scratch: the ranges' lists, the merged lists, the candidates and their exact distances, the thresholds, what
// the ranges of a query have seen per score bucket, and the zero-padded queries (int8 rows of more than 128 bytes)
namespace {
struct ScanScratch {
    size_t pid, pd, pc, mid, md, mc, cand, ex, tau, share, qpad, total = 0;
    ScanScratch(uint64_t ranges, uint32_t nq, uint32_t kk, size_t share_bytes, size_t qpad_bytes) {
        auto take = [&](size_t bytes, size_t align) {
            total = (total + align - 1) & ~(align - 1);
            total += bytes;
            return total - bytes;
        };
        const size_t lists = (size_t)ranges * nq;
        pid = take(lists * kk * 8, 1), pd = take(lists * kk * 4, 1), pc = take(lists * 4, 1);
        mid = take((size_t)nq * kk * 8, 16), md = take((size_t)nq * kk * 4, 1), mc = take((size_t)nq * 4, 1);
        cand = take((size_t)nq * kk * 4, 16), ex = take((size_t)nq * kk * 4, 1);
        tau = take((size_t)nq * 4, 16);
        share = take(share_bytes, 16);
        qpad = take(qpad_bytes, 16);
    }
};
} // namespace

// The lists of G ranges ([G][nq][kk] ids, dists; [G][nq] counts) merged into one per query. More lists than the merge has
// lanes (G > 64): ranges 0..63 and 64.. are merged into two lists of their own, then those two.
static int merge_ranges(const BruteParams& P, uint32_t G, uint32_t nq, uint32_t kk, uint64_t* ids, float* dists, uint32_t* counts,
                        int device, void* stream) {
    const uint8_t* pi = (const uint8_t*)P.part_ids;
    const uint8_t* pd = (const uint8_t*)P.part_d;
    const uint8_t* pc = (const uint8_t*)P.part_c;
    const uint64_t si = (uint64_t)nq * kk * 8, sd = (uint64_t)nq * kk * 4, sc = (uint64_t)nq * 4;
    uint64_t zeros[64];
    memset(zeros, 0, sizeof(zeros)); // the lists hold global ids already
    if (G <= 64) return merge_launch(pi, pd, pc, si, sd, sc, zeros, G, nq, kk, ids, dists, counts, device, stream);
    hipStream_t s = (hipStream_t)stream;
    uint8_t* half = nullptr; // [2] x (ids, dists, counts)
    const size_t hi = 0, hd = 2 * si, hc = hd + 2 * sd, hbytes = hc + 2 * sc;
    HIP_TRY(hipMallocAsync((void**)&half, hbytes, s));
    int rc = 0;
    for (uint32_t part = 0; part < 2 && rc == 0; ++part) {
        const uint32_t first = part * 64u, count = part == 0 ? 64u : G - 64u;
        rc = merge_launch(pi + first * si, pd + first * sd, pc + first * sc, si, sd, sc, zeros, count, nq, kk,
                          (uint64_t*)(half + hi + part * si), (float*)(half + hd + part * sd), (uint32_t*)(half + hc + part * sc),
                          device, stream);
    }
    if (rc == 0) rc = merge_launch(half + hi, half + hd, half + hc, si, sd, sc, zeros, 2, nq, kk, ids, dists, counts, device, stream);
    (void)hipFreeAsync(half, s);
    return rc;
}

// exact k nearest elements by a scan of all of them on the matrix cores (brute_force.h)
extern "C" int granne_hip_brute_force_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq, uint32_t k,
                                             uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts, void* stream) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "brute_force");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "brute_force");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!d_queries || !d_out_ids || !d_out_dists || !d_out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (k == 0 || k > BF_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "k must be in [1, %u]", BF_KMAX);
    GRANNE_HIP_ON_DEVICE(ix->device);
    hipStream_t s = (hipStream_t)stream;
    const uint64_t n = ix->n_elements;
    const uint32_t kk = k + BF_EXTRA < BF_KMAX ? k + BF_EXTRA : BF_KMAX;
    const ScanPlan S = plan_scan(ix, nq);
    const uint64_t tile = S.geo.rows;
    uint64_t G = (n + tile - 1) / tile;
    if (G > S.max_ranges) G = S.max_ranges;
    if (G < 1) G = 1;
    uint64_t per_range = (n + G - 1) / G;
    per_range = (per_range + tile - 1) / tile * tile;
    if (per_range < tile) per_range = tile;
    // The priming pass (brute_force.h, bf_tau_kernel) scans the first range alone, cut into up to 64 sub-ranges so that the
    // whole chip scans it (1/64 of the scan proper, without its lists: the best score per sub-range and query). It runs
    // when there are at least 32 ranges and its sub-ranges hold kk maxima; GRANNE_HIP_OPT_LAST_SCAN says what this call runs
    const uint64_t prime_n = per_range < n ? per_range : n;
    uint64_t prime_per = 0, Gs = 0; // (Gs stays 0 with fewer than 32 ranges)
    if (G >= 32) {
        Gs = (prime_n + tile - 1) / tile;
        if (Gs > 64) Gs = 64;
        prime_per = ((prime_n + Gs - 1) / Gs + tile - 1) / tile * tile;
        Gs = (prime_n + prime_per - 1) / prime_per;
    }
    const bool primed = G >= 32 && Gs >= kk;
    const_cast<granne_hip_index*>(ix)->last_scan.store(S.form | G << 8 | (uint64_t)(primed ? 1 : 0) << 24 | Gs << 32 | (uint64_t)kk << 40);
    const size_t share_bytes = (size_t)nq * BF_SHARE_BUCKETS * 4;
    const size_t qpad_bytes = (ix->dtype == GRANNE_HIP_I8 && ix->row_bytes > 128u) ? (size_t)nq * ix->row_bytes : 0;
    const ScanScratch o(G, nq, kk, share_bytes, qpad_bytes);
    uint8_t* scratch = nullptr;
    HIP_TRY(hipMallocAsync((void**)&scratch, o.total, s));
    struct Release {
        void* p;
        hipStream_t s;
        ~Release() { (void)hipFreeAsync(p, s); }
    } release{scratch, s};
    BruteParams P;
    P.inv_norm = nullptr;
    P.inv_gmax = nullptr;
    const uint64_t n_pad = (n + 31u) & ~31ull; // inv_norm [n_pad], then inv_gmax [n_pad / 32][2]
    if (ix->dtype == GRANNE_HIP_I8) {
        granne_hip_index* mix = const_cast<granne_hip_index*>(ix);
        std::lock_guard<std::mutex> lk(mix->norm_mu);
        if (!mix->d_inv_norm) { // (made with the index, make_scan_norms: this is the path of an index that has no layers yet)
            DevBuf norms;
            HIP_TRY(norms.alloc((size_t)inv_norm_bytes(n)));
            float* dn = norms.as<float>();
            hipLaunchKernelGGL(inv_norm_rows_kernel, dim3(grid_for(n * 8, 256)), dim3(256), 0, s, ix->d_elements.as<uint8_t>(), n, ix->row_stride, dn);
            hipLaunchKernelGGL(inv_gmax_kernel, dim3(grid_for(n_pad / 16 + 1, 256)), dim3(256), 0, s, (const float*)dn, n, dn + n_pad);
            if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return fail(GRANNE_HIP_ERR_HIP, "inv_norm_rows_kernel failed");
            mix->d_inv_norm = std::move(norms);
            mix->hbm_bytes += inv_norm_bytes(n);
        }
        P.inv_norm = mix->d_inv_norm.as<float>();
        P.inv_gmax = P.inv_norm + n_pad;
    }
    P.elements = ix->d_elements.as<uint8_t>();
    P.n = n;
    P.row_bytes = ix->row_bytes;
    P.row_stride = ix->row_stride;
    P.dim = ix->dim;
    P.queries = (const uint8_t*)d_queries;
    P.nq = nq;
    P.kk = kk;
    P.per_range = per_range;
    P.part_ids = (uint64_t*)(scratch + o.pid);
    P.part_d = (float*)(scratch + o.pd);
    P.part_c = (uint32_t*)(scratch + o.pc);
    if (S.geo.lds > 64u * 1024u) HIP_TRY(hipFuncSetAttribute((const void*)S.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)S.geo.lds));
    P.tau_in = nullptr;
    P.share_hist = nullptr;
    P.qpad = nullptr;
    if (qpad_bytes) {
        hipLaunchKernelGGL(bf_pad_queries_kernel, dim3(grid_for(qpad_bytes, 256)), dim3(256), 0, s, (const uint8_t*)d_queries, nq, ix->dim,
                           ix->row_bytes, scratch + o.qpad);
        HIP_TRY(hipGetLastError());
        P.qpad = scratch + o.qpad;
    }
    if (primed) {
        BruteParams Q = P;
        Q.n = prime_n;
        Q.per_range = prime_per;
        const BfGeometry& pg = S.prime_geo;
        if (pg.lds > 64u * 1024u) HIP_TRY(hipFuncSetAttribute((const void*)S.prime, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pg.lds));
        hipLaunchKernelGGL(S.prime, dim3((nq + pg.qt - 1) / pg.qt, (uint32_t)Gs), dim3(pg.threads), pg.lds, s, Q);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bf_tau_kernel, dim3(nq), dim3(64), 0, s, (const float*)P.part_d, (uint32_t)Gs, nq, kk, (float*)(scratch + o.tau));
        HIP_TRY(hipGetLastError());
        P.tau_in = (const float*)(scratch + o.tau);
        // the ranges of a query tell each other what they have seen (brute_force.h, BfShare)
        HIP_TRY(hipMemsetAsync(scratch + o.share, 0, share_bytes, s));
        P.share_hist = (uint32_t*)(scratch + o.share);
    }
    hipLaunchKernelGGL(S.fn, dim3((nq + S.geo.qt - 1) / S.geo.qt, (uint32_t)G), dim3(S.geo.threads), S.geo.lds, s, P);
    HIP_TRY(hipGetLastError());
    int rc = merge_ranges(P, (uint32_t)G, nq, kk, (uint64_t*)(scratch + o.mid), (float*)(scratch + o.md), (uint32_t*)(scratch + o.mc),
                          ix->device, stream);
    if (rc) return rc;
    // the candidates' distances in the reference's own arithmetic, then the k best by (distance, id)
    const uint32_t pairs = nq * kk;
    hipLaunchKernelGGL(bf_narrow_ids_kernel, dim3((pairs + 255) / 256), dim3(256), 0, s, (const uint64_t*)(scratch + o.mid),
                       (const uint32_t*)(scratch + o.mc), nq, kk, (uint32_t*)(scratch + o.cand));
    HIP_TRY(hipGetLastError());
    rc = dists_launch(ix, d_queries, nullptr, kk, (const uint32_t*)(scratch + o.cand), (uint64_t)pairs, (float*)(scratch + o.ex),
                      nullptr, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(bf_final_kernel, dim3((pairs + 255) / 256), dim3(256), 0, s, (const uint32_t*)(scratch + o.cand),
                       (const float*)(scratch + o.ex), nq, kk, k, d_out_ids, d_out_dists, d_out_counts);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// host convenience over the scan: host buffers in and out
extern "C" int granne_hip_brute_force(const granne_hip_index* ix, const void* queries, uint32_t nq, uint32_t k,
                                      uint64_t* out_ids, float* out_dists, uint32_t* out_counts) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "brute_force");
    GRANNE_HIP_F16_UNSUPPORTED(ix->dtype, "brute_force");
    if (nq == 0) return GRANNE_HIP_OK;
    if (!queries || !out_ids || !out_dists || !out_counts) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (k == 0 || k > BF_KMAX) return fail(GRANNE_HIP_ERR_INVALID, "k must be in [1, %u]", BF_KMAX);
    GRANNE_HIP_ON_DEVICE(ix->device);
    const size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    const size_t o_ids = (qb + 255) & ~(size_t)255, o_d = o_ids + (size_t)nq * k * 8, o_c = o_d + (((size_t)nq * k * 4 + 15) & ~(size_t)15);
    const size_t total = o_c + (size_t)nq * 4;
    DevBuf block;
    HIP_TRY(block.alloc(total));
    struct Settle { // (declared after the block: whatever the scan left running is over before the block is freed)
        ~Settle() { (void)hipDeviceSynchronize(); }
    } settle;
    uint8_t* const buf = block.as<uint8_t>();
    HIP_TRY(hipMemcpy(buf, queries, qb, hipMemcpyHostToDevice));
    const int rc = granne_hip_brute_force_device(ix, buf, nq, k, (uint64_t*)(buf + o_ids), (float*)(buf + o_d), (uint32_t*)(buf + o_c), nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out_ids, buf + o_ids, (size_t)nq * k * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_dists, buf + o_d, (size_t)nq * k * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counts, buf + o_c, (size_t)nq * 4, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_synth_rows_device(float* d_out, uint64_t seed, uint64_t row0, uint64_t n, uint32_t dim,
                                            int device_id, void* stream) {
    if (!d_out && n) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    hipLaunchKernelGGL(synth_rows_kernel, dim3(grid_for(n * dim, 256)), dim3(256), 0, (hipStream_t)stream, d_out, seed,
                       row0, n, dim);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

// the per-shard top-k of a batch in ONE buffer: [nq*k u64 ids][nq*k f32 dists][nq u32 counts], padded to
// 16 bytes -- what one rank contributes to the all-gather of the partitioned mode
static inline size_t packed_dists_off(uint32_t nq, uint32_t k) { return (size_t)nq * k * 8; }
static inline size_t packed_counts_off(uint32_t nq, uint32_t k) { return (size_t)nq * k * 12; }
extern "C" uint64_t granne_hip_packed_topk_bytes(uint32_t nq, uint32_t k) {
    return ((uint64_t)nq * k * 12 + (uint64_t)nq * 4 + 15) & ~(uint64_t)15;
}

static int merge_launch(const uint8_t* ids, const uint8_t* dists, const uint8_t* counts, uint64_t ids_stride,
                        uint64_t dists_stride, uint64_t counts_stride, const uint64_t* shard_offsets, uint32_t n_shards,
                        uint32_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                        int device_id, void* stream) {
    if (nq == 0) return GRANNE_HIP_OK;
    if (!ids || !dists || !counts || !shard_offsets || !d_out_ids || !d_out_dists || !d_out_counts)
        return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (n_shards == 0 || n_shards > 64) return fail(GRANNE_HIP_ERR_INVALID, "n_shards must be in [1, 64]");
    if (k == 0 || (uint64_t)n_shards * k > 4096) return fail(GRANNE_HIP_ERR_INVALID, "n_shards * k must be in [1, 4096]");
    GRANNE_HIP_ON_DEVICE(device_id);
    MergeParams P;
    P.ids = ids;
    P.dists = dists;
    P.counts = counts;
    P.ids_stride = ids_stride;
    P.dists_stride = dists_stride;
    P.counts_stride = counts_stride;
    for (uint32_t s = 0; s < 64; ++s) P.offsets[s] = s < n_shards ? shard_offsets[s] : 0;
    P.n_shards = n_shards;
    P.nq = nq;
    P.k = k;
    P.out_ids = d_out_ids;
    P.out_dists = d_out_dists;
    P.out_counts = d_out_counts;
    uint32_t C = n_shards * k;
    uint32_t lds = ((C * 4 + 7) & ~7u) + C * 8;
    hipLaunchKernelGGL(merge_topk_kernel, dim3(nq), dim3(64), lds, (hipStream_t)stream, P);
    HIP_TRY(hipGetLastError());
    return GRANNE_HIP_OK;
}

extern "C" int granne_hip_merge_topk_device(const uint64_t* d_ids, const float* d_dists, const uint32_t* d_counts,
                                            const uint64_t* shard_offsets, uint32_t n_shards, uint32_t nq, uint32_t k,
                                            uint64_t* d_out_ids, float* d_out_dists, uint32_t* d_out_counts,
                                            int device_id, void* stream) {
    return merge_launch((const uint8_t*)d_ids, (const uint8_t*)d_dists, (const uint8_t*)d_counts, (uint64_t)nq * k * 8,
                        (uint64_t)nq * k * 4, (uint64_t)nq * 4, shard_offsets, n_shards, nq, k, d_out_ids, d_out_dists,
                        d_out_counts, device_id, stream);
}

extern "C" int granne_hip_merge_topk_packed_device(const void* d_packed, const uint64_t* shard_offsets, uint32_t n_shards,
                                                   uint32_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_dists,
                                                   uint32_t* d_out_counts, int device_id, void* stream) {
    const uint8_t* base = (const uint8_t*)d_packed;
    const uint64_t stride = granne_hip_packed_topk_bytes(nq, k);
    if (!base && nq) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    return merge_launch(base, base + packed_dists_off(nq, k), base + packed_counts_off(nq, k), stride, stride, stride,
                        shard_offsets, n_shards, nq, k, d_out_ids, d_out_dists, d_out_counts, device_id, stream);
}

extern "C" int granne_hip_merge_topk_packed_strided_device(const void* d_packed, uint64_t stride_bytes,
                                                           const uint64_t* shard_offsets, uint32_t n_shards, uint32_t nq,
                                                           uint32_t k, uint64_t* d_out_ids, float* d_out_dists,
                                                           uint32_t* d_out_counts, int device_id, void* stream) {
    const uint8_t* base = (const uint8_t*)d_packed;
    if (!base && nq) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (stride_bytes < granne_hip_packed_topk_bytes(nq, k) || (stride_bytes & 3))
        return fail(GRANNE_HIP_ERR_INVALID, "stride must be a multiple of 4 and at least granne_hip_packed_topk_bytes");
    return merge_launch(base, base + packed_dists_off(nq, k), base + packed_counts_off(nq, k), stride_bytes, stride_bytes,
                        stride_bytes, shard_offsets, n_shards, nq, k, d_out_ids, d_out_dists, d_out_counts, device_id, stream);
}

extern "C" int granne_hip_search_batch_packed_device(const granne_hip_index* ix, const void* d_queries, uint32_t nq,
                                                     uint32_t max_search, uint32_t num_neighbors, void* d_packed,
                                                     uint32_t* d_status, void* stream) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    if (!d_packed && nq) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (num_neighbors == 0) return fail(GRANNE_HIP_ERR_INVALID, "num_neighbors must be > 0 for a packed result");
    uint8_t* base = (uint8_t*)d_packed;
    return granne_hip_search_batch_device(ix, d_queries, nq, max_search, num_neighbors, (uint64_t*)base,
                                          (float*)(base + packed_dists_off(nq, num_neighbors)),
                                          (uint32_t*)(base + packed_counts_off(nq, num_neighbors)), nullptr, d_status, stream);
}

// host conveniences -------------------------------------------------------------------------------
extern "C" int granne_hip_normalize_f32(float* rows, uint64_t n, uint32_t dim, int device_id) {
    if (!rows && n) return fail(GRANNE_HIP_ERR_INVALID, "rows is null");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    DevBuf d;
    size_t bytes = (size_t)n * dim * 4;
    HIP_TRY(d.alloc(bytes));
    int rc = GRANNE_HIP_OK;
    hipError_t e = hipMemcpy(d.get(), rows, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = granne_hip_normalize_f32_device(d.as<float>(), n, dim, device_id, nullptr);
    if (e == hipSuccess && rc == 0) e = hipMemcpy(rows, d.get(), bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "normalize: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int granne_hip_quantize_f32(const float* rows, int8_t* out, uint64_t n, uint32_t dim, int device_id) {
    if ((!rows || !out) && n) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (n == 0) return GRANNE_HIP_OK;
    GRANNE_HIP_ON_DEVICE(device_id);
    DevBuf d, o;
    size_t bytes = (size_t)n * dim * 4;
    HIP_TRY(d.alloc(bytes));
    hipError_t e = o.alloc((size_t)n * dim);
    int rc = GRANNE_HIP_OK;
    if (e == hipSuccess) e = hipMemcpy(d.get(), rows, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) rc = granne_hip_quantize_f32_device(d.as<float>(), o.as<int8_t>(), n, dim, device_id, nullptr);
    if (e == hipSuccess && rc == 0) e = hipMemcpy(out, o.get(), (size_t)n * dim, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GRANNE_HIP_ERR_HIP, "quantize: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int granne_hip_dist_pairs(const granne_hip_index* ix, const void* queries, uint32_t nq, const uint32_t* qidx,
                                     const uint32_t* ids, uint64_t n_pairs, float* out) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "dist_pairs");
    if (n_pairs == 0) return GRANNE_HIP_OK;
    if (!queries || !qidx || !ids || !out) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    for (uint64_t i = 0; i < n_pairs; ++i) {
        if (qidx[i] >= nq) return fail(GRANNE_HIP_ERR_INVALID, "query index out of range");
        if (ids[i] >= ix->n_elements) return fail(GRANNE_HIP_ERR_INVALID, "element id out of range");
    }
    GRANNE_HIP_ON_DEVICE(ix->device);
    size_t qb = (size_t)nq * ix->dim * query_elem_size(ix->dtype);
    DevBuf dq, dqi, did, dout;
    HIP_TRY(dq.alloc(qb));
    HIP_TRY(dqi.alloc(n_pairs * 4));
    HIP_TRY(did.alloc(n_pairs * 4));
    HIP_TRY(dout.alloc(n_pairs * 4));
    HIP_TRY(hipMemcpy(dq.get(), queries, qb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dqi.get(), qidx, n_pairs * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(did.get(), ids, n_pairs * 4, hipMemcpyHostToDevice));
    int rc = granne_hip_dist_pairs_device(ix, dq.get(), dqi.as<uint32_t>(), did.as<uint32_t>(), n_pairs, dout.as<float>(), nullptr);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, dout.get(), n_pairs * 4, hipMemcpyDeviceToHost));
    return GRANNE_HIP_OK;
}

// ------------------------------------------------------------------------------------------------
// GranneBuilder on the GPU
// ------------------------------------------------------------------------------------------------
#include "builder_host.h"

// ------------------------------------------------------------------------------------------------
// Granne::reorder on the GPU
// ------------------------------------------------------------------------------------------------
#include "reorder_host.h"

// ------------------------------------------------------------------------------------------------
// granne's file formats
// ------------------------------------------------------------------------------------------------
#include "fileformat_host.h"

// ------------------------------------------------------------------------------------------------
// the same files through the device codec, streamed in bounded memory
// ------------------------------------------------------------------------------------------------
#include "codec_host.h"

// ------------------------------------------------------------------------------------------------
// partitioned indexes driven by one host process
// ------------------------------------------------------------------------------------------------
#include "sharded_host.h"

// ------------------------------------------------------------------------------------------------
// embeddings::SumEmbeddings: the container, its files, materialised and compact indexes
// ------------------------------------------------------------------------------------------------
#include "sum_embeddings_host.h"

// ------------------------------------------------------------------------------------------------
// RwGranneBuilder on the GPU: insert into and search a live graph
// ------------------------------------------------------------------------------------------------
#include "rw_builder_host.h"

// ------------------------------------------------------------------------------------------------
// refined search: walk one index, re-rank by another's rows
// ------------------------------------------------------------------------------------------------
#include "refine_host.h"

// ------------------------------------------------------------------------------------------------
// refined search over a SumEmbeddings container: re-rank by term sums; the container as prepared rows
// ------------------------------------------------------------------------------------------------
#include "refine_se_host.h"

// ------------------------------------------------------------------------------------------------
// filtered search: the walk under an id bitmap; the bitmap makers
// ------------------------------------------------------------------------------------------------
#include "filter_host.h"

// ------------------------------------------------------------------------------------------------
// the exact selection: exact_topk over all rows or the rows an id bitmap allows; a bitmap's ids
// ------------------------------------------------------------------------------------------------
#include "exact_topk_host.h"

// ------------------------------------------------------------------------------------------------
// partitioned indexes: filtered search and the exact selection over global ids
// ------------------------------------------------------------------------------------------------
#include "sharded_ops_host.h"

// ------------------------------------------------------------------------------------------------
// post-filtered search: staged over-fetch on the ordinary search, the exact scan for what is left
// ------------------------------------------------------------------------------------------------
#include "postfilter_host.h"

// ------------------------------------------------------------------------------------------------
// range search: every element within a radius, by the exact scan and by the staged walk
// ------------------------------------------------------------------------------------------------
#include "exact_range_host.h"
#include "range_host.h"
