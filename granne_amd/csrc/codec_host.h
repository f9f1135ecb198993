// codec_host.h -- granne's index files written and read by the device codec (codec_kernels.h), streamed through a
// pinned ring so that neither side of the bus ever holds a file (host code, included by granne_hip.hip after
// fileformat_host.h, whose host codec stays the yardstick and the fallback).
//
//   staging_bytes   the pinned ring: two slots of staging_bytes / 2, each with a device segment of the same size
//                   (0: CODEC_STAGING_DEFAULT; below CODEC_STAGING_MIN: raised to it)
//   save / encode   pass 1: per layer, the chunks' record bytes (ENC_SUMS) and their exclusive scan -- 16 bytes per 60
//                   nodes, 8 of them kept until the layer is out -- which fix every layer's size, hence the header;
//                   pass 2: offset entries (ENC_TABLE), then records (ENC_DATA) in segments of whole chunks that
//                   codec_cut_kernel sizes to a slot; segment k is copied to its slot while the host writes segment k - 1
//   load            host: header, layer_sizes against the file, each blob's offset-table size and node count; then per
//                   layer segments of whole chunks {offset entries, their records} are read into a slot, uploaded,
//                   resolved (dec_offsets_kernel) and decoded straight into the final rows (dec_rows_kernel). The rows'
//                   width is a layer's largest count rounded up to 32, known only when the layer has been seen: the first
//                   pass assumes the header's num_neighbors and is repeated at the right width if that was wrong.
//   fallback        a layer of rows wider than 64 ids (and, reading, one whose chunk does not fit a slot's data part: a
//                   record longer than a 64-id one) goes through the host codec inside the same call; info[1] counts it.
#pragma once
#include <hipcub/hipcub.hpp>

#include "codec_kernels.h"

namespace granne_codec {

constexpr uint64_t STAGING_DEFAULT = GRANNE_HIP_CODEC_STAGING_DEFAULT;
constexpr uint64_t STAGING_MIN = GRANNE_HIP_CODEC_STAGING_MIN;
static_assert(STAGING_MIN / 2 - 2048 >= CODEC_CHUNK_DATA_MAX, "a slot's data part holds any chunk of 64-id records");

static uint64_t staging_of(uint64_t asked) {
    uint64_t s = asked ? asked : STAGING_DEFAULT;
    if (s < STAGING_MIN) s = STAGING_MIN;
    if (s > (4ull << 30)) s = 4ull << 30; // a segment's offsets are u32
    return s & ~(uint64_t)4095; // two slots of whole 128-byte entries
}

// what out_info reports
struct Info {
    uint64_t dev_layers = 0, host_layers = 0, dev_now = 0, dev_peak = 0, host_now = 0, host_peak = 0;
    void dev(int64_t d) {
        dev_now += d;
        if (dev_now > dev_peak) dev_peak = dev_now;
    }
    void host(int64_t d) {
        host_now += d;
        if (host_now > host_peak) host_peak = host_now;
    }
    void store(uint64_t* out) const {
        if (!out) return;
        out[0] = dev_layers, out[1] = host_layers, out[2] = dev_peak, out[3] = host_peak;
    }
};

// where encoded bytes go: a file, or a buffer of exactly the file's size
struct Sink {
    FILE* f = nullptr;
    uint8_t* mem = nullptr;
    uint64_t cap = 0, pos = 0;
    bool ok = true;
    void write(const void* p, size_t n) {
        if (!n) return;
        if (f) ok = ok && fwrite(p, 1, n, f) == n;
        else if (pos + n <= cap) memcpy(mem + pos, p, n);
        else ok = false;
        pos += n;
    }
};

// where file bytes come from: memory, or a file read in pieces (never mapped: the pages would count as the caller's)
struct Source {
    const uint8_t* mem = nullptr;
    int fd = -1;
    uint64_t len = 0;
    bool open_ro(const char* path) {
        fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) return false;
        len = (uint64_t)st.st_size;
        return true;
    }
    bool read(uint64_t off, void* dst, uint64_t n) const {
        if (off > len || n > len - off) return false;
        if (mem) {
            memcpy(dst, mem + off, n);
            return true;
        }
        uint8_t* d = (uint8_t*)dst;
        while (n) {
            const ssize_t r = pread(fd, d, n, (off_t)off);
            if (r <= 0) return false;
            d += r, off += (uint64_t)r, n -= (uint64_t)r;
        }
        return true;
    }
    ~Source() {
        if (fd >= 0) ::close(fd);
    }
};

// the pinned ring and its device segments; one stream carries the copies and the kernels in order
struct Ring {
    PinBuf pin;
    DevBuf dev[2];
    uint64_t S = 0; // bytes of a slot
    hipStream_t s = nullptr, sq = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    uint64_t pend[2] = {0, 0}; // download: bytes of the slot that wait for the sink
    int next = 0;
    Sink* sink = nullptr;
    Info* info = nullptr;

    int init(uint64_t staging, Info* inf) {
        info = inf;
        S = staging / 2;
        HIP_TRY(pin.alloc(2 * S + 64, hipHostMallocDefault)); // (+64: the words kernels report through)
        info->host((int64_t)(2 * S + 64));
        HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&sq, hipStreamNonBlocking));
        for (auto& e : ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return GRANNE_HIP_OK;
    }
    int need_segments() {
        for (auto& d : dev)
            if (!d) {
                HIP_TRY(d.alloc(S));
                info->dev((int64_t)S);
            }
        return GRANNE_HIP_OK;
    }
    uint8_t* slot(int i) const { return pin.as<uint8_t>() + (uint64_t)i * S; }
    uint64_t* words() const { return reinterpret_cast<uint64_t*>(pin.as<uint8_t>() + 2 * S); }
    // the slot to fill next, idle: what it last carried has arrived (and, downloading, has gone to the sink)
    int acquire(int* out) {
        const int i = next;
        if (busy[i]) {
            HIP_TRY(hipEventSynchronize(ev[i]));
            if (sink) sink->write(slot(i), pend[i]);
            busy[i] = false, pend[i] = 0;
        }
        *out = i;
        return GRANNE_HIP_OK;
    }
    // the slot's work has been queued on s
    int submit(int i, uint64_t download_bytes) {
        HIP_TRY(hipEventRecord(ev[i], s));
        busy[i] = true, pend[i] = download_bytes;
        next = i ^ 1;
        return GRANNE_HIP_OK;
    }
    int drain() {
        for (int k = 0; k < 2; ++k) { // the older slot first
            int i;
            int rc = acquire(&i);
            if (rc) return rc;
            next = i ^ 1;
        }
        return GRANNE_HIP_OK;
    }
    ~Ring() {
        if (s) (void)hipStreamSynchronize(s);
        if (sq) (void)hipStreamSynchronize(sq);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
        if (sq) (void)hipStreamDestroy(sq);
    }
};

static int codec_grid(uint64_t blocks) { return (int)(blocks < 1 ? 1 : blocks > 8192 ? 8192 : blocks); }

template <int MODE>
static void launch_encode(uint32_t W, hipStream_t s, uint64_t n_chunks, const uint32_t* adj, uint64_t len, uint64_t c0,
                          uint64_t* sums, const uint64_t* initial, uint8_t* out) {
    if (W == 32)
        hipLaunchKernelGGL((codec_encode_kernel<32, MODE>), dim3(codec_grid(n_chunks)), dim3(CODEC_BLOCK), 0, s, adj, len, c0, n_chunks,
                           sums, initial, out);
    else
        hipLaunchKernelGGL((codec_encode_kernel<64, MODE>), dim3(codec_grid(n_chunks)), dim3(CODEC_BLOCK), 0, s, adj, len, c0, n_chunks,
                           sums, initial, out);
}

// ---- encoder --------------------------------------------------------------------------------------------------------
struct EncLayer {
    bool on_device = false;
    uint64_t len = 0, n_chunks = 0, data_bytes = 0, blob_bytes = 0;
    DevBuf initial;            // u64 [n_chunks + 1]: offset of each chunk's first node, then the data's size
    std::vector<uint8_t> blob; // a layer of the host codec
};

// pass 1: every layer's size (and the blob of a layer the device codec does not take)
static int enc_plan(const granne_hip_index* ix, Ring& R, std::vector<EncLayer>* plan, uint64_t* num_neighbors, Info* info) {
    plan->resize(ix->layers.size());
    *num_neighbors = 0;
    for (size_t l = 0; l < ix->layers.size(); ++l) {
        const LayerHost& L = ix->layers[l];
        EncLayer& E = (*plan)[l];
        E.len = L.len;
        E.n_chunks = 1 + L.len / CODEC_CHUNK; // set_vector.rs:176-177
        if (l + 1 == ix->layers.size() && L.len) { // get_neighbors(0).len(), io.rs:20-24
            std::vector<uint32_t> row(L.dev_width);
            HIP_TRY(hipMemcpy(row.data(), L.d_adj.get(), row.size() * 4, hipMemcpyDeviceToHost));
            for (uint32_t v : row) *num_neighbors += v != GRANNE_HIP_UNUSED;
        }
        if (L.dev_width > 64) {
            // the host codec, as granne_hip_index_encode runs it: the one-layer index file's bytes behind its header
            std::vector<uint32_t> rows((size_t)L.len * L.dev_width);
            if (!rows.empty()) HIP_TRY(hipMemcpy(rows.data(), L.d_adj.get(), rows.size() * 4, hipMemcpyDeviceToHost));
            const uint32_t* ptr = rows.data();
            std::vector<uint8_t> file;
            info->host((int64_t)rows.size() * 4);
            if (granne_file::encode_index(1, &E.len, &ptr, &L.dev_width, &file))
                return fail(GRANNE_HIP_ERR_IO, "index does not fit the file format");
            E.blob.assign(file.begin() + granne_file::METADATA_LEN, file.end());
            info->host((int64_t)(file.size() + E.blob.size()));
            info->host(-(int64_t)(rows.size() * 4 + file.size()));
            E.blob_bytes = E.blob.size();
            info->host_layers++;
            continue;
        }
        E.on_device = true;
        info->dev_layers++;
        const uint64_t table_bytes = (E.n_chunks + 1) * 8;
        DevBuf sums, tmp;
        HIP_TRY(sums.alloc(table_bytes));
        HIP_TRY(E.initial.alloc(table_bytes));
        info->dev((int64_t)(2 * table_bytes));
        HIP_TRY(hipMemsetAsync(sums.as<uint64_t>() + E.n_chunks, 0, 8, R.s));
        launch_encode<ENC_SUMS>(L.dev_width, R.s, E.n_chunks, L.d_adj.as<uint32_t>(), L.len, 0, sums.as<uint64_t>(), nullptr, nullptr);
        HIP_TRY(hipGetLastError());
        size_t need = 0;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, sums.as<uint64_t>(), E.initial.as<uint64_t>(), (int)(E.n_chunks + 1), R.s));
        HIP_TRY(tmp.alloc(need));
        info->dev((int64_t)need);
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(tmp.get(), need, sums.as<uint64_t>(), E.initial.as<uint64_t>(), (int)(E.n_chunks + 1), R.s));
        HIP_TRY(hipMemcpyAsync(&R.words()[0], E.initial.as<uint64_t>() + E.n_chunks, 8, hipMemcpyDeviceToHost, R.s));
        HIP_TRY(hipStreamSynchronize(R.s));
        E.data_bytes = R.words()[0];
        E.blob_bytes = 8 + E.n_chunks * CODEC_CHUNK_BYTES + E.data_bytes;
        info->dev(-(int64_t)(table_bytes + need)); // sums and tmp go here
    }
    return GRANNE_HIP_OK;
}

// the 1024-byte header, as granne_file::encode_index makes it (serde_json's map is sorted by key, io.rs:46-63)
static int enc_header(const std::vector<EncLayer>& plan, uint64_t num_neighbors, std::vector<uint8_t>* out) {
    const size_t n = plan.size();
    std::string js = "granne{\"compressed\":true,\"granne_version\":\"0.5.2\",\"layer_counts\":[";
    for (size_t l = 0; l < n; ++l) js += (l ? "," : "") + std::to_string(plan[l].len);
    js += "],\"layer_sizes\":[";
    for (size_t l = 0; l < n; ++l) js += (l ? "," : "") + std::to_string(plan[l].blob_bytes);
    js += "],\"num_elements\":" + std::to_string(n ? plan[n - 1].len : 0);
    js += ",\"num_layers\":" + std::to_string(n);
    js += ",\"num_neighbors\":" + std::to_string(num_neighbors) + ",\"version\":2}";
    if (js.size() > granne_file::METADATA_LEN) return fail(GRANNE_HIP_ERR_IO, "index does not fit the file format");
    out->assign(granne_file::METADATA_LEN, (uint8_t)' ');
    memcpy(out->data(), js.data(), js.size());
    return GRANNE_HIP_OK;
}

// pass 2: header and blobs to R.sink, in file order
static int enc_emit(const granne_hip_index* ix, Ring& R, std::vector<EncLayer>& plan, const std::vector<uint8_t>& header) {
    R.sink->write(header.data(), header.size());
    DevBuf d_cut; // codec_cut_kernel's two words
    HIP_TRY(d_cut.alloc(16));
    for (size_t l = 0; l < plan.size(); ++l) {
        EncLayer& E = plan[l];
        const LayerHost& L = ix->layers[l];
        int rc = R.drain(); // what the host writes itself goes behind everything the ring still holds
        if (rc) return rc;
        if (!E.on_device) {
            R.sink->write(E.blob.data(), E.blob.size());
            R.info->host(-(int64_t)E.blob.size());
            std::vector<uint8_t>().swap(E.blob);
            continue;
        }
        uint8_t off_bytes[8];
        granne_file::wr_u64(off_bytes, E.n_chunks * CODEC_CHUNK_BYTES);
        R.sink->write(off_bytes, 8);
        if ((rc = R.need_segments())) return rc;
        const uint64_t* const initial = E.initial.as<uint64_t>();
        const uint32_t* const adj = L.d_adj.as<uint32_t>();
        for (uint64_t c0 = 0, per = R.S / CODEC_CHUNK_BYTES; c0 < E.n_chunks; c0 += per) {
            const uint64_t n = E.n_chunks - c0 < per ? E.n_chunks - c0 : per;
            int i;
            if ((rc = R.acquire(&i))) return rc;
            launch_encode<ENC_TABLE>(L.dev_width, R.s, n, adj, L.len, c0, nullptr, initial, R.dev[i].as<uint8_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(R.slot(i), R.dev[i].get(), n * CODEC_CHUNK_BYTES, hipMemcpyDeviceToHost, R.s));
            if ((rc = R.submit(i, n * CODEC_CHUNK_BYTES))) return rc;
        }
        for (uint64_t c0 = 0; c0 < E.n_chunks;) {
            // (asked on a stream of its own: the answer does not wait for the segment that is being copied)
            hipLaunchKernelGGL(codec_cut_kernel, dim3(1), dim3(1), 0, R.sq, initial, c0, E.n_chunks, R.S, d_cut.as<uint64_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(R.words() + 2, d_cut.get(), 16, hipMemcpyDeviceToHost, R.sq));
            HIP_TRY(hipStreamSynchronize(R.sq));
            const uint64_t c1 = R.words()[2], bytes = R.words()[3];
            if (c1 <= c0 || c1 > E.n_chunks || bytes > R.S) return fail(GRANNE_HIP_ERR_HIP, "device codec: a chunk of layer %zu does not fit a segment", l);
            int i;
            if ((rc = R.acquire(&i))) return rc;
            if (bytes) {
                launch_encode<ENC_DATA>(L.dev_width, R.s, c1 - c0, adj, L.len, c0, nullptr, initial, R.dev[i].as<uint8_t>());
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(R.slot(i), R.dev[i].get(), bytes, hipMemcpyDeviceToHost, R.s));
            }
            if ((rc = R.submit(i, bytes))) return rc;
            c0 = c1;
        }
        if ((rc = R.drain())) return rc; // (the layer's table is freed next)
        R.info->dev(-(int64_t)E.initial.capacity());
        E.initial.reset();
    }
    return R.drain();
}

// the elements file: [u64 dim][dense rows], the rows through the ring
static int enc_elements(const granne_hip_index* ix, Ring& R) {
    uint8_t hdr[8];
    granne_file::wr_u64(hdr, ix->dim);
    R.sink->write(hdr, 8);
    const uint64_t dense = (uint64_t)ix->dim * elem_size(ix->dtype);
    const uint8_t* const src = ix->d_elements.as<uint8_t>();
    int rc, i;
    if (dense <= R.S) {
        for (uint64_t r0 = 0, per = R.S / dense; r0 < ix->n_elements; r0 += per) {
            const uint64_t n = ix->n_elements - r0 < per ? ix->n_elements - r0 : per;
            if ((rc = R.acquire(&i))) return rc;
            HIP_TRY(hipMemcpy2DAsync(R.slot(i), dense, src + r0 * ix->row_stride, ix->row_stride, dense, n, hipMemcpyDeviceToHost, R.s));
            if ((rc = R.submit(i, n * dense))) return rc;
        }
    } else { // a row longer than a slot goes in pieces
        for (uint64_t r = 0; r < ix->n_elements; ++r)
            for (uint64_t o = 0; o < dense; o += R.S) {
                const uint64_t n = dense - o < R.S ? dense - o : R.S;
                if ((rc = R.acquire(&i))) return rc;
                HIP_TRY(hipMemcpyAsync(R.slot(i), src + r * ix->row_stride + o, n, hipMemcpyDeviceToHost, R.s));
                if ((rc = R.submit(i, n))) return rc;
            }
    }
    return R.drain();
}

// ---- decoder --------------------------------------------------------------------------------------------------------
struct DecLayer {
    uint64_t start = 0, size = 0;        // the blob in the file
    uint64_t off_bytes = 0, data_len = 0; // its offset table and its records
    uint64_t len = 0;
};

static inline uint16_t rd_u16(const uint8_t* p) { return (uint16_t)((uint16_t)p[0] | (uint16_t)p[1] << 8); }

// the checks of granne_file::decode_index / decode_layer that need no record: *err is the host decoder's message
static bool dec_parse(const Source& src, std::vector<DecLayer>* layers, uint64_t* num_neighbors, std::string* err) {
    uint8_t head[granne_file::METADATA_LEN];
    if (src.len < sizeof(head) || !src.read(0, head, sizeof(head)) || memcmp(head, "granne", 6) != 0) {
        *err = "Library string missing";
        return false;
    }
    const std::string js((const char*)head + 6, sizeof(head) - 6);
    uint64_t num_layers = 0;
    std::vector<uint64_t> counts, sizes;
    if (!granne_file::json_number(js, "num_layers", &num_layers) || !granne_file::json_array(js, "layer_counts", &counts) ||
        !granne_file::json_array(js, "layer_sizes", &sizes)) {
        *err = "Could not read metadata";
        return false;
    }
    if (counts.size() != num_layers || sizes.size() != num_layers) {
        *err = "metadata arrays disagree with num_layers";
        return false;
    }
    if (!granne_file::json_number(js, "num_neighbors", num_neighbors)) *num_neighbors = 0; // (a hint for the rows' width)
    uint64_t start = sizeof(head);
    layers->resize(num_layers);
    for (uint64_t l = 0; l < num_layers; ++l) {
        DecLayer& D = (*layers)[l];
        if (sizes[l] > src.len - start) { *err = "index file truncated"; return false; }
        D.start = start, D.size = sizes[l];
        start += sizes[l];
        uint8_t b[CODEC_CHUNK_BYTES];
        if (D.size < 8 || !src.read(D.start, b, 8)) { *err = "layer blob too small"; return false; }
        D.off_bytes = granne_file::rd_u64(b);
        if (D.off_bytes % CODEC_CHUNK_BYTES != 0 || D.off_bytes > D.size - 8) { *err = "bad offsets size in layer blob"; return false; }
        const uint64_t n_chunks = D.off_bytes / CODEC_CHUNK_BYTES;
        if (n_chunks == 0) { *err = "layer blob without offset chunks"; return false; }
        D.data_len = D.size - 8 - D.off_bytes;
        if (!src.read(D.start + 8 + (n_chunks - 1) * CODEC_CHUNK_BYTES, b, sizeof(b))) { *err = "index file truncated"; return false; }
        uint64_t used = 0; // offsets.rs:270-272
        while (used < CODEC_CHUNK && rd_u16(b + 8 + 2 * used) != 0xFFFF) ++used;
        const uint64_t n_off = CODEC_CHUNK * (n_chunks - 1) + used;
        if (n_off == 0) { *err = "layer blob without offsets"; return false; }
        D.len = n_off - 1;
        if (D.len != counts[l]) { *err = "layer_counts disagrees with the layer's offset table"; return false; }
    }
    return true;
}

// the elements file's rows into ix->d_elements (device rows, zero padded), through the ring
static int dec_elements(granne_hip_index* ix, const Source& src, Ring& R) {
    const uint64_t dense = (uint64_t)ix->dim * elem_size(ix->dtype), n = ix->n_elements;
    const size_t bytes = (size_t)n * ix->row_stride;
    HIP_TRY(ix->d_elements.alloc(bytes));
    ix->hbm_bytes += bytes;
    if (n == 0) return GRANNE_HIP_OK;
    uint8_t* const dst = ix->d_elements.as<uint8_t>();
    if (dense != ix->row_stride) HIP_TRY(hipMemsetAsync(dst, 0, bytes, R.s));
    int rc, i;
    if (dense <= R.S) {
        for (uint64_t r0 = 0, per = R.S / dense; r0 < n; r0 += per) {
            const uint64_t m = n - r0 < per ? n - r0 : per;
            if ((rc = R.acquire(&i))) return rc;
            if (!src.read(8 + r0 * dense, R.slot(i), m * dense)) return fail(GRANNE_HIP_ERR_IO, "elements file: short read");
            HIP_TRY(hipMemcpy2DAsync(dst + r0 * ix->row_stride, ix->row_stride, R.slot(i), dense, dense, m, hipMemcpyHostToDevice, R.s));
            if ((rc = R.submit(i, 0))) return rc;
        }
    } else {
        for (uint64_t r = 0; r < n; ++r)
            for (uint64_t o = 0; o < dense; o += R.S) {
                const uint64_t m = dense - o < R.S ? dense - o : R.S;
                if ((rc = R.acquire(&i))) return rc;
                if (!src.read(8 + r * dense + o, R.slot(i), m)) return fail(GRANNE_HIP_ERR_IO, "elements file: short read");
                HIP_TRY(hipMemcpyAsync(dst + r * ix->row_stride + o, R.slot(i), m, hipMemcpyHostToDevice, R.s));
                if ((rc = R.submit(i, 0))) return rc;
            }
    }
    return GRANNE_HIP_OK;
}

// what a pass over a layer found
struct DecFound {
    uint32_t err = 0, wider = 0, max_count = 0;
    bool host = false; // the layer is the host codec's: a chunk that fits no slot, or chunk offsets the host decoder will refuse
};

// One pass over layer D into adj ([len][W]). A slot is {tab_cap offset entries}{data_cap bytes of records}.
static int dec_pass(const Source& src, const DecLayer& D, uint32_t W, uint32_t* adj, Ring& R, uint32_t* d_off, uint32_t* d_words,
                    uint64_t tab_cap, DecFound* found) {
    const uint64_t tab_bytes = tab_cap * CODEC_CHUNK_BYTES, data_cap = R.S - tab_bytes;
    const uint64_t last_chunk = D.len / CODEC_CHUNK; // the chunk of offset `len`
    const uint64_t table = D.start + 8, data = table + D.off_bytes;
    HIP_TRY(hipMemsetAsync(d_words, 0, 16, R.s));
    int rc, i;
    for (uint64_t c0 = 0, j0 = 0; j0 < D.len;) {
        if ((rc = R.acquire(&i))) return rc;
        uint8_t* const tab = R.slot(i);
        const uint64_t n_tab = last_chunk - c0 + 1 < tab_cap ? last_chunk - c0 + 1 : tab_cap;
        if (!src.read(table + c0 * CODEC_CHUNK_BYTES, tab, n_tab * CODEC_CHUNK_BYTES)) return fail(GRANNE_HIP_ERR_IO, "index file: short read");
        // offset of node 60 c: initial + delta 0 (offsets.rs:177-187); the segment ends at the furthest chunk start -- or at
        // offset `len`, when its chunk is here -- that keeps the records within data_cap
        auto chunk_start = [&](uint64_t k, uint64_t* o) { // entry k of tab; false: not an offset inside the data
            const uint64_t init = granne_file::rd_u64(tab + k * CODEC_CHUNK_BYTES);
            if (init > D.data_len) return false;
            *o = init + rd_u16(tab + k * CODEC_CHUNK_BYTES + 8);
            return *o <= D.data_len;
        };
        uint64_t base = 0, end_off = 0, end_node = j0, prev = 0;
        if (!chunk_start(0, &base)) { found->host = true; return GRANNE_HIP_OK; }
        prev = base;
        for (uint64_t k = 1; k <= n_tab; ++k) {
            uint64_t o = 0, node = (c0 + k) * CODEC_CHUNK;
            if (k < n_tab) {
                if (!chunk_start(k, &o)) { found->host = true; return GRANNE_HIP_OK; }
                if (node > D.len) break; // (cannot happen: k <= last_chunk - c0)
            } else if (c0 + n_tab - 1 == last_chunk) { // offset `len`: entry n_tab - 1, deltas 0 .. len % 60
                const uint8_t* const e = tab + (n_tab - 1) * CODEC_CHUNK_BYTES;
                o = granne_file::rd_u64(e);
                for (uint64_t u = 0; u <= D.len % CODEC_CHUNK; ++u) o += rd_u16(e + 8 + 2 * u);
                node = D.len;
                if (o > D.data_len) { found->host = true; return GRANNE_HIP_OK; }
            } else break;
            if (o < prev) { found->host = true; return GRANNE_HIP_OK; }
            if (o - base > data_cap) break;
            prev = o, end_off = o, end_node = node;
            if (node == D.len) break;
        }
        if (end_node == j0) { found->host = true; return GRANNE_HIP_OK; } // one chunk's records do not fit a slot
        const uint64_t n_nodes = end_node - j0, span = end_off - base, up_tab = (n_nodes / CODEC_CHUNK + 1) * CODEC_CHUNK_BYTES;
        if (!src.read(data + base, tab + tab_bytes, span)) return fail(GRANNE_HIP_ERR_IO, "index file: short read");
        uint8_t* const d_tab = R.dev[i].as<uint8_t>();
        HIP_TRY(hipMemcpyAsync(d_tab, tab, up_tab < n_tab * CODEC_CHUNK_BYTES ? up_tab : n_tab * CODEC_CHUNK_BYTES, hipMemcpyHostToDevice, R.s));
        if (span) HIP_TRY(hipMemcpyAsync(d_tab + tab_bytes, tab + tab_bytes, span, hipMemcpyHostToDevice, R.s));
        hipLaunchKernelGGL(dec_offsets_kernel, dim3(codec_grid((n_nodes + CODEC_BLOCK) / CODEC_BLOCK)), dim3(CODEC_BLOCK), 0, R.s, d_tab,
                           d_tab + tab_bytes, n_nodes, base, span, d_off, d_words, d_words + 2);
        const uint64_t blocks = (n_nodes * W / 64 + CODEC_BLOCK / 64) / (CODEC_BLOCK / 64);
        if (W == 32)
            hipLaunchKernelGGL(dec_rows_kernel<32>, dim3(codec_grid(blocks)), dim3(CODEC_BLOCK), 0, R.s, d_tab + tab_bytes, (uint32_t)span,
                               d_off, j0, n_nodes, D.len, adj, d_words, d_words + 1);
        else
            hipLaunchKernelGGL(dec_rows_kernel<64>, dim3(codec_grid(blocks)), dim3(CODEC_BLOCK), 0, R.s, d_tab + tab_bytes, (uint32_t)span,
                               d_off, j0, n_nodes, D.len, adj, d_words, d_words + 1);
        HIP_TRY(hipGetLastError());
        if ((rc = R.submit(i, 0))) return rc;
        j0 = end_node, c0 = end_node / CODEC_CHUNK;
    }
    uint32_t* const w = reinterpret_cast<uint32_t*>(R.words() + 4);
    HIP_TRY(hipMemcpyAsync(w, d_words, 12, hipMemcpyDeviceToHost, R.s));
    HIP_TRY(hipStreamSynchronize(R.s));
    found->err = w[0], found->wider = w[1], found->max_count = w[2];
    return GRANNE_HIP_OK;
}

// a layer through the host decoder (granne_file::decode_layer), then the rows granne_hip_index_create_csr makes
static int dec_layer_host(granne_hip_index* ix, const Source& src, const DecLayer& D, Info* info) {
    std::vector<uint8_t> blob(D.size);
    info->host((int64_t)blob.size());
    if (!src.read(D.start, blob.data(), D.size)) return fail(GRANNE_HIP_ERR_IO, "index file: short read");
    granne_file::DecodedLayer H;
    std::string err;
    if (granne_file::decode_layer(blob.data(), blob.size(), D.len, &H, &err)) return fail(GRANNE_HIP_ERR_IO, "index file: %s", err.c_str());
    info->host((int64_t)(H.offsets.size() * 8 + H.ids.size() * 4));
    uint32_t maxdeg = 0;
    for (uint64_t j = 0; j < D.len; ++j) maxdeg = std::max<uint32_t>(maxdeg, (uint32_t)(H.offsets[j + 1] - H.offsets[j]));
    for (uint32_t id : H.ids)
        if (id >= D.len) return fail(GRANNE_HIP_ERR_IO, "index file: neighbor id outside its layer");
    LayerHost L;
    L.len = D.len;
    L.width = maxdeg;
    L.dev_width = ((maxdeg ? maxdeg : 1) + 31u) & ~31u;
    const size_t bytes = (size_t)D.len * L.dev_width * 4;
    HIP_TRY(L.d_adj.alloc(bytes));
    ix->hbm_bytes += bytes;
    DevBuf d_off, d_ids;
    HIP_TRY(d_off.alloc(H.offsets.size() * 8));
    HIP_TRY(d_ids.alloc(H.ids.size() * 4));
    info->dev((int64_t)(H.offsets.size() * 8 + H.ids.size() * 4));
    HIP_TRY(hipMemcpy(d_off.get(), H.offsets.data(), H.offsets.size() * 8, hipMemcpyHostToDevice));
    if (!H.ids.empty()) HIP_TRY(hipMemcpy(d_ids.get(), H.ids.data(), H.ids.size() * 4, hipMemcpyHostToDevice));
    if (D.len) {
        hipLaunchKernelGGL(csr_to_adj_kernel, dim3(grid_for(D.len * L.dev_width, 256)), dim3(256), 0, nullptr, d_off.as<uint64_t>(),
                           d_ids.as<uint32_t>(), L.d_adj.as<uint32_t>(), D.len, L.dev_width);
        HIP_TRY(hipDeviceSynchronize());
    }
    info->dev(-(int64_t)(H.offsets.size() * 8 + H.ids.size() * 4));
    info->host(-(int64_t)(blob.size() + H.offsets.size() * 8 + H.ids.size() * 4));
    ix->layers.push_back(std::move(L));
    info->host_layers++;
    return GRANNE_HIP_OK;
}

static int dec_error(uint32_t e) {
    return fail(GRANNE_HIP_ERR_IO, "index file: %s", e & DEC_ERR_OFFSET ? "offsets are not monotone / exceed the data"
                                                     : e & DEC_ERR_RECORD ? "malformed neighbor record"
                                                                          : "neighbor id outside its layer");
}

static int load(granne_hip_index** out, const Source& idx, const Source& el, int dtype, int device_id, uint64_t staging_bytes,
                uint64_t* out_info) {
    Info info;
    info.store(out_info);
    // elements: [u64 width][scalars] (src/slice_vector/mod.rs:213-221); width > 0, len % width == 0 (:116-118)
    uint8_t eb[8];
    if (el.len < 8 || !el.read(0, eb, 8)) return fail(GRANNE_HIP_ERR_IO, "elements file too small");
    const uint64_t dim = granne_file::rd_u64(eb), esz = elem_size(dtype), payload = el.len - 8;
    if (dim == 0 || dim > 0xFFFFFFFFull || payload % esz != 0 || (payload / esz) % dim != 0)
        return fail(GRANNE_HIP_ERR_IO, "elements file: width %llu does not divide the data", (unsigned long long)dim);
    const uint64_t n = payload / esz / dim;
    std::vector<DecLayer> layers;
    std::string err;
    uint64_t num_neighbors = 0;
    if (!dec_parse(idx, &layers, &num_neighbors, &err)) return fail(GRANNE_HIP_ERR_IO, "index file: %s", err.c_str());
    std::vector<uint64_t> lens(layers.size());
    for (size_t l = 0; l < layers.size(); ++l) lens[l] = layers[l].len;
    int rc = validate_common(out, n, (uint32_t)dim, dtype, (uint32_t)layers.size(), lens.data());
    if (rc) return rc;
    GRANNE_HIP_ON_DEVICE(device_id);
    granne_hip_index* ix = new granne_hip_index();
    ix->device = device_id;
    ix->dim = (uint32_t)dim;
    ix->dtype = dtype;
    ix->n_elements = n;
    ix->row_bytes = device_row_bytes(ix->dim, dtype);
    ix->row_stride = device_row_stride(ix->dim, dtype);
    IndexPtr made(ix);
    Ring R; // (after `made`: the ring's stream is idle before the index can go)
    if ((rc = R.init(staging_of(staging_bytes), &info))) return rc;
    if ((rc = dec_elements(ix, el, R))) return rc;
    const uint64_t tab_cap = std::max<uint64_t>(16, R.S / 16 / CODEC_CHUNK_BYTES);
    DevBuf d_off, d_words;
    for (size_t l = 0; l < layers.size(); ++l) {
        const DecLayer& D = layers[l];
        uint32_t W = num_neighbors > 32 && num_neighbors <= 64 ? 64 : 32;
        bool done = false;
        for (int attempt = 0; attempt < 3 && !done; ++attempt) {
            if ((rc = R.need_segments())) return rc;
            if (!d_off) {
                HIP_TRY(d_off.alloc((tab_cap * CODEC_CHUNK + 1) * 4));
                HIP_TRY(d_words.alloc(16));
                info.dev((int64_t)((tab_cap * CODEC_CHUNK + 1) * 4 + 16));
            }
            LayerHost L;
            L.len = D.len;
            L.dev_width = W;
            const size_t bytes = (size_t)D.len * W * 4;
            HIP_TRY(L.d_adj.alloc(bytes));
            DecFound found;
            if ((rc = dec_pass(idx, D, W, L.d_adj.as<uint32_t>(), R, d_off.as<uint32_t>(), d_words.as<uint32_t>(), tab_cap, &found))) return rc;
            HIP_TRY(hipStreamSynchronize(R.s)); // (L.d_adj may be freed below)
            if (found.host) break;
            if (found.err) return dec_error(found.err);
            const uint32_t need = ((found.max_count ? found.max_count : 1) + 31u) & ~31u;
            if (need > 64) break;
            if (need != W) {
                W = need; // the rows are as wide as the layer's longest list, like the host loader's
                continue;
            }
            L.width = found.max_count;
            ix->hbm_bytes += bytes;
            ix->layers.push_back(std::move(L));
            info.dev_layers++;
            done = true;
        }
        if (!done && (rc = dec_layer_host(ix, idx, D, &info))) return rc;
    }
    if ((rc = finish_layers(ix, R.s))) return rc; // synchronises R.s
    info.store(out_info);
    *out = made.release();
    return GRANNE_HIP_OK;
}

static int save(const granne_hip_index* ix, const char* index_path, const char* elements_path, uint64_t staging_bytes,
                void** out_bytes, uint64_t* out_len, uint64_t* out_info) {
    Info info;
    info.store(out_info);
    GRANNE_HIP_ON_DEVICE(ix->device);
    Ring R;
    int rc = R.init(staging_of(staging_bytes), &info);
    if (rc) return rc;
    if (index_path || out_bytes) {
        std::vector<EncLayer> plan;
        std::vector<uint8_t> header;
        uint64_t num_neighbors = 0;
        if ((rc = enc_plan(ix, R, &plan, &num_neighbors, &info))) return rc;
        if ((rc = enc_header(plan, num_neighbors, &header))) return rc;
        Sink sink;
        uint64_t total = header.size();
        for (const EncLayer& E : plan) total += E.blob_bytes;
        if (index_path) {
            sink.f = fopen(index_path, "wb");
            if (!sink.f) return fail(GRANNE_HIP_ERR_IO, "Could not write %s", index_path);
        } else {
            sink.cap = total;
            sink.mem = (uint8_t*)malloc(sink.cap);
            if (!sink.mem) return fail(GRANNE_HIP_ERR_IO, "out of host memory (%llu bytes)", (unsigned long long)sink.cap);
        }
        R.sink = &sink;
        rc = enc_emit(ix, R, plan, header);
        R.sink = nullptr;
        if (rc == 0 && sink.pos != total)
            rc = fail(GRANNE_HIP_ERR_HIP, "device codec: wrote %llu bytes, not the planned size", (unsigned long long)sink.pos);
        if (sink.f && fclose(sink.f) != 0) sink.ok = false;
        if (rc == 0 && !sink.ok) rc = fail(GRANNE_HIP_ERR_IO, "Could not write %s", index_path ? index_path : "the buffer");
        if (rc) {
            free(sink.mem);
            return rc;
        }
        if (out_bytes) *out_bytes = sink.mem, *out_len = sink.cap;
    }
    if (elements_path) {
        GRANNE_HIP_COMPACT_UNSUPPORTED(ix, "save_elements (write the container's own files with granne_hip_sum_embeddings_save_*)");
        Sink sink;
        sink.f = fopen(elements_path, "wb");
        if (!sink.f) return fail(GRANNE_HIP_ERR_IO, "Could not write %s", elements_path);
        R.sink = &sink;
        rc = enc_elements(ix, R);
        R.sink = nullptr;
        if (fclose(sink.f) != 0) sink.ok = false;
        if (rc) return rc;
        if (!sink.ok) return fail(GRANNE_HIP_ERR_IO, "Could not write %s", elements_path);
    }
    info.store(out_info);
    return GRANNE_HIP_OK;
}

} // namespace granne_codec

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" int granne_hip_index_encode_on_device(const granne_hip_index* ix, uint64_t staging_bytes, void** out_bytes, uint64_t* out_len,
                                                 uint64_t* out_info) {
    if (!ix || !out_bytes || !out_len) return fail(GRANNE_HIP_ERR_INVALID, "null argument");
    *out_bytes = nullptr;
    *out_len = 0;
    return granne_codec::save(ix, nullptr, nullptr, staging_bytes, out_bytes, out_len, out_info);
}

extern "C" int granne_hip_index_save_on_device(const granne_hip_index* ix, const char* index_path, const char* elements_path,
                                               uint64_t staging_bytes, uint64_t* out_info) {
    if (!ix) return fail(GRANNE_HIP_ERR_INVALID, "index is null");
    return granne_codec::save(ix, index_path, elements_path, staging_bytes, nullptr, nullptr, out_info);
}

extern "C" int granne_hip_index_load_on_device(granne_hip_index** out, const void* index_bytes, uint64_t index_len, const void* elements_bytes,
                                               uint64_t elements_len, int dtype, int device_id, uint64_t staging_bytes, uint64_t* out_info) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!index_bytes || !elements_bytes) return fail(GRANNE_HIP_ERR_INVALID, "null buffer");
    if (!known_dtype(dtype)) return fail(GRANNE_HIP_ERR_INVALID, "unknown dtype %d", dtype);
    granne_codec::Source idx, el;
    idx.mem = (const uint8_t*)index_bytes, idx.len = index_len;
    el.mem = (const uint8_t*)elements_bytes, el.len = elements_len;
    return granne_codec::load(out, idx, el, dtype, device_id, staging_bytes, out_info);
}

extern "C" int granne_hip_index_load_files_on_device(granne_hip_index** out, const char* index_path, const char* elements_path, int dtype,
                                                     int device_id, uint64_t staging_bytes, uint64_t* out_info) {
    if (!out) return fail(GRANNE_HIP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!index_path || !elements_path) return fail(GRANNE_HIP_ERR_INVALID, "null path");
    if (!known_dtype(dtype)) return fail(GRANNE_HIP_ERR_INVALID, "unknown dtype %d", dtype);
    granne_codec::Source idx, el;
    if (!idx.open_ro(index_path)) return fail(GRANNE_HIP_ERR_IO, "Could not open index file %s", index_path);
    if (!el.open_ro(elements_path)) return fail(GRANNE_HIP_ERR_IO, "Could not open elements file %s", elements_path);
    return granne_codec::load(out, idx, el, dtype, device_id, staging_bytes, out_info);
}
