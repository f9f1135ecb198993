// codec_kernels.h -- the index file's layer blobs (MultiSetVector) encoded and decoded on the device.
// The authority for every byte is granne_file::encode_node / svb_encode / encode_index / decode_node / decode_layer in
// fileformat_host.h; codec_host.h drives these kernels segment by segment.
//
// ENCODER. A layer's rows are LayerHost::d_adj, [len][W] u32 with W = 32 or 64, padded with UNUSED anywhere in the row.
// W lanes serve a row (one wavefront: a row of 64 ids, or two rows of 32). A bitonic sort of the W slots puts the ids in
// ascending order and every UNUSED (the largest u32, never an id: validate_common) behind them, which is the compaction;
// deltas, byte lengths and their prefix sum follow in registers (codec_row). A block takes one chunk of 60 nodes:
//   ENC_SUMS   the chunk's bytes of records -> sums[c]               (pass 1; an exclusive scan makes initial[c])
//   ENC_TABLE  the chunk's 128-byte offset entry {u64 initial, u16 deltas[60]}, written as 32 aligned dwords
//   ENC_DATA   the chunk's records, assembled in LDS at the destination's alignment and written as whole dwords; only
//              the up to three bytes at either end that share a dword with a neighboring chunk are byte stores
// The record lengths are computed again in every mode instead of being kept: 2 bytes a node would break the memory bound.
//
// DECODER -- why a malformed file cannot become a fault. A segment is a run of whole chunks: `tab` holds its offset
// entries, `data` its `data_len` bytes of records (data_len <= the segment buffer's size: the host cuts segments by
// offsets it has itself compared with the blob's length). dec_offsets_kernel resolves offset j = initial + the prefix of
// its chunk's deltas in u64, and stores it RELATIVE to the segment's first offset, only if base <= o <= base + data_len;
// anything else is stored as 0 and reported. Every stored word is therefore <= data_len. dec_rows_kernel clamps again
// (e = min(e, data_len), s = min(s, e)), so the record it reads is [s, e) inside `data` whatever the words hold. Within a
// record: the count byte is read only if e > s; a raw id k only if count <= W and 1 + 4 count == e - s, so its four bytes
// end at or before e; a control byte only after n_ctrl <= payload; a data byte only after pos + len <= payload for that
// lane (lanes that fail read nothing, the record is reported). It writes row j of d_adj alone -- W words at j * W with
// j < len -- and only if count <= W. Ids are compared with the layer's length before the index is handed out. Nothing read
// from the file is used as an index before one of these comparisons.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace granne_hip {

constexpr uint32_t CODEC_UNUSED = 0xFFFFFFFFu;
constexpr uint32_t CODEC_CHUNK = 60;        // offsets per chunk (offsets.rs)
constexpr uint32_t CODEC_CHUNK_BYTES = 128; // {u64 initial; u16 deltas[60]}
constexpr uint32_t CODEC_BLOCK = 256;
constexpr uint32_t CODEC_REC_MAX = 1 + 16 + 4 * 64;               // count, 16 control bytes, 64 four-byte values
constexpr uint32_t CODEC_CHUNK_DATA_MAX = CODEC_CHUNK * CODEC_REC_MAX; // 16,380 bytes: what one block assembles
enum { ENC_SUMS = 0, ENC_TABLE = 1, ENC_DATA = 2 };
// the decoder's error word
enum {
    DEC_ERR_OFFSET = 1u,  // an offset outside its segment's data (not monotone / beyond the data)
    DEC_ERR_RECORD = 2u,  // a record shorter than its count and control bytes say
    DEC_ERR_ID = 4u,      // an id outside the layer
};

// inclusive prefix sum over the W lanes of a row's group
template <uint32_t W>
__device__ __forceinline__ uint32_t codec_scan(uint32_t v, uint32_t slot) {
#pragma unroll
    for (uint32_t d = 1; d < W; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, W);
        if (slot >= d) v += o;
    }
    return v;
}

struct CodecRow {
    uint32_t value;  // this slot's number: a delta, or a padding zero (slots count .. m - 1)
    uint32_t blen;   // its stream-vbyte length, 0 past m
    uint32_t excl;   // bytes of the slots before it
    uint32_t count, m, n_ctrl;
    bool raw;
    uint32_t rec_len; // 1 + payload
};

// set_encode (set_vector.rs:117-148) of the row whose slot `slot` holds id `v`
template <uint32_t W>
__device__ __forceinline__ CodecRow codec_row(uint32_t v, uint32_t slot) {
#pragma unroll
    for (uint32_t k = 2; k <= W; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t o = __shfl_xor(v, j, W);
            const bool up = (slot & k) == 0, low = (slot & j) == 0;
            v = (up == low) ? (v < o ? v : o) : (v > o ? v : o);
        }
    }
    CodecRow r;
    const uint64_t used = __ballot(v != CODEC_UNUSED);
    r.count = W == 64 ? (uint32_t)__popcll(used) : (uint32_t)__popc((uint32_t)(used >> (threadIdx.x & 32u)));
    const uint32_t prev = __shfl_up(v, 1, W);
    r.m = r.count < 4 ? 4 : r.count;
    r.value = slot < r.count ? (slot ? v - prev : v) : 0u;
    r.blen = slot < r.m ? (r.value < (1u << 8) ? 1u : r.value < (1u << 16) ? 2u : r.value < (1u << 24) ? 3u : 4u) : 0u;
    const uint32_t incl = codec_scan<W>(r.blen, slot);
    r.excl = incl - r.blen;
    r.n_ctrl = (r.m + 3) / 4;
    const uint32_t enc = r.n_ctrl + __shfl(incl, W - 1, W);
    r.raw = enc >= 4 * r.count; // the raw form unless compression makes it smaller (:137-143)
    r.rec_len = 1 + (r.raw ? 4 * r.count : enc);
    return r;
}

// chunks [c0, c0 + n_chunks) of a layer; see the head of the file. `initial` is the layer's scanned table (ENC_TABLE,
// ENC_DATA); `out` is the segment buffer, whose byte 0 is the chunk c0's entry (ENC_TABLE) or the byte initial[c0] of the
// layer's data (ENC_DATA).
template <uint32_t W, int MODE>
__global__ __launch_bounds__(CODEC_BLOCK) void codec_encode_kernel(const uint32_t* __restrict__ adj, uint64_t len, uint64_t c0,
                                                                  uint64_t n_chunks, uint64_t* __restrict__ sums,
                                                                  const uint64_t* __restrict__ initial, uint8_t* __restrict__ out) {
    constexpr uint32_t R = 64 / W; // rows per wavefront
    __shared__ uint32_t s_len[64];
    __shared__ uint32_t s_pre[64];
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[MODE == ENC_DATA ? CODEC_CHUNK_DATA_MAX + 8 : 16];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, slot = lane & (W - 1), g = lane / W;
    for (uint64_t cc = blockIdx.x; cc < n_chunks; cc += gridDim.x) {
        const uint64_t c = c0 + cc, first = c * CODEC_CHUNK;
        __syncthreads(); // the block has left the previous chunk's LDS
        for (uint32_t p = wave; p * R < CODEC_CHUNK; p += CODEC_BLOCK / 64) {
            const uint32_t jj = p * R + g;
            const uint64_t node = first + jj;
            const bool live = node < len; // (uniform over the row's W lanes)
            const CodecRow r = codec_row<W>(live ? adj[node * W + slot] : CODEC_UNUSED, slot);
            if (slot == 0) s_len[jj] = live ? r.rec_len : 0u;
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t mine = lane < CODEC_CHUNK ? s_len[lane] : 0u;
            const uint32_t incl = codec_scan<64>(mine, lane);
            s_pre[lane] = incl - mine; // s_pre[60] = the chunk's bytes
            if (MODE == ENC_SUMS && lane == 63) sums[c] = incl;
            if (MODE == ENC_TABLE && lane < 32) {
                // delta t of the chunk: offset (first + t) - offset (first + t - 1) = the bytes of node first + t - 1; delta 0 is 0
                uint32_t w;
                const uint64_t init = first <= len ? initial[c] : 0;
                if (lane == 0) w = (uint32_t)init;
                else if (lane == 1) w = (uint32_t)(init >> 32);
                else {
                    uint32_t d[2];
#pragma unroll
                    for (uint32_t h = 0; h < 2; ++h) {
                        const uint32_t t = 2 * (lane - 2) + h;
                        d[h] = first + t <= len ? (t ? s_len[t - 1] : 0u) : 0xFFFFu;
                    }
                    w = d[0] | d[1] << 16;
                }
                reinterpret_cast<uint32_t*>(out + cc * CODEC_CHUNK_BYTES)[lane] = w;
            }
        }
        if (MODE != ENC_DATA) continue;
        __syncthreads();
        // the chunk's bytes go to dst; in LDS they start at dst's misalignment, so that LDS dword q is one global dword
        uint8_t* const dst = out + (initial[c] - initial[c0]);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u), total = s_pre[CODEC_CHUNK];
        for (uint32_t p = wave; p * R < CODEC_CHUNK; p += CODEC_BLOCK / 64) {
            const uint32_t jj = p * R + g;
            const uint64_t node = first + jj;
            const bool live = node < len;
            const CodecRow r = codec_row<W>(live ? adj[node * W + slot] : CODEC_UNUSED, slot);
            // the control byte of four slots, gathered by the first of them (a slot past m contributes nothing)
            uint32_t ctrl = r.blen ? (r.blen - 1) << (2 * (slot & 3u)) : 0u;
            ctrl |= __shfl_down(ctrl, 1, W);
            ctrl |= __shfl_down(ctrl, 2, W);
            if (!live) continue;
            uint8_t* const rec = s_buf + sh + s_pre[jj];
            if (slot == 0) rec[0] = (uint8_t)r.count;
            if (r.raw) {
                if (slot < r.count)
                    for (uint32_t b = 0; b < 4; ++b) rec[1 + 4 * slot + b] = (uint8_t)(r.value >> (8 * b));
            } else {
                if ((slot & 3u) == 0 && slot < r.m) rec[1 + slot / 4] = (uint8_t)ctrl;
                for (uint32_t b = 0; b < r.blen; ++b) rec[1 + r.n_ctrl + r.excl + b] = (uint8_t)(r.value >> (8 * b));
            }
        }
        __syncthreads();
        const uint32_t* const s_words = reinterpret_cast<const uint32_t*>(s_buf);
        for (uint32_t q = threadIdx.x; 4 * q < sh + total; q += CODEC_BLOCK) {
            uint8_t* const gq = dst - sh + 4 * q;
            if (4 * q >= sh && 4 * q + 4 <= sh + total) {
                *reinterpret_cast<uint32_t*>(gq) = s_words[q];
            } else {
                for (uint32_t b = 0; b < 4; ++b)
                    if (4 * q + b >= sh && 4 * q + b < sh + total) gq[b] = s_buf[4 * q + b];
            }
        }
    }
}

// the last chunk c1 <= c_hi with initial[c1] - initial[c0] <= budget (c1 >= c0; the host asks with a budget of at least one
// chunk's bytes, so c1 > c0 whenever c_hi > c0): out[0] = c1, out[1] = initial[c1] - initial[c0]
__global__ void codec_cut_kernel(const uint64_t* __restrict__ initial, uint64_t c0, uint64_t c_hi, uint64_t budget,
                                 uint64_t* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t base = initial[c0];
    uint64_t lo = c0, hi = c_hi; // initial is non-decreasing
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (initial[mid] - base <= budget) lo = mid;
        else hi = mid - 1;
    }
    out[0] = lo;
    out[1] = initial[lo] - base;
}

// ---- decoder --------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ uint64_t codec_rd_u64(const uint8_t* p) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p); // (entries are 128-byte aligned in the segment buffer)
    return (uint64_t)w[0] | (uint64_t)w[1] << 32;
}

// Kernel 1. Offsets i = 0 .. n_nodes of the segment's nodes (node j0 + i, j0 a multiple of 60; `tab` starts at j0's
// chunk and holds every chunk an offset up to j0 + n_nodes lies in). off[i] = offset - base when base <= offset <=
// base + data_len, else 0 and DEC_ERR_OFFSET. max_count: the largest count byte of the records that start inside the data.
__global__ __launch_bounds__(CODEC_BLOCK) void dec_offsets_kernel(const uint8_t* __restrict__ tab, const uint8_t* __restrict__ data,
                                                                 uint64_t n_nodes, uint64_t base, uint64_t data_len,
                                                                 uint32_t* __restrict__ off, uint32_t* __restrict__ err,
                                                                 uint32_t* __restrict__ max_count) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    uint32_t bad = 0, mx = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * CODEC_BLOCK + threadIdx.x; i <= n_nodes; i += (uint64_t)gridDim.x * CODEC_BLOCK) {
        const uint8_t* const ch = tab + (i / CODEC_CHUNK) * CODEC_CHUNK_BYTES;
        const uint32_t t = (uint32_t)(i % CODEC_CHUNK);
        const uint64_t init = codec_rd_u64(ch);
        uint32_t rel = 0;
        bool ok = init <= base + data_len; // (then the sum below cannot wrap: base + data_len is a length of host memory)
        if (ok) {
            uint64_t o = init;
            const uint16_t* const d = reinterpret_cast<const uint16_t*>(ch + 8);
            for (uint32_t u = 0; u <= t; ++u) o += d[u];
            ok = o >= base && o - base <= data_len;
            if (ok) rel = (uint32_t)(o - base);
        }
        if (!ok) bad = DEC_ERR_OFFSET;
        off[i] = rel;
        if (ok && i < n_nodes && rel < data_len) mx = max(mx, (uint32_t)data[rel]);
    }
    if (mx) atomicMax(&s_max, mx);
    if (bad) atomicOr(err, bad);
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(max_count, s_max);
}

// Kernel 2. Node j0 + i's record -> row j0 + i of adj ([len][W]); decode_node (set_vector.rs:91-115) and the loader's id
// check. A record of more than W ids sets *wider and leaves its row alone (the host decodes the layer again, wider).
template <uint32_t W>
__global__ __launch_bounds__(CODEC_BLOCK) void dec_rows_kernel(const uint8_t* __restrict__ data, uint32_t data_len,
                                                              const uint32_t* __restrict__ off, uint64_t j0, uint64_t n_nodes,
                                                              uint64_t len, uint32_t* __restrict__ adj, uint32_t* __restrict__ err,
                                                              uint32_t* __restrict__ wider) {
    constexpr uint32_t R = 64 / W;
    const uint32_t lane = threadIdx.x & 63u, slot = lane & (W - 1), g = lane / W;
    const uint64_t waves = (uint64_t)gridDim.x * (CODEC_BLOCK / 64), groups = (n_nodes + R - 1) / R;
    for (uint64_t p = (uint64_t)blockIdx.x * (CODEC_BLOCK / 64) + (threadIdx.x >> 6); p < groups; p += waves) {
        const uint64_t i = p * R + g;
        const bool live = i < n_nodes && j0 + i < len; // (uniform over the row's W lanes, like everything up to `slot`)
        uint32_t s = 0, e = 0;
        bool backwards = false;
        if (live) {
            const uint32_t o0 = off[i], o1 = off[i + 1];
            backwards = o0 > o1;
            e = min(o1, data_len);
            s = backwards ? e : min(o0, e);
        }
        const uint32_t rlen = e - s;
        const uint32_t count = rlen ? data[s] : 0u;
        const uint32_t plen = rlen ? rlen - 1 : 0u;
        const uint8_t* const pay = data + s + 1; // read below only at indexes < plen
        const bool fits = count <= W;
        const bool raw = rlen && plen == 4 * count;
        const uint32_t m = count < 4 ? 4 : count, n_ctrl = (m + 3) / 4; // MIN_NUMBERS_TO_ENCODE
        const bool ctrl_ok = rlen && !raw && n_ctrl <= plen;
        uint32_t bad = 0;
        if (live && !rlen) bad = backwards ? DEC_ERR_OFFSET : DEC_ERR_RECORD;
        if (rlen && !raw && !ctrl_ok) bad = DEC_ERR_RECORD;
        const uint32_t blen = (ctrl_ok && fits && slot < m) ? ((pay[slot / 4] >> (2 * (slot & 3u))) & 3u) + 1u : 0u;
        const uint32_t pos = n_ctrl + codec_scan<W>(blen, slot) - blen;
        uint32_t v = 0;
        if (raw && fits && slot < count)
            v = (uint32_t)pay[4 * slot] | (uint32_t)pay[4 * slot + 1] << 8 | (uint32_t)pay[4 * slot + 2] << 16 |
                (uint32_t)pay[4 * slot + 3] << 24;
        if (blen) {
            if (pos + blen > plen) bad = DEC_ERR_RECORD;
            else
                for (uint32_t b = 0; b < blen; ++b) v |= (uint32_t)pay[pos + b] << (8 * b);
        }
        if (slot >= count) v = 0; // the numbers that pad a short record to four
        const uint32_t id = codec_scan<W>(v, slot); // delta_decode (:157-162), wrapping like the host's
        if (fits && slot < count && id >= len) bad |= DEC_ERR_ID;
        if (bad) atomicOr(err, bad);
        if (live && !fits && slot == 0) atomicOr(wider, 1u);
        if (live && fits) adj[(j0 + i) * W + slot] = slot < count ? id : CODEC_UNUSED;
    }
}

} // namespace granne_hip
