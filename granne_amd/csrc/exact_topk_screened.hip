// exact_topk_screened.hip -- the kernels of the screened exact selection and their launchers (exact_topk_screened.h has
// the method and what this file shares with the driver). A translation unit of its own: granne_amd/build.py compiles it
// without the packed f32 instructions. It needs nothing of the library's other kernels but dist.h's dot4_i8.
#include "exact_topk_screened.h"
#include "dist.h"
#include "exact_topk_cursor.h"

namespace granne_hip {

typedef float ets_f32x16 __attribute__((ext_vector_type(16)));
typedef int ets_i32x16 __attribute__((ext_vector_type(16)));
typedef int ets_i32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 ets_b16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 ets_b16x4 __attribute__((ext_vector_type(4)));

// Which (query tile, row range) a block takes: brute_force.h's bf_block -- workgroups go to the 8 XCDs round robin by
// their linear id, so with a multiple of 8 ranges the query tiles that stream one range share an XCD and its L2.
struct EtsBlock { uint32_t qt, range; };
__device__ __forceinline__ EtsBlock ets_block() {
    const uint32_t nqt = gridDim.x, G = gridDim.y;
    const uint32_t L = blockIdx.y * nqt + blockIdx.x; // dispatch order: x fastest
    EtsBlock b;
    if ((G & 7u) == 0u) {
        const uint32_t xcd = L & 7u, slot = L >> 3;
        b.range = xcd * (G >> 3) + slot / nqt;
        b.qt = slot % nqt;
    } else {
        b.qt = blockIdx.x;
        b.range = blockIdx.y;
    }
    return b;
}

__device__ __forceinline__ float ets_width(float lo) { return (1.0f - lo) * (1.0f / (float)ETS_BUCKETS); }
__device__ __forceinline__ float ets_edge(float lo, float w, int j) { return lo + w * (float)j; }
// AFTER: the buckets end at the query's `top` where that is below 1 (no cursor: top = +inf, and this is ets_width(lo))
__device__ __forceinline__ float ets_width_top(float lo, float top) { return (__builtin_fminf(1.0f, top) - lo) * (1.0f / (float)ETS_BUCKETS); }

// A lane's view of its query's floor. ETS_RADIUS: thr = lo is the lower threshold; w and inv_w are not used.
// AFTER (the cursor forms): `top` is the query's upper threshold, read from P.tops -- COUNT: top_sure, a row
// counts with s < top; COLLECT: top_any, a row is listed with s <= top -- and the buckets lie between lo and min(1, top).
struct EtsFloor {
    float thr, lo, w, inv_w, top;
    template <int MODE, bool AFTER = false>
    __device__ __forceinline__ void init(const EtsParams& P, uint32_t q, bool qlive) {
        lo = qlive ? P.lo[q] : __builtin_inff();
        top = __builtin_inff();
        if constexpr (AFTER) top = qlive ? P.tops[q] : __builtin_inff();
        w = AFTER ? ets_width_top(lo, top) : ets_width(lo);
        inv_w = 1.0f / w;
        thr = MODE == ETS_COLLECT ? lo - P.eps2 : lo;
    }
};

// The 16 scores a lane holds of one 32-row block: rows e_blk + 8 (v / 4) + v % 4 + 4 h, its query in column `col`.
// COUNT: into the block's LDS histogram (hq: the query's column of it). COLLECT: into the query's candidate list.
// ETS_BITS: `word` is the block's word of the query's bitmap -- rows e_blk .. e_blk + 31 are its bits 0 .. 31 -- and only
// allowed rows are counted or collected. ETS_LIST: the rows are list positions; what is collected is the id at the position.
// ROLLED (COLLECT): the hits are placed by one loop over the set bits, as ets_radius16 places its rows, not by sixteen
// unrolled stores -- the 16 x 13 form over a list with its queries in the rows has no registers left for their addresses.
// AFTER: a row above the query's `top` takes no part (COUNT: at it neither): it is before the cursor, or not surely after it.
template <int MODE, int SRC, bool ROLLED = false, bool AFTER = false>
__device__ __forceinline__ void ets_take16(const EtsParams& P, const EtsFloor& F, const float (&sc)[16], uint64_t e_blk, uint64_t r1,
                                           bool whole, uint32_t q, uint32_t col, uint32_t h, uint32_t* hq, uint32_t word) {
    const uint32_t wv = word >> (4u * h); // the lane's row v: bit 8 (v / 4) + v % 4 of it
    auto allowed = [&](int v) {
        if constexpr (AFTER) {
            if (MODE == ETS_COUNT ? !(sc[v] < F.top) : !(sc[v] <= F.top)) return false;
        }
        return SRC != ETS_BITS || (wv >> (8 * (v / 4) + v % 4) & 1u) != 0u;
    };
    if constexpr (MODE == ETS_COUNT) {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const uint64_t e = e_blk + (uint32_t)(8 * (v / 4) + v % 4) + 4u * h;
            if (sc[v] >= F.thr && (whole || e < r1) && allowed(v)) {
                int j = (int)__builtin_fminf((sc[v] - F.lo) * F.inv_w, (float)(ETS_BUCKETS - 1));
                j = j < 0 ? 0 : j;
                while (j > 0 && sc[v] < ets_edge(F.lo, F.w, j)) --j; // never round up into a bucket
                atomicAdd(hq + (uint32_t)j * ETS_QT, 1u);
            }
        }
    } else {
        uint32_t mask = 0;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const uint64_t e = e_blk + (uint32_t)(8 * (v / 4) + v % 4) + 4u * h;
            mask |= (sc[v] >= F.thr && (whole || e < r1) && allowed(v)) ? 1u << v : 0u;
        }
        const uint32_t mine = (uint32_t)__builtin_popcount(mask);
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, 64);
        uint32_t base = 0;
        if (h == 0u && mine + other > 0u) base = atomicAdd(P.cnt + q, mine + other); // (hits: q is a live query)
        base = (uint32_t)__shfl((int)base, (int)col, 64);
        uint32_t pos = base + (h ? other : 0u); // the pair's lower lane first
        if constexpr (ROLLED) {
            static_assert(SRC == ETS_LIST, "the rolled placement reads the list");
            for (uint32_t m = mask; m != 0u; m &= m - 1u, ++pos) {
                const uint32_t v = (uint32_t)__builtin_ctz(m);
                if (pos < ETS_CAP) P.cand[(size_t)q * ETS_CAP + pos] = P.list[e_blk + 8u * (v >> 2) + (v & 3u) + 4u * h];
            }
            return;
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            if (mask >> v & 1u) {
                if (pos < ETS_CAP) {
                    const uint64_t e = e_blk + (uint32_t)(8 * (v / 4) + v % 4) + 4u * h;
                    P.cand[(size_t)q * ETS_CAP + pos] = SRC == ETS_LIST ? P.list[e] : (uint32_t)e;
                }
                ++pos;
            }
        }
    }
}

// ETS_RADIUS, the third epilogue (exact_range_screened): of the lane's 16 scores, the SURE rows (s >= hi:
// within the radius whatever the reference's arithmetic says) are counted in `sure` and listed by COLLECT's placement in
// P.cand[q][0 .. ETS_CAP) -- until the pair has seen the list full (the places asked for reached ETS_CAP: ETS_SURE_FULL in
// `sure`, whose count goes on) --; `sure` is the thread's own word of LDS, not a register: the 16 x 13 form over a list has
// none left for a value that lives through the scan loop. The BAND rows (lo <= s < hi) are listed in P.cand[q][ETS_CAP .. 2 ETS_CAP) by an atomic of
// the lane's own, taken only by a lane that has one. hi is read here, by the lanes with a row at or above lo: the scan
// loop holds one register less. Rows and bits as ets_take16's.
constexpr uint32_t ETS_SURE_FULL = 0x80000000u; // (a block's range has fewer rows than that)
template <int SRC>
__device__ __forceinline__ void ets_radius16(const EtsParams& P, const EtsFloor& F, const float (&sc)[16], uint64_t e_blk, uint64_t r1,
                                             bool whole, uint32_t q, uint32_t col, uint32_t h, uint32_t word, uint32_t* my_sure) {
    const uint32_t wv = word >> (4u * h);
    uint32_t in = 0, top = 0;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const uint64_t e = e_blk + (uint32_t)(8 * (v / 4) + v % 4) + 4u * h;
        const bool ok = (whole || e < r1) && (SRC != ETS_BITS || (wv >> (8 * (v / 4) + v % 4) & 1u) != 0u);
        in |= (sc[v] >= F.lo && ok) ? 1u << v : 0u;
    }
    const float hi = in ? P.hi[q] : __builtin_inff(); // (a row at or above lo: q is a live query)
#pragma unroll
    for (int v = 0; v < 16; ++v) top |= sc[v] >= hi ? 1u << v : 0u;
    top &= in;
    const uint32_t band = in & ~top;
    uint32_t bpos = 0;
    if (band != 0u) bpos = atomicAdd(P.bcnt + q, (uint32_t)__builtin_popcount(band));
    const uint32_t mine = (uint32_t)__builtin_popcount(top);
    const uint32_t other = (uint32_t)__shfl_xor((int)mine, 32, 64);
    uint32_t sure = *my_sure + mine;
    uint32_t base = ETS_CAP; // (no place)
    if (h == 0u && mine + other > 0u && !(sure & ETS_SURE_FULL)) base = atomicAdd(P.cnt + q, mine + other);
    base = (uint32_t)__shfl((int)base, (int)col, 64);
    if (mine + other > 0u && base + mine + other >= ETS_CAP) sure |= ETS_SURE_FULL; // (the same for both lanes of the pair)
    *my_sure = sure;
    uint32_t pos = base + (h ? other : 0u); // the pair's lower lane first
    uint32_t* const lists = P.cand + (size_t)q * (2u * ETS_CAP);
    // Both lists in one loop over the set bits, not unrolled: the scores are not needed any more, and the unrolled form's
    // sixteen store addresses cost the 16 x 13 form its last registers. ETS_LIST: the position is listed, not the id at
    // it (ers_pad_kernel reads the ids). Rows and positions fit 32 bits: the host refuses more elements.
    for (uint32_t m = in; m != 0u; m &= m - 1u) {
        const uint32_t v = (uint32_t)__builtin_ctz(m);
        const bool t = top >> v & 1u;
        const uint32_t at = t ? pos : bpos;
        if (at < ETS_CAP) lists[(t ? 0u : ETS_CAP) + at] = (uint32_t)e_blk + 8u * (v >> 2) + (v & 3u) + 4u * h;
        pos += t ? 1u : 0u, bpos += t ? 0u : 1u;
    }
}
// after the block's range: the lane pair's count of sure rows in one atomic per (block, query) that has any
__device__ __forceinline__ void ets_sure_flush(const EtsParams& P, uint32_t q, uint32_t h, uint32_t sure) {
    sure &= ~ETS_SURE_FULL;
    sure += (uint32_t)__shfl_xor((int)sure, 32, 64);
    if (h == 0u && sure != 0u) atomicAdd(P.sure + q, sure);
}

// the words of LDS an epilogue keeps beside the tile: the histogram, nothing, or a count per thread
constexpr uint32_t ets_mode_words(int mode) { return mode == ETS_COUNT ? ETS_BUCKETS * ETS_QT : mode == ETS_RADIUS ? ETS_THREADS : 0u; }

// a block's LDS histogram: cleared before its range, its non-zero buckets added to the queries' global ones after it
__device__ __forceinline__ void ets_hist_clear(uint32_t* lh, uint32_t tid) {
    for (uint32_t i = tid; i < ETS_BUCKETS * ETS_QT; i += ETS_THREADS) lh[i] = 0u;
}
__device__ __forceinline__ void ets_hist_flush(const EtsParams& P, const uint32_t* lh, uint32_t q0, uint32_t tid) {
    __syncthreads();
    for (uint32_t i = tid; i < ETS_BUCKETS * ETS_QT; i += ETS_THREADS) {
        const uint32_t c = lh[i], q = q0 + (i & (ETS_QT - 1u));
        if (c != 0u && q < P.nq) atomicAdd(P.hist + (size_t)q * ETS_BUCKETS + (i / ETS_QT), c);
    }
}

// The word of query q's bitmap for the 32-row block at e_blk (ETS_BITS), read by the lanes the block's test passed for
// (`hit`: a live query's); a block past the range's end (zero rows, which can pass a floor below 0) reads nothing.
template <int SRC>
__device__ __forceinline__ uint32_t ets_word(const EtsParams& P, uint32_t q, uint64_t e_blk, uint64_t r1, bool hit) {
    if constexpr (SRC == ETS_BITS) {
        if (hit && e_blk < r1) return P.filter[(size_t)q * P.filter_stride + (e_blk >> 5)];
    }
    return 0u;
}

// ETS_Q_ROWS: the place of the diagonal in a 32-row result block -- the v of the lane's 16 scores that is the score of its
// query (element qid) with itself, 16 where the block's rows e_blk .. e_blk + 31 do not hold it or the lane's half does not
// (rows 8 (v / 4) + v % 4 + 4 h). Ids and rows fit 32 bits (the host refuses more elements); a block past qid wraps to a
// large difference. `any`: some lane of the wave has its diagonal in the block -- the wave's 32 queries are consecutive
// elements, so of all the blocks of a scan at most two, and only they run the replacement.
__device__ __forceinline__ uint32_t ets_diag(uint32_t qid, bool qlive, uint64_t e_blk, uint32_t h, bool* any) {
    const uint32_t d = qid - (uint32_t)e_blk;
    *any = __ballot(d < 32u) != 0ull;
    return (qlive && d < 32u && (d >> 2 & 1u) == h) ? 4u * (d >> 3) + (d & 3u) : 16u;
}

// f32 rows of up to 16 KG components. grid = (query tiles of ETS_QT, row ranges), bf_block's order. SRC: the rows are all
// rows (ETS_ALL, ETS_BITS: P.n of them) or the rows at the positions [0, P.n) of P.list (ETS_LIST). QSRC: the queries are
// the caller's dense ones, or the elements P.q_first + q (ETS_Q_ROWS), split into their pieces straight from their rows.
// AFTER: the cursor form -- P.tops [nq] is the pass's upper threshold per query (EtsFloor, ets_take16); nothing else differs.
template <int KG, int R, int MODE, int SRC = ETS_ALL, int QSRC = ETS_Q_DENSE, bool AFTER = false>
__global__ __launch_bounds__(ETS_THREADS) void ets_b16_kernel(const EtsParams P) {
    static_assert(!AFTER || (MODE != ETS_RADIUS && QSRC == ETS_Q_DENSE), "a cursor: top-k of dense queries");
    extern __shared__ __align__(16) uint8_t smem_ets[];
    constexpr uint32_t ET = 32u * R;                // rows per tile
    constexpr uint32_t COMPS = 16u * KG;            // components per (zero padded) row
    constexpr uint32_t STRIDE_B = 2u * COMPS + 16u; // bytes per LDS row of one piece: an odd number of 16-byte units
    uint8_t* tile_hi = smem_ets;
    uint8_t* tile_lo = smem_ets + (size_t)ET * STRIDE_B;
    uint32_t* lh = reinterpret_cast<uint32_t*>(smem_ets + 2u * (size_t)ET * STRIDE_B); // COUNT: [ETS_BUCKETS][ETS_QT]; RADIUS: [ETS_THREADS]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    const EtsBlock blk = ets_block();
    const uint32_t q = blk.qt * ETS_QT + wave * 32u + col;
    const bool qlive = q < P.nq;
    if constexpr (MODE == ETS_COUNT) ets_hist_clear(lh, tid); // (the first tile's barriers stand between this and the first count)

    ets_b16x8 qh[KG], ql[KG]; // the lane's half of its query as bf16 pieces, in registers for the whole range
    {
        const float* qp;
        if constexpr (QSRC == ETS_Q_ROWS) { // ETS_LIST: P.q_first + q is a position of the list, as the scanned rows are
            uint64_t id = P.q_first + (qlive ? q : 0u);
            if constexpr (SRC == ETS_LIST) id = P.list[id];
            qp = reinterpret_cast<const float*>(P.elements + id * P.row_stride);
        } else
            qp = reinterpret_cast<const float*>(P.queries) + (size_t)(qlive ? q : 0u) * P.dim;
#pragma unroll
        for (int g = 0; g < KG; ++g) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t c = h * 8u * KG + (uint32_t)g * 8u + (uint32_t)j;
                const float v = (qlive && c < P.dim) ? qp[c] : 0.0f;
                const __bf16 hi = (__bf16)v;
                qh[g][j] = hi;
                ql[g][j] = (__bf16)(v - (float)hi);
            }
        }
    }
    EtsFloor F;
    F.init<MODE, AFTER>(P, q, qlive);
    if constexpr (MODE == ETS_RADIUS) lh[tid] = 0u; // the thread's rows with s >= hi over the whole range (and ETS_SURE_FULL)

    const uint64_t r0 = (uint64_t)blk.range * P.per_range;
    const uint64_t r1 = r0 + P.per_range < P.n ? r0 + P.per_range : P.n;
    const uint32_t row_f4 = P.row_bytes / 16u; // float4 units of a device row that hold data
    constexpr uint32_t UNITS = COMPS / 4u;     // float4 units per (padded) row
    constexpr uint32_t NPF = (ET * UNITS + ETS_THREADS - 1u) / ETS_THREADS;
    float4 pf[NPF]; // the next tile, on its way from memory while this one is scored
    auto fetch = [&](uint64_t e0) {
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) {
            const uint32_t u = tid + ETS_THREADS * j;
            const uint32_t row = u / UNITS, c4 = u - row * UNITS;
            pf[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (u < ET * UNITS && e0 + row < r1 && c4 < row_f4) {
                uint64_t id = e0 + row;
                if constexpr (SRC == ETS_LIST) id = P.list[id];
                pf[j] = *reinterpret_cast<const float4*>(P.elements + id * P.row_stride + c4 * 16u);
            }
        }
    };
    if (r0 < r1) fetch(r0);
    for (uint64_t e0 = r0; e0 < r1; e0 += ET) {
        __syncthreads(); // the previous tile has been consumed
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) { // split into the two pieces on the way to LDS
            const uint32_t u = tid + ETS_THREADS * j;
            const uint32_t row = u / UNITS, c4 = u - row * UNITS;
            if (u < ET * UNITS) {
                ets_b16x4 hi, lo;
                const float v[4] = {pf[j].x, pf[j].y, pf[j].z, pf[j].w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    hi[t] = (__bf16)v[t];
                    lo[t] = (__bf16)(v[t] - (float)hi[t]);
                }
                *reinterpret_cast<ets_b16x4*>(tile_hi + (size_t)row * STRIDE_B + c4 * 8u) = hi;
                *reinterpret_cast<ets_b16x4*>(tile_lo + (size_t)row * STRIDE_B + c4 * 8u) = lo;
            }
        }
        __syncthreads();
        if (e0 + ET < r1) fetch(e0 + ET);
        ets_f32x16 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][v] = 0.0f;
        // the fragments of the next (step, block) are read while the matrix cores work on this one
        const size_t off0 = (size_t)col * STRIDE_B + (size_t)h * 16u * KG;
        constexpr int NF = KG * R;
        ets_b16x8 ah[2], al[2];
        ah[0] = *reinterpret_cast<const ets_b16x8*>(tile_hi + off0);
        al[0] = *reinterpret_cast<const ets_b16x8*>(tile_lo + off0);
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int g = i / R, r = i % R;
            if (i + 1 < NF) {
                const int gn = (i + 1) / R, rn = (i + 1) % R;
                ah[(i + 1) & 1] = *reinterpret_cast<const ets_b16x8*>(tile_hi + off0 + (size_t)rn * 32u * STRIDE_B + (size_t)gn * 16u);
                al[(i + 1) & 1] = *reinterpret_cast<const ets_b16x8*>(tile_lo + off0 + (size_t)rn * 32u * STRIDE_B + (size_t)gn * 16u);
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], qh[g], acc[r], 0, 0, 0);
            acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], ql[g], acc[r], 0, 0, 0);
            acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i & 1], qh[g], acc[r], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // result block r: acc[r][v] ~ dot(row e0 + r*32 + 8*(v/4) + 4*h + v%4, query `col` of this wave). Few blocks hold
        // a score at or above a lane's floor: one max over the block decides for the wave.
        const bool whole = e0 + ET <= r1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (QSRC == ETS_Q_ROWS) { // the diagonal: before the block's max, the ballot and the epilogue
                bool any;
                const uint32_t vd = ets_diag((uint32_t)P.q_first + q, qlive, e0 + (uint32_t)(r * 32), h, &any);
                if (any) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[r][v] = (uint32_t)v == vd ? -__builtin_inff() : acc[r][v];
                }
            }
            float mx = acc[r][0];
#pragma unroll
            for (int v = 1; v < 16; ++v) mx = __builtin_fmaxf(mx, acc[r][v]);
            if (__ballot(mx >= F.thr)) {
                float sc[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) sc[v] = acc[r][v];
                const uint32_t word = ets_word<SRC>(P, q, e0 + (uint32_t)(r * 32), r1, qlive && mx >= F.thr);
                if constexpr (MODE == ETS_RADIUS)
                    ets_radius16<SRC>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, word, lh + tid);
                else
                    ets_take16<MODE, SRC, MODE == ETS_COLLECT && SRC == ETS_LIST && QSRC == ETS_Q_ROWS && KG == 13, AFTER>(
                        P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, lh + wave * 32u + col, word);
            }
        }
    }
    if constexpr (MODE == ETS_COUNT) ets_hist_flush(P, lh, blk.qt * ETS_QT, tid);
    if constexpr (MODE == ETS_RADIUS) ets_sure_flush(P, q, h, lh[tid]);
}

template <int KG, int R>
constexpr uint32_t ets_b16_lds(int mode) {
    return 2u * (32u * R) * (2u * 16u * KG + 16u) + ets_mode_words(mode) * 4u; // tile_hi, tile_lo, the mode's words
}

// int8 rows of up to 128 bytes: score = ((float)dot * (1 / |x|)) * (1 / |q|), the dot exact in i32
constexpr uint32_t ETS_I8_R = 4, ETS_I8_ROWS = 32u * ETS_I8_R, ETS_I8_STRIDE = 128u + 16u;
// ETS_LIST: a gathered block has no entry in inv_gmax; its bound is made from the block's own 1 / |x| on their way into
// LDS (gm, two copies by the tile's parity: one is read while the next tile's is being made).
// ETS_Q_ROWS: the lane's 16-byte groups of element P.q_first + q are the operand as they lie (device rows are zero padded),
// its 1 / |q| is the row's own P.inv_norm.
template <int MODE, int SRC = ETS_ALL, int QSRC = ETS_Q_DENSE, bool AFTER = false>
__global__ __launch_bounds__(ETS_THREADS) void ets_i8_kernel(const EtsParams P) {
    static_assert(!AFTER || (MODE != ETS_RADIUS && QSRC == ETS_Q_DENSE), "a cursor: top-k of dense queries");
    extern __shared__ __align__(16) uint8_t smem_ets[];
    constexpr int R = (int)ETS_I8_R;
    constexpr uint32_t ET = ETS_I8_ROWS, STRIDE = ETS_I8_STRIDE;
    uint8_t* tile = smem_ets;
    float* inv = reinterpret_cast<float*>(smem_ets + (size_t)ET * STRIDE); // [ET] 1 / |x|
    float* gm = inv + ET;                                                   // [2][R] inv_gmax of the tile's blocks, by lane half
    uint32_t* lh = reinterpret_cast<uint32_t*>(gm + 2 * R);                 // COUNT: [ETS_BUCKETS][ETS_QT]; RADIUS: [ETS_THREADS]
    uint32_t* gml = lh + ets_mode_words(MODE);             // ETS_LIST: [2][2][R] float bits, by parity
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    const EtsBlock blk = ets_block();
    const uint32_t q = blk.qt * ETS_QT + wave * 32u + col;
    const bool qlive = q < P.nq;
    if constexpr (MODE == ETS_COUNT) ets_hist_clear(lh, tid);
    if constexpr (SRC == ETS_LIST) {
        if (tid < 4u * R) gml[tid] = 0u; // (the first tile's first barrier stands between this and the first maximum)
    }
    ets_i32x4 qr[4]; // bytes 32 g + 16 h .. + 15 of the query (bf_i8_kernel's operand)
    float qinv = 0.0f;
    if constexpr (QSRC == ETS_Q_ROWS) {
        uint64_t id = P.q_first + (qlive ? q : 0u);
        if constexpr (SRC == ETS_LIST) id = P.list[id]; // (a position of the list, as the scanned rows are)
        const uint8_t* qp = P.elements + id * P.row_stride;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t off = (uint32_t)g * 32u + h * 16u;
            qr[g] = ets_i32x4{0, 0, 0, 0};
            if (qlive && off < P.row_bytes) qr[g] = *reinterpret_cast<const ets_i32x4*>(qp + off);
        }
        qinv = qlive ? P.inv_norm[id] : 0.0f;
    } else {
        const uint8_t* qp = P.queries + (size_t)(qlive ? q : 0u) * P.dim;
        const uint32_t last = P.dim - 1u;
        int dy = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const uint32_t c = (uint32_t)g * 32u + h * 16u + (uint32_t)w * 4u + (uint32_t)b;
                    const uint32_t raw = qp[c < last ? c : last];
                    const uint32_t keep = (qlive && c < P.dim) ? 0xFFu : 0u;
                    v |= (raw & keep) << (8 * b);
                }
                qr[g][w] = (int)v;
                dy = dot4_i8(v, v, dy);
            }
        }
        dy += __shfl_xor(dy, 32, 64); // the other half of the vector
        qinv = dy > 0 ? 1.0f / __builtin_sqrtf((float)dy) : 0.0f;
    }
    EtsFloor F;
    F.init<MODE, AFTER>(P, q, qlive);
    if constexpr (MODE == ETS_RADIUS) lh[tid] = 0u; // the thread's rows with s >= hi over the whole range (and ETS_SURE_FULL)

    const uint64_t r0 = (uint64_t)blk.range * P.per_range;
    const uint64_t r1 = r0 + P.per_range < P.n ? r0 + P.per_range : P.n;
    // 8 threads per row (16 bytes each; device rows shorter than 128 bytes are zero extended): 64 rows per round
    constexpr uint32_t NPF = ET * 8u / ETS_THREADS;
    const uint32_t my_row = tid >> 3, my_c = tid & 7u;
    const bool col_live = my_c < P.row_bytes / 16u;
    uint4 pf[NPF];
    float pfn[NPF], pfg = 0.0f;
    auto fetch = [&](uint64_t e0) {
        if constexpr (SRC != ETS_LIST) {
            if (tid < 2u * R) pfg = e0 + 32u * (tid >> 1) < r1 ? P.inv_gmax[((e0 >> 5) + (tid >> 1)) * 2u + (tid & 1u)] : 0.0f;
        }
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) {
            const uint64_t row = e0 + my_row + (ETS_THREADS / 8u) * j;
            pf[j] = make_uint4(0, 0, 0, 0);
            pfn[j] = 0.0f;
            uint64_t id = row;
            if constexpr (SRC == ETS_LIST) id = row < r1 ? P.list[row] : 0u;
            if (row < r1 && col_live) pf[j] = *reinterpret_cast<const uint4*>(P.elements + id * P.row_stride + my_c * 16u);
            if (row < r1 && my_c == 0u) pfn[j] = P.inv_norm[id];
        }
    };
    if (r0 < r1) fetch(r0);
    uint32_t par = 0; // ETS_LIST: which copy of gml this tile's maxima go to
    for (uint64_t e0 = r0; e0 < r1; e0 += ET) {
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) {
            const uint32_t row = my_row + (ETS_THREADS / 8u) * j;
            *reinterpret_cast<uint4*>(tile + (size_t)row * STRIDE + my_c * 16u) = pf[j];
            if (my_c == 0u) inv[row] = pfn[j];
            if constexpr (SRC == ETS_LIST) { // row = 32 r + 8 g4 + 4 h + t: non-negative floats order as their bits
                if (my_c == 0u) atomicMax(gml + par * 2u * R + (row >> 2 & 1u) * R + (row >> 5), __float_as_uint(pfn[j]));
            }
        }
        if constexpr (SRC != ETS_LIST) {
            if (tid < 2u * R) gm[(tid & 1u) * R + (tid >> 1)] = pfg;
        }
        __syncthreads();
        if constexpr (SRC == ETS_LIST) {
            gm = reinterpret_cast<float*>(gml + par * 2u * R);
            par ^= 1u;
            if (tid < 2u * R) gml[par * 2u * R + tid] = 0u; // the next tile's copy: last read before this tile's first barrier
        }
        if (e0 + ET < r1) fetch(e0 + ET);
        ets_i32x16 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][v] = 0;
        ets_i32x4 afrag[2][R];
#pragma unroll
        for (int r = 0; r < R; ++r) afrag[0][r] = *reinterpret_cast<const ets_i32x4*>(tile + (size_t)(r * 32 + col) * STRIDE + h * 16);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (g + 1 < 4) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    afrag[(g + 1) & 1][r] = *reinterpret_cast<const ets_i32x4*>(tile + (size_t)(r * 32 + col) * STRIDE + (g + 1) * 32 + h * 16);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[g & 1][r], qr[g], acc[r], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // the largest dot of the lane's 16 rows times the largest 1 / |x| among them bounds their scores from above
        // (products of non-negative floats are monotone; a negative dot's score is <= 0 <= the bound)
        const bool whole = e0 + ET <= r1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint32_t vd = 16u;
            bool diag = false;
            if constexpr (QSRC == ETS_Q_ROWS) { // the diagonal: out of the block's bound here, out of its scores below
                vd = ets_diag((uint32_t)P.q_first + q, qlive, e0 + (uint32_t)(r * 32), h, &diag);
                if (diag) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[r][v] = (uint32_t)v == vd ? (int)0x80000000 : acc[r][v];
                }
            }
            int im = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) im = max(im, acc[r][v]);
            const bool hit = ((float)im * gm[h * R + r]) * qinv >= F.thr;
            if (!__ballot(hit)) continue;
            float sc[16];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) { // rows r*32 + 8*g4 + 4*h + 0..3: their 1 / |x| in one read
                const float4 iv = *reinterpret_cast<const float4*>(inv + r * 32 + 8 * g4 + 4 * h);
                sc[g4 * 4 + 0] = ((float)acc[r][g4 * 4 + 0] * iv.x) * qinv;
                sc[g4 * 4 + 1] = ((float)acc[r][g4 * 4 + 1] * iv.y) * qinv;
                sc[g4 * 4 + 2] = ((float)acc[r][g4 * 4 + 2] * iv.z) * qinv;
                sc[g4 * 4 + 3] = ((float)acc[r][g4 * 4 + 3] * iv.w) * qinv;
            }
            if constexpr (QSRC == ETS_Q_ROWS) {
                if (diag) {
#pragma unroll
                    for (int v = 0; v < 16; ++v) sc[v] = (uint32_t)v == vd ? -__builtin_inff() : sc[v];
                }
            }
            const uint32_t word = ets_word<SRC>(P, q, e0 + (uint32_t)(r * 32), r1, qlive && hit);
            if constexpr (MODE == ETS_RADIUS)
                ets_radius16<SRC>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, word, lh + tid);
            else
                ets_take16<MODE, SRC, false, AFTER>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, lh + wave * 32u + col, word);
        }
    }
    if constexpr (MODE == ETS_COUNT) ets_hist_flush(P, lh, blk.qt * ETS_QT, tid);
    if constexpr (MODE == ETS_RADIUS) ets_sure_flush(P, q, h, lh[tid]);
}

constexpr uint32_t ets_i8_lds(int mode, bool list = false) {
    return ETS_I8_ROWS * ETS_I8_STRIDE + ETS_I8_ROWS * 4u + 2u * ETS_I8_R * 4u + ets_mode_words(mode) * 4u +
           (list ? 4u * ETS_I8_R * 4u : 0u);
}

// ---- the long-row forms (granne_hip_index_screen_long_rows): dense queries, rows of up to ETS_LONG_DIM_MAX ----
// f32 rows of any length up to ETS_LONG_DIM_MAX, walked in chunks of 128 components (brute_force.h's bf_b16_chunked_kernel
// with the screen's epilogues): the accumulators of a tile of 32 R rows stay in registers across the chunks; a chunk of the
// tile goes HBM -> registers -> the two bf16 pieces -> LDS, the next one (of this tile, or the first of the next) being
// fetched before this one's matrix work; a lane reads its half of its query's chunk (64 components) from memory again for
// every tile and splits it in registers -- from L2: 16 KB per wave and chunk against 12 R Mflop. What lies past a row's
// or a query's end is zero by predicate: the last chunk of a dim that is no multiple of 128, the last float4 of a dim that
// is no multiple of 4 (the device row is zero padded to 16 bytes), a query row that starts on no 16-byte boundary.
template <int R, int MODE, int SRC = ETS_ALL, bool AFTER = false>
__global__ __launch_bounds__(ETS_THREADS) void ets_b16_long_kernel(const EtsParams P) {
    static_assert(!AFTER || MODE != ETS_RADIUS, "a cursor: top-k");
    extern __shared__ __align__(16) uint8_t smem_ets[];
    constexpr int KG = 8;                           // groups of 8 components per lane half and chunk
    constexpr uint32_t ET = 32u * R;                // rows per tile
    constexpr uint32_t COMPS = ETS_LONG_CHUNK;      // components per chunk
    constexpr uint32_t STRIDE_B = 2u * COMPS + 16u; // bytes per LDS row of one piece: an odd number of 16-byte units
    static_assert(COMPS == 16u * KG, "a lane half holds KG groups of 8");
    uint8_t* tile_hi = smem_ets;
    uint8_t* tile_lo = smem_ets + (size_t)ET * STRIDE_B;
    uint32_t* lh = reinterpret_cast<uint32_t*>(smem_ets + 2u * (size_t)ET * STRIDE_B); // COUNT: [ETS_BUCKETS][ETS_QT]; RADIUS: [ETS_THREADS]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    const EtsBlock blk = ets_block();
    const uint32_t q = blk.qt * ETS_QT + wave * 32u + col;
    const bool qlive = q < P.nq;
    if constexpr (MODE == ETS_COUNT) ets_hist_clear(lh, tid); // (the first chunk's barriers stand between this and the first count)
    const float* qp = reinterpret_cast<const float*>(P.queries) + (size_t)(qlive ? q : 0u) * P.dim;
    const uint32_t nchunks = (P.dim + COMPS - 1u) / COMPS;
    const bool qvec_ok = (P.dim & 3u) == 0u && (reinterpret_cast<uintptr_t>(P.queries) & 15u) == 0u; // every query starts on 16 bytes
    EtsFloor F;
    F.init<MODE, AFTER>(P, q, qlive);
    if constexpr (MODE == ETS_RADIUS) lh[tid] = 0u; // the thread's rows with s >= hi over the whole range (and ETS_SURE_FULL)

    const uint64_t r0 = (uint64_t)blk.range * P.per_range;
    const uint64_t r1 = r0 + P.per_range < P.n ? r0 + P.per_range : P.n;
    const uint32_t row_f4 = P.row_bytes / 16u; // float4 units of a device row that hold data
    constexpr uint32_t UNITS = COMPS / 4u;     // float4 units per row and chunk: a thread keeps its column, rows 16 apart
    constexpr uint32_t NPF = ET * UNITS / ETS_THREADS;
    static_assert(UNITS == 32u && ETS_THREADS % UNITS == 0u, "unit tid + 512 j: row tid / 32 + 16 j, column tid % 32");
    const uint32_t my_row = tid / UNITS, my_c4 = tid % UNITS;
    float4 pf[NPF]; // the next chunk, on its way from memory while this one is scored
    auto fetch = [&](uint64_t e0, uint32_t c) {
        const uint32_t c4 = c * UNITS + my_c4;
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) {
            const uint64_t row = e0 + my_row + (ETS_THREADS / UNITS) * j;
            pf[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row < r1 && c4 < row_f4) {
                uint64_t id = row;
                if constexpr (SRC == ETS_LIST) id = P.list[id];
                pf[j] = *reinterpret_cast<const float4*>(P.elements + id * P.row_stride + (size_t)c4 * 16u);
            }
        }
    };
    if (r0 < r1) fetch(r0, 0u);
    for (uint64_t e0 = r0; e0 < r1; e0 += ET) {
        ets_f32x16 acc[R]; // the tile's scores so far: carried from chunk to chunk
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][v] = 0.0f;
#pragma unroll 1
        for (uint32_t c = 0; c < nchunks; ++c) {
            __syncthreads(); // the previous chunk has been consumed
#pragma unroll
            for (uint32_t j = 0; j < NPF; ++j) { // split into the two pieces on the way to LDS
                const uint32_t row = my_row + (ETS_THREADS / UNITS) * j;
                ets_b16x4 hi, lo;
                const float v[4] = {pf[j].x, pf[j].y, pf[j].z, pf[j].w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    hi[t] = (__bf16)v[t];
                    lo[t] = (__bf16)(v[t] - (float)hi[t]);
                }
                *reinterpret_cast<ets_b16x4*>(tile_hi + (size_t)row * STRIDE_B + my_c4 * 8u) = hi;
                *reinterpret_cast<ets_b16x4*>(tile_lo + (size_t)row * STRIDE_B + my_c4 * 8u) = lo;
            }
            __syncthreads();
            if (c + 1u < nchunks) fetch(e0, c + 1u);
            else if (e0 + ET < r1) fetch(e0 + ET, 0u);
            // the lane's half of its query's chunk as bf16 pieces
            ets_b16x8 qh[KG], ql[KG];
            const bool q_vec = qvec_ok && (c + 1u) * COMPS <= P.dim; // the whole chunk inside the vector, on 16 bytes: 16 loads for 64
#pragma unroll
            for (int g = 0; g < KG; ++g) {
                const uint32_t c0 = c * COMPS + h * 8u * KG + (uint32_t)g * 8u;
                float v8[8];
                if (q_vec) {
                    const float4 a = *reinterpret_cast<const float4*>(qp + c0), b = *reinterpret_cast<const float4*>(qp + c0 + 4u);
                    v8[0] = a.x, v8[1] = a.y, v8[2] = a.z, v8[3] = a.w, v8[4] = b.x, v8[5] = b.y, v8[6] = b.z, v8[7] = b.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v8[j] = c0 + (uint32_t)j < P.dim ? qp[c0 + (uint32_t)j] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float v = qlive ? v8[j] : 0.0f;
                    const __bf16 hi = (__bf16)v;
                    qh[g][j] = hi;
                    ql[g][j] = (__bf16)(v - (float)hi);
                }
            }
            // the fragments of the next (step, block) are read while the matrix cores work on this one
            const size_t off0 = (size_t)col * STRIDE_B + (size_t)h * 16u * KG;
            constexpr int NF = KG * R;
            ets_b16x8 ah[2], al[2];
            ah[0] = *reinterpret_cast<const ets_b16x8*>(tile_hi + off0);
            al[0] = *reinterpret_cast<const ets_b16x8*>(tile_lo + off0);
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int g = i / R, r = i % R;
                if (i + 1 < NF) {
                    const int gn = (i + 1) / R, rn = (i + 1) % R;
                    ah[(i + 1) & 1] = *reinterpret_cast<const ets_b16x8*>(tile_hi + off0 + (size_t)rn * 32u * STRIDE_B + (size_t)gn * 16u);
                    al[(i + 1) & 1] = *reinterpret_cast<const ets_b16x8*>(tile_lo + off0 + (size_t)rn * 32u * STRIDE_B + (size_t)gn * 16u);
                }
                __builtin_amdgcn_sched_barrier(0);
                acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], qh[g], acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i & 1], ql[g], acc[r], 0, 0, 0);
                acc[r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i & 1], qh[g], acc[r], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // result block r as in ets_b16_kernel: one max over the block decides for the wave, then the form's epilogue
        const bool whole = e0 + ET <= r1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float mx = acc[r][0];
#pragma unroll
            for (int v = 1; v < 16; ++v) mx = __builtin_fmaxf(mx, acc[r][v]);
            if (__ballot(mx >= F.thr)) {
                float sc[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) sc[v] = acc[r][v];
                const uint32_t word = ets_word<SRC>(P, q, e0 + (uint32_t)(r * 32), r1, qlive && mx >= F.thr);
                if constexpr (MODE == ETS_RADIUS)
                    ets_radius16<SRC>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, word, lh + tid);
                else
                    ets_take16<MODE, SRC, false, AFTER>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, lh + wave * 32u + col, word);
            }
        }
    }
    if constexpr (MODE == ETS_COUNT) ets_hist_flush(P, lh, blk.qt * ETS_QT, tid);
    if constexpr (MODE == ETS_RADIUS) ets_sure_flush(P, q, h, lh[tid]);
}

constexpr int ETS_B16_LONG_R = 3;
constexpr uint32_t ets_b16_long_lds(int mode) {
    return 2u * (32u * ETS_B16_LONG_R) * (2u * ETS_LONG_CHUNK + 16u) + ets_mode_words(mode) * 4u; // tile_hi, tile_lo, the mode's words
}

// int8 rows of up to ETS_LONG_DIM_MAX bytes (device rows of more than 128 bytes are zero padded to a multiple of 128),
// walked in chunks of 128 bytes: i32 accumulators carried across the chunks, the score ets_i8_kernel's expression. A chunk
// of the tile is a plain staged copy, HBM -> registers -> LDS, into one of TWO chunk buffers: a chunk is a sixth of the
// matrix work a barrier pair of ets_b16_long_kernel encloses, so the second barrier is spared -- the buffer written now was
// last read two chunks ago, before the barrier every wave has passed since. The rows' 1 / |x| and the blocks' bounds travel
// with a tile's first chunk into the copy of the tile's parity: the epilogue of the tile before may still be reading the other.
// A lane reads its 16-byte groups of its query's chunk from memory for every tile; 1 / |q| is summed over all chunks first.
template <int MODE, int SRC = ETS_ALL, bool AFTER = false>
__global__ __launch_bounds__(ETS_THREADS) void ets_i8_long_kernel(const EtsParams P) {
    static_assert(!AFTER || MODE != ETS_RADIUS, "a cursor: top-k");
    extern __shared__ __align__(16) uint8_t smem_ets[];
    constexpr int R = (int)ETS_I8_R;
    constexpr uint32_t ET = ETS_I8_ROWS, STRIDE = ETS_I8_STRIDE, CHUNK = ETS_LONG_CHUNK;
    uint8_t* tile = smem_ets;                                                    // [2][ET][STRIDE], by the chunk's parity
    float* inv = reinterpret_cast<float*>(smem_ets + 2u * (size_t)ET * STRIDE); // [2][ET] 1 / |x|, by the tile's parity
    float* gms = inv + 2u * ET;                                                  // [2][2][R] inv_gmax of the tile's blocks, by lane half
    uint32_t* lh = reinterpret_cast<uint32_t*>(gms + 4 * R);                     // COUNT: [ETS_BUCKETS][ETS_QT]; RADIUS: [ETS_THREADS]
    uint32_t* gml = lh + ets_mode_words(MODE);                                   // ETS_LIST: [2][2][R] float bits, by the tile's parity
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t col = lane & 31u, h = lane >> 5;
    const EtsBlock blk = ets_block();
    const uint32_t q = blk.qt * ETS_QT + wave * 32u + col;
    const bool qlive = q < P.nq;
    if constexpr (MODE == ETS_COUNT) ets_hist_clear(lh, tid);
    if constexpr (SRC == ETS_LIST) {
        if (tid < 4u * R) gml[tid] = 0u;
    }
    // A chunk has its one barrier AFTER its staging, so the first tile's maxima (atomicMax into gml, by every wave) are
    // raised before any barrier of the loop: this one stands between the clearing above and them.
    __syncthreads();
    const uint8_t* qp = P.queries + (size_t)(qlive ? q : 0u) * P.dim;
    const uint32_t nchunks = (P.dim + CHUNK - 1u) / CHUNK; // at least 2: the form is for rows of more than 128 bytes
    const bool qvec_ok = (P.dim & 15u) == 0u && (reinterpret_cast<uintptr_t>(P.queries) & 15u) == 0u; // every group whole, on 16 bytes
    // bytes 128 c + 32 g + 16 h .. + 15 of the query (ets_i8_kernel's operand), zero past its end
    auto load_q = [&](uint32_t c, ets_i32x4 (&qr)[4]) {
        if (qvec_ok) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint32_t off = c * CHUNK + (uint32_t)g * 32u + h * 16u;
                qr[g] = ets_i32x4{0, 0, 0, 0};
                if (qlive && off < P.dim) qr[g] = *reinterpret_cast<const ets_i32x4*>(qp + off);
            }
        } else {
            const uint32_t last = P.dim - 1u;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const uint32_t cc = c * CHUNK + (uint32_t)g * 32u + h * 16u + (uint32_t)w * 4u + (uint32_t)b;
                        const uint32_t raw = qp[cc < last ? cc : last];
                        const uint32_t keep = (qlive && cc < P.dim) ? 0xFFu : 0u;
                        v |= (raw & keep) << (8 * b);
                    }
                    qr[g][w] = (int)v;
                }
            }
        }
    };
    float qinv = 0.0f;
    {
        int dy = 0;
#pragma unroll 1
        for (uint32_t c = 0; c < nchunks; ++c) {
            ets_i32x4 qr[4];
            load_q(c, qr);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int w = 0; w < 4; ++w) dy = dot4_i8((uint32_t)qr[g][w], (uint32_t)qr[g][w], dy);
        }
        dy += __shfl_xor(dy, 32, 64); // the other half of every chunk
        qinv = dy > 0 ? 1.0f / __builtin_sqrtf((float)dy) : 0.0f;
    }
    EtsFloor F;
    F.init<MODE, AFTER>(P, q, qlive);
    if constexpr (MODE == ETS_RADIUS) lh[tid] = 0u; // the thread's rows with s >= hi over the whole range (and ETS_SURE_FULL)

    const uint64_t r0 = (uint64_t)blk.range * P.per_range;
    const uint64_t r1 = r0 + P.per_range < P.n ? r0 + P.per_range : P.n;
    // 8 threads per row and chunk (16 bytes each): 64 rows per round
    constexpr uint32_t NPF = ET * 8u / ETS_THREADS;
    const uint32_t my_row = tid >> 3, my_c = tid & 7u;
    uint4 pf[NPF];
    float pfn[NPF], pfg = 0.0f; // (of a tile's first chunk)
    auto fetch = [&](uint64_t e0, uint32_t c) {
        const uint32_t off = c * CHUNK + my_c * 16u;
        if constexpr (SRC != ETS_LIST) {
            if (c == 0u && tid < 2u * R) pfg = e0 + 32u * (tid >> 1) < r1 ? P.inv_gmax[((e0 >> 5) + (tid >> 1)) * 2u + (tid & 1u)] : 0.0f;
        }
#pragma unroll
        for (uint32_t j = 0; j < NPF; ++j) {
            const uint64_t row = e0 + my_row + (ETS_THREADS / 8u) * j;
            pf[j] = make_uint4(0, 0, 0, 0);
            uint64_t id = row;
            if constexpr (SRC == ETS_LIST) id = row < r1 ? P.list[row] : 0u;
            if (row < r1 && off < P.row_bytes) pf[j] = *reinterpret_cast<const uint4*>(P.elements + id * P.row_stride + off);
            if (c == 0u) pfn[j] = (row < r1 && my_c == 0u) ? P.inv_norm[id] : 0.0f;
        }
    };
    if (r0 < r1) fetch(r0, 0u);
    uint32_t par = 0, buf = 0; // the tile's parity (inv, gms, gml) and the chunk's (tile)
    for (uint64_t e0 = r0; e0 < r1; e0 += ET, par ^= 1u) {
        float* const inv_t = inv + par * ET;
        const float* gm = gms + par * 2u * R;
        ets_i32x16 acc[R]; // the tile's dots so far: carried from chunk to chunk
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[r][v] = 0;
#pragma unroll 1
        for (uint32_t c = 0; c < nchunks; ++c, buf ^= 1u) {
            uint8_t* const t = tile + (size_t)buf * ET * STRIDE;
#pragma unroll
            for (uint32_t j = 0; j < NPF; ++j) {
                const uint32_t row = my_row + (ETS_THREADS / 8u) * j;
                *reinterpret_cast<uint4*>(t + (size_t)row * STRIDE + my_c * 16u) = pf[j];
                if (c == 0u && my_c == 0u) {
                    inv_t[row] = pfn[j];
                    if constexpr (SRC == ETS_LIST) // row = 32 r + 8 g4 + 4 h + t: non-negative floats order as their bits
                        atomicMax(gml + par * 2u * R + (row >> 2 & 1u) * R + (row >> 5), __float_as_uint(pfn[j]));
                }
            }
            if constexpr (SRC != ETS_LIST) {
                if (c == 0u && tid < 2u * R) gms[par * 2u * R + (tid & 1u) * R + (tid >> 1)] = pfg;
            }
            __syncthreads(); // the one barrier of a chunk
            if constexpr (SRC == ETS_LIST) {
                gm = reinterpret_cast<const float*>(gml + par * 2u * R);
                // the next tile's copy: last read before this barrier, next raised after this tile's second one
                if (c == 0u && tid < 2u * R) gml[(par ^ 1u) * 2u * R + tid] = 0u;
            }
            if (c + 1u < nchunks) fetch(e0, c + 1u);
            else if (e0 + ET < r1) fetch(e0 + ET, 0u);
            ets_i32x4 qr[4];
            load_q(c, qr);
            ets_i32x4 afrag[2][R];
#pragma unroll
            for (int r = 0; r < R; ++r) afrag[0][r] = *reinterpret_cast<const ets_i32x4*>(t + (size_t)(r * 32 + col) * STRIDE + h * 16);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g + 1 < 4) {
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        afrag[(g + 1) & 1][r] = *reinterpret_cast<const ets_i32x4*>(t + (size_t)(r * 32 + col) * STRIDE + (g + 1) * 32 + h * 16);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_mfma_i32_32x32x32_i8(afrag[g & 1][r], qr[g], acc[r], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ets_i8_kernel's block test and scores: the conversion of a dot beyond 2^24 rounds, monotonely, so the largest dot
        // times the largest 1 / |x| still bounds the block's scores from above
        const bool whole = e0 + ET <= r1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            int im = 0;
#pragma unroll
            for (int v = 0; v < 16; ++v) im = max(im, acc[r][v]);
            const bool hit = ((float)im * gm[h * R + r]) * qinv >= F.thr;
            if (!__ballot(hit)) continue;
            float sc[16];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) { // rows r*32 + 8*g4 + 4*h + 0..3: their 1 / |x| in one read
                const float4 iv = *reinterpret_cast<const float4*>(inv_t + r * 32 + 8 * g4 + 4 * h);
                sc[g4 * 4 + 0] = ((float)acc[r][g4 * 4 + 0] * iv.x) * qinv;
                sc[g4 * 4 + 1] = ((float)acc[r][g4 * 4 + 1] * iv.y) * qinv;
                sc[g4 * 4 + 2] = ((float)acc[r][g4 * 4 + 2] * iv.z) * qinv;
                sc[g4 * 4 + 3] = ((float)acc[r][g4 * 4 + 3] * iv.w) * qinv;
            }
            const uint32_t word = ets_word<SRC>(P, q, e0 + (uint32_t)(r * 32), r1, qlive && hit);
            if constexpr (MODE == ETS_RADIUS)
                ets_radius16<SRC>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, word, lh + tid);
            else
                ets_take16<MODE, SRC, false, AFTER>(P, F, sc, e0 + (uint32_t)(r * 32), r1, whole, q, col, h, lh + wave * 32u + col, word);
        }
    }
    if constexpr (MODE == ETS_COUNT) ets_hist_flush(P, lh, blk.qt * ETS_QT, tid);
    if constexpr (MODE == ETS_RADIUS) ets_sure_flush(P, q, h, lh[tid]);
}

constexpr uint32_t ets_i8_long_lds(int mode, bool list = false) {
    return 2u * ETS_I8_ROWS * ETS_I8_STRIDE + 2u * ETS_I8_ROWS * 4u + 4u * ETS_I8_R * 4u + ets_mode_words(mode) * 4u +
           (list ? 4u * ETS_I8_R * 4u : 0u);
}

__global__ void ets_clear_kernel(uint32_t* p, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0u;
}

// f32 handles, once per index: the largest squared norm of a row, as the bits of a non-negative float (a NaN's bits lie
// above +inf's: it fails the test it is held to). Eight lanes per row.
__global__ void ets_max_norm2_kernel(const uint8_t* __restrict__ elements, uint64_t n, uint32_t row_bytes, uint32_t row_stride,
                                                     uint32_t* __restrict__ out) {
    const uint32_t c = threadIdx.x & 7u, units = row_bytes / 16u;
    float worst = 0.0f;
    uint32_t nan = 0;
    for (uint64_t row = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; row < ((n + 7u) & ~7ull); row += ((uint64_t)gridDim.x * blockDim.x) >> 3) {
        float s = 0.0f;
        for (uint32_t u = c; u < units; u += 8u) {
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row < n) v = *reinterpret_cast<const float4*>(elements + row * row_stride + (size_t)u * 16u);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        nan |= s != s ? 1u : 0u;
        worst = __builtin_fmaxf(worst, s);
    }
    if (c == 0u && (worst > 0.0f || nan)) atomicMax(out, nan ? 0x7FC00000u : __float_as_uint(worst));
}

// Per query of a round, before its first pass: the floor's start (+inf: an f32 query outside the norm bound, which takes no
// part in the screen), its histogram and its candidate count cleared.
template <bool I8>
__global__ void ets_init_kernel(const uint8_t* __restrict__ queries, uint32_t nq, uint32_t dim, float* __restrict__ lo,
                                                uint32_t* __restrict__ hist, uint32_t* __restrict__ cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    bool ok = true;
    if constexpr (!I8) {
        if (queries) { // (null: the queries are the handle's rows, ETS_Q_ROWS, which its verdict covers)
            const float* qp = reinterpret_cast<const float*>(queries) + (size_t)q * dim;
            float s = 0.0f;
            for (uint32_t c = 0; c < dim; ++c) s += qp[c] * qp[c];
            ok = s <= ets_norm2_test(dim); // (false for a NaN)
        }
    }
    lo[q] = ok ? ETS_LO0 : __builtin_inff();
    for (uint32_t j = 0; j < ETS_BUCKETS; ++j) hist[(size_t)q * ETS_BUCKETS + j] = 0u;
    cnt[q] = 0u;
}

// One wave per query after a COUNT pass: lane j holds bucket j. The floor rises to the highest edge with k rows at or
// above it; fewer than k rows counted in all (a set of fewer than k rows): it stays. The histogram is left cleared.
__global__ __launch_bounds__(64) void ets_select_kernel(uint32_t* __restrict__ hist, uint32_t k, float* __restrict__ lo) {
    static_assert(ETS_BUCKETS == 64u, "one bucket per lane");
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t c = hist[(size_t)q * ETS_BUCKETS + lane];
    hist[(size_t)q * ETS_BUCKETS + lane] = 0u;
    uint32_t above = 0; // rows in the buckets lane .. 63
    for (uint32_t j = 0; j < ETS_BUCKETS; ++j) {
        const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)j);
        above += j >= lane ? o : 0u;
    }
    const uint64_t have = __ballot(above >= k);
    if (lane == 0u && have != 0ull) {
        const float l = lo[q];
        if (l < 1.0f) lo[q] = ets_edge(l, ets_width(l), 63 - __builtin_clzll(have));
    }
}

// One block per query of a round, after the collecting pass: the places of its list past the count get an id that no
// handle has (dists_kernel answers +inf for it); a query with more than ETS_CAP candidates, or a floor of +inf, goes to
// the fallback list and is voided for et_rank_kernel (its row is written again by ets_scatter_kernel). q_base: the
// round's first query among the call's.
__global__ __launch_bounds__(256) void ets_pad_kernel(uint32_t* __restrict__ cand, const uint32_t* __restrict__ cnt, const float* __restrict__ lo,
                                                      uint32_t q_base, uint32_t* __restrict__ sel, uint32_t* fb_count, uint32_t* fb_list,
                                                      uint32_t* status) {
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = cnt[q];
    const bool screened = lo[q] < 1.0f;
    const bool fallback = !screened || m > ETS_CAP;
    for (uint32_t i = (fallback ? 0u : m) + tid; i < ETS_CAP; i += 256u) cand[(size_t)q * ETS_CAP + i] = 0xFFFFFFFFu;
    if (tid == 0u) {
        sel[4u * q + 0u] = 0u, sel[4u * q + 1u] = 0u, sel[4u * q + 2u] = 0u, sel[4u * q + 3u] = fallback ? 1u : 0u;
        if (status && screened) atomicMax(status + 2, m);
        if (fallback) {
            fb_list[atomicAdd(fb_count, 1u)] = q_base + q;
            if (status) atomicAdd(status + 0, 1u);
        }
    }
}

// the candidates' keys for et_rank_kernel: distance bits << 32 | id
__global__ void ets_keys_kernel(const uint32_t* __restrict__ cand, const float* __restrict__ dists, const uint32_t* __restrict__ cnt,
                                uint32_t nq, uint64_t* __restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)nq * ETS_CAP; i += (uint64_t)gridDim.x * blockDim.x)
        if ((uint32_t)(i & (ETS_CAP - 1u)) < cnt[i / ETS_CAP]) keys[i] = (uint64_t)__float_as_uint(dists[i]) << 32 | (uint64_t)cand[i];
}

// ---- the cursor forms of the three small kernels (granne_hip_exact_topk_screened_after*) ----
// ets_init_kernel with a cursor (after_dists[q], after_ids[q]; an id of all-ones: none). With the bound eps a score places
// a row before any exact arithmetic:
//   top_sure = 1 - d_after - eps rounded down: s < top_sure has d > d_after -- SURELY after the cursor, whatever its id;
//   top_any  = 1 - d_after + eps rounded up:   s > top_any  has d < d_after -- surely before it, dropped;
// what lies between is the band, which only dists_kernel and et_past decide. Both are made in double and rounded outward,
// as ets_radius_kernel makes lo and hi. d_after = 0: the reference clamps its distances at 0, so a score above 1 + eps is
// a row AT distance 0, not before it -- top_any = +inf, nothing is dropped. No cursor: both are +inf, and every kernel
// computes what it computes without one. A cursor distance that is no distance of this metric (its bits above 2.0f's: a
// sign, a NaN, +inf, beyond 2) gets no screen: lo = +inf, the query goes to exact_topk's scan, which compares bits.
template <bool I8>
__global__ void ets_init_after_kernel(const uint8_t* __restrict__ queries, uint32_t nq, uint32_t dim, float eps, const float* __restrict__ after_dists,
                                      const uint64_t* __restrict__ after_ids, float* __restrict__ lo, float* __restrict__ top_sure,
                                      float* __restrict__ top_any, uint32_t* __restrict__ hist, uint32_t* __restrict__ cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    bool ok = true;
    if constexpr (!I8) {
        const float* qp = reinterpret_cast<const float*>(queries) + (size_t)q * dim;
        float s = 0.0f;
        for (uint32_t c = 0; c < dim; ++c) s += qp[c] * qp[c];
        ok = s <= ets_norm2_test(dim); // (false for a NaN)
    }
    float ts = __builtin_inff(), ta = __builtin_inff();
    if (after_ids[q] != ~0ull) {
        const float d = after_dists[q];
        if (__float_as_uint(d) > __float_as_uint(2.0f)) ok = false;
        else {
            const double dl = 1.0 - (double)d - (double)eps, du = 1.0 - (double)d + (double)eps;
            ts = (float)dl;
            if ((double)ts > dl) ts = nextafterf(ts, -__builtin_inff());
            if (d > 0.0f) {
                ta = (float)du;
                if ((double)ta < du) ta = nextafterf(ta, __builtin_inff());
            }
        }
    }
    lo[q] = ok ? ETS_LO0 : __builtin_inff();
    top_sure[q] = ts, top_any[q] = ta;
    for (uint32_t j = 0; j < ETS_BUCKETS; ++j) hist[(size_t)q * ETS_BUCKETS + j] = 0u;
    cnt[q] = 0u;
}
// ets_select_kernel over buckets that end at min(1, top_sure): the histogram holds sure rows only, so the k witnesses of the
// new floor are all beyond the cursor, whatever the band holds. The edge is ets_take16's expression.
__global__ __launch_bounds__(64) void ets_select_after_kernel(uint32_t* __restrict__ hist, uint32_t k, float* __restrict__ lo,
                                                              const float* __restrict__ top_sure) {
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t c = hist[(size_t)q * ETS_BUCKETS + lane];
    hist[(size_t)q * ETS_BUCKETS + lane] = 0u;
    uint32_t above = 0; // rows in the buckets lane .. 63
    for (uint32_t j = 0; j < ETS_BUCKETS; ++j) {
        const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)c, (int)j);
        above += j >= lane ? o : 0u;
    }
    const uint64_t have = __ballot(above >= k);
    if (lane == 0u && have != 0ull) {
        const float l = lo[q];
        if (l < 1.0f) lo[q] = ets_edge(l, ets_width_top(l, top_sure[q]), 63 - __builtin_clzll(have));
    }
}
// ets_keys_kernel with the cursor, one block per query: only the candidates BEYOND the cursor get a key -- a band row the
// exact arithmetic puts at or before it gets none -- dense in keys[q] in any order (et_rank_kernel sorts them), as
// ers_keys_kernel keeps the rows within a radius; cnt[q] becomes their number. A query on the fallback list (cnt beyond
// ETS_CAP, or no screen: voided for et_rank_kernel) keeps its count.
__global__ __launch_bounds__(256) void ets_keys_after_kernel(const uint32_t* __restrict__ cand, const float* __restrict__ dists, uint32_t* __restrict__ cnt,
                                                             const float* __restrict__ after_dists, const uint64_t* __restrict__ after_ids,
                                                             uint64_t* __restrict__ keys) {
    __shared__ uint32_t n_keys;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t m = cnt[q];
    const uint64_t from = et_from(after_dists[q], after_ids[q]);
    if (tid == 0u) n_keys = 0u;
    __syncthreads(); // (every thread has read cnt[q])
    if (m > ETS_CAP) return;
    for (uint32_t i = tid; i < m; i += 256u) {
        const size_t at = (size_t)q * ETS_CAP + i;
        if (et_past(dists[at], cand[at], from)) keys[(size_t)q * ETS_CAP + atomicAdd(&n_keys, 1u)] = (uint64_t)__float_as_uint(dists[at]) << 32 | (uint64_t)cand[at];
    }
    __syncthreads();
    if (tid == 0u) cnt[q] = n_keys;
}

// the fallback: the listed queries, dense, for exact_topk's scan -- and its answers back into their places
__global__ void ets_gather_kernel(const uint8_t* __restrict__ queries, uint32_t qbytes, const uint32_t* __restrict__ fb_list,
                                                  uint32_t nfb, uint8_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)nfb * qbytes; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(i / qbytes), b = (uint32_t)(i - (uint64_t)f * qbytes);
        out[i] = queries[(size_t)fb_list[f] * qbytes + b];
    }
}
__global__ void ets_scatter_kernel(const uint32_t* __restrict__ fb_list, uint32_t nfb, uint32_t k, const uint64_t* __restrict__ ids,
                                                   const float* __restrict__ dists, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ xs,
                                                   uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* status) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)nfb * k; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(i / k), j = (uint32_t)(i - (uint64_t)f * k);
        const size_t q = fb_list[f];
        out_ids[q * k + j] = ids[i];
        out_dists[q * k + j] = dists[i];
        if (j == 0u) out_counts[q] = counts[f];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && status && xs[0]) atomicOr(status + 3, ETS_VOIDED);
}
// a filter that allows nothing: every query's answer is empty
__global__ void ets_empty_kernel(uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)nq * k; i += (uint64_t)gridDim.x * blockDim.x) {
        out_ids[i] = 0xFFFFFFFFFFFFFFFFull;
        out_dists[i] = __builtin_inff();
        if (i < nq) out_counts[i] = 0u; // (k >= 1)
    }
}
// the status words of a call: [1] queries routed by their shape, [3] the form
__global__ void ets_status_kernel(uint32_t* status, uint32_t routed, uint32_t form, const uint32_t* xs) {
    atomicAdd(status + 1, routed);
    atomicOr(status + 3, form | (xs && xs[0] ? ETS_VOIDED : 0u));
}

// ---- the handle's own rows as queries ----
// ets_gather_kernel's sibling: the rows first + p, p = list[f] or p_base + f, dense for exact_topk's scan.
// `allowed` (graph_filtered_host.h; null everywhere else, and in the three kernels below that take it): a filter's id list
// -- first + p is then a POSITION of it, and the element is the id at that position.
__device__ __forceinline__ uint64_t ets_element(const uint32_t* __restrict__ allowed, uint64_t x) { return allowed ? allowed[x] : x; }
__global__ void ets_gather_rows_kernel(const uint8_t* __restrict__ elements, uint32_t row_stride, uint32_t qbytes, uint64_t first,
                                       const uint32_t* __restrict__ list, uint32_t p_base, uint32_t m, uint8_t* __restrict__ out,
                                       const uint32_t* __restrict__ allowed) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (uint64_t)m * qbytes; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(i / qbytes), b = (uint32_t)(i - (uint64_t)f * qbytes);
        out[i] = elements[ets_element(allowed, first + (list ? list[f] : p_base + f)) * row_stride + b];
    }
}
// the elements of the window [first, first + count) of a filter's id list, widened (granne_hip_*_graph_filtered's out_elements)
__global__ void gf_elements_kernel(const uint32_t* __restrict__ allowed, uint64_t first, uint32_t count, uint64_t* __restrict__ out) {
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < count; p += gridDim.x * blockDim.x) out[p] = allowed[first + p];
}
// One block per row f of a scan with k + 1: element e = first + p among its own k + 1 nearest is dropped where it is listed
// (at `at`, found by the block), the last entry where it is not (more than k bit-copies with smaller ids); the k entries,
// the places past the count padded, and the count go to place p. A voided answer (count 0) stays empty.
__global__ __launch_bounds__(256) void kg_drop_self_kernel(uint64_t first, const uint32_t* __restrict__ list, uint32_t p_base, uint32_t k,
                                                           const uint64_t* __restrict__ ids, const float* __restrict__ dists,
                                                           const uint32_t* __restrict__ counts, uint64_t* __restrict__ out_ids,
                                                           float* __restrict__ out_dists, uint32_t* __restrict__ out_counts,
                                                           const uint32_t* __restrict__ allowed) {
    __shared__ uint32_t at;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const size_t p = list ? list[f] : p_base + f;
    const uint64_t e = ets_element(allowed, first + p);
    const uint32_t c = counts[f] <= k + 1u ? counts[f] : k + 1u;
    const uint64_t* const in_ids = ids + (size_t)f * (k + 1u);
    const float* const in_dists = dists + (size_t)f * (k + 1u);
    if (tid == 0u) at = c ? c - 1u : 0u;
    __syncthreads();
    for (uint32_t j = tid; j < c; j += 256u)
        if (in_ids[j] == e) at = j; // (an id is listed once)
    __syncthreads();
    const uint32_t drop = at, count = c ? c - 1u : 0u;
    for (uint32_t j = tid; j < k; j += 256u) {
        const uint32_t src = j < drop ? j : j + 1u;
        out_ids[p * k + j] = j < count ? in_ids[src] : 0xFFFFFFFFFFFFFFFFull;
        out_dists[p * k + j] = j < count ? in_dists[src] : __builtin_inff();
    }
    if (tid == 0u) out_counts[p] = count;
}

// ---- the radius scan's small kernels ----
// Per query of a round, in ets_init_kernel's place: the thresholds of its radius, made in double and rounded outward,
//   lo = 1 - r - eps rounded down: every row with d <= r scores s >= lo;  hi = 1 - r + eps rounded up: s >= hi has d <= r.
// r < 0 or NaN: no distance is within it (distances are clamped at 0): lo = hi = +inf, nothing passes, the answer is
// empty. r = +inf: lo = hi = -inf, every row is sure. An f32 query outside the norm bound: lo = +inf, hi = -inf (the only
// way hi < lo comes about), for exact_range's own scan. The query's three counters are cleared.
template <bool I8>
__global__ void ets_radius_kernel(const uint8_t* __restrict__ queries, const float* __restrict__ radii, uint32_t nq, uint32_t dim, float eps,
                                  float* __restrict__ lo, float* __restrict__ hi, uint32_t* __restrict__ sure, uint32_t* __restrict__ cnt,
                                  uint32_t* __restrict__ bcnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    bool ok = true;
    if constexpr (!I8) {
        if (queries) { // (null: the queries are the handle's rows, ETS_Q_ROWS, which its verdict covers, as in ets_init_kernel)
            const float* qp = reinterpret_cast<const float*>(queries) + (size_t)q * dim;
            float s = 0.0f;
            for (uint32_t c = 0; c < dim; ++c) s += qp[c] * qp[c];
            ok = s <= ets_norm2_test(dim); // (false for a NaN)
        }
    }
    const float r = radii[q];
    float l = __builtin_inff(), u = ok ? __builtin_inff() : -__builtin_inff();
    if (ok && r >= 0.0f) { // (false for a NaN)
        const double dl = 1.0 - (double)r - (double)eps, du = 1.0 - (double)r + (double)eps;
        l = (float)dl, u = (float)du;
        if ((double)l > dl) l = nextafterf(l, -__builtin_inff());
        if ((double)u < du) u = nextafterf(u, __builtin_inff());
        // Rows as queries (range_graph_host.h): the score of a row with itself is -inf, and -inf >= -inf would let r = +inf
        // admit it. No threshold goes below ETS_LO0: every real score is above it, so nothing else changes.
        if (!queries) l = __builtin_fmaxf(l, ETS_LO0), u = __builtin_fmaxf(u, ETS_LO0);
    }
    lo[q] = l, hi[q] = u;
    sure[q] = 0u, cnt[q] = 0u, bcnt[q] = 0u;
}

// One block per query of a round, before dists_kernel: the places of both lists past their counts get an id that no
// handle has. A list that ran over (or a query outside the bound) is not read afterwards: all of it is padded. `list`
// (ETS_LIST, else null): the scan listed positions of it; they become the ids at those positions.
__global__ __launch_bounds__(256) void ers_pad_kernel(uint32_t* __restrict__ cand, const uint32_t* __restrict__ sure, const uint32_t* __restrict__ bcnt,
                                                      const uint32_t* __restrict__ list) {
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t S = sure[q] <= ETS_CAP ? sure[q] : 0u, B = bcnt[q] <= ETS_CAP ? bcnt[q] : 0u;
    uint32_t* const mine = cand + (size_t)q * (2u * ETS_CAP);
    for (uint32_t i = tid; i < ETS_CAP; i += 256u) {
        if (i >= S) mine[i] = 0xFFFFFFFFu;
        else if (list) mine[i] = list[mine[i]];
        if (i >= B) mine[ETS_CAP + i] = 0xFFFFFFFFu;
        else if (list) mine[ETS_CAP + i] = list[mine[ETS_CAP + i]];
    }
}

// One block per query of a round, after dists_kernel has given both lists the reference's distances: the keys (distance
// bits << 32 | id) of the listed rows with d <= r, dense in keys[q] in any order (er_rank_kernel sorts them), and the
// query's path. S sure rows, B band rows, of which b_in lie within r:
//   C  outside the norm bound, or B > ETS_CAP (the band's list ran over)      -> lists.c, totals = ETS_CAP + 1
//   total = S + b_in is exact otherwise (S <= ETS_CAP: the sure list is whole and its rows are counted as keys)
//   A  total <= ETS_CAP: the keys are all of W, totals = total               B  otherwise -> lists.b, totals = total
// status (optional): [1] += 1 unless A, [2] raised to S + B of a query inside the bound.
__global__ __launch_bounds__(256) void ers_keys_kernel(const uint32_t* __restrict__ cand, const float* __restrict__ dists, const float* __restrict__ radii,
                                                       const float* __restrict__ lo, const float* __restrict__ hi, const uint32_t* __restrict__ sure,
                                                       const uint32_t* __restrict__ bcnt, uint32_t q_base, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ totals, ErsLists lists, uint32_t* status) {
    __shared__ uint32_t n_keys, n_band;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t S = sure[q], B = bcnt[q];
    const bool screened = !(hi[q] < lo[q]);
    const float r = radii[q];
    if (tid == 0u) n_keys = 0u, n_band = 0u;
    __syncthreads();
    const uint32_t ns = screened && S <= ETS_CAP ? S : 0u, nb = screened && B <= ETS_CAP ? B : 0u;
    const size_t base = (size_t)q * (2u * ETS_CAP);
    for (uint32_t i = tid; i < ns + nb; i += 256u) {
        const size_t at = base + (i < ns ? i : ETS_CAP + (i - ns));
        const float d = dists[at];
        if (d <= r) {
            if (i >= ns) atomicAdd(&n_band, 1u);
            const uint32_t p = atomicAdd(&n_keys, 1u);
            if (p < ETS_CAP) keys[(size_t)q * ETS_CAP + p] = (uint64_t)__float_as_uint(d) << 32 | (uint64_t)cand[at];
        }
    }
    __syncthreads();
    if (tid != 0u) return;
    const bool c = !screened || B > ETS_CAP;
    const uint32_t total = S <= ETS_CAP ? n_keys : S + n_band;
    const bool a = !c && total <= ETS_CAP;
    totals[q] = c ? ETS_CAP + 1u : total;
    if (c) lists.c[atomicAdd(lists.n + 1, 1u)] = q_base + q;
    else if (!a) lists.b[atomicAdd(lists.n + 0, 1u)] = q_base + q;
    if (status) {
        if (!a) atomicAdd(status + 1, 1u);
        if (screened) atomicMax(status + 2, S + B < S ? 0xFFFFFFFFu : S + B);
    }
}

__global__ void ers_voided_kernel(const uint32_t* __restrict__ counts, uint32_t np, uint32_t* status) {
    uint32_t v = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < np; i += gridDim.x * blockDim.x) v += counts[i] == 0u ? 1u : 0u;
    if (v) atomicAdd(status + 0, v), atomicOr(status + 3, ETS_VOIDED);
}
__global__ void ers_status_kernel(uint32_t* status, const uint32_t* xs, uint32_t not_a, uint32_t form) {
    if (xs && xs[0]) atomicAdd(status + 0, xs[0]);
    atomicAdd(status + 1, not_a);
    atomicOr(status + 3, form | (xs && xs[0] ? ETS_VOIDED : 0u));
}

// ---- every element's neighbours within a radius (range_graph_host.h) ----
// The elements exact_range's own scan answers (path C, routed handles), a round of them: element first + p, p = list[f] or
// p_base + f, gets its id as the one candidate of dists_kernel -- d(e, e) in the reference's arithmetic -- and its radius
// dense beside its gathered row.
__global__ void rg_self_kernel(uint64_t first, const uint32_t* __restrict__ list, uint32_t p_base, uint32_t m, const float* __restrict__ radii,
                               uint32_t* __restrict__ self_ids, float* __restrict__ out_radii, const uint32_t* __restrict__ allowed) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m) return;
    const uint32_t p = list ? list[f] : p_base + f;
    self_ids[f] = (uint32_t)ets_element(allowed, first + p);
    out_radii[f] = radii[p];
}
// kg_drop_self_kernel's rule with a radius. One block per row f of exact_range's answer for cap + 1 ([m][cap + 1], counts,
// totals): element e = first + p was counted by that scan exactly when self[f] = d(e, e) <= r (the scan's own compare; false
// for a NaN radius), and then the total drops by one. e is dropped from the listing where it is listed (at `at`, found by
// the block); where it is not and the listing is full (cap + 1 entries, all of them others that come before e or e outside
// the radius) the last entry is; a shorter listing without e is whole. A voided answer (count 0) stays empty.
__global__ __launch_bounds__(256) void rg_drop_self_kernel(uint64_t first, const uint32_t* __restrict__ list, uint32_t p_base, uint32_t cap,
                                                           const uint64_t* __restrict__ ids, const float* __restrict__ dists,
                                                           const uint32_t* __restrict__ counts, const uint32_t* __restrict__ totals,
                                                           const float* __restrict__ self, const float* __restrict__ radii,
                                                           uint64_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                           uint32_t* __restrict__ out_counts, uint32_t* __restrict__ out_totals,
                                                           const uint32_t* __restrict__ allowed) {
    __shared__ uint32_t at;
    const uint32_t f = blockIdx.x, tid = threadIdx.x;
    const size_t p = list ? list[f] : p_base + f;
    const uint64_t e = ets_element(allowed, first + p);
    const uint32_t c = counts[f] <= cap + 1u ? counts[f] : cap + 1u;
    const uint64_t* const in_ids = ids + (size_t)f * (cap + 1u);
    const float* const in_dists = dists + (size_t)f * (cap + 1u);
    if (tid == 0u) at = c == cap + 1u ? cap : 0xFFFFFFFFu;
    __syncthreads();
    for (uint32_t j = tid; j < c; j += 256u)
        if (in_ids[j] == e) at = j; // (an id is listed once)
    __syncthreads();
    const uint32_t drop = at, count = drop < c ? c - 1u : c;
    for (uint32_t j = tid; j < cap; j += 256u) {
        const uint32_t src = j < drop ? j : j + 1u;
        out_ids[p * cap + j] = j < count ? in_ids[src] : 0xFFFFFFFFFFFFFFFFull;
        out_dists[p * cap + j] = j < count ? in_dists[src] : __builtin_inff();
    }
    if (tid == 0u) {
        const bool within = self[f] <= radii[f];
        out_counts[p] = count;
        out_totals[p] = totals[f] - (within && totals[f] ? 1u : 0u);
    }
}

// ---- launchers ----
hipError_t rg_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, const float* radii, uint32_t* self_ids, float* out_radii,
                   hipStream_t s, const uint32_t* allowed) {
    hipLaunchKernelGGL(rg_self_kernel, dim3((m + 255) / 256), dim3(256), 0, s, first, list, p_base, m, radii, self_ids, out_radii, allowed);
    return hipGetLastError();
}
hipError_t rg_drop_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, uint32_t cap, const uint64_t* ids, const float* dists,
                        const uint32_t* counts, const uint32_t* totals, const float* self, const float* radii, uint64_t* out_ids, float* out_dists,
                        uint32_t* out_counts, uint32_t* out_totals, hipStream_t s, const uint32_t* allowed) {
    hipLaunchKernelGGL(rg_drop_self_kernel, dim3(m), dim3(256), 0, s, first, list, p_base, cap, ids, dists, counts, totals, self, radii, out_ids,
                       out_dists, out_counts, out_totals, allowed);
    return hipGetLastError();
}
hipError_t ers_radius(bool i8, const uint8_t* queries, const float* radii, uint32_t nq, uint32_t dim, float eps, float* lo, float* hi,
                      uint32_t* sure, uint32_t* cnt, uint32_t* bcnt, hipStream_t s) {
    hipLaunchKernelGGL(i8 ? ets_radius_kernel<true> : ets_radius_kernel<false>, dim3((nq + 255) / 256), dim3(256), 0, s, queries, radii, nq, dim, eps,
                       lo, hi, sure, cnt, bcnt);
    return hipGetLastError();
}
hipError_t ers_pad(uint32_t* cand, const uint32_t* sure, const uint32_t* bcnt, const uint32_t* list, uint32_t nq, hipStream_t s) {
    hipLaunchKernelGGL(ers_pad_kernel, dim3(nq), dim3(256), 0, s, cand, sure, bcnt, list);
    return hipGetLastError();
}
hipError_t ers_keys(const uint32_t* cand, const float* dists, const float* radii, const float* lo, const float* hi, const uint32_t* sure,
                    const uint32_t* bcnt, uint32_t nq, uint32_t q_base, uint64_t* keys, uint32_t* totals, ErsLists lists, uint32_t* status,
                    hipStream_t s) {
    hipLaunchKernelGGL(ers_keys_kernel, dim3(nq), dim3(256), 0, s, cand, dists, radii, lo, hi, sure, bcnt, q_base, keys, totals, lists, status);
    return hipGetLastError();
}
hipError_t ers_voided(const uint32_t* counts, uint32_t np, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(ers_voided_kernel, dim3((np + 255) / 256 < 64 ? (np + 255) / 256 : 64), dim3(256), 0, s, counts, np, status);
    return hipGetLastError();
}
hipError_t ers_status(uint32_t* status, const uint32_t* xs, uint32_t not_a, uint32_t form, hipStream_t s) {
    hipLaunchKernelGGL(ers_status_kernel, dim3(1), dim3(1), 0, s, status, xs, not_a, form);
    return hipGetLastError();
}

typedef void (*EtsScanFn)(const EtsParams);
static uint32_t ets_grid(uint64_t work) {
    const uint64_t g = (work + 255) / 256;
    return (uint32_t)(g > 8192 ? 8192 : g < 1 ? 1 : g);
}

uint32_t ets_tile_rows(uint32_t form) {
    return form == ETS_FORM_B16_7x4 ? 128u : form == ETS_FORM_B16_13x2 ? 64u : form == ETS_FORM_B16_LONG ? 32u * ETS_B16_LONG_R : ETS_I8_ROWS;
}

template <int MODE, int SRC, int QSRC = ETS_Q_DENSE>
static EtsScanFn ets_scan_fn(uint32_t form, uint32_t* lds) {
    if (form == ETS_FORM_B16_7x4) return *lds = ets_b16_lds<7, 4>(MODE), ets_b16_kernel<7, 4, MODE, SRC, QSRC>;
    if (form == ETS_FORM_B16_13x2) return *lds = ets_b16_lds<13, 2>(MODE), ets_b16_kernel<13, 2, MODE, SRC, QSRC>;
    if (form == ETS_FORM_I8) return *lds = ets_i8_lds(MODE, SRC == ETS_LIST), ets_i8_kernel<MODE, SRC, QSRC>;
    if constexpr (QSRC == ETS_Q_DENSE) { // the long-row forms: dense queries only
        if (form == ETS_FORM_B16_LONG) return *lds = ets_b16_long_lds(MODE), ets_b16_long_kernel<ETS_B16_LONG_R, MODE, SRC>;
        if (form == ETS_FORM_I8_LONG) return *lds = ets_i8_long_lds(MODE, SRC == ETS_LIST), ets_i8_long_kernel<MODE, SRC>;
    }
    return nullptr;
}
template <int MODE>
static EtsScanFn ets_scan_mode(uint32_t form, int src, uint32_t* lds) {
    return src == ETS_ALL    ? ets_scan_fn<MODE, ETS_ALL>(form, lds)
           : src == ETS_LIST ? ets_scan_fn<MODE, ETS_LIST>(form, lds)
           : src == ETS_BITS ? ets_scan_fn<MODE, ETS_BITS>(form, lds)
                             : nullptr;
}
static hipError_t ets_scan_launch(EtsScanFn fn, uint32_t lds, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    if (!fn) return hipErrorInvalidValue;
    if (lds > 64u * 1024u) {
        const hipError_t e = hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(fn, dim3(tiles, ranges), dim3(ETS_THREADS), lds, s, P);
    return hipGetLastError();
}

hipError_t ets_scan(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    return ets_scan_src(form, collect, ETS_ALL, tiles, ranges, P, s);
}
hipError_t ets_scan_src(uint32_t form, bool collect, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    uint32_t lds = 0;
    const EtsScanFn fn = collect ? ets_scan_mode<ETS_COLLECT>(form, src, &lds) : ets_scan_mode<ETS_COUNT>(form, src, &lds);
    return ets_scan_launch(fn, lds, tiles, ranges, P, s);
}
hipError_t ets_scan_rows(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    EtsScanFn fn = nullptr;
    uint32_t lds = 0;
    const int mode = collect ? ETS_COLLECT : ETS_COUNT;
    if (form == ETS_FORM_B16_7x4)
        lds = ets_b16_lds<7, 4>(mode), fn = collect ? ets_b16_kernel<7, 4, ETS_COLLECT, ETS_ALL, ETS_Q_ROWS> : ets_b16_kernel<7, 4, ETS_COUNT, ETS_ALL, ETS_Q_ROWS>;
    else if (form == ETS_FORM_B16_13x2)
        lds = ets_b16_lds<13, 2>(mode), fn = collect ? ets_b16_kernel<13, 2, ETS_COLLECT, ETS_ALL, ETS_Q_ROWS> : ets_b16_kernel<13, 2, ETS_COUNT, ETS_ALL, ETS_Q_ROWS>;
    else if (form == ETS_FORM_I8)
        lds = ets_i8_lds(mode), fn = collect ? ets_i8_kernel<ETS_COLLECT, ETS_ALL, ETS_Q_ROWS> : ets_i8_kernel<ETS_COUNT, ETS_ALL, ETS_Q_ROWS>;
    return ets_scan_launch(fn, lds, tiles, ranges, P, s);
}
// the nine instantiations of ETS_LIST with ETS_Q_ROWS (graph_filtered_host.h): the three forms here with
// COUNT and COLLECT, with RADIUS in ets_scan_radius_rows_list
hipError_t ets_scan_rows_list(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    uint32_t lds = 0;
    const EtsScanFn fn = collect ? ets_scan_fn<ETS_COLLECT, ETS_LIST, ETS_Q_ROWS>(form, &lds) : ets_scan_fn<ETS_COUNT, ETS_LIST, ETS_Q_ROWS>(form, &lds);
    return P.list ? ets_scan_launch(fn, lds, tiles, ranges, P, s) : hipErrorInvalidValue;
}
hipError_t ets_gather_rows(const uint8_t* elements, uint32_t row_stride, uint32_t qbytes, uint64_t first, const uint32_t* list, uint32_t p_base,
                           uint32_t m, uint8_t* out, hipStream_t s, const uint32_t* allowed) {
    hipLaunchKernelGGL(ets_gather_rows_kernel, dim3(ets_grid((uint64_t)m * qbytes)), dim3(256), 0, s, elements, row_stride, qbytes, first, list,
                       p_base, m, out, allowed);
    return hipGetLastError();
}
hipError_t gf_elements(const uint32_t* allowed, uint64_t first, uint32_t count, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(gf_elements_kernel, dim3(ets_grid(count)), dim3(256), 0, s, allowed, first, count, out);
    return hipGetLastError();
}
hipError_t kg_drop_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, uint32_t k, const uint64_t* ids, const float* dists,
                        const uint32_t* counts, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, hipStream_t s, const uint32_t* allowed) {
    hipLaunchKernelGGL(kg_drop_self_kernel, dim3(m), dim3(256), 0, s, first, list, p_base, k, ids, dists, counts, out_ids, out_dists, out_counts,
                       allowed);
    return hipGetLastError();
}
hipError_t ets_scan_radius(uint32_t form, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    uint32_t lds = 0;
    const EtsScanFn fn = ets_scan_mode<ETS_RADIUS>(form, src, &lds);
    return ets_scan_launch(fn, lds, tiles, ranges, P, s);
}
hipError_t ets_scan_radius_rows(uint32_t form, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    EtsScanFn fn = nullptr;
    uint32_t lds = 0;
    if (form == ETS_FORM_B16_7x4) lds = ets_b16_lds<7, 4>(ETS_RADIUS), fn = ets_b16_kernel<7, 4, ETS_RADIUS, ETS_ALL, ETS_Q_ROWS>;
    else if (form == ETS_FORM_B16_13x2) lds = ets_b16_lds<13, 2>(ETS_RADIUS), fn = ets_b16_kernel<13, 2, ETS_RADIUS, ETS_ALL, ETS_Q_ROWS>;
    else if (form == ETS_FORM_I8) lds = ets_i8_lds(ETS_RADIUS), fn = ets_i8_kernel<ETS_RADIUS, ETS_ALL, ETS_Q_ROWS>;
    return ets_scan_launch(fn, lds, tiles, ranges, P, s);
}
hipError_t ets_scan_radius_rows_list(uint32_t form, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    uint32_t lds = 0;
    const EtsScanFn fn = ets_scan_fn<ETS_RADIUS, ETS_LIST, ETS_Q_ROWS>(form, &lds);
    return P.list ? ets_scan_launch(fn, lds, tiles, ranges, P, s) : hipErrorInvalidValue;
}
hipError_t ets_clear(uint32_t* p, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(ets_clear_kernel, dim3(1), dim3(64), 0, s, p, n);
    return hipGetLastError();
}
hipError_t ets_max_norm2(const uint8_t* elements, uint64_t n, uint32_t row_bytes, uint32_t row_stride, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(ets_max_norm2_kernel, dim3(ets_grid(n * 8)), dim3(256), 0, s, elements, n, row_bytes, row_stride, out);
    return hipGetLastError();
}
hipError_t ets_init(bool i8, const uint8_t* queries, uint32_t nq, uint32_t dim, float* lo, uint32_t* hist, uint32_t* cnt, hipStream_t s) {
    hipLaunchKernelGGL(i8 ? ets_init_kernel<true> : ets_init_kernel<false>, dim3((nq + 255) / 256), dim3(256), 0, s, queries, nq, dim, lo, hist, cnt);
    return hipGetLastError();
}
hipError_t ets_select(uint32_t* hist, uint32_t nq, uint32_t k, float* lo, hipStream_t s) {
    hipLaunchKernelGGL(ets_select_kernel, dim3(nq), dim3(64), 0, s, hist, k, lo);
    return hipGetLastError();
}
hipError_t ets_pad(uint32_t* cand, const uint32_t* cnt, const float* lo, uint32_t nq, uint32_t q_base, uint32_t* sel, uint32_t* fb_count,
                   uint32_t* fb_list, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(ets_pad_kernel, dim3(nq), dim3(256), 0, s, cand, cnt, lo, q_base, sel, fb_count, fb_list, status);
    return hipGetLastError();
}
hipError_t ets_keys(const uint32_t* cand, const float* dists, const uint32_t* cnt, uint32_t nq, uint64_t* keys, hipStream_t s) {
    hipLaunchKernelGGL(ets_keys_kernel, dim3(ets_grid((uint64_t)nq * ETS_CAP)), dim3(256), 0, s, cand, dists, cnt, nq, keys);
    return hipGetLastError();
}
hipError_t ets_gather(const uint8_t* queries, uint32_t qbytes, const uint32_t* fb_list, uint32_t nfb, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(ets_gather_kernel, dim3(ets_grid((uint64_t)nfb * qbytes)), dim3(256), 0, s, queries, qbytes, fb_list, nfb, out);
    return hipGetLastError();
}
hipError_t ets_scatter(const uint32_t* fb_list, uint32_t nfb, uint32_t k, const uint64_t* ids, const float* dists, const uint32_t* counts,
                       const uint32_t* xs, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(ets_scatter_kernel, dim3(ets_grid((uint64_t)nfb * k)), dim3(256), 0, s, fb_list, nfb, k, ids, dists, counts, xs, out_ids,
                       out_dists, out_counts, status);
    return hipGetLastError();
}
hipError_t ets_empty(uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, hipStream_t s) {
    hipLaunchKernelGGL(ets_empty_kernel, dim3(ets_grid((uint64_t)nq * k)), dim3(256), 0, s, nq, k, out_ids, out_dists, out_counts);
    return hipGetLastError();
}
// ---- the cursor forms: the five forms x the three row sources x COUNT and COLLECT, dense queries ----
template <int MODE, int SRC>
static EtsScanFn ets_scan_after_fn(uint32_t form, uint32_t* lds) {
    if (form == ETS_FORM_B16_7x4) return *lds = ets_b16_lds<7, 4>(MODE), ets_b16_kernel<7, 4, MODE, SRC, ETS_Q_DENSE, true>;
    if (form == ETS_FORM_B16_13x2) return *lds = ets_b16_lds<13, 2>(MODE), ets_b16_kernel<13, 2, MODE, SRC, ETS_Q_DENSE, true>;
    if (form == ETS_FORM_I8) return *lds = ets_i8_lds(MODE, SRC == ETS_LIST), ets_i8_kernel<MODE, SRC, ETS_Q_DENSE, true>;
    if (form == ETS_FORM_B16_LONG) return *lds = ets_b16_long_lds(MODE), ets_b16_long_kernel<ETS_B16_LONG_R, MODE, SRC, true>;
    if (form == ETS_FORM_I8_LONG) return *lds = ets_i8_long_lds(MODE, SRC == ETS_LIST), ets_i8_long_kernel<MODE, SRC, true>;
    return nullptr;
}
template <int MODE>
static EtsScanFn ets_scan_after_mode(uint32_t form, int src, uint32_t* lds) {
    return src == ETS_ALL    ? ets_scan_after_fn<MODE, ETS_ALL>(form, lds)
           : src == ETS_LIST ? ets_scan_after_fn<MODE, ETS_LIST>(form, lds)
           : src == ETS_BITS ? ets_scan_after_fn<MODE, ETS_BITS>(form, lds)
                             : nullptr;
}
hipError_t ets_scan_after(uint32_t form, bool collect, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s) {
    uint32_t lds = 0;
    const EtsScanFn fn = collect ? ets_scan_after_mode<ETS_COLLECT>(form, src, &lds) : ets_scan_after_mode<ETS_COUNT>(form, src, &lds);
    return P.tops ? ets_scan_launch(fn, lds, tiles, ranges, P, s) : hipErrorInvalidValue;
}
hipError_t ets_init_after(bool i8, const uint8_t* queries, uint32_t nq, uint32_t dim, float eps, const float* after_dists, const uint64_t* after_ids,
                          float* lo, float* top_sure, float* top_any, uint32_t* hist, uint32_t* cnt, hipStream_t s) {
    hipLaunchKernelGGL(i8 ? ets_init_after_kernel<true> : ets_init_after_kernel<false>, dim3((nq + 255) / 256), dim3(256), 0, s, queries, nq, dim,
                       eps, after_dists, after_ids, lo, top_sure, top_any, hist, cnt);
    return hipGetLastError();
}
hipError_t ets_select_after(uint32_t* hist, uint32_t nq, uint32_t k, float* lo, const float* top_sure, hipStream_t s) {
    hipLaunchKernelGGL(ets_select_after_kernel, dim3(nq), dim3(64), 0, s, hist, k, lo, top_sure);
    return hipGetLastError();
}
hipError_t ets_keys_after(const uint32_t* cand, const float* dists, uint32_t* cnt, uint32_t nq, const float* after_dists,
                          const uint64_t* after_ids, uint64_t* keys, hipStream_t s) {
    hipLaunchKernelGGL(ets_keys_after_kernel, dim3(nq), dim3(256), 0, s, cand, dists, cnt, after_dists, after_ids, keys);
    return hipGetLastError();
}

hipError_t ets_status(uint32_t* status, uint32_t routed, uint32_t form, const uint32_t* xs, hipStream_t s) {
    hipLaunchKernelGGL(ets_status_kernel, dim3(1), dim3(1), 0, s, status, routed, form, xs);
    return hipGetLastError();
}

} // namespace granne_hip
