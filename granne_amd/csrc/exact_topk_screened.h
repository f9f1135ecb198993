// exact_topk_screened.h -- exact_topk's answer at matrix-core speed (granne_hip_exact_topk_screened_device; DESIGN.md
// 3.7b). The matrix cores give every (query, row) pair a cheap SCREEN SCORE s; a proven bound eps on |s - r|, r = 1 - the
// reference's distance, turns the score into a screen that no row of the true top-k can fail; only the survivors -- a few
// times k per query -- get the reference's arithmetic (dists_kernel) and exact_topk's (distance bits, id) ranking
// (et_rank_kernel). This header is what the two sides share: the kernels and their launchers are exact_topk_screened.hip
// (a translation unit of its own: it is compiled without the packed f32 instructions), the driver is
// exact_topk_screened_host.h.
//
//   score    f32 rows: every component in two bf16 pieces, x = xh + xl (+ a residual below 2^-18 |x|), a product as three
//            v_mfma_f32_32x32x16_bf16 (xh qh + xh ql + xl qh) accumulated in f32 -- brute_force.h's bf_b16_kernel operand
//            layout: a tile of rows split on its way to LDS, the wave's 32 queries in registers for the whole range, a
//            lane owns one query (column) and sees 16 rows per 32-row block. int8 rows: v_mfma_i32_32x32x32_i8, the exact
//            integer dot, times the row's 1 / |x| (the index's d_inv_norm) times the query's 1 / |q|.
//   bound    ets_epsilon(dtype, dim), derived in DESIGN.md 3.7b, made on the host, passed in. f32: for rows and queries
//            of squared norm at most ETS_NORM2_MAX (prepared rows are; ets_max_norm2_kernel looks once per index,
//            ets_init_kernel at every query) -- a handle or a query outside that is answered by exact_topk's own scan.
//   floor    per query a score `lo` that at least k rows reach; it starts at ETS_LO0, below every score there is. A
//            COUNT pass puts every score >= lo of a prefix of the rows into one of ETS_BUCKETS linear buckets between lo
//            and 1, edge(j) = lo + w j, w = (1 - lo) / 64 -- per (block, query) in LDS (ds_add; [bucket][query], the
//            lanes of a wave on different banks), the non-zero buckets added to the query's global histogram at the end
//            of the block's range. ets_select_kernel raises lo to the highest edge with k rows at or above it: those k
//            rows are rows of every longer prefix. The prefixes are exact_topk's (16 times the one before, the last one
//            all rows; a set of one stage is counted twice, the second time between the first floor and 1).
//   collect  the same kernel, the other epilogue: every row with s >= lo - 2 eps goes to the query's candidate list (u32
//            ids, ETS_CAP of them). Why 2 eps: the k witnesses of lo have r >= lo - eps, so the k-th best r is at least
//            that; a row of the true top-k (ties at the k-th included) has r >= the k-th best, and its own s is within
//            eps of its r. The place in the list: one atomic per (wave, query, 32-row block) that has hits, the lane
//            pair of a query sharing it; the count keeps running past ETS_CAP.
//   rank     ets_pad_kernel closes the lists (unused places: an id no handle has, which dists_kernel answers +inf) and
//            puts a query with more than ETS_CAP candidates, or outside the norm bound, on the fallback list;
//            dists_kernel gives the candidates their distances in the reference's arithmetic, ets_keys_kernel makes the
//            keys (distance bits << 32 | id), et_rank_kernel sorts them and writes the first k.
// Only comparisons against `lo` decide what is counted and collected, and count and select evaluate edge(j) by one
// expression (ets_edge; compiled with -ffp-contract=off): a bucket's count vouches for s >= its edge.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace granne_hip {

constexpr uint32_t ETS_BUCKETS = 64;
constexpr uint32_t ETS_THREADS = 512, ETS_QT = 256; // 8 waves x 32 queries
constexpr uint32_t ETS_CAP = 4096;                  // = ET_CAP: candidates per query
constexpr float ETS_LO0 = -1.25f;                   // below every screen score: |s| <= (1 + 2^-10) + eps
constexpr float ETS_NORM2_MAX = 1.0f + 0x1p-10f;    // f32: the bound holds for |x|^2, |q|^2 up to here
constexpr float ETS_NORM2_TEST = 1.0f + 0x1p-10f - 0x1p-14f; // what an f32 sum of <= 208 squares is held to (its own rounding: 208 x 2^-24)
constexpr uint32_t ETS_F32_DIM_MAX = 208, ETS_I8_DIM_MAX = 128;
enum { ETS_FORM_ROUTED = 0, ETS_FORM_B16_7x4 = 1, ETS_FORM_B16_13x2 = 2, ETS_FORM_I8 = 3, ETS_FORM_B16_LONG = 4, ETS_FORM_I8_LONG = 5 };
// The long-row forms (granne_hip_index_screen_long_rows): rows beyond the register forms' lengths, walked in
// chunks of ETS_LONG_CHUNK components with the tile's accumulators kept across the chunks. Dense queries only.
constexpr uint32_t ETS_LONG_DIM_MAX = 2048, ETS_LONG_CHUNK = 128;
constexpr bool ets_form_long(uint32_t form) { return form == ETS_FORM_B16_LONG || form == ETS_FORM_I8_LONG; }
// What an f32 sum of `dim` squares is held to so that the true sum is at most ETS_NORM2_MAX: the sum's own rounding is at
// most (dim + 4) 2^-24 of it (dim products, dim - 1 additions in any order, the lanes' three). Short rows: ETS_NORM2_TEST,
// bit for bit; long rows: 1 + 2^-10 - dim 2^-23 (exact in f32: both are multiples of 2^-23 in [1, 2)).
__host__ __device__ static inline float ets_norm2_test(uint32_t dim) {
    return dim <= ETS_F32_DIM_MAX ? ETS_NORM2_TEST : (1.0f + 0x1p-10f) - (float)dim * 0x1p-23f;
}
constexpr uint32_t ETS_VOIDED = 0x80000000u; // status[3]: exact_topk's own selection overflowed for a query handed to it
// What a scan runs over (granne_hip_exact_topk_screened_filtered*): all rows; the positions of the id list
// one shared bitmap compacts to; or all rows under a bit test, one bitmap per query -- a 32-row result block is one word of
// it, read only for the blocks that pass the wave's floor test.
enum { ETS_ALL = 0, ETS_LIST = 1, ETS_BITS = 2 };
// The epilogue of a scan: the histogram of the scores at or above the floor; the candidates at or above it; or, for a
// radius (granne_hip_exact_range_screened*), one pass that counts and lists the rows at or above `hi` and
// lists the rows between `lo` and `hi`.
enum { ETS_COUNT = 0, ETS_COLLECT = 1, ETS_RADIUS = 2 };
// Where a scan takes its queries from: the caller's dense matrix; or the handle's own rows (granne_hip_knn_graph*;
// DESIGN.md 3.7e) -- query q of a round is element q_first + q, its fragments are read from the row where it lies, and the
// score of a row with itself is replaced by -inf before anything looks at it: an element is no witness of its own floor.
enum { ETS_Q_DENSE = 0, ETS_Q_ROWS = 1 };

// The bound on |screen score - (1 - reference distance)|; 0: the shape has no screen.
static inline float ets_epsilon(int i8, uint32_t dim) {
    if (dim == 0) return 0.0f;
    if (i8) return dim <= ETS_I8_DIM_MAX ? 0x1p-20f : 0.0f;
    if (dim > ETS_F32_DIM_MAX) return 0.0f;
    const double kpad = dim <= 112 ? 112.0 : 208.0;         // components the matrix form sums (zero padded)
    const double split = 3.1 * 0x1p-18;                     // xl ql, x qr, xr q: the dropped term and the residuals
    const double mfma = 3.0 * kpad * 0x1p-23 * 1.02;        // 3 kpad exact products summed in f32, any order, rounded or truncated
    const double ref = (double)dim * 0x1p-24 * 1.01;        // the reference's dim fused steps, 32 accumulators, ordered sum
    return (float)((split + mfma + ref) * (1.0 + 0x1p-10) + 0x1p-22); // |x||q| <= 1 + 2^-10; 1 - dot, lo - 2 eps rounded
}

// The bound of the long-row forms; 0: no long-row screen for the shape (the short forms' shapes included).
// f32: ets_epsilon's terms with kpad = 128 ceil(dim / 128) -- the accumulator carried from chunk to chunk is one more
// partial sum of the same 3 kpad terms, which the any-order bound covers. int8: up to 1040 components the dot and both
// squared norms are below 2^24 and the short form's 11 roundings are all there are; beyond, four more conversions round
// (the dot on both sides, |x|^2 and |q|^2 on both sides at half weight each: 15 x 2^-24) and lo - 2 eps rounds once: 16
// units, each relative to a computed value that may exceed 1 by a few of them -- just above 2^-20; 2^-19 has the margin.
static inline float ets_epsilon_long(int i8, uint32_t dim) {
    if (dim > ETS_LONG_DIM_MAX) return 0.0f;
    if (i8) return dim <= ETS_I8_DIM_MAX ? 0.0f : dim <= 1040u ? 0x1p-20f : 0x1p-19f;
    if (dim <= ETS_F32_DIM_MAX) return 0.0f;
    const double kpad = (double)ETS_LONG_CHUNK * (double)((dim + ETS_LONG_CHUNK - 1u) / ETS_LONG_CHUNK);
    const double split = 3.1 * 0x1p-18;
    const double mfma = 3.0 * kpad * 0x1p-23 * 1.02;
    const double ref = (double)dim * 0x1p-24 * 1.01;
    return (float)((split + mfma + ref) * (1.0 + 0x1p-10) + 0x1p-22);
}
// the bound a form's kernels are given
static inline float ets_epsilon_of(uint32_t form, int i8, uint32_t dim) { return ets_form_long(form) ? ets_epsilon_long(i8, dim) : ets_epsilon(i8, dim); }

struct EtsParams {
    const uint8_t* elements;
    uint64_t n;              // the rows this pass scans (a prefix, or all)
    uint32_t row_bytes, row_stride, dim;
    const uint8_t* queries;  // dense [nq][dim] (this round's)
    uint32_t nq;
    uint64_t per_range;      // rows per range (a multiple of the tile)
    const float* inv_norm;   // int8: [n] 1 / |x|
    const float* inv_gmax;   // int8: [ceil(n / 32)][2] (brute_force.h)
    const float* lo;         // [nq] the floor; +inf: the query takes no part (outside the norm bound)
    uint32_t* hist;          // COUNT: [nq][ETS_BUCKETS]
    uint32_t* cnt;           // COLLECT: [nq]
    uint32_t* cand;          // COLLECT: [nq][ETS_CAP]
    float eps2;              // COLLECT: 2 eps
    const float* hi = nullptr;        // ETS_RADIUS: [nq] the upper threshold (lo: the lower one); cand is [nq][2][ETS_CAP]
    uint32_t* sure = nullptr;         // ETS_RADIUS: [nq] the rows with s >= hi, exact however many (cnt: the places asked for)
    uint32_t* bcnt = nullptr;         // ETS_RADIUS: [nq] the rows with lo <= s < hi
    const uint32_t* list = nullptr;   // ETS_LIST: the allowed ids, ascending; n counts its positions
    const uint32_t* filter = nullptr; // ETS_BITS: this round's bitmaps, query q's at filter + q * filter_stride
    uint64_t filter_stride = 0;       // ETS_BITS: in words
    uint64_t q_first = 0;             // ETS_Q_ROWS: the element that is this round's query 0 (queries is not read); with
                                      // ETS_LIST: its position in the list
    const float* tops = nullptr;      // the cursor forms: [nq] the pass's upper threshold (COUNT: top_sure, COLLECT: top_any)
};

// the launchers (exact_topk_screened.hip); every one is ordered on s and returns what the launch left
uint32_t ets_tile_rows(uint32_t form); // rows per tile of the form's scan
hipError_t ets_scan(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
hipError_t ets_scan_src(uint32_t form, bool collect, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
hipError_t ets_scan_radius(uint32_t form, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
hipError_t ets_empty(uint32_t nq, uint32_t k, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, hipStream_t s);
hipError_t ets_clear(uint32_t* p, uint32_t n, hipStream_t s);
hipError_t ets_max_norm2(const uint8_t* elements, uint64_t n, uint32_t row_bytes, uint32_t row_stride, uint32_t* out, hipStream_t s);
hipError_t ets_init(bool i8, const uint8_t* queries, uint32_t nq, uint32_t dim, float* lo, uint32_t* hist, uint32_t* cnt, hipStream_t s);
hipError_t ets_select(uint32_t* hist, uint32_t nq, uint32_t k, float* lo, hipStream_t s);
// sel: [nq][4] u32, exact_topk's EtSel (word 3: the query is voided for et_rank_kernel -- here: it is on the fallback list)
hipError_t ets_pad(uint32_t* cand, const uint32_t* cnt, const float* lo, uint32_t nq, uint32_t q_base, uint32_t* sel, uint32_t* fb_count,
                   uint32_t* fb_list, uint32_t* status, hipStream_t s);
hipError_t ets_keys(const uint32_t* cand, const float* dists, const uint32_t* cnt, uint32_t nq, uint64_t* keys, hipStream_t s);
hipError_t ets_gather(const uint8_t* queries, uint32_t qbytes, const uint32_t* fb_list, uint32_t nfb, uint8_t* out, hipStream_t s);
hipError_t ets_scatter(const uint32_t* fb_list, uint32_t nfb, uint32_t k, const uint64_t* ids, const float* dists, const uint32_t* counts,
                       const uint32_t* xs, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, uint32_t* status, hipStream_t s);
hipError_t ets_status(uint32_t* status, uint32_t routed, uint32_t form, const uint32_t* xs, hipStream_t s);

// ---- a cursor per query (exact_topk_after_host.h) ----
// ets_init with the cursors: lo as ets_init makes it (+inf also for a cursor distance outside [0, 2]), and per query
// top_sure (a score below it: surely after the cursor) and top_any (a score above it: surely before); +inf without one
hipError_t ets_init_after(bool i8, const uint8_t* queries, uint32_t nq, uint32_t dim, float eps, const float* after_dists, const uint64_t* after_ids,
                          float* lo, float* top_sure, float* top_any, uint32_t* hist, uint32_t* cnt, hipStream_t s);
// ets_scan_src under P.tops: COUNT is given top_sure and counts lo <= s < top, COLLECT top_any and lists lo - 2 eps <= s <= top
hipError_t ets_scan_after(uint32_t form, bool collect, int src, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
// ets_select over buckets that end at min(1, top_sure)
hipError_t ets_select_after(uint32_t* hist, uint32_t nq, uint32_t k, float* lo, const float* top_sure, hipStream_t s);
// ets_keys for the candidates beyond the cursor only, dense; cnt[q] becomes their number (et_rank_kernel's m)
hipError_t ets_keys_after(const uint32_t* cand, const float* dists, uint32_t* cnt, uint32_t nq, const float* after_dists,
                          const uint64_t* after_ids, uint64_t* keys, hipStream_t s);

// ---- the handle's own rows as queries (knn_graph_host.h) ----
// ets_scan over all rows with the queries of ETS_Q_ROWS: P.q_first, P.nq; ets_init with queries == nullptr starts them
hipError_t ets_scan_rows(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
// rows first + p -- p = list[f], or p_base + f where list is null -- f < m, as dense queries of qbytes each.
// `allowed`, here and in kg_drop_self, rg_self and rg_drop_self (graph_filtered_host.h): a filter's id
// list -- first + p is then a position of it and the element is allowed[first + p]; the outputs' places stay p.
hipError_t ets_gather_rows(const uint8_t* elements, uint32_t row_stride, uint32_t qbytes, uint64_t first, const uint32_t* list, uint32_t p_base,
                           uint32_t m, uint8_t* out, hipStream_t s, const uint32_t* allowed = nullptr);
// exact_topk's k + 1 nearest of the same m rows ([m][k + 1], counts [m]) -> the k nearest OTHERS, into place p of the outputs:
// the element dropped where it is listed, the last entry where it is not
hipError_t kg_drop_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, uint32_t k, const uint64_t* ids, const float* dists,
                        const uint32_t* counts, uint64_t* out_ids, float* out_dists, uint32_t* out_counts, hipStream_t s,
                        const uint32_t* allowed = nullptr);

// ---- the radius scan (exact_range_screened_host.h) ----
// What the queries of a call that path A does not answer are listed in: n[0] queries for exact_topk_screened(k = cap)
// (their totals are known), n[1] for exact_range's own scan; the lists hold their places among the call's queries.
struct ErsLists {
    uint32_t* n;    // [2]
    uint32_t* b;    // [nq]
    uint32_t* c;    // [nq]
};
// per query of a round: the f32 norm test, lo and hi (outside the norm bound: lo = +inf, hi = -inf), sure / cnt / bcnt cleared
hipError_t ers_radius(bool i8, const uint8_t* queries, const float* radii, uint32_t nq, uint32_t dim, float eps, float* lo, float* hi,
                      uint32_t* sure, uint32_t* cnt, uint32_t* bcnt, hipStream_t s);
// the unused places of both lists of every query: an id no handle has; list (ETS_LIST, else null): positions become ids
hipError_t ers_pad(uint32_t* cand, const uint32_t* sure, const uint32_t* bcnt, const uint32_t* list, uint32_t nq, hipStream_t s);
// after dists_kernel: keys [nq][ETS_CAP] (distance bits << 32 | id) of the listed rows with d <= r, totals [nq] for
// er_rank_kernel (path A: the keys; path B: the exact total, above ETS_CAP; path C: ETS_CAP + 1), the lists, the status words
hipError_t ers_keys(const uint32_t* cand, const float* dists, const float* radii, const float* lo, const float* hi, const uint32_t* sure,
                    const uint32_t* bcnt, uint32_t nq, uint32_t q_base, uint64_t* keys, uint32_t* totals, ErsLists lists, uint32_t* status,
                    hipStream_t s);
// ---- every element's neighbours within a radius (range_graph_host.h) ----
// ets_scan_radius over all rows with the queries of ETS_Q_ROWS (P.q_first, P.nq): the diagonal is -inf before the block's
// max, so an element is in neither of its lists and in none of its counts. ers_radius with queries == nullptr starts them.
hipError_t ets_scan_radius_rows(uint32_t form, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
// for the elements first + p -- p = list[f], or p_base + f where list is null -- f < m: their ids (dists_kernel's one
// candidate per element: d(e, e)) and their radii, dense
hipError_t rg_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, const float* radii, uint32_t* self_ids, float* out_radii,
                   hipStream_t s, const uint32_t* allowed = nullptr);
// exact_range's answer for cap + 1 over the same m rows as queries ([m][cap + 1], counts [m], totals [m]) -> the neighbours
// within the radius, into place p of the outputs: the total less one where self[f] = d(e, e) <= radii[f]; the element
// dropped where it is listed, the last entry where it is not and the listing is full
hipError_t rg_drop_self(uint64_t first, const uint32_t* list, uint32_t p_base, uint32_t m, uint32_t cap, const uint64_t* ids, const float* dists,
                        const uint32_t* counts, const uint32_t* totals, const float* self, const float* radii, uint64_t* out_ids, float* out_dists,
                        uint32_t* out_counts, uint32_t* out_totals, hipStream_t s, const uint32_t* allowed = nullptr);

// ---- the graphs of a subset (graph_filtered_host.h) ----
// The scans over the positions [0, P.n) of P.list (ETS_LIST) with the queries of ETS_Q_ROWS: query q of a round is POSITION
// P.q_first + q of the list, read from row P.list[P.q_first + q]; the diagonal is found by comparing positions, which is
// what the scanned rows are too. COLLECT lists ids, RADIUS positions, as the ETS_LIST scans with dense queries do.
hipError_t ets_scan_rows_list(uint32_t form, bool collect, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
hipError_t ets_scan_radius_rows_list(uint32_t form, uint32_t tiles, uint32_t ranges, const EtsParams& P, hipStream_t s);
// out[p] = allowed[first + p], p < count
hipError_t gf_elements(const uint32_t* allowed, uint64_t first, uint32_t count, uint64_t* out, hipStream_t s);

// status[0] += the queries of a dense answer with count 0 (voided by exact_topk's overflow), ETS_VOIDED into status[3]
hipError_t ers_voided(const uint32_t* counts, uint32_t np, uint32_t* status, hipStream_t s);
// status[0] += xs[0] (xs optional; ETS_VOIDED into [3] with it), status[1] += not_a, status[3] |= form
hipError_t ers_status(uint32_t* status, const uint32_t* xs, uint32_t not_a, uint32_t form, hipStream_t s);

} // namespace granne_hip
