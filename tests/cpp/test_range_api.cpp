// include/granne.hpp: Granne::exact_range and Granne::search_range over the range entries of the C ABI.
// Runs on an MI355X (tests/test_cpp_range.py compiles and executes it): a small f32 index from the GPU builder, then
//   - exact_range under a radius taken from exact_topk's own distances returns exactly exact_topk's prefix within it, and
//     totals counts every row within it also beyond cap; a negative radius returns nothing; under a filter of half the
//     ids the answer is the allowed part;
//   - search_range with one stage and an infinite radius, SHORT, returns what search_batch(E, E) returns, cut at cap;
//   - with the radius at the 5th exact neighbour every query ends at stage 0 with a prefix of search(16, 16);
//   - with a radius that holds everything and the EXACT fallback the answer is exact_range's, found = n;
//   - bad arguments throw with the library's message.
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <string>

#include "granne.hpp"

using namespace granne;

#define REQUIRE(c)                                                         \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

using Result = std::vector<std::pair<size_t, float>>;

static Result within(const Result& list, float r, size_t cap) {
    Result out;
    for (const auto& e : list)
        if (e.second <= r && out.size() < cap) out.push_back(e);
    return out;
}

int main() {
    std::mt19937 rng(778);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28, n = 700, nq = 9, cap = 20;
    angular::Vectors elements;
    for (size_t i = 0; i < n; ++i) {
        std::vector<float> v(dim);
        for (auto& x : v) x = u(rng);
        elements.push(angular::from(std::move(v)));
    }
    GranneBuilder<angular::Vectors> builder(BuildConfig().num_neighbors(20).max_search(30), elements);
    builder.build();
    auto index = builder.get_index();
    REQUIRE(index.len() == n);
    std::vector<decltype(index.get_element(0))> qs;
    for (size_t qi = 0; qi < nq; ++qi) qs.push_back(index.get_element(qi * 31));
    const float inf = std::numeric_limits<float>::infinity();

    // the scan: exact_topk's prefix within the radius; totals beyond cap
    const auto top = index.exact_topk(qs.data(), nq, 100);
    std::vector<float> radii(nq);
    for (size_t qi = 0; qi < nq; ++qi) radii[qi] = top[qi][qi % 2 ? 49 : 4].second;  // 50 rows (beyond cap) or 5
    std::vector<uint32_t> totals;
    auto r = index.exact_range(qs.data(), nq, radii.data(), cap, nullptr, &totals);
    for (size_t qi = 0; qi < nq; ++qi) {
        REQUIRE(r[qi] == within(top[qi], radii[qi], cap));
        REQUIRE(totals[qi] == within(top[qi], radii[qi], 100).size());
        REQUIRE(totals[qi] >= (qi % 2 ? 50u : 5u) && r[qi].size() == (qi % 2 ? cap : totals[qi]));
    }
    const std::vector<float> negative(nq, -0.5f), all(nq, 2.0f), everything(nq, inf);
    r = index.exact_range(qs.data(), nq, negative.data(), cap, nullptr, &totals);
    for (size_t qi = 0; qi < nq; ++qi) REQUIRE(r[qi].empty() && totals[qi] == 0);
    std::vector<bool> half(n);
    for (size_t i = 0; i < n; ++i) half[i] = (rng() & 1u) != 0;
    const Filter f_half = Filter::from_mask(half);
    r = index.exact_range(qs.data(), nq, all.data(), cap, &f_half, &totals);
    const auto top_half = index.exact_topk_filtered(qs.data(), nq, cap, f_half);
    for (size_t qi = 0; qi < nq; ++qi) REQUIRE(r[qi] == top_half[qi] && totals[qi] == f_half.count());

    // the walk: one stage, everything within, SHORT = the plain search cut at cap
    std::vector<uint32_t> found, stage;
    r = index.search_range(qs.data(), nq, everything.data(), cap, {50}, GRANNE_HIP_RG_FALLBACK_SHORT, &found, &stage);
    const auto plain = index.search_batch(qs.data(), nq, 50, 50);
    for (size_t qi = 0; qi < nq; ++qi) {
        REQUIRE(r[qi] == within(plain[qi], inf, cap));
        REQUIRE(found[qi] == plain[qi].size() && stage[qi] == GRANNE_HIP_RG_STAGE_SHORT);
    }
    // a radius at the 5th exact neighbour: a list of 16 reaches past it
    for (size_t qi = 0; qi < nq; ++qi) radii[qi] = top[qi][4].second;
    r = index.search_range(qs.data(), nq, radii.data(), cap, {16, 64}, GRANNE_HIP_RG_FALLBACK_EXACT, &found, &stage);
    for (size_t qi = 0; qi < nq; ++qi) {
        REQUIRE(stage[qi] == 0);
        REQUIRE(r[qi] == within(index.search(qs[qi], 16, 16), radii[qi], cap) && found[qi] == r[qi].size());
    }
    // everything within, EXACT: no list reaches past the radius, the scan answers
    r = index.search_range(qs.data(), nq, all.data(), cap, {16, 64}, GRANNE_HIP_RG_FALLBACK_EXACT, &found, &stage);
    const auto scan = index.exact_range(qs.data(), nq, all.data(), cap);
    for (size_t qi = 0; qi < nq; ++qi) REQUIRE(stage[qi] == GRANNE_HIP_RG_STAGE_EXACT && r[qi] == scan[qi] && found[qi] == n);

    // refusals carry the library's message
    auto message = [&](size_t c, std::vector<uint32_t> st, int fallback) -> std::string {
        try {
            index.search_range(qs.data(), nq, all.data(), c, st, fallback);
        } catch (const std::runtime_error& e) {
            return e.what();
        }
        return "";
    };
    REQUIRE(message(cap, {64, 16}, 1).find("strictly ascending") != std::string::npos);
    REQUIRE(message(0, {16, 64}, 1).find("cap (0)") != std::string::npos);
    REQUIRE(message(1025, {16, 64}, 1).find("cap (1025)") != std::string::npos);
    REQUIRE(message(cap, {16, 64}, 2).find("fallback") != std::string::npos);
    REQUIRE(message(cap, {}, 1).find("n_stages") != std::string::npos);
    bool threw = false;
    try {
        index.exact_range(qs.data(), nq, all.data(), 0);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("cap (0)") != std::string::npos;
    }
    REQUIRE(threw);
    threw = false;
    const std::vector<float> nan(nq, std::nanf(""));
    try {
        index.exact_range(qs.data(), nq, nan.data(), cap);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
