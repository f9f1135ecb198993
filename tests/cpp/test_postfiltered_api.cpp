// include/granne.hpp: Granne::search_postfiltered over the post-filtered entries of the C ABI.
// Runs on an MI355X (tests/test_cpp_postfiltered.py compiles and executes it): a small f32 index from the GPU builder, then
//   - a filter of all ones returns what Granne::search_batch(E_0, k) returns, every query at stage 0;
//   - under a half filter every query's answer is the allowed entries of the list of the stage that answered it;
//   - a filter of one id with a stage beyond the index's size ends at that stage with that id alone;
//   - with stages too short for a 2 % filter the EXACT fallback returns what exact_topk_filtered returns, the SHORT one a
//     prefix of the last list's allowed entries; an empty filter returns nothing;
//   - bad arguments throw with the library's message.
#include <algorithm>
#include <cstdio>
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

static Result allowed_of(const Result& list, const std::vector<bool>& mask, size_t k) {
    Result out;
    for (const auto& e : list)
        if (mask[e.first] && out.size() < k) out.push_back(e);
    return out;
}

int main() {
    std::mt19937 rng(777);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28, n = 700, nq = 9, k = 5, min_allowed = 16;
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

    std::vector<bool> half(n), sparse(n), all(n, true), none(n, false), one(n, false);
    for (size_t i = 0; i < n; ++i) {
        half[i] = (rng() & 1u) != 0;
        sparse[i] = rng() % 50u == 0;
    }
    one[123] = true;
    const Filter f_half = Filter::from_mask(half), f_sparse = Filter::from_mask(sparse), f_all = Filter::from_mask(all),
                 f_none = Filter::from_mask(none), f_one = Filter::from_mask(one);
    std::vector<decltype(index.get_element(0))> qs;
    for (size_t qi = 0; qi < nq; ++qi) qs.push_back(index.get_element(qi * 31));
    const std::vector<uint32_t> stages = {16, 64};
    std::vector<uint32_t> stage;

    // all ones: the plain search
    auto r = index.search_postfiltered(qs.data(), nq, k, f_all, min_allowed, stages, GRANNE_HIP_PF_FALLBACK_EXACT, &stage);
    REQUIRE(r == index.search_batch(qs.data(), nq, 16, k));
    REQUIRE(stage == std::vector<uint32_t>(nq, 0));

    // half: the allowed entries of the answering stage's list
    r = index.search_postfiltered(qs.data(), nq, k, f_half, min_allowed, stages, GRANNE_HIP_PF_FALLBACK_SHORT, &stage);
    for (size_t qi = 0; qi < nq; ++qi) {
        REQUIRE(stage[qi] <= 1 || stage[qi] == GRANNE_HIP_PF_STAGE_SHORT);
        const size_t E = stage[qi] == 0 ? 16 : 64;
        REQUIRE(r[qi] == allowed_of(index.search(qs[qi], E, E), half, k));
        REQUIRE(r[qi].size() == k);
    }

    // one id, a stage beyond the index: the walk runs out of graph and that stage answers
    r = index.search_postfiltered(qs.data(), nq, k, f_one, min_allowed, {16, 1024}, GRANNE_HIP_PF_FALLBACK_EXACT, &stage);
    for (size_t qi = 0; qi < nq; ++qi) REQUIRE(stage[qi] == 1 && r[qi].size() == 1 && r[qi][0].first == 123);

    // a 2 % filter under short stages: the fallbacks
    r = index.search_postfiltered(qs.data(), nq, k, f_sparse, min_allowed, stages, GRANNE_HIP_PF_FALLBACK_EXACT, &stage);
    const auto exact = index.exact_topk_filtered(qs.data(), nq, k, f_sparse);
    const auto s = index.search_postfiltered(qs.data(), nq, k, f_sparse, min_allowed, stages, GRANNE_HIP_PF_FALLBACK_SHORT);
    for (size_t qi = 0; qi < nq; ++qi) {
        REQUIRE(stage[qi] == GRANNE_HIP_PF_STAGE_EXACT);
        REQUIRE(r[qi] == exact[qi]);
        REQUIRE(s[qi] == allowed_of(index.search(qs[qi], 64, 64), sparse, k));
    }
    r = index.search_postfiltered(qs.data(), nq, k, f_none, min_allowed, stages);
    for (size_t qi = 0; qi < nq; ++qi) REQUIRE(r[qi].empty());

    // refusals carry the library's message
    auto message = [&](size_t kk, size_t m, std::vector<uint32_t> st, int fallback) -> std::string {
        try {
            index.search_postfiltered(qs.data(), nq, kk, f_half, m, st, fallback);
        } catch (const std::runtime_error& e) {
            return e.what();
        }
        return "";
    };
    REQUIRE(message(k, min_allowed, {64, 16}, 1).find("strictly ascending") != std::string::npos);
    REQUIRE(message(17, 16, {16, 64}, 1).find("min_allowed") != std::string::npos);
    REQUIRE(message(k, 17, {16, 64}, 1).find("stages[0]") != std::string::npos);
    REQUIRE(message(k, min_allowed, {16, 64}, 2).find("fallback") != std::string::npos);
    REQUIRE(message(k, min_allowed, {}, 1).find("n_stages") != std::string::npos);
    bool threw = false;
    try {
        index.search_postfiltered(qs.data(), nq, k, Filter::from_mask(std::vector<bool>(n - 1, true)), min_allowed, stages);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
