// include/granne.hpp: granne::Filter and Granne::search_filtered over the filtered-search entries of the C ABI.
// Runs on an MI355X (tests/test_cpp_filtered.py compiles and executes it): a small f32 index from the GPU builder, then
//   - Filter::from_ids / from_mask / count agree with each other and with the host's count, out-of-range ids are reported;
//   - a filter of all ones returns what Granne::search returns;
//   - under a half filter every result is allowed, ascending, and with max_search >= n it is the scan over the allowed rows;
//   - an empty filter returns nothing; max_expand = 1 returns at most the walk's entry point;
//   - a filter of the wrong length throws.
#include <algorithm>
#include <cstdio>
#include <random>

#include "granne.hpp"

using namespace granne;

#define REQUIRE(c)                                                         \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    std::mt19937 rng(4242);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28, n = 700;
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

    std::vector<bool> half(n), all(n, true), none(n, false);
    std::vector<uint64_t> half_ids;
    for (size_t i = 0; i < n; ++i) {
        half[i] = (rng() & 1u) != 0;
        if (half[i]) half_ids.push_back(i);
    }
    const Filter f_half = Filter::from_mask(half), f_all = Filter::from_mask(all), f_none = Filter::from_mask(none);
    REQUIRE(f_half.len() == n && f_half.count() == half_ids.size() && f_all.count() == n && f_none.count() == 0);
    std::vector<uint64_t> noisy = half_ids;
    noisy.push_back(half_ids[0]); // a duplicate
    noisy.push_back(n);           // out of range
    noisy.push_back(~0ull);
    uint32_t bad = 0;
    const Filter f_ids = Filter::from_ids(noisy, n, 0, &bad);
    REQUIRE(bad == 2 && f_ids.count() == half_ids.size());

    for (size_t qi = 0; qi < 8; ++qi) {
        const auto q = index.get_element(qi * 31);
        // all ones: the unfiltered search
        REQUIRE(index.search_filtered(q, f_all, 40, 10) == index.search(q, 40, 10));
        // half: allowed, ascending; by mask and by ids the same
        const auto r = index.search_filtered(q, f_half, 40, 10);
        REQUIRE(r == index.search_filtered(q, f_ids, 40, 10));
        REQUIRE(!r.empty());
        for (size_t j = 0; j < r.size(); ++j) {
            REQUIRE(half[r[j].first]);
            if (j) REQUIRE(r[j - 1].second < r[j].second || (r[j - 1].second == r[j].second && r[j - 1].first < r[j].first));
        }
        // max_search >= n: the walk visits the whole (connected) graph, `res` is the scan over the allowed rows
        const auto scan_all = index.search(q, n, n);
        REQUIRE(scan_all.size() == n);
        std::vector<std::pair<size_t, float>> want;
        for (const auto& e : scan_all)
            if (half[e.first] && want.size() < 10) want.push_back(e);
        REQUIRE(index.search_filtered(q, f_half, n, 10) == want);
        REQUIRE(index.search_filtered(q, f_none, 40, 10).empty());
        REQUIRE(index.search_filtered(q, f_all, 40, 10, 1).size() == 1);
    }
    bool threw = false;
    try {
        index.search_filtered(index.get_element(0), Filter::from_mask(std::vector<bool>(n - 1, true)), 10, 5);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
