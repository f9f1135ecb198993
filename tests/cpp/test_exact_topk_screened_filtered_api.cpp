// include/granne.hpp: Granne::exact_topk_screened_filtered. Runs on an MI355X (tests/test_cpp_exact_topk_screened_filtered.py
// compiles and executes it): a small f32 index from the GPU builder and a filter of every third id; the screened answer is
// exact_topk_filtered's, pair for pair, the screen ran, and k = 1025 throws with the entry's message.
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

int main() {
    std::mt19937 rng(780);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28, n = 700, nq = 9, k = 100;
    angular::Vectors elements;
    for (size_t i = 0; i < n; ++i) {
        std::vector<float> v(dim);
        for (auto& x : v) x = u(rng);
        elements.push(angular::from(std::move(v)));
    }
    GranneBuilder<angular::Vectors> builder(BuildConfig().num_neighbors(20).max_search(30), elements);
    builder.build();
    auto index = builder.get_index();
    std::vector<decltype(index.get_element(0))> qs;
    for (size_t qi = 0; qi < nq; ++qi) qs.push_back(index.get_element(qi * 30));
    std::vector<uint64_t> ids;
    for (uint64_t i = 0; i < n; i += 3) ids.push_back(i);
    const Filter allowed = Filter::from_ids(ids, index.num_elements());
    std::vector<uint32_t> st;
    const auto got = index.exact_topk_screened_filtered(qs.data(), nq, k, allowed, &st);
    REQUIRE(got == index.exact_topk_filtered(qs.data(), nq, k, allowed));
    REQUIRE(got[0].size() == k && got[0][0].first == 0 && got[1][0].first == 30);
    REQUIRE(st.size() == 4 && st[0] == 0 && st[1] == 0 && st[2] >= k && st[3] == 1);
    bool threw = false;
    try {
        index.exact_topk_screened_filtered(qs.data(), nq, 1025, allowed);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("exact_topk_screened_filtered: k must be in [1, 1024]") != std::string::npos;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
