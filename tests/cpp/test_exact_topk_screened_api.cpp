// include/granne.hpp: Granne::exact_topk_screened. Runs on an MI355X (tests/test_cpp_exact_topk_screened.py compiles and
// executes it): a small f32 index from the GPU builder; the screened answer is exact_topk's, pair for pair, the screen ran
// (no query routed, none on the fallback list), and k = 1025 throws with the library's message.
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
    std::mt19937 rng(779);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28, n = 700, nq = 9;
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
    for (size_t qi = 0; qi < nq; ++qi) qs.push_back(index.get_element(qi * 31));
    for (size_t k : {size_t(1), size_t(100), size_t(1024)}) {
        std::vector<uint32_t> st;
        const auto got = index.exact_topk_screened(qs.data(), nq, k, &st);
        REQUIRE(got == index.exact_topk(qs.data(), nq, k));
        REQUIRE(got[0].size() == (k < n ? k : n) && got[0][0].first == 0);
        REQUIRE(st.size() == 4 && st[0] == 0 && st[1] == 0 && st[2] >= got[0].size() && st[3] == 1);
    }
    bool threw = false;
    try {
        index.exact_topk_screened(qs.data(), nq, 1025);
    } catch (const std::runtime_error& e) {
        threw = std::string(e.what()).find("k must be in [1, 1024]") != std::string::npos;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
