// include/granne.hpp: ShardedGranne::id_span / search_filtered / exact_topk / exact_topk_filtered over the partitioned
// entries of the C ABI. Runs on an MI355X (tests/test_cpp_sharded_filtered.py compiles and executes it): three f32 shards
// from the GPU builder at offsets 0, 100 and 363 (two of them not word-aligned), then every call against per-shard calls
// merged on the host by (distance, global id) -- search_filtered under the mask's slice for the walk, and for the exact
// selection the shard's own search with max_search = num_neighbors = its length, which visits the whole (connected)
// graph and so is the scan over its rows in the same arithmetic (the idiom of test_filtered_api.cpp):
//   - id_span is the last shard's end;
//   - filtered search under a half filter, a filter of all ones (= the unfiltered sharded search) and an empty one;
//   - the exact selection over all rows and under the half filter, k above the smallest shard's size;
//   - a filter of the wrong length throws.
#include <algorithm>
#include <cstdio>
#include <random>

#include "granne.hpp"

using namespace granne;
using List = std::vector<std::pair<size_t, float>>;

#define REQUIRE(c)                                                         \
    do {                                                                   \
        if (!(c)) {                                                        \
            std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static List merged(const std::vector<List>& parts, const std::vector<uint64_t>& offsets, size_t k) {
    List all;
    for (size_t s = 0; s < parts.size(); ++s)
        for (const auto& e : parts[s]) all.emplace_back(e.first + (size_t)offsets[s], e.second);
    std::sort(all.begin(), all.end(), [](const auto& a, const auto& b) { return a.second < b.second || (a.second == b.second && a.first < b.first); });
    if (all.size() > k) all.resize(k);
    return all;
}

// equal, or the first difference on stderr
static bool same(const List& got, const List& want, const char* what, size_t query) {
    if (got == want) return true;
    std::fprintf(stderr, "%s, query %zu: %zu entries, want %zu\n", what, query, got.size(), want.size());
    for (size_t j = 0; j < std::min(got.size(), want.size()); ++j)
        if (got[j] != want[j]) {
            std::fprintf(stderr, "  [%zu] got (%zu, %.9g) want (%zu, %.9g)\n", j, got[j].first, got[j].second, want[j].first, want[j].second);
            break;
        }
    return false;
}

int main() {
    std::mt19937 rng(777);
    std::uniform_real_distribution<float> u(-0.5f, 0.5f);
    const size_t dim = 28;
    const std::vector<size_t> lengths = {100, 263, 337};
    const std::vector<uint64_t> offsets = {0, 100, 363};
    const size_t n = 700, nq = 6;
    std::vector<Granne<angular::Vectors>> shards;
    std::vector<angular::Vector> queries;
    for (size_t s = 0; s < lengths.size(); ++s) {
        angular::Vectors elements;
        for (size_t i = 0; i < lengths[s]; ++i) {
            std::vector<float> v(dim);
            for (auto& x : v) x = u(rng);
            elements.push(angular::from(std::move(v)));
        }
        GranneBuilder<angular::Vectors> builder(BuildConfig().num_neighbors(20).max_search(30), elements);
        builder.build();
        shards.push_back(builder.get_index());
        queries.push_back(elements.get_element(7));  // a row of the set: distance 0
        queries.push_back(elements.get_element(lengths[s] - 1));
    }
    ShardedGranne<angular::Vectors> sharded(shards, offsets);
    REQUIRE(sharded.id_span() == n && sharded.len() == n && sharded.num_shards() == 3);

    std::vector<bool> half(n), all(n, true), none(n, false);
    for (size_t i = 0; i < n; ++i) half[i] = (rng() & 1u) != 0;
    const Filter f_half = Filter::from_mask(half), f_all = Filter::from_mask(all), f_none = Filter::from_mask(none);
    auto local = [&](const std::vector<bool>& mask, size_t s) {
        return Filter::from_mask(std::vector<bool>(mask.begin() + offsets[s], mask.begin() + offsets[s] + lengths[s]));
    };

    const size_t ms = 40, k = 10, ke = 150; // ke: more than the first shard holds
    const auto got_half = sharded.search_filtered(queries.data(), nq, f_half, ms, k);
    const auto got_all = sharded.search_filtered(queries.data(), nq, f_all, ms, k);
    const auto got_none = sharded.search_filtered(queries.data(), nq, f_none, ms, k);
    const auto plain = sharded.search_batches(queries.data(), 1, nq, ms, k);
    const auto exact = sharded.exact_topk(queries.data(), nq, ke);
    const auto exact_half = sharded.exact_topk_filtered(queries.data(), nq, ke, f_half);
    std::vector<std::vector<List>> w_half(nq), w_exact(nq), w_exact_half(nq);
    for (size_t s = 0; s < shards.size(); ++s) {
        const Filter f = local(half, s);
        const auto a = shards[s].search_filtered_batch(queries.data(), nq, f, ms, k);
        const auto scan = shards[s].search_batch(queries.data(), nq, lengths[s], lengths[s]);
        for (size_t i = 0; i < nq; ++i) {
            REQUIRE(scan[i].size() == lengths[s]);
            List allowed;
            for (const auto& e : scan[i])
                if (half[offsets[s] + e.first]) allowed.push_back(e);
            w_half[i].push_back(a[i]);
            w_exact[i].push_back(scan[i]);
            w_exact_half[i].push_back(allowed);
        }
    }
    for (size_t i = 0; i < nq; ++i) {
        REQUIRE(same(got_half[i], merged(w_half[i], offsets, k), "search_filtered", i));
        REQUIRE(got_all[i] == plain[i]);
        REQUIRE(got_none[i].empty());
        REQUIRE(same(exact[i], merged(w_exact[i], offsets, ke), "exact_topk", i) && exact[i].size() == ke);
        REQUIRE(same(exact_half[i], merged(w_exact_half[i], offsets, ke), "exact_topk_filtered", i));
        REQUIRE(exact[i][0].second < 1e-6f); // the query is a row of the set
        for (const auto& e : got_half[i]) REQUIRE(half[e.first]);
        for (const auto& e : exact_half[i]) REQUIRE(half[e.first]);
    }
    bool threw = false;
    try {
        sharded.search_filtered(queries.data(), nq, Filter::from_mask(std::vector<bool>(n - 1, true)), ms, k);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    REQUIRE(threw);
    std::printf("ok\n");
    return 0;
}
