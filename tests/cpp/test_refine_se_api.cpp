// include/granne.hpp: RefinedSumEmbeddingsGranne and SumEmbeddings::rows_i8 reach the container entries of the C ABI, and
// their argument errors arrive as exceptions carrying the library's message. Needs no GPU: a container is host data until
// a device entry point uses it, and every argument of the new entries is checked before any device call.
#include <cstdio>
#include <string>

#include "granne.hpp"

template <class F>
static bool throws_with(const char* what, F f) {
    try {
        f();
    } catch (const std::runtime_error& e) {
        if (std::string(e.what()).find(what) != std::string::npos) return true;
        std::printf("wrong message: %s (wanted: %s)\n", e.what(), what);
        return false;
    }
    std::printf("no exception (wanted: %s)\n", what);
    return false;
}

int main() {
    const uint32_t dim = 4;
    const std::vector<float> table = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    granne::embeddings::SumEmbeddings se(table, dim, {{0, 1}, {2}, {}, {1, 1, 2}});
    if (se.len() != 4 || se.dim() != dim) return 1;
    granne::Granne<granne::angular_int::Vectors> none(nullptr); // no walk index: every call must fail before the device
    granne::RefinedSumEmbeddingsGranne<granne::angular_int::Vectors> rg(none, se);
    const granne::angular_int::Vector qw{};
    const std::vector<float> qr(dim, 0.5f);
    bool ok = true;
    ok &= throws_with("walk index is null", [&] { rg.search(qw, qr, 50, 10); });
    ok &= throws_with("max_search", [&] { rg.search(qw, qr, 20, 10, 21); });
    ok &= throws_with("candidates per query", [&] { rg.search(qw, qr, 2000, 10, 1025); });
    ok &= throws_with("k must be", [&] { rg.search(qw, qr, 50, 0); });
    ok &= throws_with("query dimension mismatch", [&] { rg.search(qw, std::vector<float>(dim + 1), 50, 10); });
    ok &= throws_with("out of range", [&] { se.rows_i8(3, 2); });
    if (!se.rows_i8(4, 0).empty()) ok = false; // nothing to do: no device either
    std::printf(ok ? "ok\n" : "FAILED\n");
    return ok ? 0 : 1;
}
