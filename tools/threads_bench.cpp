// threads_bench -- the reference's own way to throughput, measured: T host threads, each issuing single
// granne_hip_search calls (Granne::search, one query per call) on a shared index, with GRANNE_HIP_OPT_COALESCE off and
// on. Python threads would measure the GIL; this is C++ over include/granne.hpp.
//
//   workload   --elements 1000000 x --dim 100 f32 (uniform [-0.5, 0.5), normalised), built on the GPU, default config
//   legs       for T in --threads 1,4,16: option off and on alternate --rounds 3 times, --seconds 2 each, one process
//   per leg    queries/s, median and p99 call latency, mean group size (queries per grouped launch)
//   output     --out profiles/coalesce_threads.json, and a summary of the two questions it answers:
//              T = 1: is the median latency with the option on within the spread of the off legs (a lone caller pays nothing)?
//              T = max: does queries/s with the option on exceed the best off leg by more than the off legs' spread?
// Stops at the first non-zero status (exit 1). Run it under a time limit: tools/threads_bench.sh does.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "granne.hpp"

using Clock = std::chrono::steady_clock;

static uint64_t splitmix(uint64_t& x) {
    uint64_t z = (x += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static std::vector<float> random_rows(size_t n, size_t dim, uint64_t seed) {
    std::vector<float> v(n * dim);
    uint64_t x = seed;
    for (auto& f : v) f = (float)((splitmix(x) >> 40) * (1.0 / 16777216.0) - 0.5);
    granne::check(granne_hip_normalize_f32(v.data(), n, (uint32_t)dim, 0));
    return v;
}

struct Leg {
    int threads, round, on;
    double seconds, qps, median_us, p99_us, mean_group;
    uint64_t calls, launches;
};

int main(int argc, char** argv) {
    size_t n = 1000000, dim = 100, nqueries = 4096;
    double seconds = 2.0;
    int rounds = 3;
    uint32_t max_search = 50, k = 10;
    std::vector<int> thread_counts = {1, 4, 16};
    std::string out = "profiles/coalesce_threads.json";
    for (int i = 1; i + 1 < argc; i += 2) {
        const std::string a = argv[i];
        const char* v = argv[i + 1];
        if (a == "--elements") n = strtoull(v, nullptr, 10);
        else if (a == "--dim") dim = strtoull(v, nullptr, 10);
        else if (a == "--seconds") seconds = atof(v);
        else if (a == "--rounds") rounds = atoi(v);
        else if (a == "--out") out = v;
        else if (a == "--threads") {
            thread_counts.clear();
            for (const char* p = v; *p;) {
                thread_counts.push_back((int)strtol(p, (char**)&p, 10));
                if (*p == ',') ++p;
            }
        } else {
            fprintf(stderr, "unknown argument %s\n", a.c_str());
            return 2;
        }
    }
    try {
        const auto t_build = Clock::now();
        auto elements = granne::angular::Vectors::from_vec(random_rows(n, dim, 1), dim);
        granne::GranneBuilder<granne::angular::Vectors> builder(granne::BuildConfig(), elements);
        builder.build();
        auto index = builder.get_index();
        const std::vector<float> queries = random_rows(nqueries, dim, 2);
        printf("built %zu x %zu f32 in %.1f s, %zu layers\n", n, dim, std::chrono::duration<double>(Clock::now() - t_build).count(),
               index.num_layers());
        fflush(stdout);

        std::vector<Leg> legs;
        std::atomic<int> bad_status{0};
        for (int T : thread_counts)
            for (int round = 0; round < rounds; ++round)
                for (int on = 0; on < 2; ++on) {
                    index.set_coalesce(on != 0);
                    const uint64_t l0 = index.coalesced_launches(), q0 = index.coalesced_queries();
                    std::vector<std::vector<float>> lat(T);
                    std::atomic<bool> go{false};
                    std::vector<std::thread> th;
                    Clock::time_point t0;
                    for (int t = 0; t < T; ++t)
                        th.emplace_back([&, t] {
                            std::vector<uint64_t> ids(k);
                            std::vector<float> ds(k);
                            uint32_t count = 0;
                            lat[t].reserve(1 << 16);
                            while (!go.load()) std::this_thread::yield();
                            const auto end = t0 + std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double>(seconds));
                            size_t q = (size_t)t * 977;
                            for (auto a = Clock::now(); a < end && !bad_status.load();) {
                                const int rc = granne_hip_search(index.raw(), queries.data() + (q++ % nqueries) * dim, max_search, k,
                                                                 ids.data(), ds.data(), &count);
                                const auto b = Clock::now();
                                if (rc != 0) {
                                    fprintf(stderr, "status %d: %s\n", rc, granne_hip_last_error());
                                    bad_status.store(rc);
                                    break;
                                }
                                lat[t].push_back(std::chrono::duration<float, std::micro>(b - a).count());
                                a = b;
                            }
                        });
                    t0 = Clock::now();
                    go.store(true);
                    for (auto& t : th) t.join();
                    const double dt = std::chrono::duration<double>(Clock::now() - t0).count();
                    if (bad_status.load()) return 1;
                    std::vector<float> all;
                    for (auto& v : lat) all.insert(all.end(), v.begin(), v.end());
                    if (all.empty()) {
                        fprintf(stderr, "no call finished\n");
                        return 1;
                    }
                    std::sort(all.begin(), all.end());
                    Leg g;
                    g.threads = T, g.round = round, g.on = on, g.seconds = dt, g.calls = all.size();
                    g.qps = all.size() / dt;
                    g.median_us = all[all.size() / 2];
                    g.p99_us = all[std::min(all.size() - 1, all.size() * 99 / 100)];
                    g.launches = index.coalesced_launches() - l0;
                    g.mean_group = g.launches ? double(index.coalesced_queries() - q0) / g.launches : 1.0;
                    legs.push_back(g);
                    printf("T %2d round %d coalesce %d: %9.0f queries/s  median %7.1f us  p99 %7.1f us  mean group %.2f\n", T, round, on,
                           g.qps, g.median_us, g.p99_us, g.mean_group);
                    fflush(stdout);
                }

        // the two questions, against the off legs of this same run
        auto pick = [&](int T, int on, auto field) {
            std::vector<double> v;
            for (auto& g : legs)
                if (g.threads == T && g.on == on) v.push_back(field(g));
            std::sort(v.begin(), v.end());
            return v;
        };
        const int T1 = thread_counts.front(), TN = thread_counts.back();
        const auto off_med = pick(T1, 0, [](const Leg& g) { return g.median_us; });
        const auto on_med = pick(T1, 1, [](const Leg& g) { return g.median_us; });
        const auto off_qps = pick(TN, 0, [](const Leg& g) { return g.qps; });
        const auto on_qps = pick(TN, 1, [](const Leg& g) { return g.qps; });
        double group = 0;
        int ng = 0;
        for (auto& g : legs)
            if (g.threads == TN && g.on) group += g.mean_group, ++ng;
        group /= ng ? ng : 1;
        const double on_median = on_med[on_med.size() / 2];
        const bool lone_ok = on_median >= off_med.front() && on_median <= off_med.back();
        const double spread = off_qps.back() - off_qps.front();
        const bool many_ok = on_qps.front() > off_qps.back() + spread;
        const double ratio = on_qps[on_qps.size() / 2] / off_qps.back();
        printf("T = %d: median latency on %.1f us, off legs %.1f .. %.1f us: %s\n", T1, on_median, off_med.front(), off_med.back(),
               lone_ok ? "within the off legs' spread" : (on_median < off_med.front() ? "below the off legs" : "ABOVE the off legs' spread"));
        printf("T = %d: queries/s on %.0f .. %.0f, off %.0f .. %.0f: median on / best off = %.2f x, mean group %.2f: %s\n", TN,
               on_qps.front(), on_qps.back(), off_qps.front(), off_qps.back(), ratio, group,
               many_ok ? "beyond the off legs' spread" : "NOT beyond the off legs' spread");

        FILE* f = fopen(out.c_str(), "w");
        if (!f) {
            fprintf(stderr, "cannot write %s\n", out.c_str());
            return 1;
        }
        fprintf(f, "{\n \"tool\": \"tools/threads_bench.cpp\",\n \"workload\": {\"elements\": %zu, \"dim\": %zu, \"dtype\": \"f32\", "
                   "\"max_search\": %u, \"num_neighbors\": %u, \"seconds_per_leg\": %.2f, \"rounds\": %d},\n \"legs\": [\n",
                n, dim, max_search, k, seconds, rounds);
        for (size_t i = 0; i < legs.size(); ++i) {
            const Leg& g = legs[i];
            fprintf(f, "  {\"threads\": %d, \"round\": %d, \"coalesce\": %d, \"calls\": %llu, \"seconds\": %.3f, \"queries_per_s\": %.0f, "
                       "\"median_us\": %.1f, \"p99_us\": %.1f, \"grouped_launches\": %llu, \"mean_group\": %.3f}%s\n",
                    g.threads, g.round, g.on, (unsigned long long)g.calls, g.seconds, g.qps, g.median_us, g.p99_us,
                    (unsigned long long)g.launches, g.mean_group, i + 1 < legs.size() ? "," : "");
        }
        fprintf(f, " ],\n \"lone_caller\": {\"threads\": %d, \"median_us_on\": %.1f, \"median_us_off_min\": %.1f, \"median_us_off_max\": %.1f, "
                   "\"within_off_spread\": %s},\n",
                T1, on_median, off_med.front(), off_med.back(), lone_ok ? "true" : "false");
        fprintf(f, " \"many_callers\": {\"threads\": %d, \"queries_per_s_on_min\": %.0f, \"queries_per_s_on_max\": %.0f, "
                   "\"queries_per_s_off_min\": %.0f, \"queries_per_s_off_max\": %.0f, \"ratio_median_on_to_best_off\": %.3f, "
                   "\"mean_group\": %.3f, \"beyond_off_spread\": %s}\n}\n",
                TN, on_qps.front(), on_qps.back(), off_qps.front(), off_qps.back(), ratio, group, many_ok ? "true" : "false");
        fclose(f);
        printf("wrote %s\n", out.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
