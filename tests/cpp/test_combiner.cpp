// The combiner's protocol (granne_amd/csrc/combiner.h) on the CPU: a fake launch step echoes every request's tag into its
// outputs. Built by tests/test_combiner_host.py with g++ (under ThreadSanitizer where the machine has it). Exits 0 and
// prints "ok"; a failed check exits 1, the wall-clock guard exits 3.
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "../../granne_amd/csrc/combiner.h"

using granne_hip::Combiner;
using granne_hip::CombineRequest;
using Clock = std::chrono::steady_clock;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            fflush(stderr);                                                  \
            _exit(1);                                                        \
        }                                                                    \
    } while (0)

static double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// A request's "queries" are its tags, one u64 per query. The echo: ids[i][j] = tag[i], dists[i][j] = j, counts[i] = k,
// stats[i] = {tag, max_search, k}.
struct Call {
    std::vector<uint64_t> tags, ids, stats;
    std::vector<float> dists;
    std::vector<uint32_t> counts;
    CombineRequest r;
    Call(uint64_t first_tag, uint32_t nq, uint32_t max_search, uint32_t k, bool want_stats)
        : tags(nq), ids((size_t)nq * k, ~0ull), stats(want_stats ? (size_t)nq * 3 : 0), dists((size_t)nq * k, -1.f), counts(nq, ~0u) {
        for (uint32_t i = 0; i < nq; ++i) tags[i] = first_tag + i;
        r.queries = tags.data();
        r.nq = nq;
        r.ids = ids.data();
        r.dists = dists.data();
        r.counts = counts.data();
        r.stats = want_stats ? stats.data() : nullptr;
        r.max_search = max_search;
        r.num_neighbors = k;
    }
    void check_served() const {
        const uint32_t k = r.num_neighbors;
        for (uint32_t i = 0; i < r.nq; ++i) {
            CHECK(counts[i] == k);
            for (uint32_t j = 0; j < k; ++j) CHECK(ids[(size_t)i * k + j] == tags[i] && dists[(size_t)i * k + j] == (float)j);
            if (r.stats) CHECK(stats[i * 3] == tags[i] && stats[i * 3 + 1] == r.max_search && stats[i * 3 + 2] == k);
        }
    }
};

static void echo(const CombineRequest& r) {
    const uint64_t* tags = (const uint64_t*)r.queries;
    for (uint32_t i = 0; i < r.nq; ++i) {
        for (uint32_t j = 0; j < r.num_neighbors; ++j) {
            r.ids[(size_t)i * r.num_neighbors + j] = tags[i];
            r.dists[(size_t)i * r.num_neighbors + j] = (float)j;
        }
        r.counts[i] = r.num_neighbors;
        if (r.stats) {
            r.stats[i * 3] = tags[i];
            r.stats[i * 3 + 1] = r.max_search;
            r.stats[i * 3 + 2] = r.num_neighbors;
        }
    }
}

// what every launch must look like, whatever the test: one key, the announced size, within the cap, a slot of its own
struct LaunchLog {
    std::mutex mu;
    std::vector<std::vector<const CombineRequest*>> groups;
    std::atomic<int> in_slot[Combiner::DEPTH];
    std::atomic<uint32_t> max_group{0};
    LaunchLog() {
        for (auto& s : in_slot) s = 0;
    }
    void enter(const Combiner& c, unsigned slot, const CombineRequest* const* m, size_t n, uint32_t group_nq, bool keep) {
        CHECK(slot < Combiner::DEPTH && n >= 1);
        CHECK(in_slot[slot].fetch_add(1) == 0); // a slot serves one launch at a time
        uint32_t sum = 0;
        for (size_t i = 0; i < n; ++i) {
            CHECK(m[i]->max_search == m[0]->max_search && m[i]->num_neighbors == m[0]->num_neighbors);
            sum += m[i]->nq;
        }
        CHECK(sum == group_nq && group_nq <= c.cap());
        uint32_t seen = max_group.load();
        while (seen < group_nq && !max_group.compare_exchange_weak(seen, group_nq)) {
        }
        if (keep) {
            std::lock_guard<std::mutex> lk(mu);
            groups.emplace_back(m, m + n);
        }
    }
    void leave(unsigned slot) { CHECK(in_slot[slot].fetch_sub(1) == 1); }
};

// ---- exactly-once delivery: 32 threads x 2000 requests of mixed keys and nq -------------------------------------------
static void test_exactly_once(uint64_t wait_us, int per_thread) {
    constexpr int T = 32;
    constexpr uint32_t MAXNQ = 7;
    Combiner c;
    c.set_cap(16);
    c.set_wait_us(wait_us);
    LaunchLog log;
    std::vector<std::atomic<uint8_t>> served((size_t)T * per_thread * MAXNQ);
    for (auto& s : served) s = 0;
    std::atomic<uint64_t> direct_calls{0}, issued{0};
    auto launch = [&](unsigned slot, const CombineRequest* const* m, size_t n, uint32_t group_nq) {
        log.enter(c, slot, m, n, group_nq, false);
        for (size_t i = 0; i < n; ++i) {
            echo(*m[i]);
            const uint64_t* tags = (const uint64_t*)m[i]->queries;
            for (uint32_t q = 0; q < m[i]->nq; ++q) served[tags[q]].fetch_add(1);
        }
        log.leave(slot);
        return 0;
    };
    auto direct = [&](const CombineRequest&) {
        direct_calls.fetch_add(1);
        return -99;
    };
    static const uint32_t keys[3][2] = {{50, 10}, {20, 5}, {40, 10}};
    static const uint32_t nqs[4] = {1, 2, 3, MAXNQ};
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(t + 1);
            for (int i = 0; i < per_thread; ++i) {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                const uint32_t* key = keys[x % 3];
                const uint32_t nq = nqs[(x >> 8) % 4];
                Call call(((uint64_t)t * per_thread + i) * MAXNQ, nq, key[0], key[1], (x >> 16) & 1);
                CHECK(c.takes(nq));
                CHECK(c.submit(call.r, launch, direct) == 0);
                call.check_served();
                issued.fetch_add(nq);
            }
        });
    for (auto& t : th) t.join();
    uint64_t total = 0;
    for (auto& s : served) {
        CHECK(s.load() <= 1); // nobody is served twice
        total += s.load();
    }
    CHECK(total == issued.load() && c.queries() == issued.load());
    CHECK(direct_calls.load() == 0);
    CHECK(c.launches() >= 1 && c.launches() <= (uint64_t)T * per_thread);
    CHECK(log.max_group.load() <= 16 && c.queued() == 0);
    printf("exactly-once (wait %llu us): %llu queries in %llu launches, largest group %u\n", (unsigned long long)wait_us,
           (unsigned long long)c.queries(), (unsigned long long)c.launches(), log.max_group.load());
}

// ---- a launch that fails returns every member through the direct path ---------------------------------------------------
static void test_failed_launch() {
    constexpr int T = 8, N = 200;
    Combiner c;
    std::atomic<uint64_t> direct_calls{0}, launches{0};
    auto launch = [&](unsigned, const CombineRequest* const*, size_t, uint32_t) {
        launches.fetch_add(1);
        return -4; // the shared verdict nobody may take
    };
    auto direct = [&](const CombineRequest& r) {
        direct_calls.fetch_add(1);
        echo(r);
        return (int)(1000 + *(const uint64_t*)r.queries % 7); // each caller's own status
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (int i = 0; i < N; ++i) {
                Call call((uint64_t)t * N + i, 1, 50, 10, false);
                CHECK(c.submit(call.r, launch, direct) == (int)(1000 + call.tags[0] % 7));
                call.check_served();
            }
        });
    for (auto& t : th) t.join();
    CHECK(direct_calls.load() == (uint64_t)T * N && launches.load() >= 1);
    CHECK(c.launches() == 0 && c.queries() == 0 && c.queued() == 0); // only launches that served count
    // a launch step that throws is a failed launch
    auto thrower = [&](unsigned, const CombineRequest* const*, size_t, uint32_t) -> int { throw 1; };
    Call call(7, 1, 50, 10, false);
    CHECK(c.submit(call.r, thrower, direct) == 1000);
}

// both slots held inside their launch step until the test opens the gate
struct Gate {
    std::mutex mu;
    std::condition_variable cv;
    bool open = false;
    std::atomic<int> inside{0};
    void pass() {
        inside.fetch_add(1);
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return open; });
    }
    void release() {
        {
            std::lock_guard<std::mutex> lk(mu);
            open = true;
        }
        cv.notify_all();
    }
};
template <class F>
static void spin_until(F&& f) {
    while (!f()) std::this_thread::sleep_for(std::chrono::microseconds(50));
}

// ---- leadership passes to the oldest queued request; different keys never share; the cap holds ---------------------------
static void test_handover_and_cap() {
    Combiner c;
    c.set_cap(8);
    LaunchLog log;
    Gate gate;
    auto launch = [&](unsigned slot, const CombineRequest* const* m, size_t n, uint32_t group_nq) {
        log.enter(c, slot, m, n, group_nq, true);
        gate.pass();
        for (size_t i = 0; i < n; ++i) echo(*m[i]);
        log.leave(slot);
        return 0;
    };
    auto direct = [&](const CombineRequest&) {
        CHECK(false);
        return -1;
    };
    // A and B take the two slots; then C (key 1), D (key 2), E, F, G (key 1, 3 queries each) queue in that order
    std::vector<Call*> calls = {new Call(0, 1, 50, 10, false),  new Call(10, 1, 50, 10, false), new Call(20, 3, 50, 10, true),
                                new Call(30, 2, 20, 5, false),  new Call(40, 3, 50, 10, false), new Call(50, 3, 50, 10, false),
                                new Call(60, 3, 50, 10, false)};
    std::vector<std::thread> th;
    for (size_t i = 0; i < calls.size(); ++i) {
        th.emplace_back([&, i] {
            CHECK(c.submit(calls[i]->r, launch, direct) == 0);
            calls[i]->check_served();
        });
        if (i < 2) spin_until([&] { return gate.inside.load() == (int)i + 1; });
        else spin_until([&] { return c.queued() == i - 1; });
    }
    CHECK(c.launches() == 0 && c.queued() == 5);
    gate.release();
    for (auto& t : th) t.join();
    // launches: A | B | C+E (3 + 3 <= 8 < 3 + 3 + 3: the cap ends the group at F) | D alone (its key) | F+G
    CHECK(c.launches() == 5 && c.queries() == 16 && c.queued() == 0);
    CHECK(log.groups.size() == 5 && log.max_group.load() == 6);
    auto group_of = [&](const Call* x) -> const std::vector<const CombineRequest*>& {
        for (auto& g : log.groups)
            for (auto* r : g)
                if (r == &x->r) return g;
        CHECK(false);
        return log.groups[0];
    };
    const auto& gc = group_of(calls[2]);
    CHECK(gc.size() == 2 && gc[0] == &calls[2]->r && gc[1] == &calls[4]->r); // the oldest leads, arrival order inside
    CHECK(group_of(calls[3]).size() == 1);
    const auto& gf = group_of(calls[5]);
    CHECK(gf.size() == 2 && gf[0] == &calls[5]->r && gf[1] == &calls[6]->r);
    for (auto* x : calls) delete x;
}

// ---- with wait 0 a lone request is launched at once, by its own thread; the wait knob waits for the cap or the time -------
static void test_idle_and_wait() {
    Combiner c;
    std::thread::id launcher;
    auto launch = [&](unsigned, const CombineRequest* const* m, size_t n, uint32_t) {
        launcher = std::this_thread::get_id();
        for (size_t i = 0; i < n; ++i) echo(*m[i]);
        return 0;
    };
    auto direct = [&](const CombineRequest&) { return -1; };
    {
        Call call(1, 1, 50, 10, true);
        const auto t0 = Clock::now();
        CHECK(c.submit(call.r, launch, direct) == 0);
        CHECK(seconds_since(t0) < 1.0 && launcher == std::this_thread::get_id());
        call.check_served();
        CHECK(c.launches() == 1 && c.queries() == 1);
    }
    CHECK(!c.takes(0) && c.takes(64) && !c.takes(65));
    c.set_cap(4);
    CHECK(c.takes(4) && !c.takes(5));
    { // the timer: a lone request under a cap of 4 leaves after the wait
        c.set_wait_us(200 * 1000);
        Call call(2, 1, 50, 10, false);
        const auto t0 = Clock::now();
        CHECK(c.submit(call.r, launch, direct) == 0);
        const double dt = seconds_since(t0);
        CHECK(dt >= 0.2 && dt < 30.0);
        CHECK(c.launches() == 2);
    }
    { // the cap: four requests under a wait of a minute leave together as soon as the fourth is there
        c.set_wait_us(60ull * 1000 * 1000);
        const auto t0 = Clock::now();
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                Call call(100 + t, 1, 50, 10, false);
                CHECK(c.submit(call.r, launch, direct) == 0);
                call.check_served();
            });
        for (auto& t : th) t.join();
        CHECK(seconds_since(t0) < 30.0);
        CHECK(c.launches() == 3 && c.queries() == 6);
    }
}

int main() {
    std::thread([] { // the guard: a combiner that hangs must fail, not sit there
        std::this_thread::sleep_for(std::chrono::seconds(240));
        fprintf(stderr, "wall-clock guard: the combiner test did not finish in 240 s\n");
        fflush(stderr);
        _exit(3);
    }).detach();
    test_idle_and_wait();
    test_handover_and_cap();
    test_failed_launch();
    test_exactly_once(0, 2000);
    test_exactly_once(20, 200);
    printf("ok\n");
    fflush(stdout);
    _exit(0); // (the guard thread is still asleep)
}
