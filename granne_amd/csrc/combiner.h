// combiner.h -- host calls that are inside the library at the same moment share one search launch.
//
// The reference has no batch API: a host that wants throughput calls Granne::search(&self, ..) from many threads at once
// (src/index/mod.rs:140-150). Each such call used to be a launch of one walker on a stream of its
// own. A Combiner (one per index, of the flat-combining kind) lets those calls meet: a participating call queues a
// request; one of the callers becomes LEADER, takes the queued requests of its own key (max_search, num_neighbors) in
// arrival order up to the cap, runs ONE launch over the sum of their queries, hands every member its rows and its status,
// and passes leadership on. While a launch is on the GPU new arrivals queue up and the next launch takes them all: the
// group size follows the load, with no timer (GRANNE_HIP_OPT_COALESCE_WAIT_US adds one for those who want it).
//
// Plain C++17 and no HIP in here: the launch is a callable of the caller's, so the protocol is tested on a CPU
// (tests/cpp/test_combiner.cpp). granne_hip.hip supplies the two callables:
//   launch(slot, members, n, group_nq) -> int   copies the members' queries into slot `slot`'s block, runs one launch over
//                                               group_nq queries, waits for it and copies every member's rows out;
//                                               0 = every member is served
//   direct(request) -> int                      the call as it runs without a combiner
//
// Rules
//   - Requests of different keys never share a launch (the walker's instantiation depends on max_search).
//   - DEPTH = 2 launches may be in flight per index (two leaders, each with the block and stream of its slot), so the GPU
//     is not idle while one leader copies results out. 2 <= GRANNE_HIP_SEARCH_DEPTH (3): with the caller's own stream the
//     process stays within HIP's four hardware queues.
//   - No group exceeds the cap; a call takes part when its nq <= min(CALL_MAX, cap), so a leader's own request always fits.
//   - A lone caller takes the lock once on its way in and once on its way out, both uncontended -- in place of the two
//     the direct path spends on borrowing and returning a call context -- and waits for nobody.
//   - A launch that fails (any non-zero status: scratch overflow, a HIP error) gives NO member its verdict: each member
//     runs its own request through `direct` on its own thread and returns what that returns. A caller cannot tell that
//     it was grouped, except by time.
//   - Argument errors are the caller's to decide BEFORE submit(); nothing in here looks at pointers.
//   - The index must not be destroyed, nor the cap / wait changed, while a call is inside (the contract every option of
//     the index has). Nothing waits forever if the caller honours that: after every change of the queue or of a slot,
//     dispatch() leaves either no free slot or no queued request without a leader collecting for its key.
#ifndef GRANNE_HIP_COMBINER_H
#define GRANNE_HIP_COMBINER_H

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace granne_hip {

// The clock of a leader's timed wait. libstdc++ waits on a steady-clock deadline with pthread_cond_clockwait, which the
// ThreadSanitizer of GCC 11 does not know: it misses the unlock inside and reports locks that are not there. Under that
// sanitizer the deadline is the system clock's (pthread_cond_timedwait).
#if defined(__SANITIZE_THREAD__)
using CombinerClock = std::chrono::system_clock;
#else
using CombinerClock = std::chrono::steady_clock;
#endif

struct CombineRequest {
    const void* queries = nullptr; // [nq][dim], host
    uint32_t nq = 0;
    uint64_t* ids = nullptr;       // [nq][num_neighbors]
    float* dists = nullptr;        // [nq][num_neighbors]
    uint32_t* counts = nullptr;    // [nq]
    uint64_t* stats = nullptr;     // [nq][3] or null
    uint32_t max_search = 0, num_neighbors = 0;
};

class Combiner {
public:
    static constexpr uint32_t DEPTH = 2;      // launches in flight per index
    static constexpr uint32_t CALL_MAX = 64;  // GRANNE_HIP_COALESCE_CALL_MAX: larger calls never take part
    static constexpr uint32_t CAP_MAX = 1024; // GRANNE_HIP_OPT_COALESCE_MAX goes up to this (and defaults to it)

    // (set while no call is inside)
    void set_cap(uint32_t cap) { cap_.store(cap < 1 ? 1 : (cap > CAP_MAX ? CAP_MAX : cap)); }
    uint32_t cap() const { return cap_.load(); }
    void set_wait_us(uint64_t us) { wait_us_.store(us); }
    uint64_t wait_us() const { return wait_us_.load(); }
    // launches that served their members, and the queries of those launches, since construction
    uint64_t launches() const { return launches_.load(); }
    uint64_t queries() const { return queries_.load(); }
    // requests waiting for a leader right now (diagnostics and tests)
    size_t queued() {
        std::lock_guard<std::mutex> lk(mu_);
        return queue_.size();
    }

    bool takes(uint32_t nq) const {
        const uint32_t cap = cap_.load();
        return nq >= 1 && nq <= (cap < CALL_MAX ? cap : CALL_MAX);
    }

    // The whole of a participating call. `r` and the callables stay alive until it returns.
    template <class Launch, class Direct>
    int submit(const CombineRequest& r, Launch&& launch, Direct&& direct) {
        Ticket t;
        t.r = &r;
        {
            std::unique_lock<std::mutex> lk(mu_);
            queue_.push_back(&t);
            for (uint32_t s = 0; s < DEPTH; ++s) // a leader that waits for its group to fill hears of the arrival
                if (collecting_[s] && same_key(*collecting_[s]->r, r)) collecting_[s]->cv.notify_one();
            dispatch();
            while (t.state == QUEUED) t.cv.wait(lk);
            if (t.state == LEAD) lead(t, lk, launch);
        }
        if (t.state == RERUN) return direct(r);
        return t.status;
    }

private:
    enum State { QUEUED, LEAD, DONE, RERUN };
    struct Ticket { // lives on its caller's stack for the length of submit()
        const CombineRequest* r = nullptr;
        State state = QUEUED;
        uint32_t slot = 0;
        int status = 0;
        std::condition_variable cv;
    };

    static bool same_key(const CombineRequest& a, const CombineRequest& b) {
        return a.max_search == b.max_search && a.num_neighbors == b.num_neighbors;
    }
    bool has_collector(const CombineRequest& r) const {
        for (uint32_t s = 0; s < DEPTH; ++s)
            if (collecting_[s] && same_key(*collecting_[s]->r, r)) return true;
        return false;
    }

    // (mu_ held) Every free slot goes to the oldest queued request whose key nobody is collecting for.
    void dispatch() {
        for (uint32_t s = 0; s < DEPTH; ++s) {
            if (busy_[s]) continue;
            size_t i = 0;
            while (i < queue_.size() && has_collector(*queue_[i]->r)) ++i;
            if (i == queue_.size()) return;
            Ticket* t = queue_[i];
            queue_.erase(queue_.begin() + (std::ptrdiff_t)i);
            busy_[s] = true;
            collecting_[s] = t;
            t->slot = s;
            t->state = LEAD;
            t->cv.notify_one();
        }
    }

    // (mu_ held on entry and on return) t owns slot t.slot and is its key's collector.
    template <class Launch>
    void lead(Ticket& t, std::unique_lock<std::mutex>& lk, Launch& launch) {
        const uint32_t s = t.slot;
        const uint32_t cap = cap_.load();
        const uint64_t wait_us = wait_us_.load();
        if (wait_us) { // until the group has reached the cap, or this long after taking the lead
            const auto deadline = CombinerClock::now() + std::chrono::microseconds(wait_us);
            for (;;) {
                uint64_t have = t.r->nq;
                for (Ticket* q : queue_)
                    if (same_key(*q->r, *t.r)) have += q->r->nq;
                if (have >= cap) break;
                if (t.cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
            }
        }
        std::vector<Ticket*>& members = members_[s]; // the slot's own lists: no allocation once they have grown
        std::vector<const CombineRequest*>& reqs = reqs_[s];
        members.clear();
        reqs.clear();
        members.push_back(&t);
        reqs.push_back(t.r);
        uint32_t total = t.r->nq;
        for (size_t i = 0; i < queue_.size();) { // arrival order; the first that does not fit ends the group
            Ticket* q = queue_[i];
            if (!same_key(*q->r, *t.r)) {
                ++i;
                continue;
            }
            if ((uint64_t)total + q->r->nq > cap) break;
            total += q->r->nq;
            members.push_back(q);
            reqs.push_back(q->r);
            queue_.erase(queue_.begin() + (std::ptrdiff_t)i);
        }
        collecting_[s] = nullptr;
        dispatch(); // what the cap left behind may lead on the other slot
        lk.unlock();
        int rc;
        try {
            rc = launch(s, reqs.data(), reqs.size(), total);
        } catch (...) {
            rc = -1;
        }
        lk.lock();
        if (rc == 0) {
            launches_.fetch_add(1);
            queries_.fetch_add(total);
        }
        for (Ticket* m : members) { // (notified under the lock: a member's ticket is gone once it has seen its state)
            m->status = rc;
            m->state = rc == 0 ? DONE : RERUN;
            if (m != &t) m->cv.notify_one();
        }
        busy_[s] = false;
        dispatch(); // leadership passes to the oldest request still queued
    }

    std::mutex mu_;
    std::vector<Ticket*> queue_; // arrival order
    bool busy_[DEPTH] = {};
    Ticket* collecting_[DEPTH] = {};
    std::vector<Ticket*> members_[DEPTH];
    std::vector<const CombineRequest*> reqs_[DEPTH];
    std::atomic<uint32_t> cap_{CAP_MAX};
    std::atomic<uint64_t> wait_us_{0};
    std::atomic<uint64_t> launches_{0}, queries_{0};
};

} // namespace granne_hip
#endif
