#!/usr/bin/env python
"""Insert and search latency of granne_amd.RwGranneBuilder on a live graph.

    python tools/rw_insert_bench.py [--n 1000000] [--dim 100] [--max-elements 1100000] [--out profiles/rw_insert_latency.json]

Builds an n x dim f32 graph on the GPU (synthetic rows, the distribution of src/test_helper.rs:3-6), makes the Rw
handle with room for max_elements, then measures in ONE process:
  * wall time per call of 2,000 insert(1) calls and of 200 insert_batch(32) calls, each with GRANNE_HIP_RW_OPT_SMALL_OPS at
    its default and at 0 (= the device-wide radix sort, the bulk builder's phase B): median, p99, min, max after a
    warm-up of 50 / 10 calls. The graph grows by the same number of rows under both settings (< 2 % of n altogether);
    the order default / 0 / default / 0 is interleaved per block of calls so that growth does not favour either;
  * searches per second over the live layers against the same graph's static get_index snapshot: batch 1024, ef 50,
    20 calls after 5 of warm-up, median and spread.
Writes one JSON document."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(us):
    a = np.sort(np.asarray(us, np.float64))
    return {"calls": int(a.size), "median_us": float(np.median(a)), "p99_us": float(a[min(a.size - 1, int(a.size * 0.99))]),
            "min_us": float(a[0]), "max_us": float(a[-1]), "mean_us": float(a.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--max-elements", type=int, default=1100000)
    ap.add_argument("--singles", type=int, default=2000)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "rw_insert_latency.json"))
    args = ap.parse_args()
    import granne_amd as ga
    from granne_amd import rw_builder

    rng = np.random.default_rng(1)
    need = args.n + 2 * (args.singles + 50) + 2 * 32 * (args.batches + 10) + 2048
    rows = ga.normalize((rng.random((need, args.dim), dtype=np.float32) - np.float32(0.5)))
    t0 = time.perf_counter()
    b = ga.GranneBuilder("angular", rows[:args.n], max_search=50, reinsert_elements=False)
    rw = ga.RwGranneBuilder(b, args.max_elements)
    build_s = time.perf_counter() - t0
    at = [args.n]

    def take(k):
        r = rows[at[0]:at[0] + k]
        at[0] += k
        return r

    def timed_inserts(calls, size, small_ops):
        rw.set_option(rw_builder.SMALL_OPS, small_ops)
        out = []
        for _ in range(calls):
            r = take(size)
            t = time.perf_counter()
            ids = rw.insert_batch(r)
            out.append((time.perf_counter() - t) * 1e6)
            assert len(ids) == size
        return out

    result = {"n": args.n, "dim": args.dim, "max_elements": args.max_elements, "build_and_create_s": build_s,
              "num_neighbors": 30, "max_search": 50, "inserts": {}}
    for name, size, calls, warm in (("insert_1", 1, args.singles, 50), ("insert_batch_32", 32, args.batches, 10)):
        timed_inserts(warm // 2, size, 1)
        timed_inserts(warm - warm // 2, size, 0)
        t = {1: [], 0: []}
        block = max(1, calls // 4)
        done = 0
        while done < calls:
            k = min(block, calls - done)
            for opt in (1, 0):
                t[opt] += timed_inserts(k, size, opt)
            done += k
        result["inserts"][name] = {"small_ops_default": stats(t[1]), "small_ops_0": stats(t[0]),
                                   "ops_per_call": 2 * size * 30}
    rw.set_option(rw_builder.SMALL_OPS, 1)
    result["small_launches"] = rw.get_option(rw_builder.SMALL_LAUNCHES)
    result["sorted_launches"] = rw.get_option(rw_builder.SORTED_LAUNCHES)
    result["len_after"] = len(rw)

    q = ga.normalize((rng.random((1024, args.dim), dtype=np.float32) - np.float32(0.5)))
    snap = rw.get_index()

    def qps(fn):
        for _ in range(5):
            fn()
        ts = []
        for _ in range(20):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        ts = np.asarray(ts)
        return {"median_qps": float(1024 / np.median(ts)), "min_qps": float(1024 / ts.max()), "max_qps": float(1024 / ts.min())}

    result["search_batch_1024_ef50"] = {"live": qps(lambda: rw.search_batch(q, 50, 10)),
                                        "static_get_index": qps(lambda: snap.search_batch(q, 50, 10))}
    a, c = rw.search_batch(q, 50, 10), snap.search_batch(q, 50, 10)
    result["live_equals_static"] = bool((a[0] == c[0]).all() and (a[1].view(np.uint32) == c[1].view(np.uint32)).all())
    snap.close()
    rw.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
