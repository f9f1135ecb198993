#!/usr/bin/env python
"""exact_range_screened next to exact_range, whose answer it is defined as, in one process.

    python tools/exact_range_screened_bench.py [--elements 1000000] [--out profiles/exact_range_screened.json]

tools/range_bench.py's data and radii: the benchmark's mixture rows, f32 and int8, one call of 20,480 queries, cap 1024,
radii per query from a ground-truth scan (torch: not the code under test) as the distance of the query's t-th nearest row,
t = 1, 10, 100, 1,000 and 10,000 -- the mean total is then about t. A handle without layers (no graph is walked). HIP
events around each call (both entries wait on their stream inside the window), the two entries interleaved inside every
repeat, one warm-up round, medians of --reps. After the timed rounds one call of each with status words: every id,
distance byte, count and total is compared, and the screened call's words are recorded ([1] the queries path A did not
answer, of which the ones past 4,096 rows within the radius took path B and the rest path C; [2] the largest S + B).
Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--cap", type=int, default=1024)
ap.add_argument("--queries", type=int, default=20_480)
ap.add_argument("--totals", default="1,10,100,1000,10000")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_range_screened.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga

n, dim, cap, nq = opt.elements, opt.dim, opt.cap, opt.queries
s = B.stream
targets = [int(x) for x in opt.totals.split(",")]
out = {"workload": "%d x %d-d mixture, one call of %d queries, cap %d; radii per query: the ground-truth distance of the t-th nearest row, "
                   "t in %s" % (n, dim, nq, cap, targets),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each call on one stream (the calls' own stream waits are inside their windows); exact_range and "
                 "exact_range_screened interleaved inside every repeat; median of %d repeats after one warm-up round" % opt.reps,
       "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, dtype)
    g = ga.Granne.from_device("angular" if dtype == "f32" else "angular_int", rows.data_ptr(), n, dim, [], [], [])
    rows_f = torch.nn.functional.normalize(rows.float(), dim=1)
    q_f = torch.nn.functional.normalize(q.float(), dim=1)
    T = min(max(targets), n)
    gt_d = torch.cat([1.0 - torch.topk(q_f[lo:lo + 512] @ rows_f.T, T, dim=1)[0] for lo in range(0, nq, 512)])
    del rows_f, q_f
    rec = {"epsilon": float(B.lib.granne_hip_exact_topk_screen_epsilon(0 if dtype == "f32" else 1, dim)), "totals": {}}
    for t in targets:
        radii = gt_d[:, min(t, T) - 1].contiguous()
        bufs = [(torch.empty((nq, cap), dtype=torch.int64, device="cuda"), torch.empty((nq, cap), dtype=torch.float32, device="cuda"),
                 torch.empty(nq, dtype=torch.int32, device="cuda"), torch.empty(nq, dtype=torch.int32, device="cuda"),
                 torch.zeros(4, dtype=torch.int32, device="cuda")) for _ in range(2)]
        entries = {"exact_range": g.exact_range_device, "screened": g.exact_range_screened_device}

        def call(name, b, status):
            entries[name](q.data_ptr(), nq, radii.data_ptr(), cap, 0, 0, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(),
                          b[4].data_ptr() if status else 0, s)

        ms = {name: [] for name in entries}
        for rep in range(opt.reps + 1):  # round 0 warms up
            for name, b in zip(entries, bufs):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(name, b, False)
                t1.record()
                torch.cuda.synchronize()
                if rep:
                    ms[name].append(t0.elapsed_time(t1))
        for name, b in zip(entries, bufs):
            call(name, b, True)
        torch.cuda.synchronize()
        (xi, xd, xc, xt, xst), (si, sd, sc, stt, sst) = bufs
        info = {"mean_total": round(xt.float().mean().item(), 2), "max_total": int(xt.max().item())}
        for name, v in ms.items():
            info[name] = {"ms_median": round(statistics.median(v), 3), "ms_per_run": [round(x, 3) for x in v]}
        info["status"] = [int(x) & 0xFFFFFFFF for x in sst.tolist()]
        info["exact_range_status"] = [int(x) & 0xFFFFFFFF for x in xst.tolist()]
        info["path_b_queries"] = int((xt > 4096).sum().item())  # (equal totals are asserted below)
        info["path_c_queries"] = info["status"][1] - info["path_b_queries"]
        info["ids_equal"] = bool(torch.equal(si, xi))
        info["dist_bytes_equal"] = bool(torch.equal(sd.view(torch.int32), xd.view(torch.int32)))
        info["counts_equal"] = bool(torch.equal(sc, xc))
        info["totals_equal"] = bool(torch.equal(stt, xt))
        info["exact_range_over_screened"] = round(info["exact_range"]["ms_median"] / info["screened"]["ms_median"], 3)
        info["screened_queries_per_s"] = round(nq / (info["screened"]["ms_median"] * 1e-3), 1)
        rec["totals"][str(t)] = info
        bench.log(dtype, "total", t, json.dumps(info))
        assert info["ids_equal"] and info["dist_bytes_equal"] and info["counts_equal"] and info["totals_equal"], (dtype, t)
        del bufs
    rec["slower_than_exact_range_at"] = [t for t, v in rec["totals"].items() if v["exact_range_over_screened"] < 1.0]
    out["dtypes"][dtype] = rec
    g.close()
    del g, rows, q, gt_d
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({"out": opt.out, "ratios": {d: {t: v["exact_range_over_screened"] for t, v in r["totals"].items()} for d, r in out["dtypes"].items()}}))
