#!/usr/bin/env python
"""exact_topk_screened_filtered next to exact_topk_filtered, whose answer it is defined as, in one process.

    python tools/exact_topk_screened_filtered_bench.py [--elements 1000000] [--out profiles/exact_topk_screened_filtered.json]

tools/filtered_exact_bench.py's data and filters: the benchmark's mixture rows, f32 and int8, k 10, one call of 20,480 queries
under one shared random filter per selectivity (1.0, 0.5, 0.1, 0.01; the same seeds) -- the list form -- and the same four
bitmaps once per query for a call of 1,024 queries -- the bit-tested form. A handle without layers (no graph is walked).
HIP events around each call, the two entries interleaved inside every repeat, one warm-up round, medians of --reps. After
the timed rounds one call of each with status words: every id, distance byte and count is compared, and the screened call's
words ([0] fallback queries, [2] the largest survivor count) are recorded. Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--queries", type=int, default=20_480)
ap.add_argument("--per-query-queries", type=int, default=1024)
ap.add_argument("--selectivities", default="1.0,0.5,0.1,0.01")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_topk_screened_filtered.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402

n, dim, k = opt.elements, opt.dim, opt.k
s = B.stream
out = {"workload": "%d x %d-d mixture, k %d; shared: one call of %d queries under one random filter (list form); per_query: one call of %d "
                   "queries, the same bitmap once per query (bit-tested form)" % (n, dim, k, opt.queries, opt.per_query_queries),
       "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each call on one stream; exact_topk_filtered and exact_topk_screened_filtered interleaved inside every "
                 "repeat; median of %d repeats after one warm-up round" % opt.reps,
       "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q_all = B.rows("mixture", bench.SEED + 1, 0, opt.queries, dim, dtype)
    g = ga.Granne.from_device("angular" if dtype == "f32" else "angular_int", rows.data_ptr(), n, dim, [], [], [])
    rec = {"epsilon": float(B.lib.granne_hip_exact_topk_screen_epsilon(0 if dtype == "f32" else 1, dim)), "shared": {}, "per_query": {}}
    for sel in [float(x) for x in opt.selectivities.split(",")]:
        gen = torch.Generator(device="cuda").manual_seed(int(sel * 1000) + 17)
        mask = (torch.rand(n, device="cuda", generator=gen) < sel) if sel < 1.0 else torch.ones(n, dtype=torch.bool, device="cuda")
        mask8 = mask.to(torch.uint8)
        words = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
        _lib.check(B.lib.granne_hip_filter_from_mask_device(C.c_void_p(mask8.data_ptr()), n, C.c_void_p(words.data_ptr()), B.dev, B.sp))
        torch.cuda.synchronize()
        for form, nq in (("shared", opt.queries), ("per_query", opt.per_query_queries)):
            q = q_all[:nq].contiguous()
            maps, stride = (words, 0) if form == "shared" else (words[None, :].repeat(nq, 1).contiguous(), words.numel())
            bufs = [(torch.empty((nq, k), dtype=torch.int64, device="cuda"), torch.empty((nq, k), dtype=torch.float32, device="cuda"),
                     torch.empty(nq, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")) for _ in range(2)]
            entries = {"exact_topk_filtered": g.exact_topk_filtered_device, "screened": g.exact_topk_screened_filtered_device}

            def call(name, b, status):
                entries[name](q.data_ptr(), nq, k, maps.data_ptr(), stride, b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(),
                              b[3].data_ptr() if status else 0, s)

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
            (xi, xd, xc, _), (si, sd, sc, sst) = bufs
            info = {"allowed_rows": int(mask.sum().item()), "queries": nq}
            for name, v in ms.items():
                info[name] = {"ms_median": round(statistics.median(v), 3), "ms_per_run": [round(x, 3) for x in v]}
            info["status"] = [int(x) & 0xFFFFFFFF for x in sst.tolist()]
            info["fallback_queries"], info["survivors_max"] = info["status"][0], info["status"][2]
            info["ids_equal"] = bool(torch.equal(si, xi))
            info["dist_bytes_equal"] = bool(torch.equal(sd.view(torch.int32), xd.view(torch.int32)))
            info["counts_equal"] = bool(torch.equal(sc, xc))
            info["exact_topk_filtered_over_screened"] = round(info["exact_topk_filtered"]["ms_median"] / info["screened"]["ms_median"], 3)
            rec[form][str(sel)] = info
            bench.log(dtype, form, sel, json.dumps(info))
            assert info["ids_equal"] and info["dist_bytes_equal"] and info["counts_equal"], (dtype, form, sel)
            del maps, bufs
        del words, mask, mask8
    if "0.01" in rec["shared"]:
        rec["list_form_at_0.01_slower_than_exact_topk_filtered"] = rec["shared"]["0.01"]["exact_topk_filtered_over_screened"] < 1.0
    out["dtypes"][dtype] = rec
    g.close()
    del g, rows, q_all
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({"out": opt.out, "ratios": {d: {form: {x: v["exact_topk_filtered_over_screened"] for x, v in r[form].items()}
                                                  for form in ("shared", "per_query")} for d, r in out["dtypes"].items()}}))
