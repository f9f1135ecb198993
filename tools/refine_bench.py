#!/usr/bin/env python
"""Refined search measured: walk the int8 graph, re-rank by the f32 rows -- against the f32 walk, the int8 walk, and the
same result composed from the entries that existed before (int8 search with k = m, dists_device, a sort).

    python tools/refine_bench.py [--elements 10000000] [--data mixture] [--out profiles/refine_bench.json]

Builds the f32 graph, the int8 graph (GPU builder, the reference's default config) and a rows-only f32 handle over the
benchmark's structured data set, then times four legs at ef 50, k 10, m 50 with HIP events, the legs interleaved inside
every repeat (one process, one device):
    a  f32 walk            b  int8 walk            c  fused refined search            d  c's result from b(k = m) + dists + sort
once as a stream of 1024-query calls and once as one call of 20,480 queries, and records queries/s per leg, recall@10 of
a, b and c against the exact scan of the f32 rows, and whether c is at least as fast as d within d's own run-to-run spread.
Not part of bench.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--data", default="mixture", choices=["mixture", "latent", "uniform"])
ap.add_argument("--ef", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--refine-from", type=int, default=50)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--batches", type=int, default=20, help="calls per timed run of the stream shape; one call of batch x batches is the other shape")
ap.add_argument("--passes", type=int, default=10, help="a timed run goes over its calls this many times (tens of milliseconds per run)")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()  # the reference's default build config: num_neighbors 30, max_search 200, reinsertion
B = bench.Bench(args)
torch, ga = B.torch, B.ga
n, dim, ef, k, m, nq, nb = opt.elements, opt.dim, opt.ef, opt.k, opt.refine_from, opt.batch, opt.batches
big = nq * nb
s = B.stream

rows = B.rows(opt.data, bench.SEED + 100, 0, n, dim, "f32")
b_f, g_f, t_f = B.build_index(rows, "f32")
del b_f
rows8 = B.prepare(rows, "i8")  # angular_int::Vector::from of the normalised rows
b_8, g_8, t_8 = B.build_index(rows8, "i8")
del b_8, rows8
r_f = ga.Granne.from_device("angular", rows.data_ptr(), n, dim, [], [], [], device=B.dev, stream=s)
torch.cuda.synchronize()
del rows
torch.cuda.empty_cache()
bench.log("built: f32 graph %.1f s (%.2f GB), int8 graph %.1f s (%.2f GB), f32 rows handle %.2f GB" %
          (t_f, g_f.hbm_bytes() / 1e9, t_8, g_8.hbm_bytes() / 1e9, r_f.hbm_bytes() / 1e9))

q = B.rows(opt.data, bench.SEED + 1, 0, big, dim, "f32")  # queries from the elements' distribution, disjoint seed
q8 = B.prepare(q, "i8")
rg = ga.RefinedGranne(g_8, r_f)

ids = torch.empty((big, k), dtype=torch.int64, device="cuda")
ds = torch.empty((big, k), dtype=torch.float32, device="cuda")
cnt = torch.empty(big, dtype=torch.int32, device="cuda")
c_ids = torch.empty((big, m), dtype=torch.int64, device="cuda")
c_ds = torch.empty((big, m), dtype=torch.float32, device="cuda")
c_dd = torch.empty((big, m), dtype=torch.float32, device="cuda")
status = torch.zeros(8, dtype=torch.int32, device="cuda")


def leg_a(lo, cn):
    g_f.search_batch_device(q[lo:].data_ptr(), cn, ef, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0, status.data_ptr(), s)


def leg_b(lo, cn):
    g_8.search_batch_device(q8[lo:].data_ptr(), cn, ef, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0, status.data_ptr(), s)


def leg_c(lo, cn):
    rg.search_batch_device(q8[lo:].data_ptr(), q[lo:].data_ptr(), cn, ef, m, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0,
                           status.data_ptr(), status[4:].data_ptr(), s)


def leg_d(lo, cn):
    """The composition a caller had to write before: the walk's m best, their f32 distances, a sort by (distance, id)."""
    g_8.search_batch_device(q8[lo:].data_ptr(), cn, ef, m, c_ids[lo:].data_ptr(), c_ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0, status.data_ptr(), s)
    i32 = c_ids[lo:lo + cn].to(torch.int32)  # dists_device takes u32 ids; an unused slot (UINT64_MAX) becomes 0xFFFFFFFF: +inf
    r_f.dists_device(q[lo:].data_ptr(), cn, i32.data_ptr(), m, c_dd[lo:].data_ptr(), 0, s)
    key = (c_dd[lo:lo + cn].view(torch.int32).to(torch.int64) << 32) | (c_ids[lo:lo + cn] & 0xFFFFFFFF)  # distances are >= 0: bits order them
    top = torch.sort(key, dim=1).values[:, :k]
    ids[lo:lo + cn] = top & 0xFFFFFFFF
    ds[lo:lo + cn] = (top >> 32).to(torch.int32).view(torch.float32)


LEGS = {"a_f32_walk": leg_a, "b_int8_walk": leg_b, "c_refined_fused": leg_c, "d_refined_composed": leg_d}


def run_shape(name, calls):
    """calls: [(first query, count)] of one timed run. Legs interleaved inside every repeat; HIP events around each run."""
    calls = calls * opt.passes
    total = sum(c for _, c in calls)
    for _ in range(opt.warmup):
        for fn in LEGS.values():
            for lo, cn in calls:
                fn(lo, cn)
    torch.cuda.synchronize()
    ms = {leg: [] for leg in LEGS}
    for _ in range(opt.repeats):
        for leg, fn in LEGS.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for lo, cn in calls:
                fn(lo, cn)
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1))
    rec = {"queries_per_run": total, "calls_per_run": len(calls), "repeats": opt.repeats, "warmup_runs": opt.warmup, "legs": {}}
    for leg, v in ms.items():
        qps = sorted(total / (x * 1e-3) for x in v)
        rec["legs"][leg] = {"queries_per_s_median": round(qps[len(qps) // 2], 1), "queries_per_s_min": round(qps[0], 1),
                            "queries_per_s_max": round(qps[-1], 1), "ms_per_run": [round(x, 4) for x in v]}
    c, d = rec["legs"]["c_refined_fused"], rec["legs"]["d_refined_composed"]
    spread = d["queries_per_s_max"] - d["queries_per_s_min"]
    rec["condition"] = {"what": "fused (c) is not slower than composed (d): median c >= median d - the spread (max - min) of d's own repeats",
                        "c_median": c["queries_per_s_median"], "d_median": d["queries_per_s_median"], "d_spread": round(spread, 1),
                        "holds": bool(c["queries_per_s_median"] >= d["queries_per_s_median"] - spread)}
    for other in ("a_f32_walk", "b_int8_walk", "d_refined_composed"):
        rec["c_over_" + other[0]] = round(c["queries_per_s_median"] / rec["legs"][other]["queries_per_s_median"], 4)
    bench.log(name, json.dumps({k_: v["queries_per_s_median"] for k_, v in rec["legs"].items()}), json.dumps(rec["condition"]))
    return rec


out = {"workload": "%d x %d-d, %s, ef %d, k %d, refine_from %d; GPU builder, default config" % (n, dim, opt.data, ef, k, m),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "hbm_gb": {"f32_graph": round(g_f.hbm_bytes() / 1e9, 2), "int8_graph": round(g_8.hbm_bytes() / 1e9, 2), "f32_rows_handle": round(r_f.hbm_bytes() / 1e9, 2)},
       "timing": "HIP events around each run on one stream; legs interleaved inside every repeat; queries/s = queries of a run / its time"}

# the fused result equals the composed one, bit for bit, on the queries that are timed
leg_c(0, big)
torch.cuda.synchronize()
f_ids, f_ds = ids.clone(), ds.clone()
leg_d(0, big)
torch.cuda.synchronize()
out["fused_equals_composed"] = {"ids": bool(torch.equal(f_ids, ids)), "dist_bits": bool(torch.equal(f_ds.view(torch.int32), ds.view(torch.int32)))}
bench.log("fused == composed:", out["fused_equals_composed"])

# recall@10 against the exact scan of the f32 rows (the first batch)
gt = B.ground_truth(r_f, q[:nq], k, "f32")
out["recall_at_%d" % k] = {}
for leg in ("a_f32_walk", "b_int8_walk", "c_refined_fused"):
    LEGS[leg](0, nq)
    torch.cuda.synchronize()
    out["recall_at_%d" % k][leg] = round(B.recall(gt, ids[:nq], k), 4)
out["recall_at_%d" % k]["queries"] = nq
bench.log("recall:", out["recall_at_%d" % k])

out["batches_of_%d" % nq] = run_shape("stream of %d-query calls" % nq, [(i * nq, nq) for i in range(nb)])
out["one_call_of_%d" % big] = run_shape("one call of %d" % big, [(0, big)])
out["walk_status_words"] = [int(x) for x in status.cpu().numpy()]

os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({"refine_bench": opt.out, "condition_batches": out["batches_of_%d" % nq]["condition"],
                  "condition_one_call": out["one_call_of_%d" % big]["condition"]}))
