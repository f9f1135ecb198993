#!/usr/bin/env python
"""Half-precision rows measured: the int8 graph walked and re-ranked by "angular_f16" rows against the same walk re-ranked
by the f32 rows -- and, for orientation only, the f16 graph on the general walker next to the f32 graph on the register
walker.

    python tools/f16_bench.py [--elements 10000000] [--data mixture] [--out profiles/f16_rows.json]

Builds the int8 graph, the f32 graph and the f16 graph (GPU builder, the reference's default config) over the benchmark's
structured data set, and a rows-only handle of the f32 rows and of their f16 copy. Times at ef 50, k 10, m 50 with HIP
events, the legs interleaved inside every repeat (one process, one device):
    r32  int8 walk + f32 re-rank (fused)     r16  int8 walk + f16 re-rank (fused)     -- the comparison
    x32  the f32 re-rank kernel alone        x16  the f16 re-rank kernel alone        -- over the lists of one int8 walk
    w32  f32 walk (register walker)          w16  f16 walk (general walker)           -- orientation, no claim
once as a stream of 1024-query calls and once as one call of 20,480 queries, and records queries/s per leg, recall@10 of
every leg against the exact scan of the f32 rows, the overlap of r16's and r32's answers, and the HBM bytes of each rows
handle. The f32 re-rank is the baseline of the same build and the same run, not the code under test. Not part of bench.py."""
import argparse
import ctypes as C
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
ap.add_argument("--no-walks", action="store_true", help="skip the two orientation legs (and the f32 and f16 graphs they need)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_rows.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402
import time  # noqa: E402

args = bench.parse()  # the reference's default build config: num_neighbors 30, max_search 200, reinsertion
B = bench.Bench(args)
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402

n, dim, ef, k, m, nq, nb = opt.elements, opt.dim, opt.ef, opt.k, opt.refine_from, opt.batch, opt.batches
big = nq * nb
s = B.stream

rows = B.rows(opt.data, bench.SEED + 100, 0, n, dim, "f32")
rows16 = torch.empty((n, dim), dtype=torch.float16, device="cuda")
_lib.check(B.lib.granne_hip_f32_to_f16_device(C.c_void_p(rows.data_ptr()), C.c_void_p(rows16.data_ptr()), n, dim, B.dev, B.sp))
torch.cuda.synchronize()
rows8 = B.prepare(rows.clone(), "i8")  # angular_int::Vector::from of the normalised rows
b_8, g_8, t_8 = B.build_index(rows8, "i8")
del b_8, rows8
r_32 = ga.Granne.from_device("angular", rows.data_ptr(), n, dim, [], [], [], device=B.dev, stream=s)
r_16 = ga.Granne.from_device("angular_f16", rows16.data_ptr(), n, dim, [], [], [], device=B.dev, stream=s)
torch.cuda.synchronize()
g_32 = g_16 = None
t_32 = t_16 = 0.0
if not opt.no_walks:
    b_32, g_32, t_32 = B.build_index(rows, "f32")
    del b_32
    t0 = time.time()
    b_16 = ga.GranneBuilder.from_device("angular_f16", rows16.data_ptr(), n, dim, device=B.dev, stream=s, num_neighbors=args.num_neighbors,
                                        max_search=args.build_max_search, reinsert_elements=bool(args.build_reinsert),
                                        batch_max=args.batch_max, show_progress=False)
    b_16.build()
    g_16 = b_16.get_index()
    torch.cuda.synchronize()
    t_16 = time.time() - t0
    del b_16
del rows, rows16
torch.cuda.empty_cache()
bench.log("built: int8 graph %.1f s, f32 graph %.1f s, f16 graph %.1f s; rows handles f32 %.2f GB, f16 %.2f GB" %
          (t_8, t_32, t_16, r_32.hbm_bytes() / 1e9, r_16.hbm_bytes() / 1e9))

q = B.rows(opt.data, bench.SEED + 1, 0, big, dim, "f32")  # queries from the elements' distribution, disjoint seed
q8 = B.prepare(q.clone(), "i8")
rg32, rg16 = ga.RefinedGranne(g_8, r_32), ga.RefinedGranne(g_8, r_16)

ids = torch.empty((big, k), dtype=torch.int64, device="cuda")
ds = torch.empty((big, k), dtype=torch.float32, device="cuda")
cnt = torch.empty(big, dtype=torch.int32, device="cuda")
status = torch.zeros(8, dtype=torch.int32, device="cuda")


def refined(rg):
    def leg(lo, cn):
        rg.search_batch_device(q8[lo:].data_ptr(), q[lo:].data_ptr(), cn, ef, m, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0,
                               status.data_ptr(), status[4:].data_ptr(), s)
    return leg


def walk(g):
    def leg(lo, cn):
        g.search_batch_device(q[lo:].data_ptr(), cn, ef, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0, status.data_ptr(), s)
    return leg


# the re-rank kernel alone, over the lists of one int8 walk with num_neighbors = m
c_ids = torch.empty((big, m), dtype=torch.int64, device="cuda")
c_ds = torch.empty((big, m), dtype=torch.float32, device="cuda")
c_cnt = torch.empty(big, dtype=torch.int32, device="cuda")
g_8.search_batch_device(q8.data_ptr(), big, ef, m, c_ids.data_ptr(), c_ds.data_ptr(), c_cnt.data_ptr(), 0, status.data_ptr(), s)
torch.cuda.synchronize()


def rerank(r):
    def leg(lo, cn):
        r.refine_device(q[lo:].data_ptr(), cn, c_ids[lo:].data_ptr(), c_cnt[lo:].data_ptr(), m, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(),
                        cnt[lo:].data_ptr(), status[4:].data_ptr(), s)
    return leg


LEGS = {"r32_int8_walk_f32_rerank": refined(rg32), "r16_int8_walk_f16_rerank": refined(rg16),
        "x32_f32_rerank_alone": rerank(r_32), "x16_f16_rerank_alone": rerank(r_16)}
if not opt.no_walks:
    LEGS["w32_f32_walk_register"] = walk(g_32)
    LEGS["w16_f16_walk_general"] = walk(g_16)


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
    a, b = rec["legs"]["r16_int8_walk_f16_rerank"], rec["legs"]["r32_int8_walk_f32_rerank"]
    spread = b["queries_per_s_max"] - b["queries_per_s_min"]
    rec["f16_over_f32_rerank"] = round(a["queries_per_s_median"] / b["queries_per_s_median"], 4)
    rec["f16_not_slower"] = {"what": "median r16 >= median r32 - the spread (max - min) of r32's own repeats", "r16_median": a["queries_per_s_median"],
                             "r32_median": b["queries_per_s_median"], "r32_spread": round(spread, 1),
                             "holds": bool(a["queries_per_s_median"] >= b["queries_per_s_median"] - spread)}
    rec["f16_over_f32_rerank_alone"] = round(rec["legs"]["x16_f16_rerank_alone"]["queries_per_s_median"] /
                                             rec["legs"]["x32_f32_rerank_alone"]["queries_per_s_median"], 4)
    bench.log(name, json.dumps({k_: v["queries_per_s_median"] for k_, v in rec["legs"].items()}), json.dumps(rec["f16_not_slower"]))
    return rec


out = {"workload": "%d x %d-d, %s, ef %d, k %d, refine_from %d; GPU builder, default config" % (n, dim, opt.data, ef, k, m),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "rows_handle_hbm_bytes": {"f32": r_32.hbm_bytes(), "f16": r_16.hbm_bytes()},
       "hbm_gb": {"int8_graph": round(g_8.hbm_bytes() / 1e9, 2), "f32_rows_handle": round(r_32.hbm_bytes() / 1e9, 2),
                  "f16_rows_handle": round(r_16.hbm_bytes() / 1e9, 2)},
       "timing": "HIP events around each run on one stream; legs interleaved inside every repeat; queries/s = queries of a run / its time",
       "note": "w32 / w16 are for orientation only: the f16 walk runs on the general walker (one wave per query, rows staged and normalised "
               "in LDS), the f32 walk on the register walker"}
if not opt.no_walks:
    out["hbm_gb"]["f32_graph"] = round(g_32.hbm_bytes() / 1e9, 2)
    out["hbm_gb"]["f16_graph"] = round(g_16.hbm_bytes() / 1e9, 2)
    out["build_s"] = {"int8_graph": round(t_8, 1), "f32_graph": round(t_32, 1), "f16_graph": round(t_16, 1)}

# recall@10 against the exact scan of the f32 rows (the first batch), and how far the two re-ranks agree
gt = B.ground_truth(r_32, q[:nq], k, "f32")
out["recall_at_%d" % k] = {}
answers = {}
for leg, fn in LEGS.items():
    fn(0, nq)
    torch.cuda.synchronize()
    out["recall_at_%d" % k][leg] = round(B.recall(gt, ids[:nq], k), 4)
    answers[leg] = ids[:nq].clone()
out["recall_at_%d" % k]["queries"] = nq
a16, a32 = answers["r16_int8_walk_f16_rerank"], answers["r32_int8_walk_f32_rerank"]
out["r16_vs_r32"] = {"top%d_overlap" % k: round(float((a16.unsqueeze(2) == a32.unsqueeze(1)).any(dim=2).float().mean().item()), 4),
                     "identical_lists": round(float((a16 == a32).all(dim=1).float().mean().item()), 4)}
bench.log("recall:", out["recall_at_%d" % k], "r16 vs r32:", out["r16_vs_r32"])
if not opt.no_walks:
    g_16.search_batch_device(q.data_ptr(), nq, ef, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), 0, status.data_ptr(), s)
    torch.cuda.synchronize()
    out["w16_walker"] = {_lib.WALKER_GENERAL: "general", _lib.WALKER_EXACT: "exact"}.get(g_16.get_option(_lib.OPT_LAST_WALKER), "register")

out["batches_of_%d" % nq] = run_shape("stream of %d-query calls" % nq, [(i * nq, nq) for i in range(nb)])
out["one_call_of_%d" % big] = run_shape("one call of %d" % big, [(0, big)])
out["walk_status_words"] = [int(x) for x in status.cpu().numpy()]

os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({"f16_bench": opt.out, "batches": out["batches_of_%d" % nq]["f16_not_slower"],
                  "one_call": out["one_call_of_%d" % big]["f16_not_slower"], "recall": out["recall_at_%d" % k]}))
