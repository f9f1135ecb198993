#!/usr/bin/env python
"""knn_graph (granne_amd/csrc/knn_graph_host.h) next to what a caller had before it, in one process, on the
benchmark's mixture rows (f32 and int8, k = 10 and 100). Three legs, interleaved inside every repeat, medians of --reps
repeats after one warm-up round, wall-clock milliseconds around calls that end with a device synchronisation:

  knn_graph     the whole graph by one knn_graph_device call, results left on the device
  composition   get_element per row -> exact_topk_screened(k + 1) in calls of 1,024 rows -> the element stripped on the host,
                over the first --sample elements, SCALED to the whole graph (the whole of it is a million get_element calls)
  exact_topk    exact_topk_device(k + 1) over 1,024 rows gathered on the device, SCALED to the whole graph

The composition's answer for the sampled elements is asserted equal -- ids, distance bytes, counts -- to knn_graph's rows of
the same run (the data holds no bit-copies among them: asserted too). Writes profiles/knn_graph.json.

  python tools/knn_graph_bench.py [--elements 1000000] [--dim 100] [--sample 8192] [--reps 5] [--dtypes f32,i8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--sample", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ks", default="10,100")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_graph.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
n, dim, sample, s = opt.elements, opt.dim, min(opt.sample, opt.elements), B.stream
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
out = {"workload": "%d x %d-d mixture; the whole k-NN graph" % (n, dim), "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "wall clock around calls ending in a device synchronisation; the three legs interleaved inside every repeat; median of %d "
                 "repeats after one warm-up round; composition measured over the first %d elements and exact_topk over 1024, both scaled "
                 "by elements / measured" % (opt.reps, sample),
       "dtypes": {}}


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    g = ga.Granne.from_device("angular" if dtype == "f32" else "angular_int", rows.data_ptr(), n, dim, [], [], [])
    rec = {}
    for k in [int(x) for x in opt.ks.split(",")]:
        ids = torch.empty((n, k), dtype=torch.int64, device="cuda")
        ds = torch.empty((n, k), dtype=torch.float32, device="cuda")
        cnt = torch.empty(n, dtype=torch.int32, device="cuda")
        st = torch.zeros(4, dtype=torch.int32, device="cuda")
        xi, xd = torch.empty((1024, k + 1), dtype=torch.int64, device="cuda"), torch.empty((1024, k + 1), dtype=torch.float32, device="cuda")
        xc = torch.empty(1024, dtype=torch.int32, device="cuda")

        def composition():
            got = []
            for lo in range(0, sample, 1024):
                es = np.arange(lo, min(lo + 1024, sample))
                q = np.stack([g.get_element(int(e)) for e in es])
                ci, cd, _ = g.exact_topk_screened(q, k + 1)
                keep = ci != es[:, None].astype(np.uint64)
                keep &= np.cumsum(keep, axis=1) <= k  # (the element is listed: one entry leaves; it is not: the last one does)
                assert (keep.sum(axis=1) == k).all()
                got.append((ci[keep].reshape(-1, k), cd[keep].reshape(-1, k)))
            return np.concatenate([a for a, _ in got]), np.concatenate([b for _, b in got])

        def exact_topk():
            q = rows[:1024].contiguous()
            g.exact_topk_device(q.data_ptr(), 1024, k + 1, xi.data_ptr(), xd.data_ptr(), xc.data_ptr(), 0, s)

        legs = {"knn_graph": (lambda: g.knn_graph_device(0, n, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), 0, s), 1.0),
                "composition": (composition, n / sample), "exact_topk": (exact_topk, n / 1024)}
        ms = {name: [] for name in legs}
        for rep in range(opt.reps + 1):  # round 0 warms up
            for name, (call, scale) in legs.items():
                t, r = wall(call)
                if rep:
                    ms[name].append(t * scale)
                if name == "composition":
                    comp = r
            print(dtype, k, "repeat", rep, {name: v[-1:] for name, v in ms.items()}, file=sys.stderr, flush=True)
        g.knn_graph_device(0, n, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        gi, gd = ids[:sample].cpu().numpy().astype(np.uint64), ds[:sample].cpu().numpy()
        no_copies = bool((gd[:, 0] > 0).all())  # (a bit-copy of an element lies at the clamp)
        equal = gi.tobytes() == comp[0].tobytes() and gd.tobytes() == comp[1].tobytes() and bool((cnt == k).all().item())
        assert no_copies and equal, (dtype, k, no_copies, equal)
        r = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
        r["status"] = st.cpu().numpy().astype(np.uint32).tolist()
        r["equal_to_composition"] = {"elements": sample, "ids": True, "dist_bytes": True, "counts": True, "no_bit_copies": no_copies}
        r["composition_over_knn_graph"] = r["composition"]["ms"] / r["knn_graph"]["ms"]
        r["exact_topk_over_knn_graph"] = r["exact_topk"]["ms"] / r["knn_graph"]["ms"]
        rec["k%d" % k] = r
        print(dtype, k, json.dumps(r), file=sys.stderr, flush=True)
        del ids, ds, cnt
    out["dtypes"][dtype] = rec
    g.close()
    del rows, g
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
