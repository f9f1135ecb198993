#!/usr/bin/env python
"""range_graph (granne_amd/csrc/range_graph_host.h) next to what a caller had before it, in one process, on
the benchmark's mixture rows (f32 and int8). One radius per class for every element: the median, over the first --sample
elements, of knn_graph's t-th distance for t = 1, 10, 100, 1000, and half the smallest nearest distance for the class "0";
the mean total each radius really gives is measured and written. Two legs, interleaved inside every repeat, medians of --reps
repeats after one warm-up round, wall-clock milliseconds around calls that end with a device synchronisation:

  range_graph   the whole graph by one range_graph_device call (cap 1023), results left on the device
  composition   get_element per row -> exact_range_screened(cap 1024) in calls of 1,024 rows -> the element struck out on the
                host, over the first --sample elements, SCALED to the whole graph

The composition's answer for the sampled elements is asserted equal -- ids, distance bytes, counts, totals -- to range_graph's
rows of the same run. Writes profiles/range_graph.json, `slower_than_composition` per class included.

  python tools/range_graph_bench.py [--elements 1000000] [--dim 100] [--sample 8192] [--reps 5] [--dtypes f32,i8]
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
ap.add_argument("--ts", default="0,1,10,100,1000")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_graph.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
n, dim, sample, s = opt.elements, opt.dim, min(opt.sample, opt.elements), B.stream
CAP = 1023  # the composition asks exact_range_screened for CAP + 1
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
ts = [int(x) for x in opt.ts.split(",")]
out = {"workload": "%d x %d-d mixture; every element's neighbours within a radius, cap %d" % (n, dim, CAP), "csrc_sha": bench.csrc_sha(),
       "device": torch.cuda.get_device_name(0),
       "timing": "wall clock around calls ending in a device synchronisation; the two legs interleaved inside every repeat; median of %d "
                 "repeats after one warm-up round; composition measured over the first %d elements and scaled by elements / measured"
                 % (opt.reps, sample),
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
    _, kd, _ = g.knn_graph(min(max(ts), n - 1), 0, sample)
    ids = torch.empty((n, CAP), dtype=torch.int64, device="cuda")
    ds = torch.empty((n, CAP), dtype=torch.float32, device="cuda")
    cnt = torch.empty(n, dtype=torch.int32, device="cuda")
    tot = torch.empty(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(4, dtype=torch.int32, device="cuda")
    rec = {}
    for t in ts:
        radius = float(kd[:, 0].min()) / 2 if t == 0 else float(np.median(kd[:, min(t, kd.shape[1]) - 1]))
        d_r = torch.full((n,), radius, dtype=torch.float32, device="cuda")

        def composition():
            got = []
            for lo in range(0, sample, 1024):
                es = np.arange(lo, min(lo + 1024, sample))
                q = np.stack([g.get_element(int(e)) for e in es])
                ci, cd, cc, ct = g.exact_range_screened(q, radius, CAP + 1)
                # the strip: e leaves the listing, and the total where it was listed (it is listed exactly when it was counted:
                # the data holds no CAP bit-copies of an element; the outputs' equality below would show one)
                valid = np.arange(CAP + 1)[None, :] < cc[:, None]
                is_e = (ci == es[:, None].astype(np.uint64)) & valid
                keep = valid & ~is_e
                keep &= np.cumsum(keep, axis=1) <= CAP
                front = np.argsort(~keep, axis=1, kind="stable")[:, :CAP]
                oi, od = np.take_along_axis(ci, front, axis=1), np.take_along_axis(cd, front, axis=1)
                kept = keep.sum(axis=1)
                pad = np.arange(CAP)[None, :] >= kept[:, None]
                oi[pad], od[pad] = NONE, np.inf
                got.append((oi, od, kept.astype(np.uint32), (ct - is_e.any(axis=1)).astype(np.uint32)))
            return [np.concatenate([x[i] for x in got]) for i in range(4)]

        legs = {"range_graph": (lambda: g.range_graph_device(0, n, d_r.data_ptr(), CAP, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                                             tot.data_ptr(), 0, s), 1.0),
                "composition": (composition, n / sample)}
        ms = {name: [] for name in legs}
        for rep in range(opt.reps + 1):  # round 0 warms up
            for name, (call, scale) in legs.items():
                tm, r = wall(call)
                if rep:
                    ms[name].append(tm * scale)
                if name == "composition":
                    comp = r
            print(dtype, t, "repeat", rep, {name: v[-1:] for name, v in ms.items()}, file=sys.stderr, flush=True)
        st.zero_()
        g.range_graph_device(0, n, d_r.data_ptr(), CAP, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), tot.data_ptr(), st.data_ptr(), s)
        torch.cuda.synchronize()
        got = (ids[:sample].cpu().numpy().astype(np.uint64), ds[:sample].cpu().numpy(), cnt[:sample].cpu().numpy().astype(np.uint32),
               tot[:sample].cpu().numpy().astype(np.uint32))
        equal = all(a.tobytes() == np.ascontiguousarray(b).astype(a.dtype).tobytes() for a, b in zip(got, comp))
        assert equal, (dtype, t)
        r = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
        r["radius"] = radius
        r["mean_total"] = float(tot.double().mean().item())
        r["max_total"] = int(tot.max().item())
        r["status"] = st.cpu().numpy().astype(np.uint32).tolist()
        r["equal_to_composition"] = {"elements": sample, "ids": True, "dist_bytes": True, "counts": True, "totals": True}
        r["composition_over_range_graph"] = r["composition"]["ms"] / r["range_graph"]["ms"]
        r["slower_than_composition"] = r["range_graph"]["ms"] > r["composition"]["ms"]
        rec["t%d" % t] = r
        print(dtype, t, json.dumps(r), file=sys.stderr, flush=True)
    out["dtypes"][dtype] = rec
    g.close()
    del rows, g, ids, ds, cnt, tot
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
