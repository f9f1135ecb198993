#!/usr/bin/env python
"""knn_graph_filtered and range_graph_filtered (granne_amd/csrc/graph_filtered_host.h) next to what a caller
had before them, in one process, on the benchmark's mixture rows: random shared filters of a few selectivities, the WHOLE
subset graph in one call (k = 10; one radius class: the median 10th distance of the unfiltered knn_graph over the first 8,192
elements, cap 32), f32 and int8.

  filtered      one *_graph_filtered_device call over all positions of the filter's id list, results left on the device
  composition   the subset's rows gathered into a second handle (its creation included), knn_graph / range_graph on it, the
                ids mapped through the id list on the host

The two answers are asserted equal -- elements, ids, distance bytes, counts, totals -- in the same run. Writes
profiles/graph_filtered.json, `slower_than_composition` per case included.

  python tools/graph_filtered_bench.py [--elements 1000000] [--dim 100] [--reps 5] [--dtypes f32,i8] [--selectivities 0.5,0.1,0.01]
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--cap", type=int, default=32)
ap.add_argument("--selectivities", default="0.5,0.1,0.01")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_filtered.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
n, dim, k, cap, s = opt.elements, opt.dim, opt.k, opt.cap, B.stream
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
out = {"workload": "%d x %d-d mixture; the whole graph of a random subset, k = %d and one radius class (cap %d)" % (n, dim, k, cap),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "wall clock around calls ending in a device synchronisation; the two legs interleaved inside every repeat; median of %d "
                 "repeats after one warm-up round; the composition includes the gather, the second handle's creation and the host's id "
                 "translation" % opt.reps,
       "dtypes": {}}


def wall(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def through(A, ids):
    """ids of the second handle -> ids of the first"""
    o = ids.copy()
    o[ids != NONE] = A[ids[ids != NONE].astype(np.intp)]
    return o


for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    et = "angular" if dtype == "f32" else "angular_int"
    g = ga.Granne.from_device(et, rows.data_ptr(), n, dim, [], [], [])
    radius = float(np.median(g.knn_graph(10, 0, min(8192, n))[1][:, 9]))
    rec = {"radius": radius}
    for sel in [float(x) for x in opt.selectivities.split(",")]:
        mask = np.random.default_rng(bench.SEED + int(sel * 1000)).random(n) < sel
        f = ga.Filter.from_mask(mask, 0)
        A = np.nonzero(mask)[0].astype(np.uint64)
        m = len(A)
        d_A = torch.from_numpy(A.astype(np.int64)).cuda()
        for kind, width in (("knn", k), ("range", cap)):
            el = torch.empty(m, dtype=torch.int64, device="cuda")
            ids = torch.empty((m, width), dtype=torch.int64, device="cuda")
            ds = torch.empty((m, width), dtype=torch.float32, device="cuda")
            cnt, tot = torch.empty(m, dtype=torch.int32, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda")
            st = torch.zeros(4, dtype=torch.int32, device="cuda")
            d_r = torch.full((m,), radius, dtype=torch.float32, device="cuda")

            def filtered(status=0):
                if kind == "knn":
                    g.knn_graph_filtered_device(f.ptr, 0, m, k, el.data_ptr(), ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), status, s)
                else:
                    g.range_graph_filtered_device(f.ptr, 0, m, d_r.data_ptr(), cap, el.data_ptr(), ids.data_ptr(), ds.data_ptr(),
                                                  cnt.data_ptr(), tot.data_ptr(), status, s)

            def composition():
                sub = rows[d_A].contiguous()
                g2 = ga.Granne.from_device(et, sub.data_ptr(), m, dim, [], [], [])
                r = g2.knn_graph(k) if kind == "knn" else g2.range_graph(radius, cap)
                g2.close()
                return (through(A, r[0]),) + tuple(r[1:])

            legs = {"filtered": filtered, "composition": composition}
            ms = {name: [] for name in legs}
            for rep in range(opt.reps + 1):  # round 0 warms up
                for name, call in legs.items():
                    t, r = wall(call)
                    if rep:
                        ms[name].append(t)
                    if name == "composition":
                        comp = r
                print(dtype, sel, kind, "repeat", rep, {name: v[-1:] for name, v in ms.items()}, file=sys.stderr, flush=True)
            filtered(st.data_ptr())
            torch.cuda.synchronize()
            got = [ids.cpu().numpy().astype(np.uint64), ds.cpu().numpy(), cnt.cpu().numpy().astype(np.uint32)]
            if kind == "range":
                got.append(tot.cpu().numpy().astype(np.uint32))
            equal = bool((el.cpu().numpy().astype(np.uint64) == A).all()) and all(a.tobytes() == b.tobytes() for a, b in zip(got, comp))
            assert equal, (dtype, sel, kind)
            r = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
            r["allowed"] = m
            r["status"] = st.cpu().numpy().astype(np.uint32).tolist()
            r["equal_to_composition"] = equal
            r["composition_over_filtered"] = r["composition"]["ms"] / r["filtered"]["ms"]
            r["slower_than_composition"] = r["filtered"]["ms"] > r["composition"]["ms"]
            if kind == "range":
                r["mean_total"], r["largest_total"] = float(got[3].mean()), int(got[3].max())
            rec["%s_sel%g" % (kind, sel)] = r
            print(dtype, sel, kind, json.dumps(r), file=sys.stderr, flush=True)
            del el, ids, ds, cnt, tot, d_r
        f.close()
        del d_A
    out["dtypes"][dtype] = rec
    g.close()
    del rows, g
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
