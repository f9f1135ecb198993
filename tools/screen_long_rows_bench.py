#!/usr/bin/env python
"""The long-row forms of exact_topk_screened (granne_hip_index_screen_long_rows) next to the routed path of
the same handle -- the switch off: exact_topk's scan, what such a handle got before -- and to brute_force (k = 10), in one
process: per shape and k = 10, 100, 1024 the legs run interleaved (long, routed, brute_force, long, ...), one warm-up round
first, medians of --reps rounds. Per k: the times, the long call's status words (from a separate untimed call; [0] the
queries that fell back, [2] the largest number of survivors of a query), and whether all nq x k ids, distance bytes and
the counts equal the routed leg's. Writes profiles/screen_long_rows.json.

  python tools/screen_long_rows_bench.py [--n 1000000] [--nq 1024] [--reps 5] [--shapes f32:768,i8:1024]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from exact_topk_bench import SEED, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="f32:768,i8:1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen_long_rows.json"))
    a = ap.parse_args()
    import torch
    import granne_amd
    from granne_amd import _lib
    L = _lib.lib()
    result = {"n": a.n, "nq": a.nq, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "method": "legs interleaved, one warm-up round, medians", "runs": {}}
    for shape in a.shapes.split(","):
        dtype, dim = shape.split(":")[0], int(shape.split(":")[1])
        el = synth(L, _lib, torch, SEED, a.n, dim, dtype)
        q = synth(L, _lib, torch, SEED + 1, a.nq, dim, dtype)
        ix = granne_amd.Granne.from_device("angular" if dtype == "f32" else "angular_int", el.data_ptr(), a.n, dim, [], [], [])
        del el
        torch.cuda.empty_cache()
        stream = torch.cuda.current_stream().cuda_stream
        tq = q.view(torch.uint8).reshape(a.nq, -1).contiguous()
        run = {"dim": dim, "epsilon_long": float(L.granne_hip_exact_topk_screen_epsilon_long(0 if dtype == "f32" else 1, dim))}
        for k in (10, 100, 1024):
            def buffers(kk=k):
                return (torch.empty((a.nq, kk), dtype=torch.int64, device="cuda"), torch.empty((a.nq, kk), dtype=torch.float32, device="cuda"),
                        torch.empty(a.nq, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
            si, sd, sc, sst = buffers()
            xi, xd, xc, xst = buffers()
            bi, bd, bc, _ = buffers(10)

            def screened(on, ids, ds, cnt, st=None):
                ix.screen_long_rows(on)
                ix.exact_topk_screened_device(tq.data_ptr(), a.nq, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), st.data_ptr() if st is not None else 0,
                                              stream)
            legs = {"long": lambda: screened(True, si, sd, sc), "routed": lambda: screened(False, xi, xd, xc)}
            if k == 10:
                legs["brute_force"] = lambda: ix.brute_force_device(tq.data_ptr(), a.nq, 10, bi.data_ptr(), bd.data_ptr(), bc.data_ptr(), stream)
            ms = {name: [] for name in legs}
            for rep in range(a.reps + 1):  # round 0 warms up
                for name, call in legs.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    call()
                    t1.record()
                    torch.cuda.synchronize()
                    if rep:
                        ms[name].append(t0.elapsed_time(t1))
            screened(True, si, sd, sc, sst)
            screened(False, xi, xd, xc, xst)
            torch.cuda.synchronize()
            rec = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
            rec["status"] = sst.cpu().numpy().astype(np.uint32).tolist()
            rec["routed_status"] = xst.cpu().numpy().astype(np.uint32).tolist()
            rec["ids_equal_routed"] = bool((si == xi).all().item())
            rec["dist_bytes_equal_routed"] = bool((sd.view(torch.int32) == xd.view(torch.int32)).all().item())
            rec["counts_equal_routed"] = bool((sc == xc).all().item())
            rec["routed_over_long"] = rec["routed"]["ms"] / rec["long"]["ms"]
            run["k%d" % k] = rec
            print(shape, k, json.dumps(rec), file=sys.stderr)
        result["runs"][shape] = run
        ix.close()
        del q, ix
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
