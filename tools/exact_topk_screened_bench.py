#!/usr/bin/env python
"""exact_topk_screened (granne_amd/csrc/exact_topk_screened.h) next to exact_topk, whose answer it is defined as, and to
brute_force (k = 10), in one process: per element type and k = 10, 100, 1024 the legs run interleaved (screened, exact,
brute_force, screened, ...), one warm-up round first, medians of --reps rounds. Per leg: the time, the screened call's status
words (read from a separate untimed call; [2] is the largest number of survivors of a query), and whether all nq x k ids and distance bytes
equal exact_topk's. Writes profiles/exact_topk_screened.json.

  python tools/exact_topk_screened_bench.py [--n 10000000] [--dim 100] [--nq 1024] [--reps 5] [--dtypes f32,i8]
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
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,i8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_topk_screened.json"))
    a = ap.parse_args()
    import torch
    import granne_amd
    from granne_amd import _lib
    L = _lib.lib()
    result = {"n": a.n, "dim": a.dim, "nq": a.nq, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "method": "legs interleaved, one warm-up round, medians", "runs": {}}
    for dtype in a.dtypes.split(","):
        el = synth(L, _lib, torch, SEED, a.n, a.dim, dtype)
        q = synth(L, _lib, torch, SEED + 1, a.nq, a.dim, dtype)
        ix = granne_amd.Granne.from_device("angular" if dtype == "f32" else "angular_int", el.data_ptr(), a.n, a.dim, [], [], [])
        del el
        torch.cuda.empty_cache()
        stream = torch.cuda.current_stream().cuda_stream
        tq = q.view(torch.uint8).reshape(a.nq, -1).contiguous()
        run = {"epsilon": float(L.granne_hip_exact_topk_screen_epsilon(0 if dtype == "f32" else 1, a.dim))}
        for k in (10, 100, 1024):
            def buffers(kk=k):
                return (torch.empty((a.nq, kk), dtype=torch.int64, device="cuda"), torch.empty((a.nq, kk), dtype=torch.float32, device="cuda"),
                        torch.empty(a.nq, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
            si, sd, sc, sst = buffers()
            xi, xd, xc, xst = buffers()
            bi, bd, bc, _ = buffers(10)
            legs = {"screened": lambda: ix.exact_topk_screened_device(tq.data_ptr(), a.nq, k, si.data_ptr(), sd.data_ptr(), sc.data_ptr(), 0, stream),
                    "exact_topk": lambda: ix.exact_topk_device(tq.data_ptr(), a.nq, k, xi.data_ptr(), xd.data_ptr(), xc.data_ptr(), 0, stream)}
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
            ix.exact_topk_screened_device(tq.data_ptr(), a.nq, k, si.data_ptr(), sd.data_ptr(), sc.data_ptr(), sst.data_ptr(), stream)
            torch.cuda.synchronize()
            rec = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
            rec["status"] = sst.cpu().numpy().astype(np.uint32).tolist()
            rec["ids_equal_exact_topk"] = bool((si == xi).all().item())
            rec["dist_bytes_equal_exact_topk"] = bool((sd.view(torch.int32) == xd.view(torch.int32)).all().item())
            rec["counts_equal_exact_topk"] = bool((sc == xc).all().item())
            rec["exact_topk_over_screened"] = rec["exact_topk"]["ms"] / rec["screened"]["ms"]
            run["k%d" % k] = rec
            print(dtype, k, json.dumps(rec), file=sys.stderr)
        result["runs"][dtype] = run
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
