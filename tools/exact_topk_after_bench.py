#!/usr/bin/env python
"""exact_topk_screened_after at pages 1, 2, 5 and 10 of k = 1024, next to exact_topk_screened(k = 1024) --
what a first page cost before there was a cursor -- and to exact_topk_after, the unscreened form whose answer it must equal,
in one process. The cursors of page p are the last entries of page p - 1, made untimed by exact_topk_after page after page.
Per page the three legs run interleaved, one warm-up round first, medians of --reps rounds, device events around each call
(the screened calls wait on the stream at their end themselves). Per page: the times, the screened call's status words
(from a separate untimed call) and whether all nq x k ids, distance bytes and counts equal the unscreened entry's.
Writes profiles/exact_topk_after.json.

  python tools/exact_topk_after_bench.py [--n 1000000] [--dim 100] [--nq 1024] [--reps 5] [--dtypes f32,i8]
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

K, PAGES = 1024, (1, 2, 5, 10)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,i8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_topk_after.json"))
    a = ap.parse_args()
    import torch
    import granne_amd
    from granne_amd import _lib
    L = _lib.lib()
    result = {"n": a.n, "dim": a.dim, "nq": a.nq, "k": K, "reps": a.reps, "device": torch.cuda.get_device_name(0),
              "method": "legs interleaved per page, one warm-up round, medians, device events", "runs": {}}
    for dtype in a.dtypes.split(","):
        el = synth(L, _lib, torch, SEED, a.n, a.dim, dtype)
        q = synth(L, _lib, torch, SEED + 1, a.nq, a.dim, dtype)
        ix = granne_amd.Granne.from_device("angular" if dtype == "f32" else "angular_int", el.data_ptr(), a.n, a.dim, [], [], [])
        del el
        torch.cuda.empty_cache()
        stream = torch.cuda.current_stream().cuda_stream
        tq = q.view(torch.uint8).reshape(a.nq, -1).contiguous()

        def buffers():
            return (torch.empty((a.nq, K), dtype=torch.int64, device="cuda"), torch.empty((a.nq, K), dtype=torch.float32, device="cuda"),
                    torch.empty(a.nq, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"))
        si, sd, sc, sst = buffers()
        xi, xd, xc, _ = buffers()
        pi, pd, pc, _ = buffers()
        # page p's cursors: the last entries of page p - 1 (page 1: the sentinel id, no cursor)
        cursors = {1: (torch.zeros(a.nq, dtype=torch.float32, device="cuda"), torch.full((a.nq,), -1, dtype=torch.int64, device="cuda"))}
        for p in range(2, max(PAGES) + 1):
            ad, ai = cursors[p - 1]
            ix.exact_topk_after_device(tq.data_ptr(), a.nq, K, ad.data_ptr(), ai.data_ptr(), 0, 0, xi.data_ptr(), xd.data_ptr(), xc.data_ptr(), 0, stream)
            torch.cuda.synchronize()
            assert bool((xc == K).all().item())
            cursors[p] = (xd[:, -1].clone(), xi[:, -1].clone())
        run = {"epsilon": float(L.granne_hip_exact_topk_screen_epsilon(0 if dtype == "f32" else 1, a.dim))}
        for p in PAGES:
            ad, ai = cursors[p]
            args = (tq.data_ptr(), a.nq, K, ad.data_ptr(), ai.data_ptr(), 0, 0)
            legs = {"screened_after": lambda: ix.exact_topk_screened_after_device(*args, si.data_ptr(), sd.data_ptr(), sc.data_ptr(), 0, stream),
                    "exact_topk_screened_first_page": lambda: ix.exact_topk_screened_device(tq.data_ptr(), a.nq, K, pi.data_ptr(), pd.data_ptr(),
                                                                                            pc.data_ptr(), 0, stream),
                    "exact_topk_after": lambda: ix.exact_topk_after_device(*args, xi.data_ptr(), xd.data_ptr(), xc.data_ptr(), 0, stream)}
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
            ix.exact_topk_screened_after_device(*args, si.data_ptr(), sd.data_ptr(), sc.data_ptr(), sst.data_ptr(), stream)
            torch.cuda.synchronize()
            rec = {name: {"ms": statistics.median(v), "all_ms": v} for name, v in ms.items()}
            rec["status"] = sst.cpu().numpy().astype(np.uint32).tolist()
            sst.zero_()
            rec["ids_equal_exact_topk_after"] = bool((si == xi).all().item())
            rec["dist_bytes_equal_exact_topk_after"] = bool((sd.view(torch.int32) == xd.view(torch.int32)).all().item())
            rec["counts_equal_exact_topk_after"] = bool((sc == xc).all().item())
            rec["over_first_page"] = rec["screened_after"]["ms"] / rec["exact_topk_screened_first_page"]["ms"]
            run["page%d" % p] = rec
            print(dtype, p, json.dumps(rec), file=sys.stderr)
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
