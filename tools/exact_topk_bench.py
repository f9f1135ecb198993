#!/usr/bin/env python
"""exact_topk on its own (granne_hip_exact_topk_device, granne_amd/csrc/exact_topk.h) next to the matrix-core scan it is
the yardstick of: per element type, exact_topk at k = 10, 100 and 1024, brute_force at k = 10 in the same process, how
many of the nq x 10 ids the two share, and the CPU oracle's scan on a 32-query sample (time, and whether exact_topk's ids
and distance bytes equal it). Writes profiles/exact_topk.json.

  python tools/exact_topk_bench.py [--n 10000000] [--dim 100] [--nq 1024] [--reps 3] [--dtypes f32,i8] [--out profiles/exact_topk.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED = 0x6772616E6E65 + 900


def synth(L, lib_mod, torch, seed, rows, dim, dtype):
    """`rows` prepared rows of the synthetic set `seed` on the device, in chunks of 2M raw f32 rows"""
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty((rows, dim), dtype=torch.float32 if dtype == "f32" else torch.int8, device="cuda")
    for r0 in range(0, rows, 2_000_000):
        m = min(2_000_000, rows - r0)
        raw = torch.empty((m, dim), dtype=torch.float32, device="cuda")
        lib_mod.check(L.granne_hip_synth_rows_device(C.c_void_p(raw.data_ptr()), seed, r0, m, dim, 0, sp))
        if dtype == "f32":
            lib_mod.check(L.granne_hip_normalize_f32_device(C.c_void_p(raw.data_ptr()), m, dim, 0, sp))
            out[r0:r0 + m] = raw
        else:
            lib_mod.check(L.granne_hip_quantize_f32_device(C.c_void_p(raw.data_ptr()), C.c_void_p(out[r0:r0 + m].data_ptr()), m, dim, 0, sp))
        torch.cuda.synchronize()
    return out


def timed(torch, reps, call):
    """milliseconds of `call` on the current stream: the best and all of `reps` runs after one warm-up"""
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="f32,i8")
    ap.add_argument("--sample", type=int, default=32, help="queries the CPU oracle scans (0: none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_topk.json"))
    a = ap.parse_args()
    import torch
    import granne_amd
    from granne_amd import _lib
    L = _lib.lib()
    result = {"n": a.n, "dim": a.dim, "nq": a.nq, "reps": a.reps, "device": torch.cuda.get_device_name(0), "runs": {}}
    for dtype in a.dtypes.split(","):
        el = synth(L, _lib, torch, SEED, a.n, a.dim, dtype)
        q = synth(L, _lib, torch, SEED + 1, a.nq, a.dim, dtype)
        et = "angular" if dtype == "f32" else "angular_int"
        ix = granne_amd.Granne.from_device(et, el.data_ptr(), a.n, a.dim, [], [], [])
        stream = torch.cuda.current_stream().cuda_stream
        tq = q.view(torch.uint8).reshape(a.nq, -1).contiguous()
        run = {}
        ids10 = None
        for k in (10, 100, 1024):
            ids = torch.empty((a.nq, k), dtype=torch.int64, device="cuda")
            ds = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
            cnt = torch.empty(a.nq, dtype=torch.int32, device="cuda")
            st = torch.zeros(4, dtype=torch.int32, device="cuda")
            best, ms = timed(torch, a.reps, lambda: ix.exact_topk_device(tq.data_ptr(), a.nq, k, ids.data_ptr(), ds.data_ptr(),
                                                                         cnt.data_ptr(), st.data_ptr(), stream))
            status = (st.cpu().numpy().astype(np.int64) // (a.reps + 1)).tolist()  # the words accumulate over the calls
            status[2] = int(st[2].item())
            run["exact_topk_k%d" % k] = {"ms": best, "all_ms": ms, "status": status, "queries_per_s": a.nq / best * 1e3}
            if k == 10:
                ids10, ds10 = ids.cpu().numpy(), ds.cpu().numpy()
        bi = torch.empty((a.nq, 10), dtype=torch.int64, device="cuda")
        bd = torch.empty((a.nq, 10), dtype=torch.float32, device="cuda")
        bc = torch.empty(a.nq, dtype=torch.int32, device="cuda")
        best, ms = timed(torch, a.reps, lambda: ix.brute_force_device(tq.data_ptr(), a.nq, 10, bi.data_ptr(), bd.data_ptr(), bc.data_ptr(), stream))
        run["brute_force_k10"] = {"ms": best, "all_ms": ms, "last_scan": _lib.last_scan(ix.get_option(_lib.OPT_LAST_SCAN))}
        run["exact_over_brute_force_k10"] = run["exact_topk_k10"]["ms"] / best
        run["ids_shared_k10"] = int((bi.cpu().numpy() == ids10).sum())
        run["ids_total_k10"] = a.nq * 10
        if a.sample:
            from oracle import oracle
            oracle.build()
            hq = q[:a.sample].cpu().numpy()
            sec, oi, od = oracle.Index(el.cpu().numpy(), []).scan_topk(hq, 10)
            run["oracle_scan_k10"] = {"queries": a.sample, "seconds": sec, "queries_per_s": a.sample / sec,
                                      "exact_topk_ids_equal": bool((oi == ids10[:a.sample].astype(np.uint64)).all()),
                                      "exact_topk_dist_bytes_equal": od.tobytes() == ds10[:a.sample].tobytes()}
        result["runs"][dtype] = run
        print(dtype, json.dumps(run), file=sys.stderr)
        ix.close()
        del el, q, ix
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
