#!/usr/bin/env python
"""SumEmbeddings on one MI355X: materialise rate, and queries/s of the compact and the materialised index over the same
layers. Writes profiles/sum_embeddings_bench.json.

    python tools/sum_embeddings_bench.py [--n 10000000] [--dim 100] [--vocab 1000000,100000] [--build-n 0]

The layers are built by the GPU builder over the first --build-n elements (0: all) of the container; the compact and the
materialised index then share them, so the ratio compares the two element providers and nothing else."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def container(ga, rng, n, v, dim, mean_terms):
    cnt = rng.poisson(mean_terms, n).astype(np.uint64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(cnt)
    terms = np.minimum((rng.random(int(off[-1])) ** 2 * v).astype(np.int64), v - 1).astype(np.uint32)  # skewed: common words repeat
    tab = (rng.random((v, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    return ga.SumEmbeddings(tab, offsets=off, terms=terms), off, terms, tab


def timed_qps(ix, q, max_search, k, repeats):
    import torch
    nq = len(q)
    tq = torch.from_numpy(q).cuda()
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    run = lambda: ix.search_batch_device(tq.data_ptr(), nq, max_search, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), stream=s)  # noqa: E731
    run()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return nq / best, ids.cpu().numpy(), ds.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--vocab", default="1000000,100000")
    ap.add_argument("--mean-terms", type=float, default=6.0)
    ap.add_argument("--max-search", type=int, default=50)
    ap.add_argument("--batches", default="1024,20480")
    ap.add_argument("--build-max-search", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_embeddings_bench.json"))
    a = ap.parse_args()
    import torch
    import granne_amd as ga
    from granne_amd import _lib
    import ctypes as C
    records = []
    for v in [int(x) for x in a.vocab.split(",")]:
        rng = np.random.default_rng(v)
        se, off, terms, tab = container(ga, rng, a.n, v, a.dim, a.mean_terms)
        rec = dict(n=a.n, dim=a.dim, vocab=v, terms=int(off[-1]), container_hbm_bytes=se.hbm_bytes())
        # materialise: the normalised rows of every element into one device buffer
        out = torch.empty((a.n, a.dim), dtype=torch.float32, device="cuda")
        mat = lambda: _lib.check(_lib.lib().granne_hip_sum_embeddings_materialize_device(  # noqa: E731
            se._h, 0, a.n, 1, C.c_void_p(out.data_ptr()), a.dim, None))
        mat()
        torch.cuda.synchronize()
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            mat()
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        del out
        rec["materialise_s"] = best
        rec["materialise_out_bytes_per_s"] = a.n * a.dim * 4 / best
        rec["materialise_in_bytes_per_s"] = (int(off[-1]) * (4 + a.dim * 4) + 8 * a.n) / best  # ids + gathered table rows + offsets
        t0 = time.perf_counter()
        b = ga.GranneBuilder("embeddings", se, max_search=a.build_max_search)
        b.build()
        rec["build_s"] = time.perf_counter() - t0
        gix, cix = b.get_index(), b.get_index(compact=True)
        b.close()
        rec["materialised_hbm_bytes"], rec["compact_hbm_bytes"] = gix.hbm_bytes(), cix.hbm_bytes()
        for nq in [int(x) for x in a.batches.split(",")]:
            qoff = np.zeros(nq + 1, np.uint64)
            qoff[1:] = np.cumsum(np.maximum(rng.poisson(a.mean_terms, nq), 1))
            qt = np.minimum((rng.random(int(qoff[-1])) ** 2 * v).astype(np.int64), v - 1).astype(np.uint32)
            q = np.empty((nq, a.dim), np.float32)
            _lib.check(_lib.lib().granne_hip_sum_embeddings_embed(se._h, qoff.ctypes.data_as(C.c_void_p), qt.ctypes.data_as(C.c_void_p),
                                                                  nq, 1, q.ctypes.data_as(C.c_void_p)))
            mq, mi, md = timed_qps(gix, q, a.max_search, 10, a.repeats)
            cq, ci, cd = timed_qps(cix, q, a.max_search, 10, a.repeats)
            rec["batch_%d" % nq] = dict(materialised_qps=mq, compact_qps=cq, compact_over_materialised=cq / mq,
                                        same_bytes=bool((mi == ci).all() and md.tobytes() == cd.tobytes()))
        gix.close()
        cix.close()
        se.close()
        print(json.dumps(rec))
        records.append(rec)
    with open(a.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), max_search=a.max_search, records=records), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
