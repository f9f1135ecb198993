#!/usr/bin/env python
"""Refined search over a SumEmbeddings container measured: walk the int8 graph, re-rank by the container's term sums --
against the same walk re-ranked by dense rows, and against walks of the compact and of the materialised index.

    python tools/se_refine_bench.py [--elements 2000000] [--embeddings 200000] [--out profiles/se_refine.json]

A table of --embeddings x 100-d rows and --elements elements of six terms each, the terms drawn once uniformly and once
Zipf-like (P(rank r) ~ 1 / (r + 1), the ranks spread over the table by a fixed permutation), so that table rows repeat
as they do in text. Per data set, in one process on one device: the int8 rows from SumEmbeddings.to_rows_device and
their graph (GPU builder, the reference's default config), the f32 graph built over the container (materialised and
compact index over the same layers), a rows-only handle of halves; then five legs at ef 50, k 10, m 50, timed with HIP
events and interleaved inside every repeat:
    a  int8 walk + container re-rank (granne_hip_search_refined_sum_embeddings_batch_device)
    b  int8 walk + the materialised f32 rows        c  int8 walk + angular_f16 rows
    d  the compact index walked                     e  the materialised f32 index walked
once as a stream of 1024-query calls and once as one call of 20,480 queries; the re-rank kernel alone for a, b and c over
the walk's candidate lists; recall@10 of every leg against exact_topk on the materialised handle; the HBM bytes of the
handles a leg needs. (a) and (b) must return equal bytes: asserted. Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=2_000_000)
ap.add_argument("--embeddings", type=int, default=200_000)
ap.add_argument("--terms", type=int, default=6)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--data", default="uniform,zipf")
ap.add_argument("--ef", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--refine-from", type=int, default=50)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--batches", type=int, default=20, help="calls per timed run of the stream shape; one call of batch x batches is the other shape")
ap.add_argument("--passes", type=int, default=4, help="a timed run goes over its calls this many times")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se_refine.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()  # the reference's default build config: num_neighbors 30, max_search 200, reinsertion
B = bench.Bench(args)
torch, ga, lib, check = B.torch, B.ga, B.lib, B._lib.check
v, n, nt, dim = opt.embeddings, opt.elements, opt.terms, opt.dim
ef, k, m, nq, nb = opt.ef, opt.k, opt.refine_from, opt.batch, opt.batches
big = nq * nb
s = B.stream

table = B.mixture_raw(bench.SEED + 300, 0, v, dim)  # clustered, not normalised: what a trained embedding table looks like
gen = torch.Generator(device="cuda")
gen.manual_seed(bench.SEED + 301)
spread = torch.randperm(v, generator=gen, device="cuda")


def draw(kind, seed, count):
    """term ids [count, nt] (int64 on the device)"""
    gen.manual_seed(seed)
    if kind == "uniform":
        return torch.randint(0, v, (count, nt), generator=gen, device="cuda")
    u = torch.rand((count, nt), generator=gen, device="cuda", dtype=torch.float64)
    return spread[(float(v) ** u).long().sub_(1).clamp_(0, v - 1)]


def csr(ids):
    off = (torch.arange(ids.shape[0] + 1, device="cuda", dtype=torch.int64) * nt).contiguous()
    return off, ids.to(torch.int32).contiguous().view(-1)


def run_data(kind):
    off, terms = csr(draw(kind, bench.SEED + 310, n))
    torch.cuda.synchronize()
    se = ga.SumEmbeddings.from_device(table.data_ptr(), v, dim, off.data_ptr(), terms.data_ptr(), n, B.dev, s)
    distinct = int(torch.unique(terms).numel())
    del off, terms

    # the index that is walked: int8 rows made chunk by chunk from the container, and their graph
    rows8 = torch.empty((n, dim), dtype=torch.int8, device="cuda")
    se.to_rows_device("angular_int", rows8.data_ptr(), stream=s)
    b8, g8, t8 = B.build_index(rows8, "i8")
    del b8, rows8
    rows16 = torch.empty((n, dim), dtype=torch.float16, device="cuda")
    se.to_rows_device("angular_f16", rows16.data_ptr(), stream=s)
    r16 = ga.Granne.from_device("angular_f16", rows16.data_ptr(), n, dim, [], [], [], device=B.dev, stream=s)
    torch.cuda.synchronize()
    del rows16
    import time
    t0 = time.time()
    fb = ga.GranneBuilder("embeddings", se, num_neighbors=args.num_neighbors, max_search=args.build_max_search,
                          reinsert_elements=bool(args.build_reinsert), batch_max=args.batch_max)
    fb.build()
    mix, cix = fb.get_index(), fb.get_index(compact=True)
    torch.cuda.synchronize()
    tf = time.time() - t0
    del fb
    torch.cuda.empty_cache()
    bench.log("%s: %d distinct table rows named; int8 graph %.1f s, f32 graph %.1f s" % (kind, distinct, t8, tf))

    # queries: term lists from the elements' distribution, embedded and normalised through the container
    q_off, q_terms = csr(draw(kind, bench.SEED + 311, big))
    q = torch.empty((big, dim), dtype=torch.float32, device="cuda")
    check(lib.granne_hip_sum_embeddings_embed_device(se._h, C.c_void_p(q_off.data_ptr()), C.c_void_p(q_terms.data_ptr()), big, 1,
                                                     C.c_void_p(q.data_ptr()), dim, B.sp))
    q8 = B.prepare(q, "i8")
    torch.cuda.synchronize()

    ids = torch.empty((big, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((big, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(big, dtype=torch.int32, device="cuda")
    c_ids = torch.empty((big, m), dtype=torch.int64, device="cuda")
    c_ds = torch.empty((big, m), dtype=torch.float32, device="cuda")
    c_cnt = torch.empty(big, dtype=torch.int32, device="cuda")
    status = torch.zeros(8, dtype=torch.int32, device="cuda")
    sides = {"a_int8_walk_container_rerank": se, "b_int8_walk_f32_rows_rerank": mix, "c_int8_walk_f16_rows_rerank": r16}
    fused = {leg: ga.RefinedGranne(g8, side) for leg, side in sides.items()}

    def fused_leg(rg):
        def run(lo, cn):
            rg.search_batch_device(q8[lo:].data_ptr(), q[lo:].data_ptr(), cn, ef, m, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(),
                                   cnt[lo:].data_ptr(), 0, status.data_ptr(), status[4:].data_ptr(), s)
        return run

    def walk_leg(ix):
        def run(lo, cn):
            ix.search_batch_device(q[lo:].data_ptr(), cn, ef, k, ids[lo:].data_ptr(), ds[lo:].data_ptr(), cnt[lo:].data_ptr(), 0,
                                   status.data_ptr(), s)
        return run

    def rerank_leg(side):
        def run(lo, cn):
            side.refine_device(q[lo:].data_ptr(), cn, c_ids[lo:].data_ptr(), c_cnt[lo:].data_ptr(), m, k, ids[lo:].data_ptr(),
                               ds[lo:].data_ptr(), cnt[lo:].data_ptr(), status[4:].data_ptr(), s)
        return run

    legs = {leg: fused_leg(rg) for leg, rg in fused.items()}
    legs["d_compact_index_walked"] = walk_leg(cix)
    legs["e_materialised_f32_index_walked"] = walk_leg(mix)
    reranks = {leg.replace("int8_walk_", "") + "_alone": rerank_leg(side) for leg, side in sides.items()}

    def run_shape(name, which, calls):
        """calls: [(first query, count)] of one timed run. Legs interleaved inside every repeat; HIP events around each run."""
        calls = calls * opt.passes
        total = sum(c for _, c in calls)
        for _ in range(opt.warmup):
            for fn in which.values():
                for lo, cn in calls:
                    fn(lo, cn)
        torch.cuda.synchronize()
        ms = {leg: [] for leg in which}
        for _ in range(opt.repeats):
            for leg, fn in which.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for lo, cn in calls:
                    fn(lo, cn)
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1))
        rec = {"queries_per_run": total, "calls_per_run": len(calls), "repeats": opt.repeats, "warmup_runs": opt.warmup, "legs": {}}
        for leg, t in ms.items():
            qps = sorted(total / (x * 1e-3) for x in t)
            rec["legs"][leg] = {"queries_per_s_median": round(qps[len(qps) // 2], 1), "queries_per_s_min": round(qps[0], 1),
                                "queries_per_s_max": round(qps[-1], 1), "ms_per_run": [round(x, 4) for x in t]}
        bench.log(kind, name, json.dumps({leg: r["queries_per_s_median"] for leg, r in rec["legs"].items()}))
        return rec

    out = {"distinct_table_rows_named": distinct, "build_s": {"int8_graph": round(t8, 1), "f32_graph_over_container": round(tf, 1)}}
    hb = {"int8_graph": g8.hbm_bytes(), "container": se.hbm_bytes(), "materialised_f32_index": mix.hbm_bytes(),
          "f16_rows_handle": r16.hbm_bytes(), "compact_index": cix.hbm_bytes()}
    out["hbm_bytes"] = dict(hb, legs={"a_int8_walk_container_rerank": hb["int8_graph"] + hb["container"],
                                      "b_int8_walk_f32_rows_rerank": hb["int8_graph"] + hb["materialised_f32_index"],
                                      "c_int8_walk_f16_rows_rerank": hb["int8_graph"] + hb["f16_rows_handle"],
                                      "d_compact_index_walked": hb["compact_index"],
                                      "e_materialised_f32_index_walked": hb["materialised_f32_index"]})

    # (a) equals (b), bit for bit, on the queries that are timed
    legs["a_int8_walk_container_rerank"](0, big)
    torch.cuda.synchronize()
    a_ids, a_ds, a_cnt = ids.clone(), ds.clone(), cnt.clone()
    legs["b_int8_walk_f32_rows_rerank"](0, big)
    torch.cuda.synchronize()
    same = {"ids": bool(torch.equal(a_ids, ids)), "dist_bits": bool(torch.equal(a_ds.view(torch.int32), ds.view(torch.int32))),
            "counts": bool(torch.equal(a_cnt, cnt))}
    out["a_equals_b"] = same
    assert all(same.values()), same

    gt = mix.exact_topk(q[:nq].cpu().numpy(), k)[0].astype("int64")
    out["recall_at_%d" % k] = {"queries": nq}
    for leg, fn in legs.items():
        fn(0, nq)
        torch.cuda.synchronize()
        out["recall_at_%d" % k][leg] = round(B.recall(gt, ids[:nq], k), 4)
    bench.log(kind, "recall:", out["recall_at_%d" % k])

    out["batches_of_%d" % nq] = run_shape("stream of %d-query calls" % nq, legs, [(i * nq, nq) for i in range(nb)])
    out["one_call_of_%d" % big] = run_shape("one call of %d" % big, legs, [(0, big)])
    # the re-rank kernel alone, over the walk's own candidate lists
    g8.search_batch_device(q8.data_ptr(), big, ef, m, c_ids.data_ptr(), c_ds.data_ptr(), c_cnt.data_ptr(), 0, status.data_ptr(), s)
    torch.cuda.synchronize()
    out["rerank_alone_one_call_of_%d" % big] = run_shape("re-rank alone", reranks, [(0, big)])
    out["status_words"] = [int(x) for x in status.cpu().numpy()]
    for leg in ("b_int8_walk_f32_rows_rerank", "d_compact_index_walked"):
        for shape in ("batches_of_%d" % nq, "one_call_of_%d" % big):
            a = out[shape]["legs"]["a_int8_walk_container_rerank"]["queries_per_s_median"]
            out[shape]["a_over_" + leg[0]] = round(a / out[shape]["legs"][leg]["queries_per_s_median"], 4)
    for ix in (g8, r16, mix, cix, se):
        ix.close()
    torch.cuda.empty_cache()
    return out


result = {"workload": "%d elements of %d terms over a %d x %d-d table; ef %d, k %d, refine_from %d; GPU builder, default config"
                      % (n, nt, v, dim, ef, k, m),
          "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
          "timing": "HIP events around each run on one stream; legs interleaved inside every repeat; queries/s = queries of a run / its time",
          "data": {}}
for kind in opt.data.split(","):
    result["data"][kind] = run_data(kind)

os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps({"se_refine_bench": opt.out,
                  "a_over_b_and_d": {kind: {shape: [r[shape]["a_over_b"], r[shape]["a_over_d"]] for shape in r if shape.startswith(("batches_of", "one_call_of"))}
                                     for kind, r in result["data"].items()}}))
