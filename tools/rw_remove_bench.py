#!/usr/bin/env python
"""Removals on a live granne_amd.RwGranneBuilder measured: what a removed fraction costs the live search, what a remove
call costs, and what compact costs beside a fresh bulk build.

    python tools/rw_remove_bench.py [--elements 1000000] [--out profiles/rw_remove.json]

Builds an f32 graph over the benchmark's mixture data under the reference's default config (the Rw handle's own bulk
build) and, in ONE process, wall time around host-pointer calls that end in a device synchronise (as
tools/rw_insert_bench.py takes them), the legs interleaved inside every repeat:
  * `remove` and `restore` latency for 1 / 1,000 / 100,000 random ids;
  * per removed fraction 0 / 0.001 / 0.01 / 0.1 / 0.5 (random ids, cumulative): the live search_batch rate at 1,024 queries
    per call, max_search 50, k 10, beside the same walk on a get_index() snapshot under alive_filter()
    (search_filtered_batch, whose status words say how many walks the exact walker served) and, at fraction 0, beside the
    snapshot's unfiltered search_batch; recall@10 of the live answers against the snapshot's exact_topk_filtered;
  * `compact` beside GranneBuilder + RwGranneBuilder over the same surviving rows.
Every leg records the handle's removed count and its filtered-search counter. Not part of bench.py."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--ef", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--queries", type=int, default=1024)
ap.add_argument("--fractions", default="0,0.001,0.01,0.1,0.5")
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rw_remove.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
from granne_amd import rw_builder  # noqa: E402

n, dim, ef, k, nq = opt.elements, opt.dim, opt.ef, opt.k, opt.queries
rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, "f32").cpu().numpy()
q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, "f32").cpu().numpy()
torch.cuda.empty_cache()


def wall(fn):
    t = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t) * 1e3, r


def spread(ms):
    v = np.sort(np.asarray(ms, np.float64))
    return {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v[0]), 4), "ms_max": round(float(v[-1]), 4), "runs": int(v.size)}


def rate(ms):
    s = spread(ms)
    s["queries_per_s"] = round(nq / (s["ms_median"] * 1e-3), 1)
    return s


def counters(rw):
    return {"removed": rw.removed_count(), "filtered_searches": rw.get_option(rw_builder.FILTERED_SEARCHES)}


t_build, rw = wall(lambda: ga.RwGranneBuilder(ga.GranneBuilder("angular", rows), n))
bench.log("built %d x %d in %.1f s" % (n, dim, t_build / 1e3))
out = {"workload": "%d x %d-d f32 mixture, default config; calls of %d queries, max_search %d, k %d" % (n, dim, nq, ef, k),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "wall time around host-pointer calls (each ends in a device synchronise); legs interleaved inside every repeat; "
                 "median of %d repeats after %d warm-up runs" % (opt.repeats, opt.warmup),
       "build_and_create_s": round(t_build / 1e3, 2), "remove_latency": {}, "fractions": {}}
rng = np.random.default_rng(5)
order = rng.permutation(n).astype(np.uint64)

# ---- remove / restore latency, from a clean handle -------------------------------------------------------------------
for m in (1, 1000, 100000):
    ids = np.ascontiguousarray(rng.permutation(n)[:m].astype(np.uint64))
    t_rm, t_rs = [], []
    for r in range(opt.warmup + opt.repeats):
        a, got = wall(lambda: rw.remove(ids))
        assert got == (m, 0, 0)
        b, got = wall(lambda: rw.restore(ids))
        assert got == (m, 0, 0)
        if r >= opt.warmup:
            t_rm.append(a)
            t_rs.append(b)
    out["remove_latency"][str(m)] = {"remove": spread(t_rm), "restore": spread(t_rs), **counters(rw)}
    bench.log("remove", m, json.dumps(out["remove_latency"][str(m)]))

# ---- the live search under removed fractions -------------------------------------------------------------------------
done = 0
for frac in [float(x) for x in opt.fractions.split(",")]:
    upto = int(round(frac * n))
    if upto > done:
        assert rw.remove(order[done:upto]) == (upto - done, 0, 0)
        done = upto
    alive, snap = rw.alive_filter(), rw.get_index()
    legs = {"live": lambda: rw.search_batch(q, ef, k),
            "snapshot_search_filtered": lambda: snap.search_filtered_batch(q, alive, ef, k, status=True)}
    if done == 0:
        legs["snapshot_search_batch"] = lambda: snap.search_batch(q, ef, k)
    rec = {"removed_rows": done}
    try:
        ms = {name: [] for name in legs}
        for r in range(opt.warmup + opt.repeats):
            for name, fn in legs.items():
                t, _ = wall(fn)
                if r >= opt.warmup:
                    ms[name].append(t)
        for name in legs:
            rec[name] = rate(ms[name])
        ids, _ds, cnt = legs["live"]()
        s_ids, _sd, s_cnt, status = legs["snapshot_search_filtered"]()
        rec["live_equals_snapshot"] = bool((ids == s_ids).all() and (cnt == s_cnt).all())
        rec["snapshot_status"] = [int(x) for x in status]  # [1]: walks the exact walker served
        rec["exact_walker_share"] = round(int(status[1]) / nq, 4)
        gt = snap.exact_topk_filtered(q, k, alive)
        hit = sum(len(set(ids[i, :cnt[i]].tolist()) & set(gt[0][i, :gt[2][i]].tolist())) for i in range(nq))
        rec["recall_at_%d" % k] = round(hit / max(1, int(gt[2].sum())), 4)
    except ga.GranneHipError as e:
        rec["error"] = str(e)
    rec.update(counters(rw))
    out["fractions"][str(frac)] = rec
    bench.log("fraction", frac, json.dumps(rec))
    snap.close()
    alive.close()

# ---- compact beside a fresh bulk build of the same rows --------------------------------------------------------------
t_c, t_f, survivors = [], [], None
for r in range(3):
    t, (new, old_ids) = wall(lambda: rw.compact())
    survivors = old_ids
    new.close()
    t_c.append(t)
    kept = rows[old_ids.astype(np.int64)]
    t, fresh = wall(lambda: ga.RwGranneBuilder(ga.GranneBuilder("angular", kept), n))
    fresh.close()
    t_f.append(t)
out["compact"] = {"removed_rows": done, "survivors": int(len(survivors)), "compact": spread(t_c), "fresh_bulk_build": spread(t_f),
                  "note": "both include the bulk build; compact gathers the rows on the device, the fresh build uploads them from the host",
                  **counters(rw)}
bench.log("compact", json.dumps(out["compact"]))
rw.close()
os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({"out": opt.out, "fractions": list(out["fractions"])}))
