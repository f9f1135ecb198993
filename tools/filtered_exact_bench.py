#!/usr/bin/env python
"""The exact scan under an id bitmap measured beside the filtered walk: where one overtakes the other.

    python tools/filtered_exact_bench.py [--elements 1000000] [--out profiles/filtered_exact.json]

tools/filtered_bench.py's data and method: an f32 and an int8 graph (GPU builder, the reference's default config) over the
benchmark's mixture data, k 10, one call of 20,480 queries, one shared random filter per selectivity (1.0, 0.5, 0.1, 0.01;
the same seeds), HIP events around each run, the legs interleaved inside every repeat (one process, one device):
    scan     exact_topk_filtered_device: the bitmap compacted to its ids, exact_topk's passes over that list
    walk     search_filtered_batch_device at max_search 50 -- the existing entry, unchanged: the yardstick
    compact  granne_hip_filter_to_ids_device alone (the scan's first step, here with u64 ids)
and once per dtype the unfiltered exact_topk_device. Recorded per selectivity: queries/s of each leg, the scan's status words
([3]: the allowed ids), and recall@10 of the walk against the scan's answer over every query. Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--ef", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--queries", type=int, default=20_480)
ap.add_argument("--selectivities", default="1.0,0.5,0.1,0.01")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slow-repeats", type=int, default=2, help="timed runs of a leg whose run lasts more than a second")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_exact.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()
B = bench.Bench(args)
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402

n, dim, ef, k, nq = opt.elements, opt.dim, opt.ef, opt.k, opt.queries
s = B.stream
sels = [float(x) for x in opt.selectivities.split(",")]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(legs, firsts=None):
    """{name: [ms per run]}: per leg a first run (`firsts`: the time of one already made) decides whether it is slow (more
    than a second: that one warm-up run, fewer timed ones); then the timed runs, the legs interleaved inside every repeat"""
    reps = {}
    for name, fn in legs.items():
        first = firsts[name] if firsts else timed(fn)
        slow = first > 1000.0
        reps[name] = opt.slow_repeats if slow else opt.repeats
        for _ in range(0 if slow else opt.warmup - 1):
            fn()
        bench.log("leg", name, "warm-up run %.2f ms, %d timed runs" % (first, reps[name]))
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for r in range(opt.repeats):
        for name, fn in legs.items():
            if r < reps[name]:
                ms[name].append(timed(fn))
        bench.log("repeat", r, json.dumps({x: round(v[-1], 3) for x, v in ms.items() if len(v) > r}))
    return ms


def summary(v, queries=True):
    v = sorted(v)
    med = v[len(v) // 2]
    out = {"ms_median": round(med, 3), "ms_per_run": [round(x, 3) for x in v]}
    if queries:
        out["queries_per_s"] = round(nq / (med * 1e-3), 1)
    return out


def recall(gt, gt_cnt, got, got_cnt):
    """Mean share of the scan's ids (per query: as many as it returned) found in the walk's result."""
    col = torch.arange(k, device="cuda")[None, :]
    valid = col < gt_cnt[:, None]
    got = torch.where(col < got_cnt[:, None], got, torch.full_like(got, -2))
    hit = 0
    for lo in range(0, gt.shape[0], 4096):
        g, w = gt[lo:lo + 4096], got[lo:lo + 4096]
        hit += ((g.unsqueeze(2) == w.unsqueeze(1)).any(dim=2) & valid[lo:lo + 4096]).sum().item()
    return hit / max(1, valid.sum().item())


out = {"workload": "%d x %d-d mixture, k %d, one call of %d queries, one shared random filter per selectivity; GPU builder, default config; "
                   "the walk at max_search %d" % (n, dim, k, nq, ef),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each run on one stream; legs interleaved inside every repeat; median of %d repeats after %d warm-up runs "
                 "(a leg whose run lasts more than a second: %d repeats after one)" % (opt.repeats, opt.warmup, opt.slow_repeats),
       "recall": "recall@%d of the walk over all %d queries against the scan's answer (exact among the allowed rows)" % (k, nq),
       "legs": {"scan": "exact_topk_filtered_device, shared filter (list form)", "walk": "search_filtered_batch_device, max_search %d" % ef,
                "compact": "filter_to_ids_device alone", "exact_topk": "exact_topk_device over all rows, unfiltered, once per dtype"},
       "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, dtype)
    builder, g, t_build = B.build_index(rows, dtype)
    del builder
    bench.log("%s: built in %.1f s" % (dtype, t_build))
    g.set_option(_lib.OPT_SLOW_SLOTS, 1 << 20)  # (as tools/filtered_bench.py: the exact walker's containers for a selective filter)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    w_status = torch.zeros(4, dtype=torch.int32, device="cuda")
    w_ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    w_ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    w_cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    id_list = torch.empty(n, dtype=torch.int64, device="cuda")
    id_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    rec = {"build_s": round(t_build, 1), "selectivities": {}}

    def unfiltered():
        g.exact_topk_device(q.data_ptr(), nq, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), status.data_ptr(), s)

    rec["exact_topk"] = summary(measure({"exact_topk": unfiltered})["exact_topk"])
    u_ids, u_ds = ids.clone(), ds.clone()
    bench.log(dtype, "exact_topk, unfiltered:", rec["exact_topk"]["queries_per_s"], "queries/s")

    for sel in sels:
        gen = torch.Generator(device="cuda").manual_seed(int(sel * 1000) + 17)
        mask = (torch.rand(n, device="cuda", generator=gen) < sel) if sel < 1.0 else torch.ones(n, dtype=torch.bool, device="cuda")
        mask8 = mask.to(torch.uint8)
        words = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
        _lib.check(B.lib.granne_hip_filter_from_mask_device(C.c_void_p(mask8.data_ptr()), n, C.c_void_p(words.data_ptr()), B.dev, B.sp))
        torch.cuda.synchronize()
        allowed = int(mask.sum().item())

        def scan():
            g.exact_topk_filtered_device(q.data_ptr(), nq, k, words.data_ptr(), 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                         status.data_ptr(), s)

        def walk():
            g.search_filtered_batch_device(q.data_ptr(), nq, ef, k, words.data_ptr(), 0, 0, w_ids.data_ptr(), w_ds.data_ptr(), w_cnt.data_ptr(),
                                           0, w_status.data_ptr(), s)

        def compact():
            _lib.check(B.lib.granne_hip_filter_to_ids_device(C.c_void_p(words.data_ptr()), n, C.c_void_p(id_list.data_ptr()),
                                                             C.c_void_p(id_count.data_ptr()), B.dev, B.sp))

        # one run of each for what they return: the scan's status, the walk's recall against the scan, the list against torch
        status.zero_()
        w_status.zero_()
        firsts = {"scan": timed(scan), "walk": timed(walk), "compact": timed(compact)}
        st = [int(x) for x in status.tolist()]
        assert st[0] == 0 and st[3] == allowed == int(id_count.item()), (st, allowed)
        assert torch.equal(id_list[:allowed], torch.nonzero(mask)[:, 0])
        assert bool(mask[ids[torch.arange(k, device="cuda")[None, :] < cnt[:, None]]].all())
        if sel == 1.0:  # every bit set: exact_topk's answer
            assert torch.equal(ids, u_ids) and torch.equal(ds, u_ds)
        info = {"allowed_rows": allowed, "scan_status": st, "scan_mean_count": round(cnt.float().mean().item(), 2),
                "walk_recall": round(recall(ids, cnt, w_ids, w_cnt), 4), "walk_mean_count": round(w_cnt.float().mean().item(), 2),
                "walk_exact_walker_share": round(int(w_status[1].item()) / nq, 4), "walk_overflowed": int(w_status[0].item())}
        bench.log(dtype, "selectivity", sel, json.dumps(info))
        ms = measure({"scan": scan, "walk": walk, "compact": compact}, firsts)
        info["scan"], info["walk"], info["compact"] = summary(ms["scan"]), summary(ms["walk"]), summary(ms["compact"], queries=False)
        info["scan_pairs_per_s"] = round(allowed * nq / (info["scan"]["ms_median"] * 1e-3), 1)
        info["scan_over_walk"] = round(info["scan"]["queries_per_s"] / info["walk"]["queries_per_s"], 3)
        rec["selectivities"][str(sel)] = info
        bench.log(dtype, "selectivity", sel, "scan", info["scan"]["queries_per_s"], "walk", info["walk"]["queries_per_s"], "queries/s; compaction",
                  info["compact"]["ms_median"], "ms; walk recall", info["walk_recall"])
        del words, mask, mask8
    faster = [x for x in sels if rec["selectivities"][str(x)]["scan_over_walk"] > 1.0]
    slower = [x for x in sels if rec["selectivities"][str(x)]["scan_over_walk"] <= 1.0]
    rec["scan_overtakes_walk_between"] = [min(slower) if slower else None, max(faster) if faster else None]
    out["dtypes"][dtype] = rec
    del g, rows, q
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({"out": opt.out, "dtypes": {d: r["scan_overtakes_walk_between"] for d, r in out["dtypes"].items()}}))
