#!/usr/bin/env python
"""Filtered search measured: what the filter costs and what it buys.

    python tools/filtered_bench.py [--elements 1000000] [--out profiles/filtered_search.json]

Builds an f32 and an int8 graph (GPU builder, the reference's default config) over the benchmark's mixture data and, per
dtype and per random filter of selectivity 1.0, 0.5, 0.1 and 0.01, times at max_search 50, k 10, one call of 20,480
queries, HIP events around each run, the legs interleaved inside every repeat (one process, one device):
    a  the filtered walk (general walker, hand-overs on the exact walker)
    b  the same index unfiltered on the general walker (GRANNE_HIP_OPT_FORCE_GENERAL) -- what the filter costs at 1.0
    c  what a caller has without the feature: search_batch_device(max_search = k = E) on the default walker plus a filter
       of its result (torch, on the device), E doubled until its recall@10 reaches leg a's -- what the feature buys
and records per leg queries/s, the share of queries the exact walker served, mean n_expand and recall@10 against the
exact top-10 among the allowed rows (a torch scan over those rows: not the code under test). Not part of bench.py."""
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
ap.add_argument("--gt-queries", type=int, default=1024, help="recall is taken over the first this many queries")
ap.add_argument("--selectivities", default="1.0,0.5,0.1,0.01")
ap.add_argument("--e-max", type=int, default=4096, help="leg c stops doubling E here")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slow-repeats", type=int, default=3, help="timed runs of a leg whose run lasts more than a second")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_search.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()
B = bench.Bench(args)
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402

n, dim, ef, k, nq, ng = opt.elements, opt.dim, opt.ef, opt.k, opt.queries, opt.gt_queries
s = B.stream
sels = [float(x) for x in opt.selectivities.split(",")]


def exact_among_allowed(rows_f, q_f, ids_allowed):
    """Top-k of the allowed rows per query by the dot of unit rows (largest first = smallest angular distance)."""
    best_v = torch.full((q_f.shape[0], k), -3.0, device="cuda")
    best_i = torch.full((q_f.shape[0], k), -1, dtype=torch.int64, device="cuda")
    for lo in range(0, ids_allowed.numel(), 200_000):
        sub = ids_allowed[lo:lo + 200_000]
        v, j = torch.topk(q_f @ rows_f[sub].T, min(k, sub.numel()), dim=1)
        cv, ci = torch.cat([best_v, v], 1), torch.cat([best_i, sub[j]], 1)
        o = torch.topk(cv, k, dim=1).indices
        best_v, best_i = torch.gather(cv, 1, o), torch.gather(ci, 1, o)
    return best_i


def recall(gt, got):
    """Mean share of the ground truth's ids (per query: as many as there are, up to k) found in `got`."""
    valid = gt >= 0
    hit = ((gt.unsqueeze(2) == got.unsqueeze(1)).any(dim=2) & valid).sum().item()
    return hit / max(1, valid.sum().item())


out = {"workload": "%d x %d-d mixture, max_search %d, k %d, one call of %d queries; GPU builder, default config" % (n, dim, ef, k, nq),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each run on one stream; legs interleaved inside every repeat; median of %d repeats after %d warm-up runs "
                 "(a leg whose run lasts more than a second: %d repeats after one)" % (opt.repeats, opt.warmup, opt.slow_repeats),
       "recall": "recall@%d over the first %d queries against the exact top-%d among the allowed rows (torch scan)" % (k, ng, k),
       "legs": {"a": "filtered walk", "b": "unfiltered, general walker (GRANNE_HIP_OPT_FORCE_GENERAL)",
                "c": "unfiltered default walker with max_search = k = E, result filtered on the device; E doubled until recall reaches a's"},
       "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, dtype)
    builder, g, t_build = B.build_index(rows, dtype)
    del builder
    rows_f = torch.nn.functional.normalize(rows.float(), dim=1)
    q_f = torch.nn.functional.normalize(q[:ng].float(), dim=1)
    bench.log("%s: built in %.1f s" % (dtype, t_build))
    # a very selective filter visits about max_search / selectivity nodes, with their neighbors: the exact walker's containers are sized for it
    g.set_option(_lib.OPT_SLOW_SLOTS, 1 << 20)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    st = torch.zeros((nq, 3), dtype=torch.int64, device="cuda")
    rec = {"build_s": round(t_build, 1), "selectivities": {}}

    def leg_b():
        g.search_batch_device(q.data_ptr(), nq, ef, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), st.data_ptr(), status.data_ptr(), s)

    for sel in sels:
        gen = torch.Generator(device="cuda").manual_seed(int(sel * 1000) + 17)
        mask = (torch.rand(n, device="cuda", generator=gen) < sel) if sel < 1.0 else torch.ones(n, dtype=torch.bool, device="cuda")
        mask8 = mask.to(torch.uint8)
        words = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
        _lib.check(B.lib.granne_hip_filter_from_mask_device(C.c_void_p(mask8.data_ptr()), n, C.c_void_p(words.data_ptr()), B.dev, B.sp))
        torch.cuda.synchronize()
        allowed_ids = torch.nonzero(mask)[:, 0]
        gt = exact_among_allowed(rows_f, q_f, allowed_ids)

        def leg_a():
            g.search_filtered_batch_device(q.data_ptr(), nq, ef, k, words.data_ptr(), 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                           st.data_ptr(), status.data_ptr(), s)

        def counters(fn):
            status.zero_()
            fn()
            torch.cuda.synchronize()
            got = torch.where(torch.arange(k, device="cuda")[None, :] < cnt[:ng, None], ids[:ng], torch.full_like(ids[:ng], -2))
            return {"recall": round(recall(gt, got), 4), "overflowed": int(status[0].item()), "exact_walker_share": round(int(status[1].item()) / nq, 4),
                    "mean_n_expand": round(st[:, 1].float().mean().item(), 1), "mean_count": round(cnt.float().mean().item(), 2)}

        a_info = counters(leg_a)
        bench.log(dtype, "selectivity", sel, "a:", json.dumps(a_info))
        a_info["walker"] = {_lib.WALKER_GENERAL: "general", _lib.WALKER_EXACT: "exact"}.get(g.get_option(_lib.OPT_LAST_WALKER), "register")
        g.set_option(_lib.OPT_FORCE_GENERAL, 1)
        b_info = counters(leg_b)
        b_info["walker"] = {_lib.WALKER_GENERAL: "general", _lib.WALKER_EXACT: "exact"}.get(g.get_option(_lib.OPT_LAST_WALKER), "register")
        b_info["recall"] = None  # (unfiltered: its answers are not restricted to the allowed rows)
        g.set_option(_lib.OPT_FORCE_GENERAL, 0)

        # leg c: E doubled until the filtered result's recall reaches a's
        E = max(ef, k)
        while True:
            e_ids = torch.empty((nq, E), dtype=torch.int64, device="cuda")
            e_ds = torch.empty((nq, E), dtype=torch.float32, device="cuda")
            e_cnt = torch.empty(nq, dtype=torch.int32, device="cuda")

            def leg_c():
                g.search_batch_device(q.data_ptr(), nq, E, E, e_ids.data_ptr(), e_ds.data_ptr(), e_cnt.data_ptr(), 0, status.data_ptr(), s)
                ok = mask[e_ids.clamp(0, n - 1)] & (torch.arange(E, device="cuda")[None, :] < e_cnt[:, None])
                pos = torch.cumsum(ok, 1) - 1
                keep = ok & (pos < k)
                res = torch.full((nq, k), -2, dtype=torch.int64, device="cuda")
                r_, c_ = torch.nonzero(keep, as_tuple=True)
                res[r_, pos[r_, c_]] = e_ids[r_, c_]
                return res

            c_rec = recall(gt, leg_c()[:ng])
            bench.log(dtype, "selectivity", sel, "c: E", E, "recall", round(c_rec, 4))
            if c_rec >= a_info["recall"] or E * 2 > opt.e_max:
                break
            E *= 2
        c_info = {"E": E, "recall": round(c_rec, 4), "reached_a": bool(c_rec >= a_info["recall"]),
                  "walker": {_lib.WALKER_GENERAL: "general", _lib.WALKER_EXACT: "exact"}.get(g.get_option(_lib.OPT_LAST_WALKER), "register")}

        def general_b():
            g.set_option(_lib.OPT_FORCE_GENERAL, 1)
            leg_b()
            g.set_option(_lib.OPT_FORCE_GENERAL, 0)

        legs = {"a": leg_a, "b": general_b, "c": leg_c}

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1)

        # warm-up runs; a leg whose run lasts seconds (a batch the exact walker serves) gets one warm-up and --slow-repeats
        reps = {}
        for name, fn in legs.items():
            first = timed(fn)
            slow = first > 1000.0
            reps[name] = opt.slow_repeats if slow else opt.repeats
            for _ in range(0 if slow else opt.warmup - 1):
                fn()
            bench.log(dtype, "selectivity", sel, "leg", name, "warm-up run %.1f ms, %d timed runs" % (first, reps[name]))
        torch.cuda.synchronize()
        ms = {name: [] for name in legs}
        for r in range(opt.repeats):
            for name, fn in legs.items():
                if r < reps[name]:
                    ms[name].append(timed(fn))
            bench.log(dtype, "selectivity", sel, "repeat", r, json.dumps({x: round(v[-1], 2) for x, v in ms.items()}))
        for name, info in (("a", a_info), ("b", b_info), ("c", c_info)):
            v = sorted(ms[name])
            info["ms_median"] = round(v[len(v) // 2], 3)
            info["queries_per_s"] = round(nq / (v[len(v) // 2] * 1e-3), 1)
            info["ms_per_run"] = [round(x, 3) for x in ms[name]]
        rec["selectivities"][str(sel)] = {"allowed_rows": int(allowed_ids.numel()), "a": a_info, "b": b_info, "c": c_info}
        bench.log(dtype, "selectivity", sel, json.dumps({x: (rec["selectivities"][str(sel)][x]["queries_per_s"],
                                                           rec["selectivities"][str(sel)][x]["recall"]) for x in "abc"}),
                  "exact share", a_info["exact_walker_share"], "E", E)
        del e_ids, e_ds, e_cnt, gt, words, mask, mask8
    out["dtypes"][dtype] = rec
    del g, rows, rows_f, q, q_f
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({"out": opt.out, "dtypes": list(out["dtypes"])}))
