#!/usr/bin/env python
"""Range search measured: the scan under a radius beside the exact selection, the walk under a radius beside the plain
search with a cut.

    python tools/range_bench.py [--elements 1000000] [--out profiles/range_search.json]

Data and method are the other filtered tools' (tools/postfilter_bench.py): an f32 and an int8 graph (GPU builder, the
reference's default config) over the benchmark's mixture data, one call of 20,480 queries, HIP events around each run, the
legs interleaved inside every repeat (one process, one device). Radii are chosen PER QUERY from a ground-truth scan (torch:
not the code under test) as the distance of the query's t-th nearest row, t = 1, 10, 100, 1,000 and 10,000 -- the mean
total is then about t; the last is past the 4,096 keys phase A ranks, so phase B runs.
    (a) exact_range_device(cap) beside exact_topk_device(k = 10) and exact_topk_device(k = 1024) in the same repeats
    (b) search_range_batch_device(cap, stages, EXACT and SHORT) beside search_batch_device(E, E) plus a torch cut at the
        radius, E the last stage's. Recall: the share of the exact within-radius set, up to cap, that the answer holds,
        over the first --gt-queries queries. The stage histogram is recorded.
Stage sweep, per dtype, at every radius: each ascending subset of the register walkers' list sizes 60 / 124 / 252 / 508 /
1020 that ends at 1020 and is listed in SETS, with fallback SHORT; the default is the cheapest (sum of the medians over
the radii) whose recall is not below the plain search's at E = 1020 at any radius. Not part of bench.py."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--cap", type=int, default=1024)
ap.add_argument("--queries", type=int, default=20_480)
ap.add_argument("--gt-queries", type=int, default=1024, help="recall is taken over the first this many queries")
ap.add_argument("--totals", default="1,10,100,1000,10000")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_search.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()
B = bench.Bench(args)
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402
from granne_amd.index import RANGE_DEFAULT_STAGES  # noqa: E402

n, dim, cap, nq, ng = opt.elements, opt.dim, opt.cap, opt.queries, opt.gt_queries
s = B.stream
targets = [int(x) for x in opt.totals.split(",")]
SETS = [[60, 124, 252, 508, 1020], [124, 252, 508, 1020], [60, 252, 1020], [124, 508, 1020], [252, 1020], [508, 1020], [1020]]
E_LAST = 1020


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def ground_truth(rows_f, q_f):
    """per query the max(targets) nearest rows by the dot of unit rows: (distances ascending [nq, T], ids [nq, T])"""
    T = min(max(targets), n)
    ds, ids = [], []
    for lo in range(0, q_f.shape[0], 512):
        v, j = torch.topk(q_f[lo:lo + 512] @ rows_f.T, T, dim=1)
        ds.append(1.0 - v)
        ids.append(j)
    return torch.cat(ds), torch.cat(ids)


def recall(gt_ids, gt_valid, got_ids, got_cnt):
    """the share of the ground truth's within-radius ids (up to cap per query) that the answer holds, over the first ng queries"""
    hit = total = 0
    for lo in range(0, ng, 64):
        g, v = gt_ids[lo:lo + 64, :cap], gt_valid[lo:lo + 64, :cap]
        a = got_ids[lo:lo + 64]
        a = torch.where(torch.arange(a.shape[1], device="cuda")[None, :] < got_cnt[lo:lo + 64, None], a, torch.full_like(a, -2))
        hit += ((g.unsqueeze(2) == a.unsqueeze(1)).any(dim=2) & v).sum().item()
        total += v.sum().item()
    return hit / max(1, total)


def stage_histogram(stage, n_stages):
    h = {str(i): int((stage == i).sum().item()) for i in range(n_stages)}
    h["exact"] = int((stage == -1).sum().item())  # (GRANNE_HIP_RG_STAGE_EXACT as an int32)
    h["short"] = int((stage == -2).sum().item())
    return h


def medians(legs):
    for fn in legs.values():
        for _ in range(opt.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(opt.repeats):
        for name, fn in legs.items():
            ms[name].append(timed(fn))
    return {name: sorted(v)[len(v) // 2] for name, v in ms.items()}, ms


out = {"workload": "%d x %d-d mixture, one call of %d queries, cap %d; radii per query: the ground-truth distance of the t-th nearest row, "
                   "t in %s; GPU builder, default config" % (n, dim, nq, cap, targets),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each run on one stream (the range calls' own stream waits are inside their windows); legs interleaved inside "
                 "every repeat; median of %d repeats after %d warm-up runs" % (opt.repeats, opt.warmup),
       "recall": "share of the exact within-radius set, up to cap, that the answer holds; first %d queries; ground truth by a torch scan" % ng,
       "stage_sets": SETS, "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, dtype)
    builder, g, t_build = B.build_index(rows, dtype)
    del builder
    rows_f = torch.nn.functional.normalize(rows.float(), dim=1)
    q_f = torch.nn.functional.normalize(q.float(), dim=1)
    gt_d, gt_i = ground_truth(rows_f, q_f)
    del rows_f
    bench.log("%s: built in %.1f s, ground truth for %d queries" % (dtype, t_build, nq))
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, cap), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, cap), dtype=torch.float32, device="cuda")
    cnt, tot, stage = (torch.empty(nq, dtype=torch.int32, device="cuda") for _ in range(3))
    k_ids = torch.empty((nq, 1024), dtype=torch.int64, device="cuda")
    k_ds = torch.empty((nq, 1024), dtype=torch.float32, device="cuda")
    e_ids = torch.empty((nq, E_LAST), dtype=torch.int64, device="cuda")
    e_ds = torch.empty((nq, E_LAST), dtype=torch.float32, device="cuda")
    e_cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    rec = {"build_s": round(t_build, 1), "totals": {}, "stage_sweep": {}}
    sweep_ms = {tuple(st): 0.0 for st in SETS}
    sweep_ok = {tuple(st): True for st in SETS}

    for t in targets:
        radii = gt_d[:, min(t, gt_d.shape[1]) - 1].contiguous()
        gt_valid = gt_d[:ng] <= radii[:ng, None]

        def run_scan():
            g.exact_range_device(q.data_ptr(), nq, radii.data_ptr(), cap, 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), tot.data_ptr(),
                                 status.data_ptr(), s)

        def run_topk(k):
            g.exact_topk_device(q.data_ptr(), nq, k, k_ids.data_ptr(), k_ds.data_ptr(), e_cnt.data_ptr(), status.data_ptr(), s)

        def run_walk(stages, fb):
            g.search_range_batch_device(q.data_ptr(), nq, radii.data_ptr(), cap, stages, fb, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                        tot.data_ptr(), stage.data_ptr(), status.data_ptr(), 0, s)

        def run_plain():
            g.search_batch_device(q.data_ptr(), nq, E_LAST, E_LAST, e_ids.data_ptr(), e_ds.data_ptr(), e_cnt.data_ptr(), 0, status.data_ptr(), s)
            return ((e_ds <= radii[:, None]) & (torch.arange(E_LAST, device="cuda")[None, :] < e_cnt[:, None])).sum(dim=1).clamp(max=cap)

        # (a) the scan
        status.zero_()
        run_scan()
        torch.cuda.synchronize()
        a_info = {"mean_total": round(tot.float().mean().item(), 2), "max_total": int(tot.max().item()), "phase_b_queries": int(status[1].item()),
                  "voided": int(status[0].item()), "recall": round(recall(gt_i[:ng], gt_valid, ids, cnt), 4)}
        med, ms = medians({"exact_range": run_scan, "exact_topk_10": lambda: run_topk(10), "exact_topk_1024": lambda: run_topk(1024)})
        a_info.update({"ms": {x: round(v, 3) for x, v in med.items()}, "ms_per_run": {x: [round(y, 3) for y in v] for x, v in ms.items()},
                       "queries_per_s": round(nq / (med["exact_range"] * 1e-3), 1),
                       "ratio_to_exact_topk_10": round(med["exact_topk_10"] / med["exact_range"], 3),
                       "ratio_to_exact_topk_1024": round(med["exact_topk_1024"] / med["exact_range"], 3)})
        bench.log(dtype, "total", t, "scan", json.dumps(a_info["ms"]), "mean total", a_info["mean_total"], "phase B", a_info["phase_b_queries"])

        # (b) the walk: the plain search's recall at E_LAST first, then the stage sweep (SHORT), then the legs
        plain_cnt = run_plain()
        torch.cuda.synchronize()
        plain_recall = recall(gt_i[:ng], gt_valid, e_ids[:, :cap], plain_cnt.to(torch.int32))
        sweep = {}
        for st in SETS:
            status.zero_()
            run_walk(st, _lib.RG_FALLBACK_SHORT)
            torch.cuda.synchronize()
            r = recall(gt_i[:ng], gt_valid, ids, cnt)
            m3 = sorted(timed(lambda: run_walk(st, _lib.RG_FALLBACK_SHORT)) for _ in range(3))[1]
            sweep[str(st)] = {"recall": round(r, 4), "ms_median": round(m3, 3), "not_below_plain": bool(r >= plain_recall),
                              "stage_histogram": stage_histogram(stage, len(st)), "unfinished": int(status[3].item())}
            sweep_ms[tuple(st)] += m3
            sweep_ok[tuple(st)] = sweep_ok[tuple(st)] and r >= plain_recall
        rec["stage_sweep"][str(t)] = {"plain_recall_at_%d" % E_LAST: round(plain_recall, 4), "sets": sweep}
        stages = list(RANGE_DEFAULT_STAGES)
        b_info = {"stages": stages, "plain": {"E": E_LAST, "recall": round(plain_recall, 4)}}
        for name, fb in (("exact", _lib.RG_FALLBACK_EXACT), ("short", _lib.RG_FALLBACK_SHORT)):
            status.zero_()
            run_walk(stages, fb)
            torch.cuda.synchronize()
            b_info[name] = {"recall": round(recall(gt_i[:ng], gt_valid, ids, cnt), 4), "stage_histogram": stage_histogram(stage, len(stages)),
                            "unfinished": int(status[3].item()), "mean_found": round(tot.float().mean().item(), 2)}
        med, ms = medians({"exact": lambda: run_walk(stages, _lib.RG_FALLBACK_EXACT), "short": lambda: run_walk(stages, _lib.RG_FALLBACK_SHORT),
                           "plain": run_plain})
        for name in ("exact", "short", "plain"):
            b_info[name].update({"ms_median": round(med[name], 3), "queries_per_s": round(nq / (med[name] * 1e-3), 1),
                                 "ms_per_run": [round(y, 3) for y in ms[name]]})
        bench.log(dtype, "total", t, "walk", json.dumps({x: (b_info[x]["queries_per_s"], b_info[x]["recall"]) for x in ("exact", "short", "plain")}))
        rec["totals"][str(t)] = {"exact_range": a_info, "search_range": b_info}
    good = [st for st in SETS if sweep_ok[tuple(st)]]
    rec["stages_chosen"] = min(good, key=lambda st: sweep_ms[tuple(st)]) if good else SETS[0]
    rec["stage_sweep_ms_sum"] = {str(list(st)): round(v, 3) for st, v in sweep_ms.items()}
    bench.log(dtype, "stages chosen:", rec["stages_chosen"])
    out["dtypes"][dtype] = rec
    del g, rows, q, q_f, gt_d, gt_i
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({"out": opt.out, "dtypes": list(out["dtypes"]), "stages_chosen": {d: r["stages_chosen"] for d, r in out["dtypes"].items()}}))
