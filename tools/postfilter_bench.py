#!/usr/bin/env python
"""Post-filtered search measured beside the filtered walk, the torch composition it replaces and the exact scan.

    python tools/postfilter_bench.py [--elements 1000000] [--out profiles/postfiltered_search.json]

Data and method are tools/filtered_bench.py's: an f32 and an int8 graph (GPU builder, the reference's default config) over
the benchmark's mixture data, k 10, one call of 20,480 queries, shared random filters of selectivity 1.0, 0.5, 0.1 and
0.01, HIP events around each run, the legs interleaved inside every repeat (one process, one device):
    a  search_filtered_batch_device at max_search 50: the filtered walk, the yardstick
    c  that tool's torch composition: search_batch_device(max_search = k = E) plus a filter of its result on the device,
       E doubled until its recall@10 reaches leg a's
    d  search_postfiltered_batch_device, min_allowed 50, stages from filters.postfilter_stages(50, count / n, margin =
       the margin the sweep below chose), fallback EXACT
    e  exact_topk_filtered_device
Per leg: queries/s and recall@10 against the exact top-10 among the allowed rows (a torch scan: not the code under test);
for d the stage histogram and status[3]. A leg whose first run lasts more than a second (the filtered walk at 0.1 and 0.01)
is timed by that first run (and by --slow-repeats further runs, none by default: one such run lasts up to a minute).
Margin sweep, per dtype, before the legs: d with margin 1.0 / 1.25 / 1.5 / 2.0 at selectivity 0.1 and 0.01; the chosen
margin is the smallest whose recall is not below leg a's at both. Take-kernel overhead, at selectivity 1.0: d with the one
stage [50] beside search_batch_device(50, 50) in the same repeats. Not part of bench.py."""
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
ap.add_argument("--min-allowed", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--queries", type=int, default=20_480)
ap.add_argument("--gt-queries", type=int, default=1024, help="recall is taken over the first this many queries")
ap.add_argument("--selectivities", default="1.0,0.5,0.1,0.01")
ap.add_argument("--sweep-selectivities", default="0.1,0.01")
ap.add_argument("--margins", default="1.0,1.25,1.5,2.0")
ap.add_argument("--e-max", type=int, default=4096, help="leg c stops doubling E here")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--slow-repeats", type=int, default=0,
                help="further timed runs of a leg whose first run lasts more than a second (0: the first run is its measurement)")
ap.add_argument("--dtypes", default="f32,i8")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postfiltered_search.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import bench  # noqa: E402

args = bench.parse()
B = bench.Bench(args)
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402
from granne_amd.filters import postfilter_stages  # noqa: E402

n, dim, ef, k, nq, ng, M = opt.elements, opt.dim, opt.ef, opt.k, opt.queries, opt.gt_queries, opt.min_allowed
s = B.stream
sels = [float(x) for x in opt.selectivities.split(",")]
sweep_sels = [float(x) for x in opt.sweep_selectivities.split(",")]
margins = [float(x) for x in opt.margins.split(",")]
WALKER = {_lib.WALKER_GENERAL: "general", _lib.WALKER_EXACT: "exact", _lib.WALKER_REGISTER: "register", _lib.WALKER_REGISTER_WIDE: "register"}


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


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stage_histogram(stage, n_stages):
    h = {str(i): int((stage == i).sum().item()) for i in range(n_stages)}
    h["exact"] = int((stage == -1).sum().item())  # (GRANNE_HIP_PF_STAGE_EXACT as an int32)
    return h


out = {"workload": "%d x %d-d mixture, k %d, one call of %d queries, one shared random filter per selectivity; GPU builder, default config; "
                   "the walk at max_search %d, post-filtered search at min_allowed %d, fallback EXACT" % (n, dim, k, nq, ef, M),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each run on one stream (the post-filtered call's own stream waits are inside its window); legs interleaved "
                 "inside every repeat; median of %d repeats after %d warm-up runs (a leg whose first run lasts more than a second: that run, or "
                 "the median of %d further ones where that is not 0)" % (opt.repeats, opt.warmup, opt.slow_repeats),
       "recall": "recall@%d over the first %d queries against the exact top-%d among the allowed rows (torch scan)" % (k, ng, k),
       "legs": {"a": "search_filtered_batch_device, max_search %d" % ef,
                "c": "search_batch_device(max_search = k = E) + a torch filter of the result; E doubled until recall reaches a's",
                "d": "search_postfiltered_batch_device, stages = postfilter_stages(%d, count / n, margin = the sweep's choice)" % M,
                "e": "exact_topk_filtered_device"},
       "dtypes": {}}

for dtype in opt.dtypes.split(","):
    rows = B.rows("mixture", bench.SEED + 100, 0, n, dim, dtype)
    q = B.rows("mixture", bench.SEED + 1, 0, nq, dim, dtype)
    builder, g, t_build = B.build_index(rows, dtype)
    del builder
    rows_f = torch.nn.functional.normalize(rows.float(), dim=1)
    q_f = torch.nn.functional.normalize(q[:ng].float(), dim=1)
    bench.log("%s: built in %.1f s" % (dtype, t_build))
    g.set_option(_lib.OPT_SLOW_SLOTS, 1 << 20)  # (the filtered walk's hand-overs at low selectivity, as tools/filtered_bench.py)
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    stage = torch.empty(nq, dtype=torch.int32, device="cuda")
    rec = {"build_s": round(t_build, 1), "selectivities": {}, "margin_sweep": {}}

    def make_filter(sel):
        gen = torch.Generator(device="cuda").manual_seed(int(sel * 1000) + 17)
        mask = (torch.rand(n, device="cuda", generator=gen) < sel) if sel < 1.0 else torch.ones(n, dtype=torch.bool, device="cuda")
        mask8 = mask.to(torch.uint8)
        words = torch.zeros((n + 31) // 32, dtype=torch.int32, device="cuda")
        _lib.check(B.lib.granne_hip_filter_from_mask_device(C.c_void_p(mask8.data_ptr()), n, C.c_void_p(words.data_ptr()), B.dev, B.sp))
        torch.cuda.synchronize()
        allowed_ids = torch.nonzero(mask)[:, 0]
        return mask, words, allowed_ids, exact_among_allowed(rows_f, q_f, allowed_ids)

    def got_ids():
        return torch.where(torch.arange(k, device="cuda")[None, :] < cnt[:ng, None], ids[:ng], torch.full_like(ids[:ng], -2))

    def run_a(words):
        g.search_filtered_batch_device(q.data_ptr(), nq, ef, k, words.data_ptr(), 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), 0,
                                       status.data_ptr(), s)

    def run_d(words, stages):
        g.search_postfiltered_batch_device(q.data_ptr(), nq, k, M, stages, _lib.PF_FALLBACK_EXACT, words.data_ptr(), 0, ids.data_ptr(),
                                           ds.data_ptr(), cnt.data_ptr(), stage.data_ptr(), status.data_ptr(), stream=s)

    def info_a(words, gt):
        status.zero_()
        first = timed(lambda: run_a(words))
        return {"recall": round(recall(gt, got_ids()), 4), "overflowed": int(status[0].item()),
                "exact_walker_share": round(int(status[1].item()) / nq, 4), "first_run_ms": round(first, 3)}

    def info_d(words, gt, stages):
        status.zero_()
        run_d(words, stages)
        torch.cuda.synchronize()
        return {"stages": list(stages), "recall": round(recall(gt, got_ids()), 4), "stage_histogram": stage_histogram(stage, len(stages)),
                "unfinished": int(status[3].item()), "overflowed": int(status[0].item()), "mean_count": round(cnt.float().mean().item(), 2)}

    # ---- the margin sweep: leg a's recall at the sweep's selectivities, then d at every margin ------------------------
    a_infos, chosen = {}, None
    ok_at = {m: True for m in margins}
    for sel in sweep_sels:
        mask, words, allowed_ids, gt = make_filter(sel)
        a_infos[sel] = info_a(words, gt)
        bench.log(dtype, "selectivity", sel, "a:", json.dumps(a_infos[sel]))
        rec["margin_sweep"][str(sel)] = {"a_recall": a_infos[sel]["recall"], "margins": {}}
        for m in margins:
            stages = postfilter_stages(M, allowed_ids.numel() / n, margin=m)
            d = info_d(words, gt, stages)
            for _ in range(opt.warmup - 1):
                run_d(words, stages)
            ms = sorted(timed(lambda: run_d(words, stages)) for _ in range(3))
            d["ms_median"] = round(ms[1], 3)
            d["queries_per_s"] = round(nq / (ms[1] * 1e-3), 1)
            d["not_below_a"] = bool(d["recall"] >= a_infos[sel]["recall"])
            ok_at[m] = ok_at[m] and d["not_below_a"]
            rec["margin_sweep"][str(sel)]["margins"][str(m)] = d
            bench.log(dtype, "selectivity", sel, "margin", m, json.dumps(d))
        del mask, words, allowed_ids, gt
    good = [m for m in margins if ok_at[m]]
    chosen = min(good) if good else max(margins)
    rec["margin_chosen"] = chosen
    rec["margin_reaches_a_at_every_sweep_selectivity"] = bool(good)
    bench.log(dtype, "margin chosen:", chosen, "(reaches a: %s)" % bool(good))

    # ---- the legs ---------------------------------------------------------------------------------------------------
    for sel in sels:
        mask, words, allowed_ids, gt = make_filter(sel)
        a_info = a_infos.get(sel) or info_a(words, gt)
        stages = postfilter_stages(M, allowed_ids.numel() / n, margin=chosen)
        d_info = info_d(words, gt, stages)
        d_info["margin"] = chosen
        d_info["last_walker"] = WALKER.get(g.get_option(_lib.OPT_LAST_WALKER), "?")

        def leg_e():
            g.exact_topk_filtered_device(q.data_ptr(), nq, k, words.data_ptr(), 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), status.data_ptr(), s)

        status.zero_()
        leg_e()
        torch.cuda.synchronize()
        e_info = {"recall": round(recall(gt, got_ids()), 4), "overflowed": int(status[0].item())}

        E = max(ef, k)  # leg c: E doubled until the filtered result's recall reaches a's
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
        c_info = {"E": E, "recall": round(c_rec, 4), "reached_a": bool(c_rec >= a_info["recall"])}

        legs = {"a": lambda: run_a(words), "c": leg_c, "d": lambda: run_d(words, stages), "e": leg_e}
        infos = {"a": a_info, "c": c_info, "d": d_info, "e": e_info}
        if sel == 1.0:  # the take kernel's cost: one stage of 50 beside the plain search with max_search = k = 50
            p_ids = torch.empty((nq, ef), dtype=torch.int64, device="cuda")
            p_ds = torch.empty((nq, ef), dtype=torch.float32, device="cuda")
            p_cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
            legs["plain_50_50"] = lambda: g.search_batch_device(q.data_ptr(), nq, ef, ef, p_ids.data_ptr(), p_ds.data_ptr(), p_cnt.data_ptr(), 0,
                                                                 status.data_ptr(), s)
            legs["d_one_stage_50"] = lambda: run_d(words, [ef])
            infos["plain_50_50"] = {"what": "search_batch_device(%d, %d)" % (ef, ef)}
            infos["d_one_stage_50"] = {"what": "search_postfiltered_batch_device, stages [%d], min_allowed %d" % (ef, ef)}

        reps, firsts = {}, {}
        for name, fn in legs.items():
            first = infos[name].get("first_run_ms") if name == "a" else None
            if first is None or first <= 1000.0:
                first = timed(fn)
            slow = first > 1000.0
            firsts[name] = first
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
            bench.log(dtype, "selectivity", sel, "repeat", r, json.dumps({x: round(v[-1], 2) for x, v in ms.items() if len(v) > r}))
        for name, info in infos.items():
            v = sorted(ms[name] or [firsts[name]])  # (a slow leg with --slow-repeats 0: its first run is its measurement)
            info["ms_median"] = round(v[len(v) // 2], 3)
            info["queries_per_s"] = round(nq / (v[len(v) // 2] * 1e-3), 1)
            info["ms_per_run"] = [round(x, 3) for x in ms[name]]
        if sel == 1.0:
            infos["take_overhead_ms"] = round(infos["d_one_stage_50"]["ms_median"] - infos["plain_50_50"]["ms_median"], 3)
        infos["allowed_rows"] = int(allowed_ids.numel())
        rec["selectivities"][str(sel)] = infos
        bench.log(dtype, "selectivity", sel, json.dumps({x: (infos[x]["queries_per_s"], infos[x].get("recall")) for x in legs}), "stages", stages,
                  "histogram", d_info["stage_histogram"])
        del e_ids, e_ds, e_cnt, gt, words, mask
    out["dtypes"][dtype] = rec
    del g, rows, rows_f, q, q_f
    torch.cuda.empty_cache()

out["margin_default"] = max(r["margin_chosen"] for r in out["dtypes"].values())
os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({"out": opt.out, "dtypes": list(out["dtypes"]), "margin_default": out["margin_default"]}))
