#!/usr/bin/env python
"""Filters and the exact selection on a partitioned index, measured.

    python tools/sharded_filtered_bench.py [--shards 8] [--rows 1000003] [--out profiles/sharded_filtered.json]

Builds `--shards` int8 shards of `--rows` x 100-d mixture rows each on one GPU (GPU builder, the reference's default config)
behind one granne_hip_sharded handle. 1,000,003 rows per shard put every shard but the first at an offset that is no
multiple of 32, so every filtered call pays its seven slice launches. Per random shared filter of selectivity 1.0, 0.5, 0.1
and 0.01, at max_search 50, k 10, HIP events around each run on one stream, the legs interleaved inside every repeat:
    a  sharded search_batch with GRANNE_HIP_OPT_FORCE_GENERAL on every shard (the unfiltered walk on the walker the filter uses)
    b  granne_hip_sharded_search_filtered_batch_device
    c  what a caller had before: a loop over the shards of search_filtered_batch_device under slices made on the host (made
       once, outside the timed region) and granne_hip_merge_topk_device
    d  granne_hip_sharded_exact_topk_filtered_device over the first --gt-queries queries; recall@10 of b against it
and, without an index,
    e  granne_hip_filter_slice_device alone over the handle's bitmap and over 2^30 bits, word-aligned and not, with the lane
       hand-over (GRANNE_HIP_FILTER_SLICE_HANDOVER=1) and with two loads per lane (the form that ships), beside a
       device-to-device copy of the same bytes.
Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shards", type=int, default=8)
ap.add_argument("--rows", type=int, default=1_000_003, help="per shard")
ap.add_argument("--dim", type=int, default=100)
ap.add_argument("--ef", type=int, default=50)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--queries", type=int, default=4096)
ap.add_argument("--selective-queries", type=int, default=256, help="queries per call below selectivity 0.05 (the exact walker serves them)")
ap.add_argument("--gt-queries", type=int, default=256)
ap.add_argument("--selectivities", default="1.0,0.5,0.1,0.01")
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--slow-repeats", type=int, default=3, help="timed runs of a leg whose run lasts more than a second")
ap.add_argument("--big-bits", type=int, default=1 << 30)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sharded_filtered.json"))
opt = ap.parse_args()
sys.argv = [sys.argv[0]]

import numpy as np  # noqa: E402

import bench  # noqa: E402

B = bench.Bench(bench.parse())
torch, ga = B.torch, B.ga
from granne_amd import _lib  # noqa: E402
from granne_amd.sharded import ShardedHost  # noqa: E402

G, n, dim, ef, k = opt.shards, opt.rows, opt.dim, opt.ef, opt.k
s, lib = B.stream, B.lib
p = C.c_void_p


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(legs):
    """name -> sorted ms of the timed runs: one warm-up run each, then the legs in turn inside every repeat"""
    reps = {}
    for name, fn in legs.items():
        first = timed(fn)
        reps[name] = opt.slow_repeats if first > 1000.0 else opt.repeats
        bench.log("  leg", name, "warm-up %.2f ms, %d timed runs" % (first, reps[name]))
    ms = {name: [] for name in legs}
    for r in range(opt.repeats):
        for name, fn in legs.items():
            if r < reps[name]:
                ms[name].append(timed(fn))
    return {name: sorted(v) for name, v in ms.items()}


def median(v):
    return v[len(v) // 2]


out = {"workload": "%d shards x %d x %d-d int8 mixture rows on one GPU, max_search %d, k %d; GPU builder, default config" % (G, n, dim, ef, k),
       "csrc_sha": bench.csrc_sha(), "device": torch.cuda.get_device_name(0),
       "timing": "HIP events around each run on one stream; one warm-up run per leg, then the legs interleaved inside every repeat; median of "
                 "%d runs (%d for a leg whose run lasts more than a second)" % (opt.repeats, opt.slow_repeats),
       "legs": {"a": "sharded search_batch, general walker forced on every shard", "b": "sharded search_filtered_batch_device",
                "c": "per-shard search_filtered_batch_device under host-made slices + merge_topk_device, one stream",
                "d": "sharded exact_topk_filtered_device"},
       "selectivities": {}, "slice": {}}

# ---- (e) the slice alone: no index needed -------------------------------------------------------------------------
for bits in (G * n, opt.big_bits):
    words = (bits + 31) // 32
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, device="cuda")
    dst = torch.empty(words, dtype=torch.int32, device="cuda")
    rec = {}
    for label, first in (("aligned", 64), ("unaligned", 77)):
        n_out = bits - 128
        ow = (n_out + 31) // 32

        def run_slice():
            _lib.check(lib.granne_hip_filter_slice_device(p(src.data_ptr()), bits, 0, 1, first, n_out, p(dst.data_ptr()), ow, B.dev, B.sp))

        def run_copy():
            dst[:ow].copy_(src[2:2 + ow])

        os.environ["GRANNE_HIP_FILTER_SLICE_HANDOVER"] = "1"
        hand = interleaved({"slice": run_slice, "copy": run_copy})
        os.environ["GRANNE_HIP_FILTER_SLICE_HANDOVER"] = "0"  # the form that ships
        two = interleaved({"slice": run_slice})
        gb = 2 * ow * 4 / 1e9  # read + written
        rec[label] = {"hand_over_ms": round(median(hand["slice"]), 4), "two_loads_ms": round(median(two["slice"]), 4),
                      "d2d_copy_ms": round(median(hand["copy"]), 4), "hand_over_GBps": round(gb / (median(hand["slice"]) * 1e-3), 1),
                      "two_loads_GBps": round(gb / (median(two["slice"]) * 1e-3), 1), "d2d_copy_GBps": round(gb / (median(hand["copy"]) * 1e-3), 1),
                      "hand_over_runs_ms": [round(x, 4) for x in hand["slice"]], "two_loads_runs_ms": [round(x, 4) for x in two["slice"]]}
        bench.log("slice", bits, label, json.dumps({x: rec[label][x] for x in ("hand_over_ms", "two_loads_ms", "d2d_copy_ms")}))
    out["slice"][str(bits)] = rec
    del src, dst
torch.cuda.empty_cache()

# ---- the partitioned index --------------------------------------------------------------------------------------------
gixs, keep = [], []
for sh in range(G):
    rows = B.rows("mixture", bench.SEED + 100, sh * n, n, dim, "i8")
    builder, g, t_build = B.build_index(rows, "i8")
    g.set_option(_lib.OPT_SLOW_SLOTS, 1 << 20)  # a very selective filter visits about max_search / selectivity nodes
    gixs.append(g)
    keep.append((rows, builder))
    bench.log("shard %d built in %.1f s" % (sh, t_build))
offsets = [sh * n for sh in range(G)]
host = ShardedHost(gixs, offsets)
span = host.id_span()
assert span == G * n
nq_all = max(opt.queries, opt.selective_queries, opt.gt_queries)
q_all = B.rows("mixture", bench.SEED + 1, 0, nq_all, dim, "i8")
sp_words = (span + 31) // 32

for sel in [float(x) for x in opt.selectivities.split(",")]:
    nq = opt.queries if sel >= 0.05 else opt.selective_queries
    ng = min(nq, opt.gt_queries)
    q = q_all[:nq].contiguous()
    gen = torch.Generator(device="cuda").manual_seed(int(sel * 1000) + 17)
    mask = (torch.rand(span, device="cuda", generator=gen) < sel) if sel < 1.0 else torch.ones(span, dtype=torch.bool, device="cuda")
    words = torch.zeros(sp_words, dtype=torch.int32, device="cuda")
    _lib.check(lib.granne_hip_filter_from_mask_device(p(mask.to(torch.uint8).data_ptr()), span, p(words.data_ptr()), B.dev, B.sp))
    torch.cuda.synchronize()
    mask_h = mask.cpu().numpy()
    # leg c's slices: made on the host, once
    local = []
    for sh in range(G):
        part = np.packbits(mask_h[offsets[sh]:offsets[sh] + n], bitorder="little")
        part = np.concatenate([part, np.zeros(-len(part) % 4, np.uint8)]).view(np.int32)
        local.append(torch.from_numpy(part.copy()).cuda())
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    cnt = torch.empty(nq, dtype=torch.int32, device="cuda")
    status = torch.zeros(4, dtype=torch.int32, device="cuda")
    c_ids = torch.empty((G, nq, k), dtype=torch.int64, device="cuda")
    c_ds = torch.empty((G, nq, k), dtype=torch.float32, device="cuda")
    c_cnt = torch.empty((G, nq), dtype=torch.int32, device="cuda")
    m_ids, m_ds, m_cnt = torch.empty_like(ids), torch.empty_like(ds), torch.empty_like(cnt)
    e_ids, e_ds, e_cnt = torch.empty((ng, k), dtype=torch.int64, device="cuda"), torch.empty((ng, k), dtype=torch.float32, device="cuda"), \
        torch.empty(ng, dtype=torch.int32, device="cuda")
    offs_c = (C.c_uint64 * G)(*offsets)

    def leg_a():
        host.search_batch_device(q.data_ptr(), nq, ef, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), status.data_ptr(), s)

    def leg_b():
        host.search_filtered_batch_device(q.data_ptr(), nq, ef, k, words.data_ptr(), 0, 0, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(),
                                          status.data_ptr(), s)

    def leg_c():
        for sh, g in enumerate(gixs):
            g.search_filtered_batch_device(q.data_ptr(), nq, ef, k, local[sh].data_ptr(), 0, 0, c_ids[sh].data_ptr(), c_ds[sh].data_ptr(),
                                           c_cnt[sh].data_ptr(), 0, status.data_ptr(), s)
        _lib.check(lib.granne_hip_merge_topk_device(p(c_ids.data_ptr()), p(c_ds.data_ptr()), p(c_cnt.data_ptr()), offs_c, G, nq, k,
                                                    p(m_ids.data_ptr()), p(m_ds.data_ptr()), p(m_cnt.data_ptr()), B.dev, B.sp))

    def leg_d():
        lib.granne_hip_sharded_exact_topk_filtered_device(host._h, p(q.data_ptr()), ng, k, p(words.data_ptr()), 0, p(e_ids.data_ptr()),
                                                          p(e_ds.data_ptr()), p(e_cnt.data_ptr()), p(status.data_ptr()), B.sp)

    bench.log("selectivity", sel, "nq", nq)
    for g in gixs:
        g.set_option(_lib.OPT_FORCE_GENERAL, 1)
    ms_a = interleaved({"a": leg_a})  # (the option is per index: leg a runs beside nothing that must not see it)
    for g in gixs:
        g.set_option(_lib.OPT_FORCE_GENERAL, 0)
    ms = interleaved({"b": leg_b, "c": leg_c, "d": leg_d})
    ms["a"] = ms_a["a"]
    # b against c (the same bits) and against d (recall)
    status.zero_()
    leg_b()
    torch.cuda.synchronize()
    st_b = status.cpu().tolist()
    b_ids, b_cnt = ids.clone(), cnt.clone()
    leg_c()
    status.zero_()
    leg_d()
    torch.cuda.synchronize()
    st_d = status.cpu().tolist()
    same = bool((b_ids == m_ids).all().item() and (b_cnt == m_cnt).all().item())
    valid = torch.arange(k, device="cuda")[None, :] < e_cnt[:, None]
    got = torch.where(torch.arange(k, device="cuda")[None, :] < b_cnt[:ng, None], b_ids[:ng], torch.full_like(b_ids[:ng], -2))
    hit = ((e_ids.unsqueeze(2) == got.unsqueeze(1)).any(dim=2) & valid).sum().item()
    rec = {"allowed_rows": int(mask.sum().item()), "queries": nq, "b_equals_c": same, "recall_at_10_of_b": round(hit / max(1, valid.sum().item()), 4),
           "status_b": st_b, "status_d": st_d}
    for name, count in (("a", nq), ("b", nq), ("c", nq), ("d", ng)):
        rec[name] = {"ms_median": round(median(ms[name]), 3), "queries_per_s": round(count / (median(ms[name]) * 1e-3), 1),
                     "ms_per_run": [round(x, 3) for x in ms[name]]}
    out["selectivities"][str(sel)] = rec
    bench.log("selectivity", sel, json.dumps({x: rec[x]["queries_per_s"] for x in "abcd"}), "b == c", same, "recall", rec["recall_at_10_of_b"])
    del local, mask, words

os.makedirs(os.path.dirname(opt.out), exist_ok=True)
with open(opt.out, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps({"out": opt.out, "selectivities": list(out["selectivities"])}))
