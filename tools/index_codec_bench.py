#!/usr/bin/env python
"""Host codec against device codec on one index: save and load_files, seconds and peak host memory.

    python tools/index_codec_bench.py [--out profiles/index_codec.json] [--dir DIR] [--scale 1.0] [--staging BYTES]
                                      [--sweep 16777216,268435456,1073741824]

Shape: a six-layer pyramid [14, 198, 2963, 44445, 666667, 10000000] (x --scale) over 100-byte int8 elements; the bottom
layer's rows hold 30 ids, the others 15. The adjacency is SYNTHETIC: ids drawn uniformly from the layer on the device
(torch), which is what an index looks like before Granne::reorder -- deltas of about len / 30, so mostly three-byte values
at the bottom. Elements are random int8.

What is timed (measuring-on-mi355x): wall-clock seconds (time.perf_counter) around the synchronous library calls, host work
included; the four legs alternate (save host, save on-device, load_files host, load_files on-device) over three repeats in
one process, after one untimed round that warms code objects and allocators. Files go to one directory (--dir, default the
working directory) and are read back right after they were written: the page cache is WARM for every load leg and absorbs
every save leg's writes (no fsync); nothing here can drop it. Every repeat checks that the two codecs wrote the same bytes
and loaded the same index. Peak host RSS (ru_maxrss) is taken per leg in a fresh child process each, one after another:
the child loads or makes the index first, and reports the peak before and after the leg.

The baseline is the host codec in the same run. Figures go to --out as one JSON document."""
import argparse
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PYRAMID = [14, 198, 2963, 44445, 666667, 10000000]
LEGS = ["save_host", "save_on_device", "load_files_host", "load_files_on_device"]


def make_index(scale):
    """The synthetic index, made on the device. Returns (Granne, layer lens)."""
    import numpy as np
    import torch
    import granne_amd
    lens = [max(1, int(round(n * scale))) for n in PYRAMID]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x67726E)
    layers = []
    for l, n in enumerate(lens):
        cnt = min(30 if l + 1 == len(lens) else 15, n)
        rows = torch.full((n, 30), -1, dtype=torch.int32, device="cuda")
        rows[:, :cnt] = torch.randint(0, n, (n, cnt), generator=gen, device="cuda", dtype=torch.int32)
        layers.append(rows)
    el = torch.randint(-127, 128, (lens[-1], 100), generator=gen, device="cuda", dtype=torch.int8)
    gix = granne_amd.Granne.from_device("angular_int", el.data_ptr(), lens[-1], 100, lens, [r.data_ptr() for r in layers], [30] * len(lens))
    torch.cuda.synchronize()
    del layers, el
    torch.cuda.empty_cache()
    return gix, lens


def same_file(a, b):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


def run_leg(leg, gix, d, staging):
    """One leg; returns (seconds, info words or None, loaded index or None)."""
    import granne_amd
    hi, he, di, de = (os.path.join(d, n) for n in ("host.index", "host.elements", "dev.index", "dev.elements"))
    t0 = time.perf_counter()
    out = None
    if leg == "save_host":
        gix.save(hi, he)
    elif leg == "save_on_device":
        gix.save(di, de, on_device=True, staging_bytes=staging)
    elif leg == "load_files_host":
        out = granne_amd.Granne.from_files(hi, "angular_int", he)
    else:
        out = granne_amd.Granne.from_files(hi, "angular_int", he, on_device=True, staging_bytes=staging)
    dt = time.perf_counter() - t0
    info = (out if out is not None else gix).last_codec_info if "on_device" in leg else None
    return dt, info, out


def child_times(args):
    import numpy as np
    gix, lens = make_index(args.scale)
    d = args.dir
    res = {leg: [] for leg in LEGS}
    infos = {}
    for rep in range(-1, 3):  # rep -1 warms up and is not recorded
        loaded = {}
        for leg in LEGS:
            dt, info, out = run_leg(leg, gix, d, args.staging)
            if rep >= 0:
                res[leg].append(round(dt, 4))
            if info:
                infos[leg] = list(info)
            if out is not None:
                loaded[leg] = out
        assert same_file(os.path.join(d, "host.index"), os.path.join(d, "dev.index")), "the index files differ"
        assert same_file(os.path.join(d, "host.elements"), os.path.join(d, "dev.elements")), "the elements files differ"
        a, b = loaded["load_files_host"], loaded["load_files_on_device"]
        assert a.hbm_bytes() == b.hbm_bytes() and a.num_layers() == b.num_layers() == len(lens)
        rng = np.random.default_rng(rep + 1)
        for l, n in enumerate(lens):
            for i in [0, n - 1] + [int(x) for x in rng.integers(0, n, 200)]:
                assert a.get_neighbors(i, l) == b.get_neighbors(i, l), (l, i)
        for x in loaded.values():
            x.close()
    out = {"layer_lens": lens, "index_file_bytes": os.path.getsize(os.path.join(d, "host.index")),
           "elements_file_bytes": os.path.getsize(os.path.join(d, "host.elements")), "seconds": res, "info_words": infos,
           "checked": "every repeat: files byte-identical; loaded indexes equal in hbm_bytes and in 202 sampled neighbor lists per layer"}
    print("RESULT " + json.dumps(out))


def child_rss(args):
    """Peak RSS of one leg. A save leg needs the index first: it is loaded from the files of the timing child through the
    device codec with a 16 MiB ring, which keeps the peak before the leg low."""
    import granne_amd
    d = args.dir
    gix = None
    if args.leg.startswith("save"):
        gix = granne_amd.Granne.from_files(os.path.join(d, "host.index"), "angular_int", os.path.join(d, "host.elements"), on_device=True,
                                           staging_bytes=16 << 20)
    else:
        import torch
        torch.zeros(1, device="cuda")  # the runtime is up before the peak is read
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    dt, info, out = run_leg(args.leg, gix, d, args.staging)
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print("RESULT " + json.dumps({"peak_rss_kib_before": before, "peak_rss_kib_after": after, "seconds": round(dt, 4)}))


def spawn(argv):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stdout.write(p.stdout)
        raise SystemExit("child %s failed (exit %d)" % (argv, p.returncode))
    return json.loads(lines[-1][7:])


def measure(common):
    """The timing child, then one child per leg for the peak RSS."""
    doc = spawn(["--child", "times"] + common)
    doc["peak_host_rss"] = {leg: spawn(["--child", "rss", "--leg", leg] + common) for leg in LEGS}
    doc["median_seconds"] = {leg: sorted(v)[len(v) // 2] for leg, v in doc["seconds"].items()}
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_codec.json"))
    ap.add_argument("--dir", default=None)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--staging", type=int, default=0)
    ap.add_argument("--sweep", default="", help="comma-separated staging sizes measured the same way and recorded under staging_sweep")
    ap.add_argument("--child", default=None)
    ap.add_argument("--leg", default=None)
    args = ap.parse_args()
    if args.child == "times":
        return child_times(args)
    if args.child == "rss":
        return child_rss(args)
    d = tempfile.mkdtemp(prefix="index_codec_", dir=args.dir or os.getcwd())
    try:
        common = ["--dir", d, "--scale", str(args.scale), "--staging", str(args.staging)]
        doc = measure(common)
        doc["staging_sweep"] = {}
        for s in [int(x) for x in args.sweep.split(",") if x]:
            other = measure(["--dir", d, "--scale", str(args.scale), "--staging", str(s)])
            doc["staging_sweep"][str(s)] = {k: other[k] for k in ("seconds", "median_seconds", "peak_host_rss", "info_words")}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    doc["staging_bytes"] = args.staging or (64 << 20)
    doc["what"] = ("synthetic adjacency (uniform ids, made on the device), 100-byte int8 elements; wall-clock seconds around the "
                   "synchronous calls, legs alternating over three repeats after one warm-up round, one process; files on one "
                   "filesystem, page cache warm (read back right after writing, no fsync); peak RSS per leg in a fresh child each")
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["median_seconds"]), json.dumps(doc["peak_host_rss"]))


if __name__ == "__main__":
    main()
